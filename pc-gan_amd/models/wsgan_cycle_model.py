"""WSGANCycleModel -- the reference's attribute-conditioned cycle model (models/wsgan_cycle_model.py:13-269) on the
HIP path: G(image, attribute) with an unconditional PatchGAN, an AlexNet identity term and an encoder E that is TRAINED
here (it regresses the attribute back: x -> y -> x and y -> x -> y cycles).  SURVEY.md 8(f) rank 1 / config 5.

Same plugin surface as the reference (flags, defaults, loss / visual / model names, step order: D first, then G and E
together).  Differences, all stated where they occur: the reference's default generator name `unet_128` raises
NotImplementedError from define_G -- pass `--which_model_netG unet` (the same U-Net: like the reference, this model does not
hand `--n_layers_G` on, so its `unet` always has the default 7 downsamplings), `unet_256` or `resnet_9blocks`; the BicycleGAN U-Nets (`unet_*_input`, `unet_*_all`) are outside the hot path; `--use_bicycle_E`
(another encoder family) raises.  The AlexNet identity term runs on its hip.ops.branch('IP'), beside the discriminator's
pass (IP_ON_BRANCH); data parallelism is the shared module's (models/wsgan_shared.py).

WSGANBiGANModel derives from this class and changes CONDITIONAL_D, LOSS_NAMES, adversarial_terms() and forward()'s context.
"""
from . import networks
from .wsgan_shared import WSGANBase, sum_terms
from ..util.util import upsample2d

_COMMON_FLAGS = [   # reference models/wsgan_cycle_model.py:18-32
    ('--norm_G', dict(type=str, default='instance')),
    ('--norm_D', dict(type=str, default='batch')),
    ('--embedding_nc', dict(type=int, default=1)),
    ('--which_model_netE', dict(type=str, default='resnet18')),
    ('--use_bicycle_E', dict(action='store_true')),
    ('--pooling_E', dict(type=str, default='max')),
    ('--cnn_dim_E', dict(type=int, nargs='+', default=[64, 1])),
    ('--cnn_pad_E', dict(type=int, default=1)),
    ('--cnn_relu_slope_E', dict(type=float, default=0.7)),
    ('--fineSize_E', dict(type=int, default=224)),
    ('--pretrained_model_path_E', dict(type=str, default='pretrained_models/resnet18-5c106cde.pth')),
    ('--attr_mean', dict(type=float, nargs='*', default=[0.0])),
    ('--attr_std', dict(type=float, nargs='*', default=[100])),
    ('--display_visuals', dict(action='store_true')),
]
_TRAIN_FLAGS = [    # :33-41
    ('--lambda_x', dict(type=float, default=1.0)),
    ('--lambda_y', dict(type=float, default=1.0)),
    ('--lambda_IP', dict(type=float, default=1.0)),
    ('--which_model_netIP', dict(type=str, default='alexnet')),
    ('--fineSize_IP', dict(type=int, default=224)),
    ('--pretrained_model_path_IP', dict(type=str, default='pretrained_models/alexnet-owt-4df8aa71.pth')),
    ('--no_trick', dict(action='store_true')),
    ('--identity_preserving_criterion', dict(type=str, default='mse')),
]
_DEFAULT_OVERRIDES = dict(pool_size=0, no_lsgan=True, norm='instance', dataset_mode='wsgan_cycle',
                          which_model_netG='unet_128', which_model_netD='n_layers', n_layers_D=4, batchSize=10,
                          loadSize=140, fineSize=128, display_visuals=True, save_epoch_freq=2)   # :44-55



class WSGANCycleModel(WSGANBase):
    COMMON_FLAGS, TRAIN_FLAGS, DEFAULT_OVERRIDES = _COMMON_FLAGS, _TRAIN_FLAGS, _DEFAULT_OVERRIDES
    SOURCE = 'real_x'
    IP_ON_BRANCH = True
    LOSS_NAMES = ['G_GAN', 'G_IP', 'cycle_x', 'cycle_y', 'D_real', 'D_fake']
    CONDITIONAL_D = False   # unconditional discriminator: nz = 0, called D(image)   (:98-100)

    # ------------------------------------------------------------------ construction (reference :59-146)
    def initialize(self, opt):
        WSGANBase.initialize(self, opt)
        assert opt.embedding_nc == 1
        self.loss_names = list(self.LOSS_NAMES)
        self.visual_names = ['real_x', 'fake_x', 'rec_x'] if self.isTrain else ['real_x']
        self.model_names = ['G', 'E', 'D'] if self.isTrain else ['G', 'E']

        self.netG = self.define_G()
        if opt.use_bicycle_E:
            raise NotImplementedError('pcgan_amd: --use_bicycle_E (define_E_bicycle) is outside the MI355X hot path')
        self.netE = networks.define_E(opt.which_model_netE, 3, init_type=opt.init_type, pooling=opt.pooling_E,
                                      cnn_dim=opt.cnn_dim_E, cnn_pad=opt.cnn_pad_E,
                                      cnn_relu_slope=opt.cnn_relu_slope_E, gpu_ids=self.gpu_ids)
        if self.isTrain and not opt.continue_train:
            getattr(self.netE, 'module', self.netE).load_base(opt.pretrained_model_path_E)

        if self.isTrain:
            self.netD = self.define_D(opt.embedding_nc if self.CONDITIONAL_D else 0)
            self.netIP = self.define_IP()
            assert opt.pool_size == 0
            self.define_criteria()
            self.criterionAR = networks.MSELoss()
            self.define_optimizers(('G', 'E', 'D'), opt.lr)
        self.define_attr_normalize()
        if self.isTrain:
            self.define_transforms()

    # ------------------------------------------------------------------ the step (reference :148-256)
    def set_input(self, input):
        if self.isTrain:
            self.real_x = self.to_act(input['A'])
            self.real_y = self.attr_normalize(input['B_attr'].to(self.device, non_blocking=True))
            self.image_paths = input['B_paths']
            self.real_x_IP = upsample2d(self.real_x, self.opt.fineSize_IP)
            self.real_x_E = upsample2d(self.real_x, self.opt.fineSize_E)
        self.end_set_input(input)

    def set_attr_B(self, attr):
        self.real_y = self.attr_normalize(attr)

    def forward(self):
        # (the encoder input is NOT passed through transform_E here, as in the reference :170)
        self.fake_x = self.netG(self.real_x, self.real_y)
        self.fake_x_IP = upsample2d(self.fake_x, self.opt.fineSize_IP)
        self.fake_x_E = upsample2d(self.fake_x, self.opt.fineSize_E)
        self.fake_y = self.netE(self.real_x_E)
        self.rec_x = self.netG(self.real_x, self.fake_y)
        self.rec_y = self.netE(self.fake_x_E)

    def sample_from_prior(self):
        # A -> B, the attribute is B's
        return self.netG(self.real_x, self.real_y)

    def judge(self, image, rating):
        return self.netD(image, rating) if self.CONDITIONAL_D else self.netD(image)

    def backward_D(self):
        # the generated side detached: (G(y), y) = (fake_x, real_y) against (x, E(x)) = (real_x, fake_y)
        self.loss_D_fake = self.criterionGAN(self.judge(self.fake_x.detach(), self.real_y), False)
        self.loss_D_real = self.criterionGAN(self.judge(self.real_x, self.fake_y.detach()), True)
        self.loss_D = (self.loss_D_fake + self.loss_D_real) * 0.5
        self.loss_D.backward()

    def adversarial_terms(self):
        self.loss_G_GAN = self.criterionGAN(self.judge(self.fake_x, self.real_y), True)
        return [self.loss_G_GAN]

    def backward_GE(self):
        o = self.opt
        b_ip = self.identity_term(self.real_x_IP, self.fake_x_IP)     # AlexNet branch beside the discriminator branch (different nets)
        adversarial = self.adversarial_terms()
        self.loss_cycle_x = self.criterionCycle(self.rec_x, self.real_x) * o.lambda_x if o.lambda_x > 0.0 else 0.0
        self.loss_cycle_y = self.criterionAR(self.rec_y, self.real_y) * o.lambda_y if o.lambda_y > 0.0 else 0.0
        b_ip.join(self.loss_G_IP)
        self.loss_G = sum_terms(adversarial + [self.loss_G_IP, self.loss_cycle_x, self.loss_cycle_y])
        self.loss_G.backward()

    def optimize_parameters(self):
        self.forward()
        self.update(['D'], self.backward_D, {'D': True})
        self.update(['G', 'E'], self.backward_GE, {'D': False})
