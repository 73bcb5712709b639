"""WSGANContModel -- the reference's continuous-label CGAN baseline (models/wsgan_cont_model.py:15-327) on the HIP path: G(image,
attribute) against a conditional PatchGAN D(image, attribute), an AlexNet identity term and an auxiliary attribute regressor E
(define_AR: the network regression.py trains; its `latest_net.pth` is what `--pretrained_model_path_E` loads, whole and strict).

Same plugin surface as the reference: flags and defaults, the 11 loss names, visual / model names, assertions, and the step order
forward -> D -> E -> G (models/wsgan_shared.py: WSGANPairModel, with the differences from the reference that wsgan_disc shares).
E's BatchNorm stays in train mode in all of its passes (real_B_E, the detached fake under --train_aux_on_fake, fake_B_E in the G
update), D's in all five of its passes.  Disabled loss terms are the Python float 0.0.

The reference's default generator name `unet_128` raises NotImplementedError from define_G -- pass `--which_model_netG unet` (the same
U-Net: like the reference, this model does not hand `--n_layers_G` on, so `unet` means 7 downsamplings), `unet_256` or
`resnet_<n>blocks`.

Stated difference from the reference, this model's own: real_A_E is never read by the reference and is not computed.
"""
import numpy as np
import torch

from . import networks
from .wsgan_shared import WSGANPairModel
from ..util.util import upsample2d

_COMMON_FLAGS = [   # reference models/wsgan_cont_model.py:21-26
    ('--norm_G', dict(type=str, default='instance')),
    ('--norm_D', dict(type=str, default='batch')),
    ('--embedding_nc', dict(type=int, default=1)),
    ('--attr_mean', dict(type=float, nargs='*', default=[0.0])),
    ('--attr_std', dict(type=float, nargs='*', default=[100])),
    ('--display_visuals', dict(action='store_true')),
]
_TRAIN_FLAGS = [    # :28-49
    ('--which_model_netE', dict(type=str, default='resnet18')),
    ('--pretrained_model_path_E', dict(type=str, default='pretrained_models/auxiliary_regresser.pth')),
    ('--pooling_E', dict(type=str, default='avg')),
    ('--cnn_dim_E', dict(type=int, nargs='+', default=[64, 1])),
    ('--cnn_pad_E', dict(type=int, default=1)),
    ('--cnn_relu_slope_E', dict(type=float, default=0.7)),
    ('--lr_E', dict(type=float, default=0.0002)),
    ('--fineSize_E', dict(type=int, default=224)),
    ('--lambda_L1', dict(type=float, default=0.0)),
    ('--lambda_IP', dict(type=float, default=1.0)),
    ('--lambda_AR', dict(type=float, default=1.0)),
    ('--lambda_A', dict(type=float, default=0.5)),
    ('--lambda_A_GAN', dict(type=float, default=0.5)),
    ('--which_model_netIP', dict(type=str, default='alexnet')),
    ('--fineSize_IP', dict(type=int, default=224)),
    ('--pretrained_model_path_IP', dict(type=str, default='pretrained_models/alexnet-owt-4df8aa71.pth')),
    ('--identity_preserving_criterion', dict(type=str, default='mse')),
    ('--relabel_D', dict(type=int, nargs='*', default=[0, 1, 0])),
    ('--no_mixed_label_D', dict(action='store_true')),
    ('--weight_label_D', dict(nargs='*', type=float, default=[0.5, 0, 0.5])),
    ('--train_aux_on_fake', dict(action='store_true')),
    ('--detach_fake_B', dict(action='store_true')),
]
_DEFAULT_OVERRIDES = dict(pool_size=0, no_lsgan=True, norm='instance', dataset_mode='wsgan_cont', which_model_netG='unet_128',
                          which_model_netD='n_layers', n_layers_D=4, batchSize=10, loadSize=128, fineSize=128, display_visuals=True,
                          save_epoch_freq=2)   # :52-63


class WSGANContModel(WSGANPairModel):
    COMMON_FLAGS, TRAIN_FLAGS, DEFAULT_OVERRIDES = _COMMON_FLAGS, _TRAIN_FLAGS, _DEFAULT_OVERRIDES
    AUX, AUX_LOSS, G_AUX_TERM = 'E', 'AR', 'z_rec'      # netE is called 'E' but it is the auxiliary regressor
    G_SUM = ('G_GAN', 'G_IP', 'G_L1', 'G_cycle', 'z_rec', 'G_GAN_cycle')     # reference :287

    # ------------------------------------------------------------------ construction (reference :67-154)
    def initialize(self, opt):
        WSGANPairModel.initialize(self, opt)
        assert opt.embedding_nc == 1
        self.loss_names = ['G_GAN', 'G_GAN_cycle', 'G_IP', 'G_L1', 'G_cycle', 'z_rec',
                           'D_real_right', 'D_real_wrong', 'D_fake', 'AR_real', 'AR_fake']
        self.visual_names = ['real_A', 'fake_B', 'real_B', 'rec_A'] if self.isTrain else ['real_A']
        self.model_names = ['G', 'D', 'E'] if self.isTrain else ['G']

        self.define_pair_nets()
        if self.isTrain:
            self.netE = networks.define_AR(opt.which_model_netE, 3, init_type=opt.init_type, pooling=opt.pooling_E,
                                           cnn_dim=opt.cnn_dim_E, cnn_pad=opt.cnn_pad_E, cnn_relu_slope=opt.cnn_relu_slope_E,
                                           gpu_ids=self.gpu_ids)
            self.load_aux(opt.pretrained_model_path_E)
            assert opt.pool_size == 0
            self.define_criteria()
            self.criterionAR = networks.MSELoss()
            self.define_optimizers(('G', 'D', 'E'), opt.lr_E)
        self.define_attr_normalize()
        if self.isTrain:
            self.define_transforms()
            self.relabel_D = opt.relabel_D
            if len(opt.weight_label_D) > 0:
                assert len(opt.weight_label_D) == len(opt.relabel_D)
                total = sum(opt.weight_label_D)
                self.weight_label_D = [w / total for w in opt.weight_label_D]
            else:
                self.weight_label_D = None
            self._relabel_lut = torch.tensor(np.array(self.relabel_D, dtype=np.float32), device=self.device)

    # ------------------------------------------------------------------ the step (reference :163-314)
    def set_input(self, input):
        if self.isTrain:
            if not self.opt.no_mixed_label_D:
                prefix = ''
                self.label_AB = input['label']
            else:
                # one label for the whole batch (A < B or A > B), drawn as the reference draws it
                self.label_AB = [np.random.choice(range(len(self.relabel_D)), p=self.weight_label_D)]
                prefix = str(self.label_AB[0]) + '_'
            self.real_A = self.to_act(input[prefix + 'A'])
            self.real_B = self.to_act(input[prefix + 'B'])
            self.attr_A = input[prefix + 'A_attr'].to(self.device, non_blocking=True)
            self.attr_B = input[prefix + 'B_attr'].to(self.device, non_blocking=True)
            self.image_paths = input[prefix + 'B_paths']
            lab = self.label_AB if isinstance(self.label_AB, torch.Tensor) else torch.as_tensor(np.asarray(self.label_AB))
            self._label_dev = lab.to(self.device, dtype=torch.int64, non_blocking=True).reshape(-1)
            self.real_A_IP = upsample2d(self.real_A, self.opt.fineSize_IP)
            self.real_B_E = upsample2d(self.real_B, self.opt.fineSize_E)     # (real_A_E of the reference is never read)
        self.end_set_input(input)

    def conditioning(self):
        return self.attr_normalize(self.attr_A), self.attr_normalize(self.attr_B)

    def sample_from_prior(self):
        # A -> B, the attribute is B's
        return self.netG(self.real_A, self.attr_normalize(self.attr_B))

    def backward_D(self):
        self.loss_D_fake = self.criterionGAN(self.netD(self.fake_B.detach(), self.embedding_B), False)
        self.loss_D_real_right = self.criterionGAN(self.netD(self.real_B, self.embedding_B), True)
        # "real image, wrong attribute": per-sample target relabel_D[label] (device-side LUT gather)
        target = self._relabel_lut.index_select(0, self._label_dev)
        self.loss_D_real_wrong = self.criterionGAN(self.netD(self.real_B, self.embedding_A), target)
        self.loss_D = (self.loss_D_fake + (self.loss_D_real_right + self.loss_D_real_wrong) * 0.5) * 0.5
        self.loss_D.backward()

    def _ar_loss(self, image_E):
        """criterionAR(netE(transform_E(image_E)), embedding_B): pooling and MSE as one node where the regressor pools"""
        E = getattr(self.netE, 'module', self.netE)
        x = self.transform_E(image_E)
        if E.pooling in ('avg', 'max'):
            return E.regress(x, self.embedding_B.reshape(self.embedding_B.size(0), -1), 0.0)[0]
        pred = self.netE(x)
        return self.criterionAR(pred, self.embedding_B.expand_as(pred).contiguous())

    aux_loss = _ar_loss
