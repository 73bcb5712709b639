"""WSGANContModel -- the reference's continuous-label CGAN baseline (models/wsgan_cont_model.py:15-327) on the HIP path: G(image,
attribute) against a conditional PatchGAN D(image, attribute), an AlexNet identity term and an auxiliary attribute regressor E
(define_AR: the network regression.py trains; its `latest_net.pth` is what `--pretrained_model_path_E` loads, whole and strict).

Same plugin surface as the reference: flags and defaults, the 11 loss names, visual / model names, assertions, and the step order
forward -> D -> E (backward_AR) -> G.  E's BatchNorm stays in train mode in all of its passes (real_B_E, the detached fake under
--train_aux_on_fake, fake_B_E in the G update), D's in all five of its passes.  Disabled loss terms are the Python float 0.0.

The reference's default generator name `unet_128` raises NotImplementedError from define_G -- pass `--which_model_netG unet` (the same
U-Net: like the reference, this model does not hand `--n_layers_G` on, so `unet` means 7 downsamplings), `unet_256` or
`resnet_<n>blocks`.

Stated differences from the reference:
  * real_A_E is never read by the reference and is not computed;
  * when fineSize_IP == fineSize_E one upsample2d(fake_B) feeds both the identity net and the regressor;
  * fake_B, rec_A and that shared resized image reach their consumers through hip.functional.fan_out, so the gradients coming back
    are summed by one kernel launch each (csrc/grad_fanin.hip) where autograd would chain binary adds.  PCGAN_FANOUT=0 (read once,
    when this module is imported) hands the tensors on unchanged and autograd accumulates as before;
  * data parallelism is one process per GPU + RCCL all-reduce of the flat gradient buffers instead of nn.DataParallel.
Everything this model issues runs on the main stream (no branches); the library's parameter-gradient side stream is as elsewhere.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import networks
from .base_model import BaseModel
from ..hip import functional as HF
from ..hip import parallel
from ..hip.optim import FusedAdam
from ..util.util import upsample2d

_FANOUT = os.environ.get('PCGAN_FANOUT', '1') != '0'

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


def _fan(x, n):
    """x for n consumers: n aliases whose gradients one launch sums (or x itself n times: PCGAN_FANOUT=0, one consumer, no graph)"""
    if not _FANOUT or n < 2 or not x.requires_grad:
        return [x] * n
    return list(HF.fan_out(x, n))


class WSGANContModel(BaseModel):
    def name(self):
        return 'WSGANContModel'

    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        for flag, kw in _COMMON_FLAGS + (_TRAIN_FLAGS if is_train else []):
            parser.add_argument(flag, **kw)
        parser.set_defaults(**_DEFAULT_OVERRIDES)
        return parser

    # ------------------------------------------------------------------ construction (reference :67-154)
    def initialize(self, opt):
        BaseModel.initialize(self, opt)
        assert opt.input_nc == opt.output_nc
        assert opt.embedding_nc == 1
        self.attr_bins = opt.attr_bins
        self.loss_names = ['G_GAN', 'G_GAN_cycle', 'G_IP', 'G_L1', 'G_cycle', 'z_rec',
                           'D_real_right', 'D_real_wrong', 'D_fake', 'AR_real', 'AR_fake']
        self.visual_names = ['real_A', 'fake_B', 'real_B', 'rec_A'] if self.isTrain else ['real_A']
        self.model_names = ['G', 'D', 'E'] if self.isTrain else ['G']

        self.netG = networks.define_G(opt.input_nc, opt.output_nc, opt.embedding_nc, opt.ngf,
                                      which_model_netG=opt.which_model_netG, norm=opt.norm_G, nl=opt.nl,
                                      dropout=opt.dropout, init_type=opt.init_type, gpu_ids=self.gpu_ids,
                                      upsample=opt.upsample, size=opt.fineSize)
        if self.isTrain:
            self.netD = networks.define_D(opt.output_nc, opt.embedding_nc, opt.ndf, opt.which_model_netD, opt.n_layers_D, opt.norm_D,
                                          opt.no_lsgan, opt.init_type, num_Ds=opt.num_Ds, gpu_ids=self.gpu_ids, size=opt.fineSize)
            self.netIP = networks.define_IP(opt.which_model_netIP, opt.input_nc, self.gpu_ids)     # not saved
            getattr(self.netIP, 'module', self.netIP).load_pretrained(opt.pretrained_model_path_IP)
            # netE is called 'E' but it is the auxiliary regressor
            self.netE = networks.define_AR(opt.which_model_netE, 3, init_type=opt.init_type, pooling=opt.pooling_E,
                                           cnn_dim=opt.cnn_dim_E, cnn_pad=opt.cnn_pad_E, cnn_relu_slope=opt.cnn_relu_slope_E,
                                           gpu_ids=self.gpu_ids)
            if not opt.continue_train and opt.pretrained_model_path_E:
                state = torch.load(opt.pretrained_model_path_E, map_location='cpu')
                getattr(self.netE, 'module', self.netE).load_state_dict(state, strict=True)

            assert opt.pool_size == 0
            self.criterionGAN = networks.GANLoss(use_lsgan=not opt.no_lsgan, tensor=self.Tensor)
            self.criterionL1 = networks.L1Loss()
            crit = opt.identity_preserving_criterion.lower()
            if crit == 'mse':
                self.criterionIP = networks.MSELoss()
            elif crit == 'l1':
                self.criterionIP = networks.L1Loss()
            else:
                raise NotImplementedError('Not Implemented')
            self.criterionCycle = networks.L1Loss()
            self.criterionAR = networks.MSELoss()

            for net in (self.netG, self.netD, self.netE, self.netIP):
                parallel.broadcast_parameters(net)
            betas = (opt.beta1, 0.999)
            self.optimizer_G = FusedAdam(self.netG.parameters(), lr=opt.lr, betas=betas)
            self.optimizer_D = FusedAdam(self.netD.parameters(), lr=opt.lr, betas=betas)
            self.optimizer_E = FusedAdam(self.netE.parameters(), lr=opt.lr_E, betas=betas)
            self.optimizers = [self.optimizer_G, self.optimizer_D, self.optimizer_E]   # the reference's order (:133-135)
            self.set_requires_grad(self.netIP, False)   # no optimizer in the reference either: its gradients are unused

        self.attr_mean, self.attr_std = opt.attr_mean, opt.attr_std
        mean, std = opt.attr_mean[0], opt.attr_std[0]
        self.attr_normalize = lambda x: (x - mean) / std
        if opt.display_visuals:
            self.pre_generate_embeddings()
        if self.isTrain:
            self.transform_IP = networks.Normalize((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))
            self.transform_E = networks.Normalize((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))
            self.relabel_D = opt.relabel_D
            if len(opt.weight_label_D) > 0:
                assert len(opt.weight_label_D) == len(opt.relabel_D)
                total = sum(opt.weight_label_D)
                self.weight_label_D = [w / total for w in opt.weight_label_D]
            else:
                self.weight_label_D = None
            self._relabel_lut = torch.tensor(np.array(self.relabel_D, dtype=np.float32), device=self.device)

    def pre_generate_embeddings(self):
        arr = np.array(self.opt.attr_bins).reshape(len(self.opt.attr_bins), 1, 1, 1, 1)
        self.fixed_embeddings = [self.attr_normalize(torch.Tensor(arr[i]).to(self.device)) for i in range(arr.shape[0])]

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
        else:
            self.real_A = self.to_act(input['A'])
            self.image_paths = input['A_paths']
            if 'B_attr' in input:
                self.attr_B = input['B_attr'].to(self.device, non_blocking=True)
                self.image_paths = input['B_paths']
        self.current_iter += 1
        self.current_batch_size = int(self.real_A.size(0))

    def forward(self):
        o = self.opt
        self.embedding_A = self.attr_normalize(self.attr_A)
        self.embedding_B = self.attr_normalize(self.attr_B)
        self.fake_B = self.netG(self.real_A, self.embedding_B)
        # who reads fake_B in backward_G: the discriminator join, the second generator pass, the L1 term and the resize(s) feeding
        # the identity net and the regressor -- one alias each, in this order (the order of the gradient sum)
        want_ip, want_e = o.lambda_IP > 0.0, o.lambda_AR > 0.0
        shared = want_ip and want_e and o.fineSize_IP == o.fineSize_E
        readers = ['D'] + ([] if o.detach_fake_B else ['G2']) + (['L1'] if o.lambda_L1 > 0.0 else [])
        readers += ['big'] if shared else (['IP'] if want_ip else []) + (['E'] if want_e else [])
        fb = dict(zip(readers, _fan(self.fake_B, len(readers))))
        self._fake_B_D, self._fake_B_L1 = fb['D'], fb.get('L1')
        if shared:
            self.fake_B_IP, self.fake_B_E = _fan(upsample2d(fb['big'], o.fineSize_E), 2)
        else:
            # a term that is switched off reads nothing; --train_aux_on_fake still needs the (detached) regressor input
            self.fake_B_IP = upsample2d(fb['IP'], o.fineSize_IP) if want_ip else None
            self.fake_B_E = None
            if want_e or o.train_aux_on_fake:
                self.fake_B_E = upsample2d(fb['E'] if want_e else self.fake_B.detach(), o.fineSize_E)
        self.rec_A = self.netG(self.fake_B.detach() if o.detach_fake_B else fb['G2'], self.embedding_A)
        # rec_A is read by the discriminator (--lambda_A_GAN) and by the cycle L1 (--lambda_A)
        readers = (['D'] if o.lambda_A_GAN > 0.0 else []) + (['cycle'] if o.lambda_A > 0.0 else [])
        ra = dict(zip(readers, _fan(self.rec_A, len(readers))))
        self._rec_A_D, self._rec_A_cycle = ra.get('D'), ra.get('cycle')

    def test(self):
        return

    def sample_from_prior(self):
        # A -> B, the attribute is B's
        return self.netG(self.real_A, self.attr_normalize(self.attr_B))

    def sample_from_label(self, label):
        attr_B = torch.Tensor([self.attr_bins[label]]).reshape(1, 1, 1, 1).to(self.device)
        return self.netG(self.real_A, self.attr_normalize(attr_B))

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

    def backward_AR(self):
        self.loss_AR_real = self._ar_loss(self.real_B_E)
        self.loss_AR_fake = self._ar_loss(self.fake_B_E.detach()) if self.opt.train_aux_on_fake else 0.0
        self.loss_AR = (self.loss_AR_fake + self.loss_AR_real) * 0.5
        self.loss_AR.backward()

    def backward_G(self):
        o = self.opt
        self.loss_G_GAN = self.criterionGAN(self.netD(self._fake_B_D, self.embedding_B), True)
        if o.lambda_A_GAN > 0.0:
            self.loss_G_GAN_cycle = self.criterionGAN(self.netD(self._rec_A_D, self.embedding_A), True) * o.lambda_A_GAN
        else:
            self.loss_G_GAN_cycle = 0.0
        self.loss_G_L1 = self.criterionL1(self._fake_B_L1, self.real_A) * o.lambda_L1 if o.lambda_L1 > 0.0 else 0.0
        if o.lambda_IP > 0.0:
            with torch.no_grad():
                feature_A = self.netIP(self.transform_IP(self.real_A_IP))
            self.loss_G_IP = self.criterionIP(self.netIP(self.transform_IP(self.fake_B_IP)), feature_A) * o.lambda_IP
        else:
            self.loss_G_IP = 0.0
        self.loss_z_rec = self._ar_loss(self.fake_B_E) * o.lambda_AR if o.lambda_AR > 0.0 else 0.0
        self.loss_G_cycle = self.criterionCycle(self._rec_A_cycle, self.real_A) * o.lambda_A if o.lambda_A > 0.0 else 0.0
        self.loss_G = self.loss_G_GAN + self.loss_G_IP + self.loss_G_L1 + self.loss_G_cycle + self.loss_z_rec + self.loss_G_GAN_cycle
        self.loss_G.backward()

    def optimize_parameters(self):
        self.forward()
        # update D
        self.set_requires_grad(self.netD, True)
        self.optimizer_D.zero_grad()
        self.backward_D()
        parallel.sync_gradients(self.optimizer_D)
        self.optimizer_D.step()
        parallel.ddp_check(self.optimizer_D, 'D')
        # update E
        self.set_requires_grad(self.netE, True)
        self.optimizer_E.zero_grad()
        self.backward_AR()
        parallel.sync_gradients(self.optimizer_E)
        self.optimizer_E.step()
        parallel.ddp_check(self.optimizer_E, 'E')
        # update G
        self.set_requires_grad(self.netD, False)
        self.set_requires_grad(self.netE, False)
        self.optimizer_G.zero_grad()
        self.backward_G()
        parallel.sync_gradients(self.optimizer_G)
        self.optimizer_G.step()
        parallel.ddp_check(self.optimizer_G, 'G')

    def get_current_visuals(self):
        self.set_requires_grad(self.netG, False)
        ret = OrderedDict()
        for name in self.visual_names:
            if isinstance(name, str):
                ret[name] = getattr(self, name)
        if self.opt.display_visuals:
            for L, embedding in enumerate(self.fixed_embeddings):
                ret['attr_' + str(L)] = self.netG(self.real_A[0:1, ...], embedding)
        self.set_requires_grad(self.netG, True)
        return ret
