"""WSGANDiscModel -- the reference's class-label CGAN baseline (models/wsgan_disc_model.py:14-311) on the HIP path: G(image, one-hot
class) against a conditional PatchGAN D(image, one-hot class), an AlexNet identity term and an auxiliary classifier AC (define_AC: the
network classification.py trains; `--pretrained_model_path_AC` loads its state dict, whole and strict).

Same plugin surface as the reference: flags and defaults, the 11 loss names, visual / model names, assertions, and the step order
forward -> D -> AC -> G.  One (label_A, label_B, label_B_not) triple is drawn per step from Python's global `random`, or read from
`--train_label_pairs`.  AC's BatchNorm stays in train mode in all of its passes (real_B_AC, the detached fake under
--train_aux_on_fake, fake_B_AC in the G update, where its parameters are frozen and only d loss / d input is formed), D's in all five of
its passes.  Disabled loss terms are the Python float 0.0.

This is the one wsgan model whose reference accepts `--pool_size N > 0`: one ImagePool per class keeps a history of generated images,
and the batch D sees as "fake" comes from the pool of label_B.  The pool lives on the device and a query is one kernel launch
(util/image_pool.py, csrc/image_pool.hip); with the default `--pool_size 0` nothing is launched.

The reference's default generator name `unet_128` raises NotImplementedError from define_G -- pass `--which_model_netG unet` (the same
U-Net: like the reference, this model does not hand `--n_layers_G` on, so `unet` means 7 downsamplings), `unet_256` or
`resnet_<n>blocks`.

Stated differences from the reference:
  * label_B_not is drawn with random.sample(sorted(...), 1): the reference samples from a set, which Python >= 3.11 refuses; for the
    ints 0 .. K-1 a set iterates in ascending order, so under one seed this is the reference's own draw on Python <= 3.10;
  * when fineSize_IP == fineSize_AC one upsample2d(fake_B) feeds both the identity net and the classifier;
  * fake_B, rec_A and that shared resized image reach their consumers through hip.functional.fan_out, so the gradients coming back
    are summed by one kernel launch each (csrc/grad_fanin.hip) where autograd would chain binary adds.  PCGAN_FANOUT=0 (read once,
    when this module is imported) hands the tensors on unchanged and autograd accumulates as before;
  * the head of AC and its CrossEntropyLoss are one node (ResNet.classify, csrc/linear_head.hip);
  * a torch.distributed run of more than one rank is refused: one label triple per GLOBAL batch needs a draw shared by all ranks.
Everything this model issues runs on the main stream (no branches); the library's parameter-gradient side stream is as elsewhere.
"""
import os
import random
from collections import OrderedDict

import numpy as np
import torch

from . import networks
from .base_model import BaseModel
from ..hip import functional as HF
from ..hip import parallel
from ..hip.optim import FusedAdam
from ..util.image_pool import ImagePool
from ..util.util import upsample2d, get_attr_label

_FANOUT = os.environ.get('PCGAN_FANOUT', '1') != '0'

_COMMON_FLAGS = [   # reference models/wsgan_disc_model.py:20-23
    ('--norm_G', dict(type=str, default='instance', help='instance normalization or batch normalization')),
    ('--norm_D', dict(type=str, default='batch', help='instance normalization or batch normalization')),
    ('--embedding_nc', dict(type=int, default=5, help='# of embedding channels')),
    ('--display_visuals', dict(action='store_true', help='display aging visuals if True')),
]
_TRAIN_FLAGS = [    # :25-43
    ('--lambda_L1', dict(type=float, default=0.0, help='weight for L1 loss')),
    ('--lambda_IP', dict(type=float, default=1.0, help='weight for identity preserving loss')),
    ('--lambda_AC', dict(type=float, default=1, help='weight for auxiliary classifier')),
    ('--lambda_A', dict(type=float, default=0.5, help='weight for cycle consistency loss')),
    ('--lambda_A_GAN', dict(type=float, default=0.5, help='weight for GAN loss on rec_A')),
    ('--which_model_netIP', dict(type=str, default='alexnet', help='model type for IP loss')),
    ('--which_model_netAC', dict(type=str, default='resnet18', help='model type for AC loss')),
    ('--pooling_AC', dict(type=str, default='avg', help='which pooling layer in AC')),
    ('--dropout_AC', dict(type=float, default=0.5, help='p in dropout layer')),
    ('--fineSize_IP', dict(type=int, default=224, help='fineSize for IP')),
    ('--fineSize_AC', dict(type=int, default=224, help='fineSize for AC')),
    ('--pretrained_model_path_IP', dict(type=str, default='pretrained_models/alexnet-owt-4df8aa71.pth',
                                        help='pretrained model path to IP net')),
    ('--pretrained_model_path_AC', dict(type=str, default='pretrained_models/auxiliary_classifier.pth',
                                        help='pretrained model path to AC net')),
    ('--train_label_pairs', dict(type=str, default='', help='file path of train label pairs')),
    ('--lr_AC', dict(type=float, default=0.0002, help='learning rate for AC')),
    ('--train_aux_on_fake', dict(action='store_true', help='if True, train AC on fake images')),
    ('--identity_preserving_criterion', dict(type=str, default='mse', help='which criterion to use for identity preserving loss')),
    ('--detach_fake_B', dict(action='store_true', help='if True, detach fake_B when computing rec_A')),
    ('--label_as_group', dict(action='store_true')),
]
_DEFAULT_OVERRIDES = dict(pool_size=0, no_lsgan=True, norm='instance', dataset_mode='wsgan_disc', which_model_netG='unet_128',
                          which_model_netD='n_layers', n_layers_D=4, batchSize=10, loadSize=128, fineSize=128, display_visuals=True,
                          save_epoch_freq=2)   # :46-57


def _fan(x, n):
    """x for n consumers: n aliases whose gradients one launch sums (or x itself n times: PCGAN_FANOUT=0, one consumer, no graph)"""
    if not _FANOUT or n < 2 or not x.requires_grad:
        return [x] * n
    return list(HF.fan_out(x, n))


class WSGANDiscModel(BaseModel):
    def name(self):
        return 'WSGANDiscModel'

    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        for flag, kw in _COMMON_FLAGS + (_TRAIN_FLAGS if is_train else []):
            parser.add_argument(flag, **kw)
        parser.set_defaults(**_DEFAULT_OVERRIDES)
        return parser

    # ------------------------------------------------------------------ construction (reference :61-151)
    def initialize(self, opt):
        BaseModel.initialize(self, opt)
        assert opt.input_nc == opt.output_nc
        assert opt.embedding_nc == opt.num_classes
        if parallel.is_distributed() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError('pcgan_amd: wsgan_disc draws one label triple per global batch from the process-local generator; '
                                      'a run of %d ranks would need a shared draw and is not supported'
                                      % torch.distributed.get_world_size())
        self.attr_bins = opt.attr_bins
        self.attr_bins_with_inf = opt.attr_bins + [float('inf')]
        self.loss_names = ['G_GAN', 'G_GAN_cycle', 'G_IP', 'G_L1', 'G_AC', 'G_cycle',
                           'D_real_right', 'D_real_wrong', 'D_fake', 'AC_real', 'AC_fake']
        self.visual_names = ['real_A', 'fake_B', 'real_B', 'rec_A'] if self.isTrain else ['real_A']
        self.model_names = ['G', 'D', 'AC'] if self.isTrain else ['G']

        self.netG = networks.define_G(opt.input_nc, opt.output_nc, opt.embedding_nc, opt.ngf,
                                      which_model_netG=opt.which_model_netG, norm=opt.norm_G, nl=opt.nl,
                                      dropout=opt.dropout, init_type=opt.init_type, gpu_ids=self.gpu_ids,
                                      upsample=opt.upsample, size=opt.fineSize)
        if self.isTrain:
            self.netD = networks.define_D(opt.output_nc, opt.embedding_nc, opt.ndf, opt.which_model_netD, opt.n_layers_D, opt.norm_D,
                                          opt.no_lsgan, opt.init_type, num_Ds=opt.num_Ds, gpu_ids=self.gpu_ids, size=opt.fineSize)
            self.netIP = networks.define_IP(opt.which_model_netIP, opt.input_nc, self.gpu_ids)     # not saved
            getattr(self.netIP, 'module', self.netIP).load_pretrained(opt.pretrained_model_path_IP)
            self.netAC = networks.define_AC(opt.which_model_netAC, opt.input_nc, opt.init_type, opt.num_classes,
                                            pooling=opt.pooling_AC, dropout=opt.dropout_AC, gpu_ids=self.gpu_ids)
            if not opt.continue_train and opt.pretrained_model_path_AC:
                state = torch.load(opt.pretrained_model_path_AC, map_location='cpu')
                getattr(self.netAC, 'module', self.netAC).load_state_dict(state, strict=True)

            self.fake_B_pool = [ImagePool(opt.pool_size) for _ in range(opt.num_classes)]
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

            betas = (opt.beta1, 0.999)
            self.optimizer_G = FusedAdam(self.netG.parameters(), lr=opt.lr, betas=betas)
            self.optimizer_D = FusedAdam(self.netD.parameters(), lr=opt.lr, betas=betas)
            self.optimizer_AC = FusedAdam(self.netAC.parameters(), lr=opt.lr_AC, betas=betas)
            self.optimizers = [self.optimizer_G, self.optimizer_D, self.optimizer_AC]   # the reference's order (:127-129)
            self.set_requires_grad(self.netIP, False)   # no optimizer in the reference either: its gradients are unused

            if opt.train_label_pairs:
                with open(opt.train_label_pairs, 'r') as f:
                    self.train_label_pairs = [line.rstrip('\n') for line in f.readlines()]
            else:
                self.train_label_pairs = None

        self.pre_generate_embeddings()
        self._label_cache = {}
        if self.isTrain:
            self.transform_IP = networks.Normalize((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))
            self.transform_AC = networks.Normalize((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))

    def pre_generate_embeddings(self):
        K = self.opt.num_classes
        eye = np.eye(K, dtype=np.float32)
        self.one_hot_labels = [torch.from_numpy(eye[L].copy()).view(1, K, 1, 1).to(self.device) for L in range(K)]

    def sample_label_pairs(self):
        """(label_A, label_B, label_B_not), reference :153-160"""
        K = self.opt.num_classes
        if self.train_label_pairs:
            labels_AnB = self.train_label_pairs[self.current_iter % len(self.train_label_pairs)].split()
        else:
            labels_AnB = random.sample(range(K), 2)
        label_B = int(labels_AnB[1])
        return int(labels_AnB[0]), label_B, random.sample(sorted(set(range(K)) - set([label_B])), 1)[0]

    def _class_labels(self, L, batch):
        """(batch,) int64 on the device, all L: the classifier's target (the reference builds it three times a step)"""
        key = (int(L), int(batch))
        if key not in self._label_cache:
            self._label_cache[key] = torch.full((key[1],), key[0], dtype=torch.int64, device=self.device)
        return self._label_cache[key]

    # ------------------------------------------------------------------ the step (reference :162-298)
    def set_input(self, input):
        if self.isTrain:
            self.label_A, self.label_B, self.label_B_not = self.sample_label_pairs()
            self.real_A = self.to_act(input[self.label_A])
            self.real_B = self.to_act(input[self.label_B])
            self.real_A_IP = upsample2d(self.real_A, self.opt.fineSize_IP)
            self.real_B_AC = upsample2d(self.real_B, self.opt.fineSize_AC)
            self.image_paths = input['path_' + str(self.label_B)]
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
        self.fake_B = self.netG(self.real_A, self.one_hot_labels[self.label_B])
        # who reads fake_B in backward_G: the discriminator join, the second generator pass, the L1 term and the resize(s) feeding
        # the identity net and the classifier -- one alias each, in this order (the order of the gradient sum)
        want_ip, want_ac = o.lambda_IP > 0.0, o.lambda_AC > 0.0
        shared = want_ip and want_ac and o.fineSize_IP == o.fineSize_AC
        readers = ['D'] + ([] if o.detach_fake_B else ['G2']) + (['L1'] if o.lambda_L1 > 0.0 else [])
        readers += ['big'] if shared else (['IP'] if want_ip else []) + (['AC'] if want_ac else [])
        fb = dict(zip(readers, _fan(self.fake_B, len(readers))))
        self._fake_B_D, self._fake_B_L1 = fb['D'], fb.get('L1')
        if shared:
            self.fake_B_IP, self.fake_B_AC = _fan(upsample2d(fb['big'], o.fineSize_AC), 2)
        else:
            # a term that is switched off reads nothing; --train_aux_on_fake still needs the (detached) classifier input
            self.fake_B_IP = upsample2d(fb['IP'], o.fineSize_IP) if want_ip else None
            self.fake_B_AC = None
            if want_ac or o.train_aux_on_fake:
                self.fake_B_AC = upsample2d(fb['AC'] if want_ac else self.fake_B.detach(), o.fineSize_AC)
        self.rec_A = self.netG(self.fake_B.detach() if o.detach_fake_B else fb['G2'], self.one_hot_labels[self.label_A])
        # rec_A is read by the discriminator (--lambda_A_GAN) and by the cycle L1 (--lambda_A)
        readers = (['D'] if o.lambda_A_GAN > 0.0 else []) + (['cycle'] if o.lambda_A > 0.0 else [])
        ra = dict(zip(readers, _fan(self.rec_A, len(readers))))
        self._rec_A_D, self._rec_A_cycle = ra.get('D'), ra.get('cycle')

    def test(self):
        return

    def sample_from_prior(self):
        # A -> B, the class is the bin of B's attribute
        label_B = [get_attr_label(float(attr.squeeze()), self.attr_bins_with_inf) for attr in self.attr_B]
        embedding_B = torch.cat([self.one_hot_labels[L] for L in label_B], dim=0)
        return self.netG(self.real_A, embedding_B)

    def sample_from_label(self, label):
        return self.netG(self.real_A, self.one_hot_labels[label])

    def backward_D(self):
        one_hot = self.one_hot_labels
        # the "fake" batch comes from the history of label_B (--pool_size 0: fake_B itself, nothing launched)
        self._fake_B_from_pool = self.fake_B_pool[self.label_B].query(self.fake_B).detach()
        self.loss_D_fake = self.criterionGAN(self.netD(self._fake_B_from_pool, one_hot[self.label_B]), False)
        self.loss_D_real_right = self.criterionGAN(self.netD(self.real_B, one_hot[self.label_B]), True)
        self.loss_D_real_wrong = self.criterionGAN(self.netD(self.real_B, one_hot[self.label_B_not]), False)
        self.loss_D = (self.loss_D_fake + (self.loss_D_real_right + self.loss_D_real_wrong) * 0.5) * 0.5
        self.loss_D.backward()

    def _ac_loss(self, image_AC):
        """criterionAC(netAC(transform_AC(image_AC)), label_B): linear head and cross entropy as one node"""
        AC = getattr(self.netAC, 'module', self.netAC)
        return AC.classify(self.transform_AC(image_AC), self._class_labels(self.label_B, image_AC.size(0)))[0]

    def backward_AC(self):
        self.loss_AC_real = self._ac_loss(self.real_B_AC)
        self.loss_AC_fake = self._ac_loss(self.fake_B_AC.detach()) if self.opt.train_aux_on_fake else 0.0
        self.loss_AC = (self.loss_AC_fake + self.loss_AC_real) * 0.5
        self.loss_AC.backward()

    def backward_G(self):
        o = self.opt
        self.loss_G_GAN = self.criterionGAN(self.netD(self._fake_B_D, self.one_hot_labels[self.label_B]), True)
        if o.lambda_A_GAN > 0.0:
            self.loss_G_GAN_cycle = self.criterionGAN(self.netD(self._rec_A_D, self.one_hot_labels[self.label_A]), True) * o.lambda_A_GAN
        else:
            self.loss_G_GAN_cycle = 0.0
        self.loss_G_L1 = self.criterionL1(self._fake_B_L1, self.real_A) * o.lambda_L1 if o.lambda_L1 > 0.0 else 0.0
        if o.lambda_IP > 0.0:
            with torch.no_grad():
                feature_A = self.netIP(self.transform_IP(self.real_A_IP))
            self.loss_G_IP = self.criterionIP(self.netIP(self.transform_IP(self.fake_B_IP)), feature_A) * o.lambda_IP
        else:
            self.loss_G_IP = 0.0
        self.loss_G_AC = self._ac_loss(self.fake_B_AC) * o.lambda_AC if o.lambda_AC > 0.0 else 0.0
        self.loss_G_cycle = self.criterionCycle(self._rec_A_cycle, self.real_A) * o.lambda_A if o.lambda_A > 0.0 else 0.0
        self.loss_G = self.loss_G_GAN + self.loss_G_IP + self.loss_G_L1 + self.loss_G_AC + self.loss_G_cycle + self.loss_G_GAN_cycle
        self.loss_G.backward()

    def optimize_parameters(self):
        self.forward()
        # update D
        self.set_requires_grad(self.netD, True)
        self.optimizer_D.zero_grad()
        self.backward_D()
        self.optimizer_D.step()
        # update AC
        self.set_requires_grad(self.netAC, True)
        self.optimizer_AC.zero_grad()
        self.backward_AC()
        self.optimizer_AC.step()
        # update G
        self.set_requires_grad(self.netD, False)
        self.set_requires_grad(self.netAC, False)
        self.optimizer_G.zero_grad()
        self.backward_G()
        self.optimizer_G.step()

    def get_current_visuals(self):
        self.set_requires_grad(self.netG, False)
        ret = OrderedDict()
        for name in self.visual_names:
            if isinstance(name, str):
                ret[name] = getattr(self, name)
        if self.opt.display_visuals:
            for L in range(self.opt.num_classes):
                ret['attr_' + str(L)] = self.netG(self.real_A[0:1, ...], self.one_hot_labels[L])
        self.set_requires_grad(self.netG, True)
        return ret
