"""WSGANDiscModel -- the reference's class-label CGAN baseline (models/wsgan_disc_model.py:14-311) on the HIP path: G(image, one-hot
class) against a conditional PatchGAN D(image, one-hot class), an AlexNet identity term and an auxiliary classifier AC (define_AC: the
network classification.py trains; `--pretrained_model_path_AC` loads its state dict, whole and strict).

Same plugin surface as the reference: flags and defaults, the 11 loss names, visual / model names, assertions, and the step order
forward -> D -> AC -> G (models/wsgan_shared.py: WSGANPairModel, with the differences from the reference that wsgan_cont shares).
One (label_A, label_B, label_B_not) triple is drawn per step from Python's global `random`, or read from `--train_label_pairs`.
AC's BatchNorm stays in train mode in all of its passes (real_B_AC, the detached fake under --train_aux_on_fake, fake_B_AC in the G
update, where its parameters are frozen and only d loss / d input is formed), D's in all five of its passes.  Disabled loss terms are
the Python float 0.0.

This is the one wsgan model whose reference accepts `--pool_size N > 0`: one ImagePool per class keeps a history of generated images,
and the batch D sees as "fake" comes from the pool of label_B.  The pool lives on the device and a query is one kernel launch
(util/image_pool.py, csrc/image_pool.hip); with the default `--pool_size 0` nothing is launched.

The reference's default generator name `unet_128` raises NotImplementedError from define_G -- pass `--which_model_netG unet` (the same
U-Net: like the reference, this model does not hand `--n_layers_G` on, so `unet` means 7 downsamplings), `unet_256` or
`resnet_<n>blocks`.

Stated differences from the reference, this model's own:
  * label_B_not is drawn with random.sample(sorted(...), 1): the reference samples from a set, which Python >= 3.11 refuses; for the
    ints 0 .. K-1 a set iterates in ascending order, so under one seed this is the reference's own draw on Python <= 3.10;
  * the head of AC and its CrossEntropyLoss are one node (ResNet.classify, csrc/linear_head.hip);
  * a torch.distributed run of more than one rank is refused: one label triple per GLOBAL batch needs a draw shared by all ranks.
"""
import random

import numpy as np
import torch

from . import networks
from .wsgan_shared import WSGANPairModel
from ..util.image_pool import ImagePool
from ..util.util import upsample2d, get_attr_label

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


class WSGANDiscModel(WSGANPairModel):
    COMMON_FLAGS, TRAIN_FLAGS, DEFAULT_OVERRIDES = _COMMON_FLAGS, _TRAIN_FLAGS, _DEFAULT_OVERRIDES
    ONE_RANK_REFUSAL = ('pcgan_amd: wsgan_disc draws one label triple per global batch from the process-local generator; '
                        'a run of %d ranks would need a shared draw and is not supported')
    AUX, AUX_LOSS, G_AUX_TERM = 'AC', 'AC', 'G_AC'
    G_SUM = ('G_GAN', 'G_IP', 'G_L1', 'G_AC', 'G_cycle', 'G_GAN_cycle')     # reference :271

    # ------------------------------------------------------------------ construction (reference :61-151)
    def initialize(self, opt):
        WSGANPairModel.initialize(self, opt)
        assert opt.embedding_nc == opt.num_classes
        self.attr_bins_with_inf = opt.attr_bins + [float('inf')]
        self.loss_names = ['G_GAN', 'G_GAN_cycle', 'G_IP', 'G_L1', 'G_AC', 'G_cycle',
                           'D_real_right', 'D_real_wrong', 'D_fake', 'AC_real', 'AC_fake']
        self.visual_names = ['real_A', 'fake_B', 'real_B', 'rec_A'] if self.isTrain else ['real_A']
        self.model_names = ['G', 'D', 'AC'] if self.isTrain else ['G']

        self.define_pair_nets()
        if self.isTrain:
            self.netAC = networks.define_AC(opt.which_model_netAC, opt.input_nc, opt.init_type, opt.num_classes,
                                            pooling=opt.pooling_AC, dropout=opt.dropout_AC, gpu_ids=self.gpu_ids)
            self.load_aux(opt.pretrained_model_path_AC)
            self.fake_B_pool = [ImagePool(opt.pool_size) for _ in range(opt.num_classes)]
            self.define_criteria()
            self.define_optimizers(('G', 'D', 'AC'), opt.lr_AC)
            if opt.train_label_pairs:
                with open(opt.train_label_pairs, 'r') as f:
                    self.train_label_pairs = [line.rstrip('\n') for line in f.readlines()]
            else:
                self.train_label_pairs = None
        self.pre_generate_embeddings()
        self._label_cache = {}
        if self.isTrain:
            self.define_transforms()

    def pre_generate_embeddings(self):
        K = self.opt.num_classes
        eye = np.eye(K, dtype=np.float32)
        self.one_hot_labels = [torch.from_numpy(eye[L].copy()).view(1, K, 1, 1).to(self.device) for L in range(K)]

    def embeddings_to_show(self):
        return self.one_hot_labels

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
        self.end_set_input(input)

    def conditioning(self):
        return self.one_hot_labels[self.label_A], self.one_hot_labels[self.label_B]

    def sample_from_prior(self):
        # A -> B, the class is the bin of B's attribute
        label_B = [get_attr_label(float(attr.squeeze()), self.attr_bins_with_inf) for attr in self.attr_B]
        embedding_B = torch.cat([self.one_hot_labels[L] for L in label_B], dim=0)
        return self.netG(self.real_A, embedding_B)

    def sample_from_label(self, label):
        return self.netG(self.real_A, self.one_hot_labels[label])

    def backward_D(self):
        # the "fake" batch comes from the history of label_B (--pool_size 0: fake_B itself, nothing launched)
        self._fake_B_from_pool = self.fake_B_pool[self.label_B].query(self.fake_B).detach()
        self.loss_D_fake = self.criterionGAN(self.netD(self._fake_B_from_pool, self.embedding_B), False)
        self.loss_D_real_right = self.criterionGAN(self.netD(self.real_B, self.embedding_B), True)
        self.loss_D_real_wrong = self.criterionGAN(self.netD(self.real_B, self.one_hot_labels[self.label_B_not]), False)
        self.loss_D = (self.loss_D_fake + (self.loss_D_real_right + self.loss_D_real_wrong) * 0.5) * 0.5
        self.loss_D.backward()

    def _ac_loss(self, image_AC):
        """criterionAC(netAC(transform_AC(image_AC)), label_B): linear head and cross entropy as one node"""
        AC = getattr(self.netAC, 'module', self.netAC)
        return AC.classify(self.transform_AC(image_AC), self._class_labels(self.label_B, image_AC.size(0)))[0]

    aux_loss = _ac_loss
