"""Test-side twin of the wsgan_cont step (reference models/wsgan_cont_model.py:163-314) in plain torch, any dtype: resnet / U-Net
generator and conditional PatchGAN of oracle.networks_ref / unet_ref, the regressor of regression_ref, AlexNet identity features.
Every ReLU / LeakyReLU and max pooling is a taped one, so DecisionTape.replay works on it.  Pinned to the reference itself by
tests/golden/cont_step*.npz (scripts/make_cont_golden.py, tests/test_cont_oracle_golden.py).

Also the ONE description of the fixture variants -- command lines, seeded batches, seeded weights -- which the fixture generator, the
CPU test and the GPU test share."""
import os
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import regression_ref as R
import unet_ref as U
from oracle import networks_ref as N
from oracle import weights as W
from oracle.step_ref import gan_loss, upsample2d

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LOSS_NAMES = ['G_GAN', 'G_GAN_cycle', 'G_IP', 'G_L1', 'G_cycle', 'z_rec', 'D_real_right', 'D_real_wrong', 'D_fake', 'AR_real', 'AR_fake']
NP_SEED = 4242          # numpy's global generator is seeded with NP_SEED + it before set_input (--no_mixed_label_D draws the label)
SEED_G, SEED_D, SEED_E, SEED_IP = 19, 20, 45, 40
ATTR_MEAN, ATTR_STD = 0.0, 100.0          # the model's own defaults: attributes in [0, 60) become targets in [0, 0.6)
# The regressor of the fixture stands for a TRAINED one, which is what --pretrained_model_path_E names in use: it answers near its
# targets.  Its last convolution is shrunk by E_HEAD_DAMP and its last bias set to the targets' mean, 0.3.  With plain seeded weights
# (and targets (attr - 35) / 20) it answered about 1.3 from every target, and the gradient of that one loss term was ALL of the
# generator's gradient: in the float64 twin, || g - g(lambda_AR = 0) || / || g || was 0.95 .. 1.00 for every weight tensor, so the other
# readers of fake_B -- the discriminator, the second generator pass, the L1 and identity terms -- were invisible in it, and what the
# gradient checks saw was the one badly conditioned path (max pooling over a bilinearly enlarged image, BatchNorm over 16 values per
# channel in layer4).  E_HEAD_DAMP is set on the twin alone, by that share: at 0.03 no resnet variant has more than a third of the
# generator's gradient from the regressor term (median over the weight tensors: default 0.11, detach_no_A_GAN 0.30, aux_on_fake_L1 0.03;
# unet, whose regressor runs at 128 x 128, 0.64), so every reader weighs in; the twin in fp32 stays within 1.4 % of the twin in fp64.
E_HEAD_DAMP, E_HEAD_BIAS = 0.03, 0.3
GRAD_STRIDE = 997

# name -> (extra command line, overrides of the twin's options)
VARIANTS = OrderedDict([
    ('default', ([], {})),
    ('aux_on_fake_L1', (['--train_aux_on_fake', '--lambda_L1', '0.5'], dict(train_aux_on_fake=True, lambda_L1=0.5))),
    ('detach_no_A_GAN', (['--detach_fake_B', '--lambda_A_GAN', '0'], dict(detach_fake_B=True, lambda_A_GAN=0.0))),
    ('no_mixed_label_D', (['--no_mixed_label_D'], dict(no_mixed_label_D=True))),
    ('unet', (['--which_model_netG', 'unet', '--fineSize', '128', '--loadSize', '128', '--batchSize', '2', '--fineSize_E', '128',
               '--fineSize_IP', '128'], dict(netG='unet', fineSize=128, batch=2, fineSize_E=128, fineSize_IP=128))),
    ('norm_D_instance', (['--norm_D', 'instance'], dict(norm_D='instance'))),
])
DEFAULTS = dict(netG='resnet_9blocks', fineSize=32, batch=4, fineSize_E=64, fineSize_IP=64, norm_D='batch', lambda_L1=0.0, lambda_IP=1.0,
                lambda_AR=1.0, lambda_A=0.5, lambda_A_GAN=0.5, relabel_D=[0, 1, 0], weight_label_D=[0.5, 0.0, 0.5], no_mixed_label_D=False,
                train_aux_on_fake=False, detach_fake_B=False, lr=2e-4, lr_E=2e-4, beta1=0.5, identity_preserving_criterion='mse',
                attr_mean=[ATTR_MEAN], attr_std=[ATTR_STD])


def fixture_path(name):
    return os.path.join(GOLD, 'cont_step.npz' if name == 'default' else 'cont_step_%s.npz' % name)


def options(name):
    o = dict(DEFAULTS)
    o.update(VARIANTS[name][1])
    return SimpleNamespace(**o)


def argv(name, root, e_path, ip_path, gpu_ids):
    """the training command line of a variant (the reference's parser and this project's take the same one)"""
    base = ['train.py', '--dataroot', root, '--model', 'wsgan_cont', '--name', 'g_cont_' + name, '--checkpoints_dir', root,
            '--gpu_ids', gpu_ids, '--which_model_netG', 'resnet_9blocks', '--which_model_netD', 'n_layers', '--n_layers_D', '3',
            '--ngf', '8', '--ndf', '8', '--fineSize', '32', '--loadSize', '32', '--fineSize_E', '64', '--fineSize_IP', '64',
            '--batchSize', '4', '--pretrained_model_path_E', e_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1',
            '--attr_bins', '[10, 30, 50]', '--attr_mean', str(ATTR_MEAN), '--attr_std', str(ATTR_STD)]
    return base + VARIANTS[name][0]


def _set(it, seed, o, prefix=''):
    n, s = o.batch, o.fineSize
    return {prefix + 'A': W.seeded_tensor((n, 3, s, s), 900 + seed + it), prefix + 'B': W.seeded_tensor((n, 3, s, s), 950 + seed + it),
            prefix + 'A_attr': (W.seeded_tensor((n, 1, 1, 1), 1000 + seed + it) + 1.0) * 30.0,       # attributes in [0, 60)
            prefix + 'B_attr': (W.seeded_tensor((n, 1, 1, 1), 1050 + seed + it) + 1.0) * 30.0,
            prefix + 'A_paths': ['a'] * n, prefix + 'B_paths': ['b'] * n}


def batch(name, it):
    """the seeded input dict of iteration `it` of a variant, as WSGANContDataset's loader yields it"""
    o = options(name)
    if o.no_mixed_label_D:      # one pair set per label that has lines (0 and 2 here)
        ret = _set(it, 0, o, '0_')
        ret.update(_set(it, 20, o, '2_'))
        return ret
    ret = _set(it, 0, o)
    ret['label'] = torch.tensor(([0, 1, 2, 1] if it == 0 else [2, 0, 1, 0])[:o.batch], dtype=torch.int64)
    return ret


def generator_weights(sd, which):
    """seeded weights with the last convolution shrunk so that tanh stays in its linear range (oracle.weights.damp_generator_head)"""
    sd = dict(W.fill_state_dict(sd, SEED_G))
    last = 'model.26.weight' if which.startswith('resnet') else 'model.model.3.weight'
    sd[last] = sd[last] * 0.05
    return sd


def regressor_weights(sd):
    """the regressor's seeded state dict -- the file --pretrained_model_path_E names -- with its last convolution shrunk by E_HEAD_DAMP
    (see there)"""
    sd = dict(W.fill_state_dict(sd, SEED_E))
    sd['cnn.3.weight'] = sd['cnn.3.weight'] * E_HEAD_DAMP
    sd['cnn.3.bias'] = torch.full_like(sd['cnn.3.bias'], E_HEAD_BIAS)
    return sd


class WSGANContStepRef:
    """the reference's optimize_parameters(): forward, D, E (backward_AR), G.  transform_E / transform_IP are the identity."""

    LOSS_NAMES = LOSS_NAMES

    def __init__(self, netG, netD, netE, netIP, opt):
        self.opt = opt
        self.netG, self.netD, self.netE, self.netIP = netG, netD, netE, netIP
        betas = (opt.beta1, 0.999)
        self.optimizer_G = torch.optim.Adam(netG.parameters(), lr=opt.lr, betas=betas)
        self.optimizer_D = torch.optim.Adam(netD.parameters(), lr=opt.lr, betas=betas)
        self.optimizer_E = torch.optim.Adam(netE.parameters(), lr=opt.lr_E, betas=betas)
        self.weight_label_D = [w / sum(opt.weight_label_D) for w in opt.weight_label_D]
        self.dtype = next(netG.parameters()).dtype
        self.grads = {}

    def attr_normalize(self, x):
        return (x - self.opt.attr_mean[0]) / self.opt.attr_std[0]

    def set_input(self, input):
        o = self.opt
        if not o.no_mixed_label_D:
            prefix, self.label_AB = '', [int(v) for v in input['label']]
        else:
            self.label_AB = [int(np.random.choice(range(len(o.relabel_D)), p=self.weight_label_D))]
            prefix = str(self.label_AB[0]) + '_'
        self.real_A, self.real_B = input[prefix + 'A'].to(self.dtype), input[prefix + 'B'].to(self.dtype)
        self.attr_A, self.attr_B = input[prefix + 'A_attr'].to(self.dtype), input[prefix + 'B_attr'].to(self.dtype)
        self.real_A_IP = upsample2d(self.real_A, o.fineSize_IP)
        self.real_B_E = upsample2d(self.real_B, o.fineSize_E)

    def forward(self):
        o = self.opt
        self.embedding_A = self.attr_normalize(self.attr_A)
        self.embedding_B = self.attr_normalize(self.attr_B)
        self.fake_B = self.netG(self.real_A, self.embedding_B)
        self.fake_B_IP = upsample2d(self.fake_B, o.fineSize_IP)
        self.fake_B_E = upsample2d(self.fake_B, o.fineSize_E)
        self.rec_A = self.netG(self.fake_B.detach() if o.detach_fake_B else self.fake_B, self.embedding_A)

    def backward_D(self):
        o = self.opt
        self.loss_D_fake = gan_loss(self.netD(self.fake_B.detach(), self.embedding_B), False)
        self.loss_D_real_right = gan_loss(self.netD(self.real_B, self.embedding_B), True)
        self.loss_D_real_wrong = gan_loss(self.netD(self.real_B, self.embedding_A), [o.relabel_D[L] for L in self.label_AB])
        self.loss_D = (self.loss_D_fake + (self.loss_D_real_right + self.loss_D_real_wrong) * 0.5) * 0.5
        self.loss_D.backward()

    def backward_AR(self):
        self.loss_AR_real = F.mse_loss(self.netE(self.real_B_E), self.embedding_B)
        if self.opt.train_aux_on_fake:
            self.loss_AR_fake = F.mse_loss(self.netE(self.fake_B_E.detach()), self.embedding_B)
        else:
            self.loss_AR_fake = 0.0
        self.loss_AR = (self.loss_AR_fake + self.loss_AR_real) * 0.5
        self.loss_AR.backward()

    def backward_G(self):
        o = self.opt
        self.loss_G_GAN = gan_loss(self.netD(self.fake_B, self.embedding_B), True)
        self.loss_G_GAN_cycle = gan_loss(self.netD(self.rec_A, self.embedding_A), True) * o.lambda_A_GAN if o.lambda_A_GAN > 0.0 else 0.0
        self.loss_G_L1 = F.l1_loss(self.fake_B, self.real_A) * o.lambda_L1 if o.lambda_L1 > 0.0 else 0.0
        if o.lambda_IP > 0.0:
            feature_A = self.netIP(self.real_A_IP).detach()
            crit = F.mse_loss if o.identity_preserving_criterion.lower() == 'mse' else F.l1_loss
            self.loss_G_IP = crit(self.netIP(self.fake_B_IP), feature_A) * o.lambda_IP
        else:
            self.loss_G_IP = 0.0
        self.loss_z_rec = F.mse_loss(self.netE(self.fake_B_E), self.embedding_B) * o.lambda_AR if o.lambda_AR > 0.0 else 0.0
        self.loss_G_cycle = F.l1_loss(self.rec_A, self.real_A) * o.lambda_A if o.lambda_A > 0.0 else 0.0
        self.loss_G = self.loss_G_GAN + self.loss_G_IP + self.loss_G_L1 + self.loss_G_cycle + self.loss_z_rec + self.loss_G_GAN_cycle
        self.loss_G.backward()

    @staticmethod
    def _requires_grad(net, flag):
        for p in net.parameters():
            p.requires_grad = flag

    def _grab(self, tag, net):
        self.grads[tag] = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in net.named_parameters()}

    def optimize_parameters(self):
        self.forward()
        self._requires_grad(self.netD, True)
        self.optimizer_D.zero_grad()
        self.backward_D()
        self._grab('D', self.netD)
        self.optimizer_D.step()
        self._requires_grad(self.netE, True)
        self.optimizer_E.zero_grad()
        self.backward_AR()
        self._grab('E', self.netE)
        self.optimizer_E.step()
        self._requires_grad(self.netD, False)
        self._requires_grad(self.netE, False)
        self.optimizer_G.zero_grad()
        self.backward_G()
        self._grab('G', self.netG)
        self.optimizer_G.step()

    def losses(self):
        return {n: float(getattr(self, 'loss_' + n)) for n in self.LOSS_NAMES}


def build_twin(name, dtype=torch.float32):
    """the twin of a fixture variant with the fixture's seeded weights"""
    o = options(name)
    if o.netG == 'unet':
        G = U.UnetGeneratorRef(3, 3, 1, 7, 8, 'instance')
    else:
        G = N.ResnetGeneratorRef(3, 3, 1, 8, 'instance', 9)
    G.load_state_dict(generator_weights(G.state_dict(), o.netG))
    D = N.NLayerDiscriminatorRef(3, 1, 8, 3, o.norm_D, True)
    D.load_state_dict(W.fill_state_dict(D.state_dict(), SEED_D))
    E = R.RegressionNetworkRef(R.ResNetTrunkRef('resnet18'), 'avg', (64, 1), 1, 0.7)
    E.load_state_dict(regressor_weights(E.state_dict()))
    IP = N.AlexNetFeatureRef(3, 'None')
    IP.load_state_dict(W.fill_state_dict(IP.state_dict(), SEED_IP))
    for net in (G, D, E, IP):
        net.to(dtype)
    return WSGANContStepRef(G, D, E, IP, o)
