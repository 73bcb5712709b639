"""Test-side twin of the wsgan_bigan step (reference models/wsgan_bigan_model.py:152-249) in plain torch, any dtype: the resnet / U-Net
generator and conditional PatchGAN of oracle.networks_ref / unet_ref, the trained encoder and the AlexNet identity features of
oracle.networks_ref, the step of oracle.step_ref.WSGANCycleStepRef with the joint-pair discriminator passes in place of the
unconditional ones.  Every ReLU / LeakyReLU and max pooling is a taped one, so DecisionTape.replay works on it.  Pinned to the reference
itself by tests/golden/bigan_step*.npz (scripts/make_bigan_golden.py, tests/test_bigan_oracle_golden.py).

Also the ONE description of the fixture variants -- command lines, seeded batches, seeded weights -- which the fixture generator, the
CPU test and the GPU tests share."""
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F

import unet_ref as U
from oracle import networks_ref as N
from oracle import step_ref as S
from oracle import weights as W
from oracle.step_ref import gan_loss

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LOSS_NAMES = ['G_GAN', 'E_GAN', 'G_IP', 'cycle_x', 'cycle_y', 'D_real', 'D_fake']
SEED_G, SEED_D, SEED_E_BASE, SEED_E_HEAD, SEED_IP = 19, 20, 31, 33, 40
ATTR_MEAN, ATTR_STD = 35.0, 20.0          # attributes in [0, 60) become targets in [-1.75, 1.25)
# The encoder of the fixture stands for one that has been TRAINED for a while: it answers near its targets.  Its last convolution is
# shrunk by E_HEAD_DAMP and its last bias set to the targets' mean, E_HEAD_BIAS (cont_ref.regressor_weights does the same).  With plain
# seeded weights the encoder answers far from every target, and the gradient of the one cycle_y term (through the max pooling over a
# bilinearly enlarged image) is nearly all of the generator's AND of the encoder's gradient: the float64 twin gave, for the share of
# cycle_y in G's gradient -- the median over the weight tensors of || g - g(lambda_y = 0) || / || g || -- in the default variant 1.000
# with the head as seeded (E_GAN then 0.024 of the encoder's gradient), 0.999 with the head times 0.1, 0.986 times 0.03, 0.889 times 0.01,
# 0.502 times 0.003: neither the discriminator's reading of fake_x nor the rating gradients this model adds would be visible in a step
# test.  The term's gradient is the factor times the spread of the targets, which does not shrink, hence the small factor.
# Conditions on the fixtures, measured on the float64 twin alone (scripts/make_bigan_golden.py --shares prints them), E_HEAD_DAMP = 0.001:
#   (a) lambda_y_0: the E_GAN term is at least half of || grad E ||: 1.000 (|| g - g(without E_GAN) || / || g || over the whole encoder;
#       the cycle_x share through G's rating input is 1e-7);
#   (b) resnet variants that keep lambda_y: cycle_y supplies at most half of G's gradient:
#           default 0.191, norm_D_instance 0.100, ip_l1_no_cycle_x 0.192, no_ip 0.193
#       (E_GAN is then 0.21 of the encoder's gradient, 0.07 under --norm_D instance).
E_HEAD_DAMP, E_HEAD_BIAS = 0.001, -0.25
GRAD_STRIDE = 997
UNET_IT1_STRIDE = 32      # the U-Net variant's second iteration keeps every 32nd pixel of its images
IMAGES = ('fake_x', 'rec_x', 'fake_y', 'rec_y', 'real_y')

# name -> (extra command line, overrides of the twin's options)
VARIANTS = OrderedDict([
    ('default', ([], {})),
    ('lambda_y_0', (['--lambda_y', '0'], dict(lambda_y=0.0))),
    ('unet', (['--which_model_netG', 'unet', '--fineSize', '128', '--loadSize', '128', '--batchSize', '2', '--fineSize_E', '128',
               '--fineSize_IP', '128'], dict(netG='unet', fineSize=128, batch=2, fineSize_E=128, fineSize_IP=128))),
    ('norm_D_instance', (['--norm_D', 'instance'], dict(norm_D='instance'))),
    ('ip_l1_no_cycle_x', (['--identity_preserving_criterion', 'l1', '--lambda_x', '0'],
                          dict(identity_preserving_criterion='l1', lambda_x=0.0))),
    ('no_ip', (['--lambda_IP', '0'], dict(lambda_IP=0.0))),
])
DEFAULTS = dict(netG='resnet_9blocks', fineSize=32, batch=4, fineSize_E=64, fineSize_IP=64, norm_D='batch', lambda_x=1.0, lambda_y=1.0,
                lambda_IP=1.0, lr=2e-4, beta1=0.5, identity_preserving_criterion='mse', attr_mean=[ATTR_MEAN], attr_std=[ATTR_STD])


def fixture_path(name):
    return os.path.join(GOLD, 'bigan_step.npz' if name == 'default' else 'bigan_step_%s.npz' % name)


def options(name, **extra):
    o = dict(DEFAULTS)
    o.update(VARIANTS[name][1])
    o.update(extra)
    return o


def argv(name, root, e_path, ip_path, gpu_ids):
    """the training command line of a variant (the reference's parser and this project's take the same one)"""
    base = ['train.py', '--dataroot', root, '--model', 'wsgan_bigan', '--name', 'g_bigan_' + name, '--checkpoints_dir', root,
            '--gpu_ids', gpu_ids, '--which_model_netG', 'resnet_9blocks', '--which_model_netD', 'n_layers', '--n_layers_D', '3',
            '--ngf', '8', '--ndf', '8', '--fineSize', '32', '--loadSize', '32', '--fineSize_E', '64', '--fineSize_IP', '64',
            '--batchSize', '4', '--pretrained_model_path_E', e_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1',
            '--attr_bins', '[10, 30, 50]', '--attr_mean', str(ATTR_MEAN), '--attr_std', str(ATTR_STD)]
    return base + VARIANTS[name][0]


def batch(name, it):
    """the seeded input dict of iteration `it` of a variant, as WSGANCycleDataset's loader yields it"""
    o = options(name)
    n, s = o['batch'], o['fineSize']
    return {'A': W.seeded_tensor((n, 3, s, s), 700 + it), 'B_attr': (W.seeded_tensor((n, 1, 1, 1), 800 + it) + 1.0) * 30.0,
            'A_paths': ['a'] * n, 'B_paths': ['b'] * n}


def generator_weights(sd, which):
    """seeded weights with the last convolution shrunk so that tanh stays in its linear range (oracle.weights.damp_generator_head)"""
    sd = dict(W.fill_state_dict(sd, SEED_G))
    last = 'model.26.weight' if which.startswith('resnet') else 'model.model.3.weight'
    sd[last] = sd[last] * 0.05
    return sd


def encoder_base_weights(sd):
    """the plain ResNet state dict --pretrained_model_path_E names (load_base)"""
    return W.fill_state_dict(sd, SEED_E_BASE)


def encoder_weights(sd, damp=E_HEAD_DAMP):
    """the encoder's whole seeded state dict: the trunk as encoder_base_weights fills it, the head seeded, its last convolution shrunk by
    E_HEAD_DAMP and its last bias set to E_HEAD_BIAS (see there)"""
    cpu = {k: v.detach().cpu() for k, v in sd.items()}
    base = encoder_base_weights({k[len('base.model.'):]: v for k, v in cpu.items() if k.startswith('base.model.')})
    head = W.fill_state_dict(cpu, SEED_E_HEAD)
    out = {k: (base[k[len('base.model.'):]] if k.startswith('base.model.') else head[k]) for k in cpu}
    last = [k for k in cpu if k.startswith('cnn.') and k.endswith('.weight') and cpu[k].dim() == 4][-1]
    out[last] = out[last] * damp
    bias = last[:-len('weight')] + 'bias'
    out[bias] = torch.full_like(out[bias], E_HEAD_BIAS) if damp != 1.0 else out[bias]
    return out


class WSGANBiGANStepRef(S.WSGANCycleStepRef):
    """the reference's optimize_parameters(): forward, D, then G and E together; D judges (image, rating) pairs.  transform_E /
    transform_IP are the identity (the reference never applies transform_E and AlexNet's is folded into the seeded weights' scale)."""

    LOSS_NAMES = LOSS_NAMES

    def __init__(self, netG, netD, netE, netIP, **opts):
        super().__init__(netG, netD, netE, netIP, **opts)
        self.opt.E_GAN = opts.get('E_GAN', True)        # False: the term is left out (measuring its share; never in a fixture)
        self.dtype = next(netG.parameters()).dtype

    def set_input(self, input):
        super().set_input(input['A'].to(self.dtype), input['B_attr'].to(self.dtype))

    def backward_D(self):
        """:189-199"""
        self.loss_D_fake = gan_loss(self.netD(self.fake_x.detach(), self.real_y), False)
        self.loss_D_real = gan_loss(self.netD(self.real_x, self.fake_y.detach()), True)
        self.loss_D = (self.loss_D_fake + self.loss_D_real) * 0.5
        self.loss_D.backward()

    def backward_GE(self):
        """:201-233"""
        o = self.opt
        self.loss_G_GAN = gan_loss(self.netD(self.fake_x, self.real_y), True)
        self.loss_E_GAN = gan_loss(self.netD(self.real_x, self.fake_y), False)
        if o.lambda_IP > 0.0:
            feature_A = self.netIP(self.real_x_IP).detach()
            crit = F.mse_loss if o.identity_preserving_criterion.lower() == 'mse' else F.l1_loss
            self.loss_G_IP = crit(self.netIP(self.fake_x_IP), feature_A) * o.lambda_IP
        else:
            self.loss_G_IP = 0.0
        self.loss_cycle_x = F.l1_loss(self.rec_x, self.real_x) * o.lambda_x if o.lambda_x > 0.0 else 0.0
        self.loss_cycle_y = F.mse_loss(self.rec_y, self.real_y) * o.lambda_y if o.lambda_y > 0.0 else 0.0
        e_gan = self.loss_E_GAN if o.E_GAN else 0.0
        self.loss_GE = self.loss_G_GAN + e_gan + self.loss_G_IP + self.loss_cycle_x + self.loss_cycle_y
        self.loss_GE.backward()


def build_twin(name, dtype=torch.float32, damp=E_HEAD_DAMP, **extra):
    """the twin of a fixture variant with the fixture's seeded weights (`extra`: option overrides for measuring a term's share)"""
    o = options(name, **extra)
    if o['netG'] == 'unet':
        G = U.UnetGeneratorRef(3, 3, 1, 7, 8, 'instance')
    else:
        G = N.ResnetGeneratorRef(3, 3, 1, 8, 'instance', 9)
    G.load_state_dict(generator_weights(G.state_dict(), o['netG']))
    D = N.NLayerDiscriminatorRef(3, 1, 8, 3, o['norm_D'], True)
    D.load_state_dict(W.fill_state_dict(D.state_dict(), SEED_D))
    E = N.SiameseFeatureRef(N.ResNetFeatureRef('resnet18'), 'max', (64, 1), 1, 0.7, False)
    E.load_state_dict(encoder_weights(E.state_dict(), damp))
    IP = N.AlexNetFeatureRef(3, 'None')
    IP.load_state_dict(W.fill_state_dict(IP.state_dict(), SEED_IP))
    for net in (G, D, E, IP):
        net.to(dtype)
    keep = ('fineSize_E', 'fineSize_IP', 'attr_mean', 'attr_std', 'lambda_x', 'lambda_y', 'lambda_IP', 'lr', 'beta1',
            'identity_preserving_criterion', 'E_GAN')
    return WSGANBiGANStepRef(G, D, E, IP, **{k: v for k, v in o.items() if k in keep})


def _gnorm(gd):
    return float(torch.sqrt(sum(g.double().pow(2).sum() for g in gd.values() if g is not None)))


def shares(name, damp=E_HEAD_DAMP):
    """float64 twin, iteration 0: (median over G's weight tensors of || g - g(lambda_y = 0) || / || g ||, the same over the whole of E for
    the E_GAN term) -- the two conditions on the fixtures"""
    def grads(**extra):
        t = build_twin(name, torch.float64, damp, **extra)
        t.set_input(batch(name, 0))
        t.optimize_parameters()
        return t.grads
    full = grads()
    no_y, no_e = grads(lambda_y=0.0), grads(E_GAN=False)
    per = [float((g - no_y['G'][k]).norm() / g.norm()) for k, g in full['G'].items() if g is not None and float(g.norm()) > 1e-9]
    diff = {k: g - no_e['E'][k] for k, g in full['E'].items() if g is not None}
    return float(torch.tensor(per).median()), _gnorm(diff) / _gnorm(full['E'])
