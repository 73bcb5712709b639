"""CPU twins of the multi-scale PatchGAN (test infrastructure): D_NLayersMulti of the reference (models/networks.py:1883-1949) restated on
stock torch modules and F.avg_pool2d, and the wsgan_cycle step that drives it.  The stacks use oracle.networks_ref's replayable
TapedLeakyReLU and norm factory, the Sequential indices and the registration names (`model.<i>` for one scale, `model0.<i>`, `model1.<i>`,
... for several) of the reference, so one state_dict fits the reference, this twin and the HIP module, in float32 or float64.  Every
convolution has a bias, whatever the norm; the widths shrink cumulatively (ndf = int(round(ndf / 2 ** (i + 1))) on the running ndf)."""
import torch.nn as nn
import torch.nn.functional as F

from oracle import networks_ref as N
from oracle import step_ref as S


def widths(ndf, num_D):
    out = [ndf]
    for i in range(num_D - 1):
        ndf = int(round(ndf / (2 ** (i + 1))))
        out.append(ndf)
    return out


def stack(input_nc, ndf, n_layers, norm, use_sigmoid):
    nl = N.norm_layer_of(norm)
    s = [nn.Conv2d(input_nc, ndf, 4, stride=2, padding=1), N.TapedLeakyReLU(0.2, True)]
    mult = 1
    for n in range(1, n_layers):
        prev, mult = mult, min(2 ** n, 8)
        s += [nn.Conv2d(ndf * prev, ndf * mult, 4, stride=2, padding=1), nl(ndf * mult), N.TapedLeakyReLU(0.2, True)]
    prev, mult = mult, min(2 ** n_layers, 8)
    s += [nn.Conv2d(ndf * prev, ndf * mult, 4, stride=1, padding=1), nl(ndf * mult), N.TapedLeakyReLU(0.2, True),
          nn.Conv2d(ndf * mult, 1, 4, stride=1, padding=1)]
    if use_sigmoid:
        s += [nn.Sigmoid()]
    return nn.Sequential(*s)


def down(x):
    return F.avg_pool2d(x, 3, stride=2, padding=1, count_include_pad=False)


class MultiScaleDiscriminatorRef(nn.Module):
    def __init__(self, input_nc, ndf=64, n_layers=3, norm='batch', use_sigmoid=True, num_D=1):
        super().__init__()
        self.num_D = num_D
        if num_D == 1:
            self.model = stack(input_nc, ndf, n_layers, norm, use_sigmoid)
        else:
            for i, w in enumerate(widths(ndf, num_D)):
                self.add_module('model%d' % i, stack(input_nc, w, n_layers, norm, use_sigmoid))

    def forward(self, x):
        if self.num_D == 1:
            return self.model(x)
        out = []
        for i in range(self.num_D):
            out.append(getattr(self, 'model%d' % i)(x))
            if i != self.num_D - 1:
                x = down(x)
        return out


def gan_loss_sum(preds, target):
    """GANLoss over a list of patch maps (reference models/networks.py:386-420): the sum of the per-scale losses"""
    loss = 0.0
    for p in (preds if isinstance(preds, list) else [preds]):
        loss = loss + S.gan_loss(p, target)
    return loss


class WSGANCycleMultiDStepRef(S.WSGANCycleStepRef):
    """oracle.step_ref.WSGANCycleStepRef with a discriminator that returns a list: D_fake, D_real and G_GAN are sums over the scales"""

    def backward_D(self):
        self.loss_D_fake = gan_loss_sum(self.netD(self.fake_x.detach()), False)
        self.loss_D_real = gan_loss_sum(self.netD(self.real_x), True)
        self.loss_D = (self.loss_D_fake + self.loss_D_real) * 0.5
        self.loss_D.backward()

    def backward_GE(self):
        o = self.opt
        self.loss_G_GAN = gan_loss_sum(self.netD(self.fake_x), True)
        if o.lambda_IP > 0.0:
            feature_A = self.netIP(self.real_x_IP).detach()
            crit = F.mse_loss if o.identity_preserving_criterion.lower() == 'mse' else F.l1_loss
            self.loss_G_IP = crit(self.netIP(self.fake_x_IP), feature_A) * o.lambda_IP
        else:
            self.loss_G_IP = 0.0
        self.loss_cycle_x = F.l1_loss(self.rec_x, self.real_x) * o.lambda_x if o.lambda_x > 0.0 else 0.0
        self.loss_cycle_y = F.mse_loss(self.rec_y, self.real_y) * o.lambda_y if o.lambda_y > 0.0 else 0.0
        self.loss_G = self.loss_G_GAN + self.loss_G_IP + self.loss_cycle_x + self.loss_cycle_y
        self.loss_G.backward()


def build_cycle_multid_oracle(dtype=None):
    """The oracle-side twin of scripts/make_multid_golden.py: cycle_step (tests/test_cycle_oracle_golden.py: build_cycle_oracle with the
    two-scale discriminator: --n_layers_D 2 --ndf 8 --num_Ds 2)."""
    import torch
    from oracle import weights as W
    dtype = dtype or torch.float32
    G = N.ResnetGeneratorRef(3, 3, 1, 8, 'instance', 9)
    G.load_state_dict(W.damp_generator_head(W.fill_state_dict(G.state_dict(), 19)))
    D = MultiScaleDiscriminatorRef(3, 8, 2, 'batch', True, 2)
    D.load_state_dict(W.fill_state_dict(D.state_dict(), 20))
    E = N.SiameseFeatureRef(N.ResNetFeatureRef('resnet18'), 'max', (64, 1), 1, 0.7, False)
    esd = E.state_dict()
    base = W.fill_state_dict({k[len('base.model.'):]: v for k, v in esd.items() if k.startswith('base.model.')}, 31)
    head = W.fill_state_dict(esd, 33)
    for k in esd:
        esd[k] = base[k[len('base.model.'):]] if k.startswith('base.model.') else head[k]
    E.load_state_dict(esd)
    IP = N.AlexNetFeatureRef(3, 'None')
    IP.load_state_dict(W.fill_state_dict(IP.state_dict(), 40))
    for net in (G, D, E, IP):
        net.to(dtype)
    return WSGANCycleMultiDStepRef(G, D, E, IP, fineSize_E=64, fineSize_IP=64, attr_mean=[35.0], attr_std=[20.0])
