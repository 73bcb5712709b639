"""CPU twin of the projection discriminator (test infrastructure): NLayerProjectionDiscriminator of the reference with proj=True
(models/networks.py:787-838), restated from its formula on stock torch modules.  `phi` mirrors oracle.networks_ref.NLayerDiscriminatorRef
without the last convolution -- same Sequential indices, the replayable TapedLeakyReLU -- so one state_dict (phi.*, psi.*, l_y.*) fits the
reference, this twin and the HIP module, in float32 or float64."""
import torch
import torch.nn as nn

from oracle import networks_ref as N


class ProjectionDiscriminatorRef(nn.Module):
    def __init__(self, input_nc, nz, ndf=64, n_layers=3, norm='batch', use_sigmoid=True):
        super().__init__()
        nl = N.norm_layer_of(norm)
        bias = norm == 'instance'
        s = [nn.Conv2d(input_nc, ndf, 4, stride=2, padding=1), N.TapedLeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            s += [nn.Conv2d(ndf * prev, ndf * mult, 4, stride=2, padding=1, bias=bias), nl(ndf * mult), N.TapedLeakyReLU(0.2, True)]
        prev, mult = mult, min(2 ** n_layers, 8)
        s += [nn.Conv2d(ndf * prev, ndf * mult, 4, stride=1, padding=1, bias=bias), nl(ndf * mult), N.TapedLeakyReLU(0.2, True)]
        self.phi = nn.Sequential(*s)
        self.psi = nn.Conv2d(ndf * mult, 1, 1, padding=1)
        self.l_y = nn.Conv2d(nz, ndf * mult, 1)
        self.nz, self.sigm = nz, use_sigmoid

    def forward(self, x, y):
        return head(self.phi(x), y.reshape(-1, self.nz), self.psi.weight, self.psi.bias, self.l_y.weight, self.l_y.bias, self.sigm)


def head(p, y, psi_w, psi_b, ly_w, ly_b, sigmoid):
    """the head alone, written out: p (B, C, H, W), y (By, nz) with By in {1, B}; parameters in nn.Conv2d's shapes"""
    B, C = p.shape[0], p.shape[1]
    h = p.sum(dim=(2, 3))                                                    # (B, C): plane SUMS
    wy = y @ ly_w.reshape(C, -1).t() + ly_b                                  # (By, C), broadcasts over the batch when By = 1
    s = (h * wy).sum(dim=1)                                                  # (B,)
    out = (s + psi_b).reshape(B, 1, 1, 1).expand(B, 1, 3, 3).clone()         # psi's padding: eight cells see zeros, i.e. the bias alone
    out[:, 0, 1, 1] = out[:, 0, 1, 1] + h @ psi_w.reshape(C)
    return torch.sigmoid(out) if sigmoid else out
