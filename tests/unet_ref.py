"""CPU twin of the U-Net generator (test infrastructure): UnetGenerator / UnetSkipConnectionBlock of the reference
(models/networks.py:659-733), restated from its formulas on stock torch modules with the reference's Sequential indices, so one
state_dict (model.model.0.weight, model.model.1.model.1.weight, ...) fits the reference, this twin and the HIP module, in float32 or
float64.

The reference's blocks work IN PLACE: the first module of every block but the outermost is LeakyReLU(0.2, inplace=True), so the `x` of
`torch.cat([x, self.model(x)], 1)` has already been overwritten and the skip carries t = LeakyReLU(x).  The twin says that out of
place -- t = lrelu(x), then cat(t, body(t)) -- which is what tests/golden/unet.npz (recorded from the reference) pins.  The parent's
ReLU then acts on the whole concatenation, a fresh tensor.

Activations are oracle.networks_ref.TapedReLU / TapedLeakyReLU: with DecisionTape.replay set they apply another run's sign decisions,
in this order per block: LeakyReLU of the block input; [innermost: ReLU after the down-convolution]; the parent's ReLU over the
concatenation that the block returns."""
import torch
import torch.nn as nn

from oracle import networks_ref as N


class UnetBlockRef(nn.Module):
    def __init__(self, outer_nc, inner_nc, norm, input_nc=None, sub=None, outermost=False):
        super().__init__()
        nl = N.norm_layer_of(norm)
        bias = norm == 'instance'
        self.outermost, innermost = outermost, sub is None
        down = nn.Conv2d(outer_nc if input_nc is None else input_nc, inner_nc, 4, stride=2, padding=1, bias=bias)
        up = nn.ConvTranspose2d(inner_nc if innermost else 2 * inner_nc, outer_nc, 4, stride=2, padding=1, bias=bias or outermost)
        if outermost:
            m = [down, sub, N.TapedReLU(), up, nn.Tanh()]
        elif innermost:
            m = [N.TapedLeakyReLU(0.2), down, N.TapedReLU(), up, nl(outer_nc)]
        else:
            m = [N.TapedLeakyReLU(0.2), down, nl(inner_nc), sub, N.TapedReLU(), up, nl(outer_nc)]
        self.model = nn.Sequential(*m)

    def forward(self, x):
        if self.outermost:
            return self.model(x)
        t = self.model[0](x)
        return torch.cat([t, self.model[1:](t)], 1)


class UnetGeneratorRef(nn.Module):
    def __init__(self, input_nc, output_nc, nz=1, num_downs=7, ngf=64, norm='instance'):
        super().__init__()
        b = UnetBlockRef(ngf * 8, ngf * 8, norm)
        for _ in range(num_downs - 5):
            b = UnetBlockRef(ngf * 8, ngf * 8, norm, sub=b)
        for mult in (4, 2, 1):
            b = UnetBlockRef(ngf * mult, ngf * mult * 2, norm, sub=b)
        self.model = UnetBlockRef(output_nc, ngf, norm, input_nc=input_nc + nz, sub=b, outermost=True)

    def forward(self, x, z=None):
        return self.model(N._cat_z(x, z))


# parameters / state_dict entries at (input_nc, output_nc, nz) = (3, 3, 1), measured on the reference (tests/golden/unet.npz holds the
# same figures): (which_model_netG, n_layers_G, ngf, norm) -> (parameters, entries)
REFERENCE_COUNTS = {
    ('unet', 5, 8, 'instance'): (261683, 41), ('unet', 5, 8, 'batch'): (261843, 46),
    ('unet', 6, 8, 'instance'): (458419, 51), ('unet', 6, 8, 'batch'): (458707, 58),
    ('unet', 7, 64, 'instance'): (41826691, 61), ('unet', 7, 64, 'batch'): (41830019, 70),
    ('unet_256', 8, 64, 'instance'): (54410627, 71), ('unet_256', 8, 64, 'batch'): (54414979, 82),
}
