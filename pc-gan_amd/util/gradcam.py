"""Grad-CAM on the HIP modules: capture a layer's output A in one single-image pass of the rating encoder, obtain g = d rating / dA and
hand both to the map kernel (hip.ops.gradcam_map, csrc/gradcam.hip).  Written for `siamese.py --mode attention`; it stands where the
reference's util/gradcam.py (PropBase / GradCAM2) stands, but is not a port of that hierarchy.

Where the reference's text cannot be followed literally:

  * GradCAM2.forward unpacks five values from a network that returns three or four and cannot run.  What it evidently means is done:
    one pass per image (`forward_once`), the rating being the first output (also for --noisy nets).
  * WHICH GRADIENT.  The reference back-propagates feature1 - feature2 through both branches and keeps whichever backward hook fired
    last.  Here each image's map uses the gradient of ITS OWN rating: for image B that is the literal reading with the opposite sign
    (d(r_A - r_B) / dA_B = - d r_B / dA_B); for image A it is the same.
  * The gradient is taken with torch.autograd.grad with respect to the captured tensor only: the pass is cut at the captured output (the
    tensor handed on is a detached leaf), parameters are frozen for its duration, so no parameter gradient is computed and no `.grad` is
    left behind.  No backward hooks, no model.zero_grad().
  * Like the reference (and `--mode embedding`) the net is NOT switched to eval(): with one image per pass BatchNorm normalises with that
    image's statistics and Dropout2d stays active.
  * The guided-ReLU variant (`update_relus`, commented out in the reference's call) would need a flag inside the fused norm-backward
    kernels; it is out of scope.

LAYER NAMES are those of named_modules(), equal to the reference's because the state-dict keys are.  The HIP modules fuse the activation
into the normalisation and call some containers' children directly, so a name resolves as follows:

  * a convolution, `base.model.maxpool` or a residual block `layerN.M` is hooked directly;
  * a Sequential stage (`base.model.layerN`, `cnn`, a block's `downsample`) resolves to its last child, whose output is the stage's output;
  * a BatchNorm, an `*.relu`, a drop layer, `base` and `base.model` raise ValueError: the fused normalisation's output is the reference's
    post-ReLU tensor and no pre-activation tensor exists on this path;
  * a name that does not exist raises ValueError quoting it ("invalid layers", as the reference does);
  * a pass in which the layer captured nothing raises as well.
"""
import torch
import torch.nn as tnn

from ..hip import nn as hnn
from ..hip import ops
from ..models.resnet import BasicBlock, Bottleneck

MAP_TYPES = ('raw', 'pw', 'pw_cw', 'cw_pos')
SUPPORTED_KINDS = ('a convolution, base.model.maxpool, a residual block (layerN.M) or a Sequential stage (base.model.layerN, cnn, '
                   'downsample), which resolves to its last child')


def resolve_layer(net, name):
    """(resolved name, module to hook) of a named_modules() name; ValueError for a missing name or a kind that cannot be captured"""
    mods = dict(net.named_modules())
    if not name or name not in mods:
        raise ValueError('invalid layers: {}'.format(name))
    m, resolved, stage = mods[name], name, False
    while isinstance(m, tnn.Sequential) and len(m) > 0:
        resolved, m, stage = '%s.%d' % (resolved, len(m) - 1), m[len(m) - 1], True
    if stage or isinstance(m, (hnn.Conv2d, hnn.MaxPool2d, BasicBlock, Bottleneck)):
        return resolved, m
    raise ValueError('layer {} ({}) cannot be captured on the HIP path; supported: {}'.format(name, type(m).__name__, SUPPORTED_KINDS))


class GradCAM(object):
    """gcam = GradCAM(net, 'base.model.layer1.0.conv1'); hmap = gcam.map(image, 'cw_pos') -- net a SiameseFeature or SiameseNetwork on
    the GPU, image one normalised (N, 3, H, W) batch (the script passes one image)."""

    def __init__(self, net, layer):
        self.net = net
        self.layer = layer
        self.resolved, self.module = resolve_layer(net, layer)

    def _rating(self, image):
        if hasattr(self.net, 'forward_once'):
            return self.net.forward_once(image)[0]
        out = self.net(image)
        return out[0] if isinstance(out, (tuple, list)) else out

    def _pass(self, image, hook):
        """one pass with the parameters frozen; returns the rating"""
        params = [p for p in self.net.parameters() if p.requires_grad]
        handle = self.module.register_forward_hook(hook) if hook is not None else None
        for p in params:
            p.requires_grad_(False)
        try:
            with torch.enable_grad():
                return self._rating(image)
        finally:
            for p in params:
                p.requires_grad_(True)
            if handle is not None:
                handle.remove()

    def capture(self, image):
        """(A, g): the layer's output in the pass of `image` and the gradient of the rating(s) with respect to it"""
        box = []

        def hook(mod, args, out):
            leaf = out.detach().requires_grad_(True)
            ent = out.__dict__.get('_pcgan_amax')       # operand maxima the producing kernel left for the next convolution
            if ent is not None:
                leaf._pcgan_amax = ent
            box.append(leaf)
            return leaf

        rating = self._pass(image.detach(), hook)
        if not box:
            raise ValueError('layer {} ({}) captured nothing in the pass: the network does not call it'.format(self.layer, self.resolved))
        A = box[-1]
        (g,) = torch.autograd.grad([rating], [A], grad_outputs=[torch.ones_like(rating)])
        return A.detach().contiguous(), g.contiguous()

    def input_gradient(self, image):
        """d rating / d image, the plain saliency of the reference's get_attention (siamese.py:988-999), per image of its own rating"""
        x = image.detach().clone().requires_grad_(True)
        rating = self._pass(x, None)
        (g,) = torch.autograd.grad([rating], [x], grad_outputs=[torch.ones_like(rating)])
        return g

    def map(self, image, kind='raw'):
        """the (N, 1, H, W) fp32 map of the captured layer"""
        if kind not in MAP_TYPES:
            raise ValueError('map type {} (one of {})'.format(kind, ' | '.join(MAP_TYPES)))
        A, g = self.capture(image)
        return ops.gradcam_map(A, g, kind)
