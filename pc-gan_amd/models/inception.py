"""Inception-v3 feature network for FID on the HIP path (reference models/inception.py: InceptionV3 over the blocks of torchvision's
inception_v3(pretrained=True), used by compute_fid_score.py:56-57,260-290).

The network is restated from torchvision's published architecture (module and state_dict names, kernel shapes, channel counts: the
feature path holds 94 BasicConv2d = Conv2d(bias=False) + eval BatchNorm2d(eps=0.001) + ReLU); tests/inception_ref.py restates it again
with stock torch modules and checks it against torchvision's published parameter count.  Weights come from a torchvision-layout
state_dict supplied by the user (nothing is downloaded).  Every BatchNorm is folded into its convolution once per load
(pcgan_iconv_pack); the forward is HIP kernels only (csrc/inception.hip): one pass for resize + normalisation, one implicit-GEMM launch
per convolution writing its channel slice of the Mixed block's output, the InceptionA / C / E pool branch as a 3x3 convolution with taps
w / 9 (avg_pool2d with count_include_pad=True, then the 1x1 conv), the InceptionB / D pool branch as a slice max pool.  Forward only:
an input that requires grad is refused."""
import torch

from pcgan_amd.hip import inception as I

# ---- architecture (torchvision's Inception3 feature path) ---------------------------------------------------------------------------
# a conv: (name, C_in, K, (R, S), stride, (pad_h, pad_w))


def _cv(name, cin, k, ks, stride=1, pad=None):
    ks = (ks, ks) if isinstance(ks, int) else ks
    if pad is None:
        pad = (0, 0) if stride == 2 else ((ks[0] - 1) // 2, (ks[1] - 1) // 2)
    return (name, cin, k, ks, stride, pad)


# A Mixed block: (name, C_in, branches, pool) where a branch is (chain, fork): the chain runs convs in sequence and its last result
# (or, with a fork, each fork conv applied to it) goes to the block output at the next channel offset; pool is ('avg', conv) -- the
# branch_pool conv on avg_pool2d(3, 1, 1) -- or ('max', None): max_pool2d(3, 2) of the block input.
def _A(n, cin, pf):
    return (n, cin, [([_cv(n + '.branch1x1', cin, 64, 1)], []),
                     ([_cv(n + '.branch5x5_1', cin, 48, 1), _cv(n + '.branch5x5_2', 48, 64, 5)], []),
                     ([_cv(n + '.branch3x3dbl_1', cin, 64, 1), _cv(n + '.branch3x3dbl_2', 64, 96, 3),
                       _cv(n + '.branch3x3dbl_3', 96, 96, 3)], [])],
            ('avg', _cv(n + '.branch_pool', cin, pf, 1)))


def _B(n, cin):
    return (n, cin, [([_cv(n + '.branch3x3', cin, 384, 3, 2)], []),
                     ([_cv(n + '.branch3x3dbl_1', cin, 64, 1), _cv(n + '.branch3x3dbl_2', 64, 96, 3),
                       _cv(n + '.branch3x3dbl_3', 96, 96, 3, 2)], [])],
            ('max', None))


def _C(n, cin, c7):
    return (n, cin, [([_cv(n + '.branch1x1', cin, 192, 1)], []),
                     ([_cv(n + '.branch7x7_1', cin, c7, 1), _cv(n + '.branch7x7_2', c7, c7, (1, 7)),
                       _cv(n + '.branch7x7_3', c7, 192, (7, 1))], []),
                     ([_cv(n + '.branch7x7dbl_1', cin, c7, 1), _cv(n + '.branch7x7dbl_2', c7, c7, (7, 1)),
                       _cv(n + '.branch7x7dbl_3', c7, c7, (1, 7)), _cv(n + '.branch7x7dbl_4', c7, c7, (7, 1)),
                       _cv(n + '.branch7x7dbl_5', c7, 192, (1, 7))], [])],
            ('avg', _cv(n + '.branch_pool', cin, 192, 1)))


def _D(n, cin):
    return (n, cin, [([_cv(n + '.branch3x3_1', cin, 192, 1), _cv(n + '.branch3x3_2', 192, 320, 3, 2)], []),
                     ([_cv(n + '.branch7x7x3_1', cin, 192, 1), _cv(n + '.branch7x7x3_2', 192, 192, (1, 7)),
                       _cv(n + '.branch7x7x3_3', 192, 192, (7, 1)), _cv(n + '.branch7x7x3_4', 192, 192, 3, 2)], [])],
            ('max', None))


def _E(n, cin):
    return (n, cin, [([_cv(n + '.branch1x1', cin, 320, 1)], []),
                     ([_cv(n + '.branch3x3_1', cin, 384, 1)],
                      [_cv(n + '.branch3x3_2a', 384, 384, (1, 3)), _cv(n + '.branch3x3_2b', 384, 384, (3, 1))]),
                     ([_cv(n + '.branch3x3dbl_1', cin, 448, 1), _cv(n + '.branch3x3dbl_2', 448, 384, 3)],
                      [_cv(n + '.branch3x3dbl_3a', 384, 384, (1, 3)), _cv(n + '.branch3x3dbl_3b', 384, 384, (3, 1))])],
            ('avg', _cv(n + '.branch_pool', cin, 192, 1)))


STEM0 = [_cv('Conv2d_1a_3x3', 3, 32, 3, 2), _cv('Conv2d_2a_3x3', 32, 32, 3, 1, (0, 0)), _cv('Conv2d_2b_3x3', 32, 64, 3)]
STEM1 = [_cv('Conv2d_3b_1x1', 64, 80, 1), _cv('Conv2d_4a_3x3', 80, 192, 3, 1, (0, 0))]
MIXED2 = [_A('Mixed_5b', 192, 32), _A('Mixed_5c', 256, 64), _A('Mixed_5d', 288, 64), _B('Mixed_6a', 288),
          _C('Mixed_6b', 768, 128), _C('Mixed_6c', 768, 160), _C('Mixed_6d', 768, 160), _C('Mixed_6e', 768, 192)]
MIXED3 = [_D('Mixed_7a', 768), _E('Mixed_7b', 1280), _E('Mixed_7c', 2048)]


def _mixed_convs(block):
    _, _, branches, (_, pool_conv) = block
    out = [c for chain, fork in branches for c in chain + fork]
    return out + ([pool_conv] if pool_conv is not None else [])


def feature_convs():
    """every conv of the feature path, in forward order (94)"""
    out = STEM0 + STEM1
    for b in MIXED2 + MIXED3:
        out += _mixed_convs(b)
    return out


BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')
FID_INCEPTION_CLASSES = 1008     # pytorch-fid's FIDInception weights: a different network (count_include_pad=False, max pool in 7c)


def expected_shapes():
    """torchvision key -> shape for every feature-path parameter / buffer the loader needs"""
    shapes = {}
    for name, cin, k, (r, s), _, _ in feature_convs():
        shapes[name + '.conv.weight'] = (k, cin, r, s)
        for b in BN_KEYS:
            shapes['%s.bn.%s' % (name, b)] = (k,)
    return shapes


def check_state_dict(sd):
    """validate a torchvision-layout Inception-v3 state_dict (host only, before any device use); returns the feature-path entries.
    AuxLogits.* and fc.* are ignored, num_batches_tracked too; missing keys, wrong shapes, unknown keys and pytorch-fid's 1008-class
    FID weights raise."""
    if not isinstance(sd, dict):
        raise TypeError('Inception weights: expected a state_dict (dict of tensors), got %s' % type(sd).__name__)
    fc = sd.get('fc.weight')
    if fc is not None and tuple(fc.shape)[0] == FID_INCEPTION_CLASSES:
        raise ValueError('Inception weights: fc.weight has %d rows -- these are pytorch-fid\'s FIDInception weights '
                         '(pt_inception-2015-12-05), a different network (count_include_pad=False pools, a max pool in Mixed_7c). '
                         'The reference computes FID with torchvision\'s inception_v3 (1000 classes): supply that file '
                         '(inception_v3_google-*.pth).' % FID_INCEPTION_CLASSES)
    want = expected_shapes()
    missing = sorted(k for k in want if k not in sd)
    if missing:
        raise KeyError('Inception weights: %d missing keys (not a torchvision inception_v3 state_dict?), e.g. %s'
                       % (len(missing), ', '.join(missing[:5])))
    unknown = sorted(k for k in sd if k not in want and not k.startswith(('AuxLogits.', 'fc.')) and not k.endswith('num_batches_tracked'))
    if unknown:
        raise KeyError('Inception weights: unexpected keys, e.g. %s' % ', '.join(unknown[:5]))
    for k, shape in want.items():
        v = sd[k]
        if not torch.is_tensor(v) or tuple(v.shape) != shape:
            raise ValueError('Inception weights: %s has shape %s, expected %s' % (k, tuple(getattr(v, 'shape', ())), shape))
    return {k: sd[k] for k in want}


def check_classifier_state_dict(sd):
    """check_state_dict plus the classifier head of torchvision's inception_v3 (host only, before any device use): fc.weight
    (classes, 2048) and fc.bias (classes,); returns the number of classes"""
    check_state_dict(sd)
    w, b = sd.get('fc.weight'), sd.get('fc.bias')
    if w is None or b is None:
        raise KeyError('Inception weights: no fc.weight / fc.bias -- the Inception Score needs the classifier head of torchvision\'s '
                       'inception_v3 (fc: 2048 -> 1000), not only the feature path')
    if not (torch.is_tensor(w) and torch.is_tensor(b)) or w.dim() != 2 or w.shape[1] != 2048 or tuple(b.shape) != (w.shape[0],):
        raise ValueError('Inception weights: fc.weight %s / fc.bias %s, expected (classes, 2048) / (classes,)'
                         % (tuple(getattr(w, 'shape', ())), tuple(getattr(b, 'shape', ()))))
    return int(w.shape[0])


def load_state_dict_file(weights):
    if isinstance(weights, dict):
        return weights
    sd = torch.load(weights, map_location='cpu')
    if isinstance(sd, dict) and 'state_dict' in sd and isinstance(sd['state_dict'], dict):
        sd = sd['state_dict']
    return sd


class InceptionV3(object):
    """The reference's InceptionV3 (models/inception.py) on the HIP path: forward(x) returns the requested block outputs, sorted by
    index: 0 -> (64, 73, 73) after the first max pool, 1 -> (192, 35, 35) after the second, 2 -> (768, 17, 17) (input of the aux
    classifier), 3 -> (2048, 1, 1) after the final average pool.  x: (N, 3, H, W) float32 images in [0, 1]."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}
    MEAN = (0.485, 0.456, 0.406)
    STD = (0.229, 0.224, 0.225)

    def __init__(self, output_blocks=[DEFAULT_BLOCK_INDEX], resize_input=True, normalize_input=True, weights=None, gpu_ids=[0]):
        self.resize_input = resize_input
        self.normalize_input = normalize_input
        self.output_blocks = sorted(output_blocks)
        if not self.output_blocks or min(self.output_blocks) < 0:
            raise ValueError('output_blocks must be a non-empty list of block indices 0..3')
        self.last_needed_block = max(output_blocks)
        assert self.last_needed_block <= 3, 'Last possible output block index is 3'
        self.gpu_ids = list(gpu_ids)
        if not self.gpu_ids:
            raise ValueError('InceptionV3 runs on the GPU only (HIP path, no CPU fallback): gpu_ids must name a device')
        self.device = torch.device('cuda', self.gpu_ids[0])
        self.packed = None
        if weights is not None:
            self.load_state_dict(weights)

    def load_state_dict(self, weights):
        """weights: a path to a torchvision inception_v3 .pth, or the state_dict itself.  Validated on the host first, then every
        BatchNorm is folded into its convolution and packed on the device (once per load)."""
        sd = check_state_dict(load_state_dict_file(weights))
        packed = {}
        with torch.cuda.device(self.device), torch.no_grad():
            for name, cin, k, ks, stride, pad in feature_convs():
                dev = lambda t: t.detach().to(self.device, torch.float32).contiguous()     # noqa: E731
                w = dev(sd[name + '.conv.weight'])
                bn = tuple(dev(sd['%s.bn.%s' % (name, b)]) for b in BN_KEYS)
                packed[name] = I.iconv_pack(w, bn, eps=1e-3, pool_expand=name.endswith('branch_pool'))
        self.packed = packed
        return self

    def eval(self):
        return self

    def __call__(self, x):
        return self.forward(x)

    # ---- forward ----------------------------------------------------------------------------------------------------------------
    def _conv(self, spec, x, out=None, k_off=0):
        name, cin, k, (r, s), stride, pad = spec
        if name.endswith('branch_pool'):
            r, s, stride, pad = 3, 3, 1, (1, 1)
        return I.iconv_fwd(x, self.packed[name], k, r, s, stride, pad, relu=True, out=out, k_off=k_off)

    def _mixed(self, block, x):
        _, cin, branches, (pool_kind, pool_conv) = block
        N, _, H, W = x.shape
        k_total = sum(spec[2] for chain, fork in branches for spec in (fork or chain[-1:]))
        k_total += pool_conv[2] if pool_kind == 'avg' else cin
        # InceptionB / D reduce 3x3 / 2 (their stride-2 convs and the max pool agree), the others keep the size
        P, Q = (I.out_size(H, 3, 2, 0), I.out_size(W, 3, 2, 0)) if pool_kind == 'max' else (H, W)
        y = torch.empty((N, k_total, P, Q), dtype=torch.float32, device=x.device)
        off = 0
        for chain, fork in branches:
            t = x
            for spec in (chain if fork else chain[:-1]):
                t = self._conv(spec, t)
            for spec in (fork if fork else chain[-1:]):
                self._conv(spec, t, out=y, k_off=off)
                off += spec[2]
        if pool_kind == 'avg':
            self._conv(pool_conv, x, out=y, k_off=off)
        else:
            I.maxpool_slice(x, 3, 2, out=y, k_off=off)
        return y

    def _block(self, idx, x):
        if idx == 0:
            for spec in STEM0:
                x = self._conv(spec, x)
            return I.maxpool_slice(x, 3, 2)
        if idx == 1:
            for spec in STEM1:
                x = self._conv(spec, x)
            return I.maxpool_slice(x, 3, 2)
        for b in (MIXED2 if idx == 2 else MIXED3):
            x = self._mixed(b, x)
        return I.global_avg_pool(x) if idx == 3 else x

    def prepare(self, x):
        """resize to 299 x 299 (align_corners=False) and normalize_input, one HIP pass; neither: x itself"""
        if not (self.resize_input or self.normalize_input):
            return x
        scale = shift = None
        if self.normalize_input:
            scale = [s / 0.5 for s in self.STD]
            shift = [(m - 0.5) / 0.5 for m in self.MEAN]
        return I.prep(x, (299, 299) if self.resize_input else None, scale, shift)

    def forward(self, inp):
        if inp.requires_grad:
            raise RuntimeError('InceptionV3 (HIP) is forward-only: the input requires grad and there is no backward pass')
        if self.packed is None:
            raise RuntimeError('InceptionV3: no weights loaded (pass weights= or call load_state_dict)')
        if inp.dtype != torch.float32:
            raise RuntimeError('InceptionV3 (HIP) takes float32 images, got %s' % inp.dtype)
        if inp.dim() != 4 or inp.shape[1] != 3:
            raise ValueError('InceptionV3 takes (N, 3, H, W) images, got %s' % (tuple(inp.shape),))
        outp = []
        with torch.no_grad(), torch.cuda.device(self.device):
            x = self.prepare(inp.to(self.device).contiguous())
            for idx in range(self.last_needed_block + 1):
                x = self._block(idx, x)
                if idx in self.output_blocks:
                    outp.append(x)
        return outp


class InceptionV3Classifier(InceptionV3):
    """torchvision's inception_v3(transform_input=False) in eval mode, as the reference's Inception Score runs it
    (compute_inception_score.py:28-30, util/inception_score.py:37-41): blocks 0-3 of InceptionV3, dropout (the identity in eval mode),
    then fc 2048 -> classes and the softmax in one HIP call (pcgan_linear_softmax_fwd).  The input pass only resizes to 299 x 299 by
    default: the dataset transform has normalised the images already.  The weights file must hold fc.weight / fc.bias."""

    def __init__(self, weights=None, resize_input=True, normalize_input=False, gpu_ids=[0]):
        self.fc_weight = self.fc_bias = None
        self.num_classes = None
        super().__init__([InceptionV3.DEFAULT_BLOCK_INDEX], resize_input, normalize_input, weights, gpu_ids)

    def load_state_dict(self, weights):
        sd = load_state_dict_file(weights)
        classes = check_classifier_state_dict(sd)
        InceptionV3.load_state_dict(self, sd)
        with torch.cuda.device(self.device), torch.no_grad():
            self.fc_weight = sd['fc.weight'].detach().to(self.device, torch.float32).contiguous()
            self.fc_bias = sd['fc.bias'].detach().to(self.device, torch.float32).contiguous()
        self.num_classes = classes
        return self

    def __call__(self, x, probs=False):
        return self.forward(x, probs)

    def forward(self, inp, probs=False):
        """logits (N, classes); with probs=True (logits, softmax probabilities)"""
        pooled = InceptionV3.forward(self, inp)[0]
        with torch.no_grad(), torch.cuda.device(self.device):
            logits, p = I.linear_softmax(pooled.flatten(1), self.fc_weight, self.fc_bias)
        return (logits, p) if probs else logits
