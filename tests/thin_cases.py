"""Case table, data makers, float64 reference, bounds and an arithmetic emulation of the thin convolutions (csrc/thin_conv.hip: the fp16
two-piece kernels thin_conv_kernel<7,7,1>, <7,7,2>, <4,4,2> behind pcgan_conv2d_fwd_thin / pcgan_conv2d_bwd_data_thin).  A plain module:
shared by tests/test_thin_cases.py, which checks the table and the emulation on the CPU, and tests/test_gpu_thin_cases.py, which runs it.

A case is one direct call of the C-ABI: geometry (N, C, H, W, K, R, S, stride, pad, pad_mode) of the CONVOLUTION (the data gradient gathers
its K channels and produces its C), a fused activation, a bias, the kind of data, and `want` = (kernel, host form), which `classify` must
derive from the geometry (thin_geometry / run_thin restated in `accepts` and `classify`; the CPU test holds `accepts` against the library).
Host forms: fwd_zero, fwd_reflect, dgrad_zero (a forward-form convolution of dy with flipped weights at zero padding 6 - pad), dgrad_reflect
(the same on the padded grid (H + 2 pad) x (W + 2 pad) into the workspace, then reflect_fold_kernel).

Section A, kind 'signed' (conv_f32_cases._signed): |x|, |w|, |dy|, |bias| in [0.75, 1.25] with random signs; the tanh / sigmoid cases
multiply the weights by 2^-4 (`wexp`) so that |ref| stays near 1.  Reference: split_arith.reference (float64, autograd through
the reflection: it sums the mirror images); the same call on absolute values gives A.  Per element
    |y - ref| <= E = (2 (3 Kp + 8) 2^-24 + 2^-20) A,      Kp = 16 NST = 208 (7x7) | 64 (4x4)
Each scaled operand splits as h + l with relative error <= 2^-22; the dropped (l,l) product is <= 2^-22 of the term; with the second-order
terms that is under 4 x 2^-22 = 2^-20.  The three piece products per term are exact in fp32 and accumulating them is 3 Kp additions (the
padding slots of the last stage included), bounded as conv_f32_cases bounds a sum (factor 2); the 8 covers the bias and the up to 5
additions of the fold; scaling by powers of two is exact.  Fused activations are 1-Lipschitz: + 2^-22 |act(ref)|.
Condition (CPU, and again before each launch): max E < TERM_MIN 2^wexp / 2, half the smallest possible term -- one lost, doubled or shifted
term in any element fails.

Section B, exact data: every partial sum of the kernel is an integer multiple of one quantum and bounded by A quanta, so any order of fp32
accumulation is exact when A < 2^24 quanta (asserted per case), and the test is out == ref for every element.
  'xlow': the activation tensor holds integers in [-(2^b - 1), 2^b - 1] with one element pinned to 2^b - 1 (b = 15 unless the mirror
          images of a reflect gradient need less), weights in {-1, 0, +1}, bias integers in [-64, 64], activation none / ReLU /
          LeakyReLU(0.25).  The tensor's scale is 2^(14 - b): every value splits into an 11-bit h and an l of up to 4 bits, exactly.
  'wlow': weights are 15-bit integers, each row of the pass's weight matrix (output channel forward, input channel for the data gradient)
          times 2^j, j in [-20, 20], rows 0 and 1 at +20 and -20; the activation tensor in {-1, 0, +1}; no bias.
  'xlow16' (section C): 'xlow' with every magnitude but the pinned one <= 16.
`emulate` restates the arithmetic (scale, split to fp16, the three piece products accumulated in fp32, scale back, bias, activation) in
torch; the CPU test holds it equal to the float64 reference and shows that it stops being equal when one low piece is zeroed or one tap is
shifted.

Section C data (ranges): `range_data` -- randn as in tests/test_gpu_thin.py, the kinds of tests/test_gpu_wgrad_rowring.py."""
import collections
import functools

import torch

from oracle import ops_ref as R
import split_arith
from conv_f32_cases import _signed, TERM_MIN
# (SLOPE, per_row_rel: the tests reach them through this module)
from split_arith import U, SLOPE, out_size, _ints, _fwd64, _dgrad64, pow2_scale, split2h, per_row_rel, range_scale

NT = 256                        # threads of a workgroup (thread_max_of_partials strides by it)
TH, TW = 8, 32                  # the workgroup's tile of output pixels
KERNELS = ('<7,7,1>', '<7,7,2>', '<4,4,2>')
# every (kernel, host form) pair the library accepts: reflection and the data gradient are stride 1, 7x7
ACCEPTED = (('<7,7,1>', 'fwd_zero'), ('<7,7,1>', 'fwd_reflect'), ('<7,7,2>', 'fwd_zero'), ('<4,4,2>', 'fwd_zero'),
            ('<7,7,1>', 'dgrad_zero'), ('<7,7,1>', 'dgrad_reflect'))
ACT_NAMES = ('none', 'relu', 'lrelu', 'tanh', 'sigmoid')

Case = collections.namedtuple('Case', 'sect name pass_ geom act bias wexp kind bits want claims seed')
Data = collections.namedtuple('Data', 'src w b ref A rowexp')


# ---- thin_geometry / run_thin, restated ------------------------------------------------------------------------------------------------------
def accepts(pass_, geom, f32=True):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    k77, k44 = (Rr, S) == (7, 7), (Rr, S) == (4, 4)
    if not f32:
        return False
    if pass_ == 'fwd':
        if C > 4 or K % 64 != 0 or K > 256:
            return False
        if not ((k77 and st in (1, 2)) or (k44 and st == 2)):
            return False
        return not (pm == 1 and (st != 1 or pad >= H or pad >= W))
    if K > 4 or C % 64 != 0 or C > 256 or not k77 or st != 1:
        return False
    return pm == 1 or Rr - 1 - pad >= 0


def classify(pass_, geom):
    """(kernel, host form) of an accepted shape"""
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    assert accepts(pass_, geom)
    if pass_ == 'fwd':
        return '<%d,%d,%d>' % (Rr, S, st), 'fwd_reflect' if pm == 1 else 'fwd_zero'
    return '<7,7,1>', 'dgrad_reflect' if pm == 1 else 'dgrad_zero'


def rows_of(c):
    """M: the channels the pass produces"""
    return c.geom[4] if c.pass_ == 'fwd' else c.geom[1]


def gathered(c):
    return c.geom[1] if c.pass_ == 'fwd' else c.geom[4]


def nst(c):
    return (c.geom[5] * c.geom[6] * 4 + 15) // 16


def pq(c):
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    return out_size(H, Rr, st, pad), out_size(W, S, st, pad)


def src_shape(c):
    N, C, H, W, K = c.geom[:5]
    return (N, C, H, W) if c.pass_ == 'fwd' else (N, K) + pq(c)


def out_shape(c):
    N, C, H, W, K = c.geom[:5]
    return (N, K) + pq(c) if c.pass_ == 'fwd' else (N, C, H, W)


def grid(c):
    """the plane the KERNEL writes: the output, or the padded grid of a reflect gradient (folded afterwards)"""
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    if c.pass_ == 'fwd':
        return pq(c)
    return (H + 2 * pad, W + 2 * pad) if pm == 1 else (H, W)


def packed_bytes(c):
    return (rows_of(c) // 32) * nst(c) * 2 * 64 * 16 + 4 * rows_of(c)


def workspace_bytes(c):
    gh, gw = grid(c)
    return 4 * c.geom[0] * rows_of(c) * gh * gw if c.want[1] == 'dgrad_reflect' else 0


CLAIMS = {
    'one_tile': lambda c: grid(c) == (TH, TW),
    'tile_plus_one': lambda c: grid(c) == (TH + 1, TW + 1),
    'whole_tiles': lambda c: grid(c)[0] % TH == 0 and grid(c)[1] % TW == 0,
    'x_tiles': lambda c: grid(c)[1] > TW,
    'y_tiles': lambda c: grid(c)[0] > TH,
    'ragged': lambda c: grid(c)[0] % TH != 0 or grid(c)[1] % TW != 0,
    'under_a_tile': lambda c: grid(c)[0] < TH and grid(c)[1] < TW,
    'images': lambda c: c.geom[0] > 1,
    'all_mirror': lambda c: c.geom[9] == 1 and c.geom[2] <= c.geom[8] + 1 and c.geom[3] <= c.geom[8] + 1,      # every row and column has a mirror image
    'plane_under_filter': lambda c: c.geom[2] < c.geom[5] and c.geom[3] < c.geom[6],
    'fold_both_sides': lambda c: c.want[1] == 'dgrad_reflect' and c.geom[2] < 2 * c.geom[8] + 2 and c.geom[3] < 2 * c.geom[8] + 2,
    'fold_at_2pad2': lambda c: c.want[1] == 'dgrad_reflect' and c.geom[2] == 2 * c.geom[8] + 2 and c.geom[3] == 2 * c.geom[8] + 2,
    'valid': lambda c: c.geom[8] == 0,
    'full_pad': lambda c: c.geom[9] == 0 and c.geom[8] == c.geom[5] - 1,
}


# ---- data, reference, bound --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def data(c):
    """(src, w, bias, float64 reference BEFORE the activation, A, row exponents) of a case on the CPU: made once, shared, never written to"""
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    fwd = c.pass_ == 'fwd'
    g = torch.Generator().manual_seed(sum(v * (i + 1) * 7919 for i, v in enumerate(c.geom)) + 104729 * c.seed + (17 if fwd else 0)
                                      + 1299709 * ('signed', 'xlow', 'wlow', 'xlow16').index(c.kind))
    M = rows_of(c)
    rowexp = None
    if c.kind == 'signed':
        src, w = _signed(g, *src_shape(c)), _signed(g, K, C, Rr, S) * 2.0 ** c.wexp
        b = _signed(g, M) if c.bias else None
    elif c.kind in ('xlow', 'xlow16'):
        top = 2 ** c.bits - 1
        src = _ints(g, -top, top, src_shape(c)) if c.kind == 'xlow' else _ints(g, -16, 16, src_shape(c))
        src.view(-1)[src.numel() // 2 + 3] = top
        w = _ints(g, -1, 1, (K, C, Rr, S))
        b = _ints(g, -64, 64, (M,)) if c.bias else None
    else:
        top = 2 ** c.bits - 1
        src = _ints(g, -1, 1, src_shape(c))
        rowexp = torch.randint(-20, 21, (M,), generator=g)
        rowexp[0], rowexp[1] = 20, -20
        mag = torch.pow(2.0, rowexp.float())
        w = _ints(g, -top, top, (K, C, Rr, S)) * (mag.view(K, 1, 1, 1) if fwd else mag.view(1, C, 1, 1))
        assert not c.bias
        b = None
    ref, A = reference(c, src, w, b)
    assert tuple(ref.shape) == out_shape(c)
    return Data(src, w, b, ref, A, rowexp)


def reference(c, src, w, b):
    """(float64 result before the activation, the same call on absolute values) of the case's geometry on the given operands"""
    return split_arith.reference(c.pass_, c.geom, src, w, b)


def slope_of(c):
    return split_arith.slope_of(c.kind)


def bounds(c, A=None, ref=None):
    """(E, the bound on |y - act(ref)|, act(ref)) per element"""
    d = data(c)
    A = d.A if A is None else A
    ref = d.ref if ref is None else ref
    E = (2 * (3 * 16 * nst(c) + 8) * U + 2.0 ** -20) * A
    aref = R.activation(ref, c.act, slope_of(c))
    return E, E + (2.0 ** -22 * aref.abs() if c.act else 0.0), aref


def condition(c):
    """(largest E of the case, what it has to stay under: half the smallest possible term)"""
    return float(bounds(c)[0].max()), TERM_MIN * 2.0 ** c.wexp / 2


def quanta(c):
    """exact kinds: the largest A of the case in units of its quantum (1 for 'xlow'; 2^j of the row for 'wlow'); must stay under 2^24"""
    return split_arith.quanta(data(c))


# ---- the kernel's arithmetic in torch --------------------------------------------------------------------------------------------------------
def emulate(c, perturb=None):
    """scale, split, the three piece products (l,h) (h,l) (h,h) each summed exactly and accumulated in fp32, scale back with the two
    reciprocals, bias, activation -- as float64 for the comparison.  perturb: 'zero_xl' / 'zero_wl' zero ONE non-zero low piece of the
    activation tensor / of the weights; 'shift_tap' moves ONE high weight piece to the neighbouring tap"""
    d = data(c)
    fwd = c.pass_ == 'fwd'
    K, C = c.geom[4], c.geom[1]
    sx = pow2_scale(float(d.src.abs().max()))
    rowmax = d.w.abs().amax(dim=(1, 2, 3)) if fwd else d.w.abs().amax(dim=(0, 2, 3))
    sw = torch.tensor([pow2_scale(float(v)) for v in rowmax])
    xh, xl = split2h(d.src * sx)
    wh, wl = split2h(d.w * (sw.view(K, 1, 1, 1) if fwd else sw.view(1, C, 1, 1)))
    if perturb in ('zero_xl', 'zero_wl'):
        t = xl if perturb == 'zero_xl' else wl
        nz = torch.nonzero(t.view(-1))
        assert nz.numel() > 0, 'no non-zero low piece to drop'
        t.view(-1)[int(nz[nz.numel() // 2])] = 0.0
    elif perturb == 'shift_tap':
        k, ci = K // 2, C // 2
        nz = torch.nonzero(wh[k, ci].view(-1) != wh[k, ci].view(-1).roll(1))
        i = int(nz[0])
        wh = wh.clone()
        wh[k, ci].view(-1)[i] = wh[k, ci].view(-1)[i - 1]
    f = _fwd64 if fwd else _dgrad64

    def piece(a, w):
        r = f(a.double(), w.double(), None, c.geom)
        assert bool((r.float().double() == r).all()), 'a piece sum is no fp32 number'
        return r.float()
    acc = (piece(xh, wl) + piece(xl, wh)) + piece(xh, wh)
    y = acc * (1.0 / sw).view(1, -1, 1, 1) * (1.0 / sx)
    if d.b is not None:
        y = y + d.b.view(1, -1, 1, 1)
    return R.activation(y, c.act, slope_of(c)).double(), (xl, wl)


# ---- section C: operand ranges ---------------------------------------------------------------------------------------------------------------
RANGE_KINDS = ('wide_range', 'huge', 'tiny')


def range_data(c, kind):
    """randn operands as in tests/test_gpu_thin.py under the kinds of tests/test_gpu_wgrad_rowring.py; returns (src, w, float64 reference)"""
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    g = torch.Generator().manual_seed(1000 + RANGE_KINDS.index(kind) + (17 if c.pass_ == 'fwd' else 0))
    w = torch.randn(K, C, Rr, S, generator=g) * 0.05
    src = torch.randn(*src_shape(c), generator=g)
    # wide_range: magnitudes over eight / twelve decades inside one tensor; tiny: true values near 1e-34 -- normal fp32, but sx sits at the
    # +100 clamp and the filter rows need 2^30; huge: true values near 1e20
    src, w = range_scale(kind, g, src, w, (8, -6), (12, -14), (1e-30, 1e-4), (1e12, 1e8))
    f = _fwd64 if c.pass_ == 'fwd' else _dgrad64
    return src, w, f(src.double(), w.double(), None, c.geom)


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
CASES = []


def _geom(pass_, kern, N, C, H, W, K, pad, pm):
    Rr, S, st = {'<7,7,1>': (7, 7, 1), '<7,7,2>': (7, 7, 2), '<4,4,2>': (4, 4, 2)}[kern]
    return (N, C, H, W, K, Rr, S, st, pad, pm)


def _add(sect, pass_, kern, form, shape, claims=(), act=0, bias=False, wexp=0, kind='signed', bits=15, seed=0):
    N, C, H, W, K, pad = shape
    geom = _geom(pass_, kern, N, C, H, W, K, pad, 1 if form.endswith('reflect') else 0)
    name = '%s-%s-%dx%dx%dx%d-k%d-p%d%s%s%s' % (form, kern[1:-1].replace(',', ''), N, C, H, W, K, pad, '-bias' if bias else '',
                                               '-' + ACT_NAMES[act] if act else '', '' if kind == 'signed' else '-%s%d' % (kind, bits))
    CASES.append(Case(sect, name, pass_, geom, act, bias, wexp, kind, bits, (kern, form), tuple(claims), seed))


# A. lost, doubled or misplaced terms.  N, C, H, W, K, pad of the convolution; the data gradient produces C and gathers K.
# forward <7,7,1>, reflection
_add('A', 'fwd', '<7,7,1>', 'fwd_reflect', (2, 4, 9, 33, 64, 3), ('tile_plus_one', 'images'), act=1, bias=True)
_add('A', 'fwd', '<7,7,1>', 'fwd_reflect', (1, 3, 4, 4, 128, 3), ('all_mirror', 'under_a_tile'))          # the smallest legal plane
_add('A', 'fwd', '<7,7,1>', 'fwd_reflect', (1, 2, 8, 32, 192, 3), ('one_tile',), bias=True)
_add('A', 'fwd', '<7,7,1>', 'fwd_reflect', (1, 1, 16, 64, 256, 3), ('whole_tiles', 'x_tiles', 'y_tiles'))
_add('A', 'fwd', '<7,7,1>', 'fwd_reflect', (2, 4, 12, 40, 64, 1), ('ragged', 'images'), act=2, bias=True)      # 8 x 36 outputs
_add('A', 'fwd', '<7,7,1>', 'fwd_reflect', (1, 4, 6, 7, 64, 5), ('ragged', 'y_tiles'))                         # 10 x 11 outputs, pad H - 1
# forward <7,7,1>, zero padding
_add('A', 'fwd', '<7,7,1>', 'fwd_zero', (2, 3, 10, 39, 64, 0), ('valid', 'x_tiles', 'images'), bias=True)      # 4 x 33 outputs
_add('A', 'fwd', '<7,7,1>', 'fwd_zero', (2, 4, 9, 33, 128, 3), ('tile_plus_one',), act=1, bias=True)
_add('A', 'fwd', '<7,7,1>', 'fwd_zero', (1, 4, 3, 5, 64, 6), ('plane_under_filter', 'full_pad'))
# forward <7,7,2>
_add('A', 'fwd', '<7,7,2>', 'fwd_zero', (2, 3, 17, 65, 64, 3), ('tile_plus_one', 'images'), act=2, bias=True)
_add('A', 'fwd', '<7,7,2>', 'fwd_zero', (1, 4, 16, 64, 128, 3), ('one_tile',), bias=True)
_add('A', 'fwd', '<7,7,2>', 'fwd_zero', (1, 1, 21, 23, 192, 0), ('valid',), act=1, bias=True)                 # 8 x 9 outputs
_add('A', 'fwd', '<7,7,2>', 'fwd_zero', (1, 2, 9, 9, 256, 2), ('under_a_tile',))
# forward <4,4,2>
_add('A', 'fwd', '<4,4,2>', 'fwd_zero', (2, 4, 18, 66, 64, 1), ('tile_plus_one', 'images'), act=2, bias=True)
_add('A', 'fwd', '<4,4,2>', 'fwd_zero', (1, 3, 16, 64, 128, 1), ('one_tile',), bias=True)
_add('A', 'fwd', '<4,4,2>', 'fwd_zero', (3, 4, 17, 19, 64, 1), ('images',), act=3, bias=True, wexp=-4)          # 8 x 9 outputs
_add('A', 'fwd', '<4,4,2>', 'fwd_zero', (1, 2, 6, 8, 192, 0), ('valid', 'under_a_tile'), act=4, bias=True, wexp=-4)
_add('A', 'fwd', '<4,4,2>', 'fwd_zero', (1, 1, 5, 5, 256, 2), ('under_a_tile',), act=1, bias=True)
_add('A', 'fwd', '<4,4,2>', 'fwd_zero', (2, 4, 18, 66, 64, 1), ('tile_plus_one',), act=4, bias=True, wexp=-4, seed=1)
_add('A', 'fwd', '<4,4,2>', 'fwd_zero', (1, 3, 16, 64, 128, 1), ('one_tile',), act=3, bias=True, wexp=-4, seed=1)
# data gradient, zero padding
_add('A', 'dgrad', '<7,7,1>', 'dgrad_zero', (2, 64, 9, 33, 3, 3), ('tile_plus_one', 'images'))
_add('A', 'dgrad', '<7,7,1>', 'dgrad_zero', (1, 128, 10, 39, 1, 0), ('valid', 'ragged', 'x_tiles'))
_add('A', 'dgrad', '<7,7,1>', 'dgrad_zero', (1, 192, 3, 5, 2, 6), ('full_pad', 'under_a_tile'))
_add('A', 'dgrad', '<7,7,1>', 'dgrad_zero', (1, 256, 8, 32, 4, 3), ('one_tile',))
_add('A', 'dgrad', '<7,7,1>', 'dgrad_zero', (1, 64, 12, 20, 4, 1), ('y_tiles',))
_add('A', 'dgrad', '<7,7,1>', 'dgrad_zero', (1, 64, 8, 9, 3, 5), ())
# data gradient, reflection: the kernel writes the padded grid, reflect_fold_kernel folds it
_add('A', 'dgrad', '<7,7,1>', 'dgrad_reflect', (2, 64, 9, 33, 3, 3), ('images', 'x_tiles', 'y_tiles'))          # grid 15 x 39
_add('A', 'dgrad', '<7,7,1>', 'dgrad_reflect', (1, 64, 4, 4, 4, 3), ('fold_both_sides', 'all_mirror'))          # up to 9 images
_add('A', 'dgrad', '<7,7,1>', 'dgrad_reflect', (1, 128, 8, 8, 2, 3), ('fold_at_2pad2',))
_add('A', 'dgrad', '<7,7,1>', 'dgrad_reflect', (1, 64, 12, 40, 1, 1), ('x_tiles', 'y_tiles'))                   # grid 14 x 42
_add('A', 'dgrad', '<7,7,1>', 'dgrad_reflect', (1, 64, 6, 7, 3, 5), ('fold_both_sides',))                       # grid 16 x 17: whole tiles in y

# B. exact pieces: both data kinds on one ragged case of each (kernel, form) pair, and 'xlow' on the two small reflect planes
for _kind in ('xlow', 'wlow'):
    _x = _kind == 'xlow'
    _add('B', 'fwd', '<7,7,1>', 'fwd_reflect', (2, 4, 9, 33, 64, 3), ('tile_plus_one',), act=1 if _x else 0, bias=_x, kind=_kind)
    _add('B', 'fwd', '<7,7,1>', 'fwd_zero', (2, 3, 10, 39, 64, 0), ('x_tiles',), bias=_x, kind=_kind)
    _add('B', 'fwd', '<7,7,2>', 'fwd_zero', (2, 3, 17, 65, 64, 3), ('tile_plus_one',), act=2 if _x else 0, bias=_x, kind=_kind)
    _add('B', 'fwd', '<4,4,2>', 'fwd_zero', (2, 4, 18, 66, 64, 1), ('tile_plus_one',), act=1 if _x else 0, bias=_x, kind=_kind)
    _add('B', 'dgrad', '<7,7,1>', 'dgrad_zero', (2, 64, 9, 33, 3, 3), ('tile_plus_one',), kind=_kind)
    _add('B', 'dgrad', '<7,7,1>', 'dgrad_reflect', (2, 64, 9, 33, 3, 3), ('x_tiles',), kind=_kind)
_add('B', 'dgrad', '<7,7,1>', 'dgrad_reflect', (1, 64, 4, 4, 4, 3), ('fold_both_sides',), kind='xlow', bits=12)
_add('B', 'dgrad', '<7,7,1>', 'dgrad_reflect', (1, 128, 8, 8, 2, 3), ('fold_at_2pad2',), kind='xlow', bits=14)

BY_NAME = collections.OrderedDict(('%s.%s' % (c.sect, c.name), c) for c in CASES)
assert len(BY_NAME) == len(CASES), 'case names must be unique'

# section C: the case whose maxima array the test builds by hand (every magnitude but the pinned 2^15 - 1 is <= 16), and the two range cases
MAXPOS = Case('C', 'maxpos', 'fwd', _geom('fwd', '<7,7,1>', 1, 4, 8, 32, 64, 3, 1), 1, True, 0, 'xlow16', 15, ('<7,7,1>', 'fwd_reflect'), ('one_tile',), 0)
RANGE_FWD = BY_NAME['A.fwd_reflect-771-2x4x9x33-k64-p3-bias-relu']._replace(sect='C', act=0, bias=False)
RANGE_DGRAD = BY_NAME['A.dgrad_reflect-771-2x64x9x33-k3-p3']._replace(sect='C')
MAXPOS_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4096, 4100, 4103)


def maxima_slots(n):
    """split_arith.maxima_slots at NT = 256: from 1024 slots on the end of the first 4-in-flight round of 256 threads, from 4096 on the
    second and the third load in flight"""
    return split_arith.maxima_slots(n, NT)
