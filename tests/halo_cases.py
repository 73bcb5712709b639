"""Case table, data makers, float64 reference, bounds and an arithmetic emulation of the window ("halo") kernel (csrc/halo_conv.hip:
bsplit_halo_kernel<MODE, PK, TA, QW>, the forward and the data gradient of the reflection-padded 3x3 stride-1 convolution of the residual
blocks).  A plain module: shared by tests/test_halo_cases.py, which checks the table and the emulation on the CPU, and
tests/test_gpu_halo_cases.py, which runs it.

Twelve instantiations: pass_ in ('fwd', 'dgrad') x pk in ('f16x2': two scaled fp16 pieces of fp32 tensors, pcgan_conv2d_*_hsplit;
'bf16x3': three bf16 pieces of fp32 tensors; 'bf16': bf16 tensors as they are -- both through pcgan_conv2d_*_bsplit while option
bsplit_halo is 1) x image width in (32, 64).  A case is one direct call of the C-ABI on `shape` = (N, gathered channels, H, W, produced
channels): the data gradient gathers the K channels of the convolution and produces its C.  `accepts` restates halo_geometry.

Section A, kind 'signed' (conv_f32_cases._signed): |x|, |w|, |dy|, |bias|, |addend| in [0.75, 1.25] with random signs; tanh / sigmoid cases
multiply the weights by 2^wexp so that |ref| stays near 1.  Reference: split_arith.reference (float64, autograd through the
reflection); the same call on absolute values gives A.  Kp = 9 x gathered channels terms per element.  Per element |y - ref| <= E:
  f16x2   E = (2 (3 Kp + 8) 2^-24 + 2^-20) A.  Each scaled operand splits as h + l with relative error <= 2^-22, the dropped (l,l) product
          is <= 2^-22 of the term, with the second-order terms under 2^-20.  The three piece products per term are exact in fp32 and
          accumulating them is 3 Kp additions, bounded as conv_f32_cases bounds a sum (factor 2); the 8 covers the bias, the residual
          addend and the three fp32 additions of a four-source sum entry of the data gradient.  A sum entry is split AFTER the sum: its
          split error is 2^-22 of the sum, at most 2^-22 of the sum of its sources' magnitudes, which is what A counts for it (a sum past
          fp16's 65504 keeps h = 65504 and l = the rest, under 32, to 2^-7: 2^-23 of the sum).  Scaling by powers of two is exact.
  bf16x3  E = (2 (6 Kp + 8) 2^-24 + 2^-24) A.  x = h + m + l exactly (3 x 8 bits); |m| <= 2^-9 |x|, |l| <= 2^-18 |x|.  Six products per
          term, each exact in fp32 (8 x 8 bits); the dropped pairs (1,2), (2,1), (2,2) are <= (2 x 2^-27 + 2^-36) < 2^-25 of the term.
  bf16    inputs and weights are bf16 numbers, every product is exact, the accumulation is Kp additions in fp32, the stored result is ONE
          round-to-nearest-even to bf16: E = 2 (Kp + 8) 2^-24 A + half a bf16 ulp at |act(ref)| + the first part.  The data gradient
          rounds every sum entry to bf16 once more (put_split casts the fp32 sum): here |dy| sits on the grid 2^-5, so every two- and
          four-source sum (<= 5 = 160 x 2^-5) IS a bf16 number and that rounding is exact (asserted on the CPU) -- with free bf16 values
          it is up to 2^-8 of a third of A on the fold rows, which would leave no room for the condition.
Fused activations are 1-Lipschitz: + 2^-22 |act(ref)|.
Condition (CPU, and again before each launch): max E < TERM_MIN 2^wexp / 2, half the smallest possible term -- one lost, doubled or
shifted term in any element fails.  It holds at 32 and (f16x2) 64 gathered channels, not at 96: that shape is in section B only.  bf16
tensors: half a bf16 ulp at |ref| in [64, 128) is 0.25 of the 0.281 allowed, so the condition holds at 32 gathered channels only.

Section B, exact data: every partial sum of the kernel is an integer multiple of one quantum and bounded by A quanta, so any order of
fp32 accumulation is exact when A < 2^24 quanta (asserted per case), and the test is out == ref for every element ('bf16': == the
round-to-nearest-even bf16 of the exact result).
  'xlow': the gathered tensor holds integers with one element pinned to 2^b - 1, weights in {-1, 0, +1}, bias integers in [-64, 64],
          activation none / ReLU / LeakyReLU(0.25).  b per piece form so that every value -- and in the data gradient every four-source
          sum -- splits exactly: f16x2 15 bits forward (11 + 4), 13 in the data gradient (no sum past 65504: section C holds that); bf16 8 bits forward, 6 in the data gradient
          (4 x 63 < 256).  bf16x3 splits 24 bits exactly, but A < 2^24 leaves no room for 288 terms of that size: the pinned element has
          23 bits (22 in the data gradient), every 97th element `wide` = 20 bits (non-zero third piece), the rest 12.
  'wlow': the low pieces sit in the weights; the gathered tensor in {-1, 0, +1}, no bias.  f16x2: 15-bit integers, each row of the pass's
          weight matrix times 2^j, j in [-20, 20], rows 0 and 1 at +20 and -20; bf16x3: 15-bit integers (and one case per pass where every
          61st weight has 19 bits: a non-zero third piece); bf16: 8-bit integers.  At 96 gathered channels 14 bits: 864 terms, A < 2^24.
  'fold': data gradient only.  dy is zero except in ONE source class of the sum entries -- rows {0, 2}, rows {H-3, H-1}, columns {0, 2},
          columns {W-3, W-1}, or one of the four corners (2 x 2 sources) -- where the sources of every entry hold distinct integers
          (1 + (5 r + 3 c + 7 k + 11 n) mod 59), weights integers in [-3, 3]: a swapped use_lo / use_hi or c0 / c1, or a lane that reads
          the shifted entry where it should read the sum, is a wrong integer in a known element.
`emulate` restates the kernel's arithmetic in torch: the scale, the window with the mirror (forward) or with the zero ring and the sum
rows and columns (data gradient), the split, the piece products of each form accumulated in fp32, the scale back per row, bias,
activation, addend.  The CPU test holds it equal to the float64 reference on section B data and shows that it stops being equal when
one low piece is zeroed, one window entry takes a wrong source, or one tap is shifted.

Section C data: `range_data` (randn under the kinds of tests/test_gpu_bf16x6.py), the maxima-slot case, the four-corner overflow data."""
import collections
import functools

import torch

from oracle import ops_ref as R
import split_arith
from conv_f32_cases import _signed, TERM_MIN
# (SLOPE, per_row_rel: the tests reach them through this module)
from split_arith import U, SLOPE, _ints, _bf16, _fwd64, _dgrad64, half_ulp_bf16, pow2_scale, split2h, split3, per_row_rel, range_scale

NT = 512                        # threads of a workgroup (thread_max_of_partials strides by it)
PKS = ('f16x2', 'bf16x3', 'bf16')
INSTANTIATIONS = tuple((p, k, w) for p in ('fwd', 'dgrad') for k in PKS for w in (32, 64))
ACT_NAMES = ('none', 'relu', 'lrelu', 'tanh', 'sigmoid')
KINDS = ('signed', 'xlow', 'wlow', 'fold', 'xlow16')
FOLDS = ('rows_lo', 'rows_hi', 'cols_lo', 'cols_hi', 'corner_ll', 'corner_lh', 'corner_hl', 'corner_hh')

# (N, gathered, H, W, produced)
S_ONE = (1, 32, 4, 32, 256)         # one tile per image holds rows 1 and H-2; one chunk pair
S_W64 = (2, 32, 4, 64, 256)         # width 64: rows {0, 1} and {2, 3} in different tiles; the image index is in the offsets
S_W64_3 = (1, 32, 6, 64, 256)       # width 64, three tiles: the middle one holds no fold row
S_W32_3 = (2, 32, 12, 32, 256)      # three tiles at width 32: first, middle, last
S_PAIRS2 = (1, 64, 8, 32, 512)      # two chunk pairs, two 256-row weight tiles (a_tile, piece_bytes)
S_PAIRS3 = (1, 96, 8, 32, 256)      # three chunk pairs: the window buffers alternate across pairs.  Exact data only
SHAPES = (S_ONE, S_W64, S_W64_3, S_W32_3, S_PAIRS2, S_PAIRS3)

Case = collections.namedtuple('Case', 'sect name pass_ pk shape act bias add wexp kind bits wide fold seed')
Data = collections.namedtuple('Data', 'src w b add ref A rowexp')


# ---- halo_geometry and the sizes of the packed buffers, restated ---------------------------------------------------------------------------
def accepts(gathered, H, W, produced):
    return W in (32, 64) and H >= 4 and H % (128 // W) == 0 and gathered % 32 == 0 and produced % 256 == 0


def geom(c):
    """the CONVOLUTION's (N, C, H, W, K, R, S, stride, pad, pad_mode)"""
    N, G, H, W, M = c.shape
    return (N, G, H, W, M, 3, 3, 1, 1, 1) if c.pass_ == 'fwd' else (N, M, H, W, G, 3, 3, 1, 1, 1)


def inst(c):
    return (c.pass_, c.pk, c.shape[3])


def src_shape(c):
    N, G, H, W, M = c.shape
    return (N, G, H, W)


def out_shape(c):
    N, G, H, W, M = c.shape
    return (N, M, H, W)


def kp(c):
    return 9 * c.shape[1]


def packed_bytes(c):
    """what the library asks for: [pieces][M / 256][chunk x tap][32 x 256 bytes]; f16x2: + the row maxima (256-byte aligned); the
    bf16-piece data gradient: three row classes, of which the window kernel reads the first"""
    N, G, H, W, M = c.shape
    image = (M // 256) * (G // 16) * 9 * 32 * 256
    if c.pk == 'f16x2':
        return 2 * image + (4 * M + 255) // 256 * 256
    return (3 if c.pk == 'bf16x3' else 1) * image * (3 if c.pass_ == 'dgrad' else 1)


def tiles_per_image(c):
    return c.shape[2] // (128 // c.shape[3])


def fold_mask(fold, H, W):
    """(H, W) mask of one source class of the data gradient's sum entries"""
    rows = {'lo': (0, 2), 'hi': (H - 3, H - 1)}
    cols = {'lo': (0, 2), 'hi': (W - 3, W - 1)}
    m = torch.zeros(H, W, dtype=torch.bool)
    kind, which = fold.split('_')
    if kind == 'rows':
        m[list(rows[which])] = True
    elif kind == 'cols':
        m[:, list(cols[which])] = True
    else:
        side = {'l': 'lo', 'h': 'hi'}
        for r in rows[side[which[0]]]:
            for q in cols[side[which[1]]]:
                m[r, q] = True
    return m


# ---- data, reference, bound ------------------------------------------------------------------------------------------------------------------
def xlow(g, pk, shape, bits, wide):
    """the operand of an 'xlow' case that holds the low pieces: integers with one element pinned to 2^bits - 1.  bf16x3: 12-bit values,
    every 97th element `wide` bits (a non-zero third piece); 'xlow16': magnitudes <= 16 under the pinned one; else `bits` bits"""
    top = 2 ** bits - 1
    if pk == 'xlow16':
        t = _ints(g, -16, 16, shape)
    elif pk == 'bf16x3':
        t = _ints(g, -4095, 4095, shape)
        big = _ints(g, -(2 ** wide - 1), 2 ** wide - 1, shape)
        t = torch.where((torch.arange(t.numel()) % 97 == 5).view(t.shape), big, t)
    else:
        t = _ints(g, -top, top, shape)
    t.view(-1)[t.numel() // 2 + 3] = top
    return t


def wlow(g, shape, bits, wide):
    """the operand of a 'wlow' case that holds the low pieces: `bits`-bit integers, every 61st of `wide` bits where wide is set"""
    top = 2 ** bits - 1
    t = _ints(g, -top, top, shape)
    if wide:
        big = _ints(g, -(2 ** wide - 1), 2 ** wide - 1, shape)
        t = torch.where((torch.arange(t.numel()) % 61 == 7).view(t.shape), big, t)
    return t


def fold(which, N, G, H, W):
    """dy of a 'fold' case: zero except in ONE source class, where the sources of every sum entry hold distinct integers"""
    n_, k_, r_, q_ = torch.meshgrid(torch.arange(N), torch.arange(G), torch.arange(H), torch.arange(W), indexing='ij')
    v = (1 + (5 * r_ + 3 * q_ + 7 * k_ + 11 * n_) % 59).float() * (1 - 2 * (k_ % 2)).float()
    return v * fold_mask(which, H, W).view(1, 1, H, W).float()


@functools.lru_cache(maxsize=None)
def data(c):
    """(src, w, bias, addend, float64 reference BEFORE the activation and the addend, A, row exponents) of a case on the CPU: made once,
    shared, never written to.  w is the convolution's weight tensor [K][C][3][3] whatever the pass"""
    N, G, H, W, M = c.shape
    gm = geom(c)
    K, C = gm[4], gm[1]
    fwd = c.pass_ == 'fwd'
    g = torch.Generator().manual_seed(sum(v * (i + 1) * 7919 for i, v in enumerate(c.shape)) + 104729 * c.seed + (17 if fwd else 0)
                                      + 1299709 * KINDS.index(c.kind) + 15485863 * PKS.index(c.pk)
                                      + (32452843 * (1 + FOLDS.index(c.fold)) if c.fold else 0))
    rowexp, b, add = None, None, None
    if c.kind == 'signed':
        src, w = _signed(g, N, G, H, W), _signed(g, K, C, 3, 3) * 2.0 ** c.wexp
        if c.pk == 'bf16':
            src = (src * 32).round() / 32 if not fwd else _bf16(src)      # data gradient: the grid on which every sum entry is a bf16 number
            w = _bf16(w)
        b = _signed(g, M) if c.bias else None
        add = _signed(g, N, M, H, W) if c.add else None
    elif c.kind in ('xlow', 'xlow16'):
        src = xlow(g, 'xlow16' if c.kind == 'xlow16' else c.pk, (N, G, H, W), c.bits, c.wide)
        w = _ints(g, -1, 1, (K, C, 3, 3))
        b = _ints(g, -64, 64, (M,)) if c.bias else None
        add = _ints(g, -4096, 4096, (N, M, H, W)) if c.add else None
    elif c.kind == 'wlow':
        src = _ints(g, -1, 1, (N, G, H, W))
        w = wlow(g, (K, C, 3, 3), c.bits, c.wide)
        if c.pk == 'f16x2':
            rowexp = torch.randint(-20, 21, (M,), generator=g)
            rowexp[0], rowexp[1] = 20, -20
            mag = torch.pow(2.0, rowexp.float())
            w = w * (mag.view(K, 1, 1, 1) if fwd else mag.view(1, C, 1, 1))
        assert not c.bias and not c.add
    else:
        assert c.kind == 'fold' and not fwd and not c.bias and not c.add
        src = fold(c.fold, N, G, H, W)
        w = _ints(g, -3, 3, (K, C, 3, 3))
    ref, A = reference(c, src, w, b)
    if add is not None:
        A = A + add.double().abs()
    assert tuple(ref.shape) == out_shape(c)
    return Data(src, w, b, add, ref, A, rowexp)


def reference(c, src, w, b):
    """(float64 result before the activation, the same call on absolute values) of the case's geometry on the given operands"""
    return split_arith.reference(c.pass_, geom(c), src, w, b)


def slope_of(c):
    return split_arith.slope_of(c.kind)


def expected(c, ref=None):
    """act(ref) + addend in float64: what the call should produce"""
    d = data(c)
    out = R.activation(d.ref if ref is None else ref, c.act, slope_of(c))
    return out + d.add.double() if d.add is not None else out


def bounds(c, A=None, ref=None, pk=None):
    """(E of the accumulation, the bound on |y - expected|, expected) per element"""
    d = data(c)
    A = d.A if A is None else A
    pk = pk or c.pk
    want = expected(c, ref)
    if pk == 'f16x2':
        E = (2 * (3 * kp(c) + 8) * U + 2.0 ** -20) * A
    elif pk == 'bf16x3':
        E = (2 * (6 * kp(c) + 8) * U + 2.0 ** -24) * A
    else:
        E = 2 * (kp(c) + 8) * U * A
    bound = E + (2.0 ** -22 * want.abs() if c.act else 0.0)
    if pk == 'bf16':
        bound = bound + half_ulp_bf16(want.abs() + bound)
    return E, bound, want


def condition(c):
    """(largest bound of the case, what it has to stay under: half the smallest possible term)"""
    return float(bounds(c)[1].max()), TERM_MIN * 2.0 ** c.wexp / 2


def quanta(c):
    """exact kinds: the largest A of the case in units of its quantum (1, or 2^j of the row for 'wlow' on f16x2); must stay under 2^24"""
    return split_arith.quanta(data(c))


# ---- the kernel's arithmetic in torch --------------------------------------------------------------------------------------------------------
def window(c, src, wrong=None):
    """what the nine taps of every output pixel read, [N][G][H][W][3][3] in fp32.  forward: the reflection-padded input.  data gradient:
    dy with a ring of zeros, except that row 1 reads the sum dy[2] + dy[0] through tap 2 and row H-2 the sum dy[H-3] + dy[H-1] through
    tap 0, columns alike, corners four sources ((a + b) + (c + d) in fp32, as patch_write adds them).  wrong = (n, g, y, x, r, s): that ONE
    entry takes a neighbouring source row instead"""
    N, G, H, W = src.shape
    win = torch.zeros(N, G, H, W, 3, 3)
    if c.pass_ == 'fwd':
        xp = torch.nn.functional.pad(src, (1, 1, 1, 1), mode='reflect')
        for r in range(3):
            for s in range(3):
                win[..., r, s] = xp[:, :, r:r + H, s:s + W]
        if wrong is not None:
            n, g, y, x, r, s = wrong
            win[n, g, y, x, r, s] = xp[n, g, y + r, x + s + 1] if x + s + 1 < W + 2 else xp[n, g, y + r, x + s - 1]
        return win

    def sources(i, t, L):
        if i == 1 and t == 2:
            return (2, 0)
        if i == L - 2 and t == 0:
            return (L - 3, L - 1)
        j = i - 1 + t
        return (j,) if 0 <= j < L else ()

    def table(L):       # [L][3][2] source indices, L = the zero slot behind the tensor
        return torch.tensor([[(list(sources(i, t, L)) + [L, L])[:2] for t in range(3)] for i in range(L)])
    srcz = torch.nn.functional.pad(src, (0, 1, 0, 1))
    ri, ci = table(H).view(H, 1, 3, 1, 2), table(W).view(1, W, 1, 3, 2)
    at = lambda a, b: srcz[:, :, ri[..., a].expand(H, W, 3, 3), ci[..., b].expand(H, W, 3, 3)]
    win = (at(0, 0) + at(0, 1)) + (at(1, 0) + at(1, 1))      # r0: (c0 + c1), r1: (c0 + c1), then the two rows
    if wrong is not None:
        n, g, y, x, r, s = wrong
        assert y == 1 and r == 2 and 2 <= x < W - 2 and s == 1, 'the wrong source is written for the sum row {2, 0}'
        win[n, g, y, x, r, s] = src[n, g, 2, x] + src[n, g, 1, x]      # row 1 where row 0 belongs
    return win


def weight_matrix(c, w):
    """[produced][gathered][3][3] as the taps of `window` meet it: the forward weights, or the flipped and transposed ones"""
    return w if c.pass_ == 'fwd' else w.flip(2, 3).transpose(0, 1).contiguous()


def emulate(c, perturb=None):
    """scale, window, split, the piece products of the form each summed exactly and accumulated in fp32, scale back per row, bias,
    activation, addend -- as float64 for the comparison.  perturb: 'zero_low' zeroes ONE entry of the lowest piece that has a non-zero
    one (of the window for 'xlow', of the weights for 'wlow'); 'wrong_source' lets ONE window entry read a neighbouring source; 'shift_tap' moves ONE high
    weight piece to the neighbouring tap.  Returns (result, lowest pieces of window and weights)"""
    d = data(c)
    N, G, H, W, M = c.shape
    dg = c.pass_ == 'dgrad'
    wrong = None
    if perturb == 'wrong_source':
        if dg:
            pick = torch.nonzero(d.src[0, :, 0, 2:W - 2] != d.src[0, :, 1, 2:W - 2])
            assert pick.numel() > 0, 'rows 0 and 1 do not differ anywhere'
            wrong = (0, int(pick[0][0]), 1, int(pick[0][1]) + 2, 2, 1)
        else:
            pick = torch.nonzero(d.src[0, :, 1, 1:W - 1] != d.src[0, :, 1, 2:W])
            wrong = (0, int(pick[0][0]), 0, int(pick[0][1]) + 1, 0, 1)      # the mirror row -1 = row 1, one column to the right
    win = window(c, d.src, wrong)
    wm = weight_matrix(c, d.w)
    sx, sw = 1.0, torch.ones(M)
    if c.pk == 'f16x2':
        sx = pow2_scale(float(d.src.abs().max()))
        sw = torch.tensor([pow2_scale(float(v)) for v in wm.abs().amax(dim=(1, 2, 3))])
        xp, wp = list(split2h(win * sx, sums=dg)), list(split2h(wm * sw.view(M, 1, 1, 1)))
        pairs = ((1, 0), (0, 1), (0, 0))                   # (weight piece, window piece): (l,h) (h,l) (h,h)
    elif c.pk == 'bf16x3':
        xp, wp = split3(win), split3(wm)
        pairs = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
    else:
        xp, wp = [_bf16(win)], [_bf16(wm)]
        pairs = ((0, 0),)
    if perturb == 'zero_low':
        low = [t for t in (wp if c.kind == 'wlow' else xp)[1:] if bool((t != 0).any())]
        assert low, 'no non-zero low piece to drop'
        t = low[-1]
        nz = torch.nonzero(t.view(-1))
        t.view(-1)[int(nz[nz.numel() // 2])] = 0.0
    elif perturb == 'shift_tap':
        m, g_ = M // 2, G // 2
        flat = wp[0][m, g_].view(-1)
        nz = torch.nonzero(flat != flat.roll(1))
        i = int(nz[0])
        wp[0] = wp[0].clone()
        wp[0][m, g_].view(-1)[i] = wp[0][m, g_].view(-1)[i - 1]

    def piece(a, b):
        r = (a.permute(0, 2, 3, 1, 4, 5).reshape(N * H * W, G * 9).double() @ b.reshape(M, G * 9).double().t())
        assert bool((r.float().double() == r).all()), 'a piece sum is no fp32 number'
        return r.float().view(N, H, W, M).permute(0, 3, 1, 2)
    acc = None
    for pa, pb in pairs:
        p = piece(xp[pb], wp[pa])
        acc = p if acc is None else acc + p
    y = (acc * (1.0 / sx)) * (1.0 / sw).view(1, -1, 1, 1) if c.pk == 'f16x2' else acc
    if d.b is not None:
        y = y + d.b.view(1, -1, 1, 1)
    y = R.activation(y, c.act, slope_of(c))
    if d.add is not None:
        y = y + d.add
    if c.pk == 'bf16':
        y = _bf16(y)
    return y.double(), (xp[-1], wp[-1])


def exact_expected(c):
    """section B: the float64 result as the call stores it (bf16 tensors: rounded to nearest-even once)"""
    want = expected(c)
    if c.pk == 'bf16':
        assert bool((want.float().double() == want).all())
        return _bf16(want.float()).double()
    return want


# ---- section C ---------------------------------------------------------------------------------------------------------------------------
RANGE_KINDS = ('wide_range', 'huge', 'tiny')


def range_data(c, kind):
    """randn operands under the kinds of tests/test_gpu_bf16x6.py; returns (src, w, float64 reference)"""
    N, G, H, W, M = c.shape
    gm = geom(c)
    g = torch.Generator().manual_seed(2000 + RANGE_KINDS.index(kind) + (17 if c.pass_ == 'fwd' else 0) + W)
    src = torch.randn(N, G, H, W, generator=g)
    w = torch.randn(gm[4], gm[1], 3, 3, generator=g) * 0.05
    # wide_range: magnitudes over twelve decades inside one tensor
    src, w = range_scale(kind, g, src, w, (12, -9), (6, -3), (1e-30, 1e-6), (1e12, 1e8))
    f = _fwd64 if c.pass_ == 'fwd' else _dgrad64
    return src, w, f(src.double(), w.double(), None, gm)


MAXPOS_N = (1, 2, 3, 4, 5, 7, 2047, 2048, 2049, 8192, 8200, 8203)


def maxima_slots(n):
    """split_arith.maxima_slots at NT = 512: from 4 NT = 2048 slots on the end of the first 4-in-flight round, from 16 NT = 8192 on the
    second and the third load in flight"""
    return split_arith.maxima_slots(n, NT)


def corner_data(c, which):
    """the four-corner overflow of the f16x2 data gradient.  'constant': dy = 1 - 2^-13 everywhere (four sources of a corner sum entry
    scale to 4 x 16382 = 65528 under pow2_scale(max): over fp16's 65504).  'one_plane': only the four sources of each corner entry of ONE
    plane sit at the tensor's maximum, everything else is 2^-6 of it.  Returns (dy, w, ref, A)"""
    N, G, H, W, M = c.shape
    assert c.pass_ == 'dgrad' and c.pk == 'f16x2'
    g = torch.Generator().manual_seed(4242 + W)
    w = _signed(g, geom(c)[4], geom(c)[1], 3, 3)
    top = 1.0 - 2.0 ** -13
    if which == 'constant':
        dy = torch.full((N, G, H, W), top)
    else:
        dy = _signed(g, N, G, H, W) * 2.0 ** -6
        for r in (0, 2, H - 3, H - 1):
            for q in (0, 2, W - 3, W - 1):
                dy[N - 1, G // 2, r, q] = top
    ref, A = reference(c, dy, w, None)
    return dy, w, ref, A


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
CASES = []
XLOW_BITS = {('f16x2', 'fwd'): 15, ('f16x2', 'dgrad'): 13, ('bf16x3', 'fwd'): 23, ('bf16x3', 'dgrad'): 22, ('bf16', 'fwd'): 8, ('bf16', 'dgrad'): 6}
WLOW_BITS = {'f16x2': 15, 'bf16x3': 15, 'bf16': 8}


def _add(sect, pass_, pk, shape, act=0, bias=False, add=False, wexp=0, kind='signed', bits=0, wide=0, fold='', seed=0):
    name = '%s-%s-%dx%dx%dx%d-m%d%s%s%s%s%s' % ((pass_, pk) + shape + (
        '-bias' if bias else '', '-' + ACT_NAMES[act] if act else '', '-add' if add else '',
        '' if kind == 'signed' else '-%s%s' % (kind, ('_' + fold) if fold else (str(bits) + ('w%d' % wide if wide else ''))), '-s%d' % seed if seed else ''))
    CASES.append(Case(sect, name, pass_, pk, shape, act, bias, add, wexp, kind, bits, wide, fold, seed))


# A. lost, doubled or misplaced terms: every instantiation on the first shape of its width and on the three-tile shape of each width
for _pk in PKS:
    _add('A', 'fwd', _pk, S_ONE, act=1, bias=True)
    _add('A', 'fwd', _pk, S_W64, act=2, bias=True)
    _add('A', 'fwd', _pk, S_W64_3)
    _add('A', 'fwd', _pk, S_W32_3, bias=True)
    for _s in (S_ONE, S_W64, S_W64_3, S_W32_3):
        _add('A', 'dgrad', _pk, _s)
# f16x2: tanh and sigmoid, two chunk pairs and two weight tiles, the data gradient with a signed addend on every shape
_add('A', 'fwd', 'f16x2', S_ONE, act=3, bias=True, wexp=-5)
_add('A', 'fwd', 'f16x2', S_W64, act=4, bias=True, wexp=-5)
_add('A', 'fwd', 'f16x2', S_PAIRS2, act=1, bias=True)
_add('A', 'dgrad', 'f16x2', S_PAIRS2)
for _s in (S_ONE, S_W64, S_W64_3, S_W32_3, S_PAIRS2):
    _add('A', 'dgrad', 'f16x2', _s, add=True)

# B. exact pieces
for _pk in PKS:
    _wd = 20 if _pk == 'bf16x3' else 0
    _bf, _bd = XLOW_BITS[(_pk, 'fwd')], XLOW_BITS[(_pk, 'dgrad')]
    _add('B', 'fwd', _pk, S_ONE, act=1, bias=True, kind='xlow', bits=_bf, wide=_wd)
    _add('B', 'fwd', _pk, S_W64, act=2, bias=True, kind='xlow', bits=_bf, wide=_wd)
    _add('B', 'fwd', _pk, S_PAIRS2, bias=True, kind='xlow', bits=_bf, wide=_wd)
    _add('B', 'fwd', _pk, S_PAIRS3, kind='xlow', bits=_bf, wide=_wd)
    _add('B', 'dgrad', _pk, S_ONE, kind='xlow', bits=_bd, wide=_wd)
    _add('B', 'dgrad', _pk, S_W64, kind='xlow', bits=_bd, wide=_wd, add=_pk == 'f16x2')
    _add('B', 'dgrad', _pk, S_PAIRS2, kind='xlow', bits=_bd, wide=_wd)
    _add('B', 'dgrad', _pk, S_PAIRS3, kind='xlow', bits=_bd, wide=_wd)
    for _pass in ('fwd', 'dgrad'):
        for _s in (S_ONE, S_W64, S_PAIRS3):
            _add('B', _pass, _pk, _s, kind='wlow', bits=WLOW_BITS[_pk] - (1 if _s == S_PAIRS3 and _pk != 'bf16' else 0))      # (864 terms: A < 2^24)
    for _s in (S_ONE, S_W32_3, S_W64, S_W64_3):      # H = 4 and three tiles per image, both widths
        for _f in FOLDS:
            _add('B', 'dgrad', _pk, _s, kind='fold', fold=_f)
_add('B', 'fwd', 'bf16x3', S_ONE, kind='wlow', bits=15, wide=19)
_add('B', 'dgrad', 'bf16x3', S_W64, kind='wlow', bits=15, wide=19)

BY_NAME = collections.OrderedDict(('%s.%s' % (c.sect, c.name), c) for c in CASES)
assert len(BY_NAME) == len(CASES), 'case names must be unique'

# section C (f16x2): the case whose maxima array the test builds by hand (every magnitude but the pinned one is <= 16), the range cases,
# the corner cases
MAXPOS = {'fwd': Case('C', 'maxpos-fwd', 'fwd', 'f16x2', S_ONE, 1, True, False, 0, 'xlow16', 15, 0, '', 0),
          'dgrad': Case('C', 'maxpos-dgrad', 'dgrad', 'f16x2', S_ONE, 0, False, False, 0, 'xlow16', 13, 0, '', 0)}
RANGE = {(p, w): Case('C', 'range-%s-%d' % (p, w), p, 'f16x2', S_ONE if w == 32 else S_W64, 0, False, False, 0, 'signed', 0, 0, '', 0)
         for p in ('fwd', 'dgrad') for w in (32, 64)}
CORNER = {w: Case('C', 'corner-%d' % w, 'dgrad', 'f16x2', S_ONE if w == 32 else S_W64_3, 0, False, False, 0, 'signed', 0, 0, '', 0) for w in (32, 64)}
