"""Case table, data makers, float64 reference, bounds, the host restated and an arithmetic emulation of the per-tap bf16-piece convolution
(csrc/bsplit_conv.hip: bsplit_conv_fwd_kernel<MODE, BM, NP, TA>, its packs, padded copy and split reduce in csrc/bsplit_pack.hip, the host
in csrc/bf16x6_conv.hip).  A plain module, CPU only, no library load at import: shared by tests/test_bsplit_cases.py, which checks the
table, the emulation and the restated host on the CPU, and tests/test_gpu_bsplit_cases.py, which runs it.

Sixteen instantiations: mode in ('fwd_zero', 'fwd_reflect', 'dgrad', 'wgrad') x BM in (128, 256) x piece form in ('bf16x3': fp32 tensors
as three bf16 pieces, six products; 'bf16': bf16 tensors as they are, one product).  A case is one direct call of the C-ABI
(pcgan_conv2d_bsplit_pack + _fwd_bsplit | _bsplit_dgrad_pack + _bwd_data_bsplit | _bwd_weight_bsplit) on the CONVOLUTION's geometry
(N, C, H, W, K, R, S, 1, pad, pad_mode) under the library options of the case (`opts`: only "bsplit_halo").  `want` is the launch record
(pcgan_bsplit_last_launch without the sequence number: RECORD) the case is there to hit; `plan` -- the host restated: bsplit_refusal, the
two other predicates, halo_geometry and the option, bsplit_bm, pack_geom, the three pixel-tile runs of the data gradient,
bsplit_wgrad_splits, the workspace, pad_copy_form -- must reproduce it, and `claims` are the predicates of CLAIMS the case is there for.

Section A, kind 'signed' (conv_f32_cases._signed): magnitudes in [0.75, 1.25] with random signs; tanh / sigmoid cases multiply the weights
by 2^wexp.  Reference: split_arith.reference in float64 (autograd through the reflection), split_arith.wgrad64 for the weight gradient;
the same call on absolute values gives A.  Kp = terms per element (forward C R S, data gradient 9 K, weight gradient N H W), s = splits of
the weight gradient (0 otherwise).  Per element:
  bf16x3                      |y - want| <= (2 (6 Kp + s + 8) 2^-24 + 2^-24) A: the derivation of tests/halo_cases.py -- x = h + m + l exactly,
                              six products per term, each exact in fp32, the dropped pairs under 2^-25 of the term; 6 Kp additions
                              bounded with the factor 2 of conv_f32_cases; the 8 covers the bias, the fp32 mirror sum b + b2 and folded
                              weight of the data gradient, the reduce over the splits is s.
  bf16, forward / data grad.  the _bf16_bound form of tests/test_gpu_hgemm.py with E = 2 (Kp + 8) 2^-24 A:
                              2^-8 (|want| + E) + E + 2^-22 |want| + 1e-30 -- every product exact, Kp additions, ONE rounding of the store.
  bf16, weight gradient       2 (Kp + s + 8) 2^-24 A only: the output is fp32 and every product is exact.
Fused activations (1-Lipschitz) add 2^-22 |act(ref)|.
The rounding order of the bf16 data gradient is the kernel's contract: the column-mirror sum b + b2 of the two dy elements is formed in
fp32 and rounded to bf16 ONCE (stash), and the folded row-class weight w[2-r'] + w[r'] is formed in fp32 and rounded to bf16 ONCE (the
pack).  The bf16 data-gradient cases of section A put |dy| and |w| on the grid 2^-5: sums of two such values up to 2.5 are multiples of
2^-5 below 2^7 of them, i.e. bf16 numbers, so both roundings are exact (asserted on the CPU) and the bound has no term for them.
Condition (CPU, and again before each launch): the largest bound of the case is under TERM_MIN 2^wexp / 2, half the smallest possible
term -- one lost, doubled or shifted term in any element fails.  It caps bf16x3 cases at Kp <= 448, bf16-output cases at 16 gathered
channels x 9 taps (2^-8 |ref| must stay under it: |ref| < 72), the bf16 weight gradient only by the fp32 term count; the 5x5 case on 16
channels (400 terms) and the two option cases (288 terms) are in section A with fp32 tensors only.

Section B, exact data: every partial sum is an integer below 2^24 (asserted per case on A), so every order of fp32 accumulation is exact
and the gate is out == ref in every element (bf16 forward / data gradient: == the round-to-nearest-even bf16 of the exact integer).
  'xlow'  the gathered operand holds the low pieces (halo_cases.xlow: bf16x3 12-bit values, every 97th 20 bits, one pinned to 2^23 - 1,
          2^22 - 1 in the data gradient where two sources are summed before the split; bf16 8 bits, 6 in the data gradient), the other
          operand in {-1, 0, 1}; weight gradient: the low pieces in x.
  'wlow'  halo_cases.wlow in the weights (bf16x3 15 bits, every 61st 19: a third piece; bf16 8 bits, 7 in the data gradient so that the
          folded weight stays a bf16 number); weight gradient: in dy, which bsplit_pack_dy_kernel splits.
  'mid'   bf16x3, the 16- and 32-channel 1x1 shapes: both operands 9-bit integers, so both have a middle piece and (m, m) carries bits.
  'fold'  data gradient: halo_cases.fold, dy zero except in one of the eight source classes FOLDS, weights in [-3, 3].  Here the row fold
          lives in the packed weights and the column fold in offT[9 + t]: a corner class exercises both at once.
  The accumulate case adds into an integer base.

Section C, operand ranges (bf16x3; the form has no scaling): randn operands under 'relu_normal', 'wide_range', 'huge' and 'tiny' on one
shape per pass; 'tiny' keeps the smallest kept piece product (2^-16 of a term and less) a normal fp32 number, 'tiny2' is one step further
down (products below 2^-126) and is recorded, not gated.

`emulate` restates the kernel's arithmetic in torch: split3, the gather (zero ring or mirror; data gradient: zero ring, the three row
classes with their folded weights, the column-mirror sum before the split, rounded once for bf16 tensors), the six products in the kernel's
order (l,h) (h,l) (m,m) (m,h) (h,m) (h,h) accumulated in fp32 stage by stage in K order (16-channel chunk, tap, channel), the weight
gradient's partial sums split by split and bsplit_wgrad_reduce_kernel's two-accumulator order, bias, activation, the bf16 store.
PERTURBATIONS are faults applied to `emulate` only -- a kernel made wrong on purpose is never run on a GPU."""
import collections
import functools

import torch

from oracle import ops_ref as R
import split_arith
from conv_f32_cases import _signed, TERM_MIN
from halo_cases import xlow, wlow, fold, FOLDS, XLOW_BITS, WLOW_BITS
from split_arith import U, _ints, _bf16, cdiv, out_size, split3, per_row_rel, range_scale, wgrad64      # (per_row_rel: for the tests)

MODES = ('fwd_zero', 'fwd_reflect', 'dgrad', 'wgrad')       # BS_FWD_ZERO, BS_FWD_REFLECT, BS_DGRAD_REFLECT, BS_WGRAD
PKS = ('bf16x3', 'bf16')
INSTANTIATIONS = tuple((m, bm, pk) for m in MODES for bm in (128, 256) for pk in PKS)
ACT_NAMES = ('none', 'relu', 'lrelu', 'tanh', 'sigmoid')
KINDS = ('signed', 'xlow', 'wlow', 'fold', 'relu_normal', 'wide_range', 'huge', 'tiny', 'tiny2', 'mid')
OPTIONS = {'bsplit_halo': 1}      # the library's default
RECORD = ('kernel', 'mode', 'bm', 'dtype', 'row_tiles', 'tiles', 'stages', 'splits', 'stages_per_split', 'copy')
MAXTAP = 25
PER_TAP, WINDOW = 0, 1

Case = collections.namedtuple('Case', 'sect name pass_ geom pk act bias wexp kind bits wide fold acc opts want claims seed')
# src: the gathered tensor (x | dy | x); w: the weights [K][C][R][S] (weight gradient: dy); base: what accumulate = 1 adds into
Data = collections.namedtuple('Data', 'src w b base ref A')
Plan = collections.namedtuple('Plan', RECORD + ('packed_bytes', 'ws_bytes', 'tstart', 'here', 'rows', 'chan', 'taps', 'Ptot', 'P', 'Q'))


def options(opts):
    o = dict(OPTIONS)
    o.update(dict(opts))
    assert sorted(o) == sorted(OPTIONS), opts
    return o


# ---- the host, restated ----------------------------------------------------------------------------------------------------------------------
def refusal(geom):
    """bsplit_refusal: 0 takes, 2 shape, 3 reflection pad too large, 4 beyond 2 GiB"""
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    if not (st == 1 and C % 16 == 0 and Rr * S <= MAXTAP and K >= 32):
        return 2
    if not (pm == 0 or (pad < H and pad < W)):
        return 3
    if not N * C * H * W * 4 < 2 ** 31:
        return 4
    return 0


def dgrad_supported(geom):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    return (st == 1 and pm == 1 and pad == 1 and Rr == 3 and S == 3 and K % 16 == 0 and C >= 32 and H >= 4 and W >= 4
            and N * K * H * W * 4 < 2 ** 31)


def bm_of(rows):
    return 256 if rows % 256 == 0 else 128


def wgrad_supported(geom):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    return (st == 1 and pm == 1 and Rr == 3 and S == 3 and pad == 1 and W % 16 == 0 and K in (128, 256)
            and N * C * (H + 2) * (W + 2) * 4 < 2 ** 31 and N * H * W * 3 * 2 * bm_of(K) < 2 ** 31)


def supported(pass_, geom):
    return {'fwd': lambda: refusal(geom) == 0, 'dgrad': lambda: dgrad_supported(geom), 'wgrad': lambda: wgrad_supported(geom)}[pass_]()


def halo_geometry(chan, rows_out, H, W):
    return W in (32, 64) and H >= 4 and H % (128 // W) == 0 and chan % 32 == 0 and rows_out % 256 == 0


def pad_copy_form(planes, H, W, pad):
    Hp, Wp = H + 2 * pad, W + 2 * pad
    return 2 if (Wp % 2 == 0 and Wp <= 128 and Hp * Wp <= 8192 and planes >= 1024) else 1


def wgrad_splits(geom, bm):
    """bsplit_wgrad_splits: (splits, stages per split)"""
    N, C, H, W, K = geom[:5]
    nst = N * H * W // 16
    tiles = cdiv(C * 9, 128) * cdiv(K, bm)
    want = max(1, (256 if bm == 256 else 512) // tiles)
    if want > nst // 8:
        want = max(1, nst // 8)
    per = cdiv(nst, want)
    return cdiv(nst, per), per


def _up256(v):
    return cdiv(v, 256) * 256


def plan_of(pass_, geom, pk, opts=()):
    """what the entry point of the pass launches for a supported call: the record, the sizes it names, and what the claims read"""
    o = options(opts)
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    assert supported(pass_, geom), (pass_, geom)
    np_, dt = (3, 0) if pk == 'bf16x3' else (1, 1)
    P, Q = out_size(H, Rr, 1, pad), out_size(W, S, 1, pad)
    T = Rr * S
    if pass_ == 'wgrad':
        bm = bm_of(K)
        nMt, nst = cdiv(K, bm), N * H * W // 16
        splits, per = wgrad_splits(geom, bm)
        ws = _up256(N * C * (H + 2) * (W + 2) * 4) + _up256(3 * nMt * nst * 32 * bm) + splits * nMt * bm * C * 9 * 4
        here = tuple(min(per, nst - s * per) for s in range(splits))
        return Plan(PER_TAP, 3, bm, dt, nMt, cdiv(C * 9, 128), nst, splits, per, pad_copy_form(N * C, H, W, 1), 0, ws, (), here, K, N * H * W, 9,
                    C * 9, P, Q)
    rows, chan = (K, C) if pass_ == 'fwd' else (C, K)
    bm = bm_of(rows)
    nMt, nst = cdiv(rows, bm), chan // 16 * T
    image = np_ * nMt * nst * 32 * bm
    packed = image if pass_ == 'fwd' else 3 * image
    window = o['bsplit_halo'] != 0 and halo_geometry(chan, rows, H, W) and (pass_ == 'dgrad' or (pm == 1 and T == 9 and Rr == 3 and pad == 1))
    if window:
        return Plan(WINDOW, 0 if pass_ == 'fwd' else 1, 256, dt, cdiv(rows, 256), N * H * W // 128, nst, 1, nst, 0, packed, 0, (), (nst,), rows, chan, T,
                    N * H * W, P, Q)
    if pass_ == 'fwd':
        return Plan(PER_TAP, 1 if pm == 1 else 0, bm, dt, nMt, cdiv(N * P * Q, 128), nst, 1, nst, 0, packed, 0, (), (nst,), rows, chan, T, N * P * Q, P, Q)
    tstart, t = [], 0
    for r in (H - 2, 1, 1):
        tstart.append(t)
        t += cdiv(N * r * W, 128)
    return Plan(PER_TAP, 2, bm, dt, nMt, t, nst, 1, nst, 0, packed, 0, tuple(tstart) + (t,), (nst,), rows, chan, T, N * H * W, P, Q)


def plan(case):
    return plan_of(case.pass_, case.geom, case.pk, case.opts)


def record(pl):
    return tuple(pl[:len(RECORD)])


def inst(case):
    w = dict(zip(RECORD, case.want))
    return (MODES[w['mode']], w['bm'], case.pk)


def kp(case):
    N, C, H, W, K, Rr, S = case.geom[:7]
    return {'fwd': C * Rr * S, 'dgrad': 9 * K, 'wgrad': N * H * W}[case.pass_]


class _View(object):
    """a Plan plus the fields of the case that the claims read"""

    def __init__(self, case):
        self.__dict__.update(plan(case)._asdict())
        self.N, self.C, self.H, self.W, self.K, self.R, self.S, self.st, self.pad, self.pm = case.geom
        self.pass_, self.pk, self.acc, self.opts = case.pass_, case.pk, case.acc, options(case.opts)
        self.fwd, self.dg, self.wg = case.pass_ == 'fwd', case.pass_ == 'dgrad', case.pass_ == 'wgrad'
        self.per_tap = self.kernel == PER_TAP
        self.PQ = self.P * self.Q
        self.phase_pixels = (self.N * (self.H - 2) * self.W, self.N * self.W, self.N * self.W) if self.dg else ()
        self.starts = tuple(s * self.stages_per_split for s in range(self.splits))


CLAIMS = {
    # pipeline: global loads three stages ahead, stage pair unrolled
    'nst_1': lambda v: v.fwd and v.stages == 1 and v.taps == 1 and v.chan == 16,
    'nst_2': lambda v: v.fwd and v.stages == 2 and v.taps == 1,
    'nst_3': lambda v: v.fwd and v.stages == 3 and v.taps == 1,
    'nst_4': lambda v: v.fwd and v.stages == 4 and v.taps == 1,
    'nst_5': lambda v: v.fwd and v.stages == 5 and v.taps == 1 and v.chan == 80,
    'nst_9_dead_stage': lambda v: v.fwd and v.stages == 9,
    'nst_25_maxtap': lambda v: v.fwd and v.stages == 25 and v.taps == MAXTAP,
    # pixel tiles
    'ptot_under_128': lambda v: v.fwd and v.Ptot < 128 and v.tiles == 1,
    'ptot_ragged_tiles': lambda v: v.fwd and v.Ptot % 128 != 0 and v.tiles >= 2,
    'tile_crosses_image': lambda v: v.fwd and v.PQ % 128 != 0 and v.N > 1 and v.Ptot > v.PQ and v.PQ < 128,
    'one_full_tile': lambda v: v.fwd and v.Ptot == 128 and v.tiles == 1,
    # row tiles
    'm_32': lambda v: not v.wg and v.rows == 32 and v.bm == 128,
    'm_40_ragged': lambda v: not v.wg and v.rows == 40 and v.bm == 128 and v.row_tiles == 1,
    'm_384_three_tiles': lambda v: v.rows == 384 and v.bm == 128 and v.row_tiles == 3,
    'm_256': lambda v: not v.wg and v.rows == 256 and v.bm == 256 and v.row_tiles == 1,
    'm_512_two_tiles': lambda v: not v.wg and v.rows == 512 and v.bm == 256 and v.row_tiles == 2,
    # padding
    'zero_pad_1_four_sides': lambda v: v.fwd and v.pm == 0 and v.pad == 1 and v.R == 3 and v.S == 3 and v.H >= 2 and v.W >= 2,
    'pad_0_valid': lambda v: v.fwd and v.pad == 0 and v.R == 3 and v.P == v.H - 2,
    'reflect_3x3_window_refuses': lambda v: v.fwd and v.pm == 1 and v.pad == 1 and v.R == 3 and v.opts['bsplit_halo'] == 1 and v.per_tap
    and not halo_geometry(v.chan, v.rows, v.H, v.W),
    'reflect_5x5_pad_h_minus_1': lambda v: v.fwd and v.pm == 1 and v.R == 5 and v.pad == 2 and (v.H, v.W) == (3, 5),
    # data gradient
    'dgrad_4x4': lambda v: v.dg and v.per_tap and v.H == 4 and v.W == 4,
    'dgrad_phases_1_2_under_128': lambda v: v.dg and v.per_tap and v.phase_pixels[1] < 128,
    'dgrad_phase0_three_tiles_ragged': lambda v: v.dg and v.per_tap and v.tstart[1] >= 3 and v.phase_pixels[0] % 128 != 0 and v.tstart[:3] == (0, v.tstart[1], v.tstart[1] + 1),
    'dgrad_odd_h_w': lambda v: v.dg and v.per_tap and v.H % 2 == 1 and v.W % 2 == 1,
    'dgrad_c_256': lambda v: v.dg and v.per_tap and v.C == 256 and v.bm == 256,
    'dgrad_c_512': lambda v: v.dg and v.per_tap and v.C == 512 and v.bm == 256 and v.row_tiles == 2,
    # weight gradient
    'wgrad_one_split': lambda v: v.wg and v.stages < 16 and v.splits == 1,
    'wgrad_three_odd_splits': lambda v: v.wg and v.stages == 27 and v.here == (9, 9, 9),
    'wgrad_ragged_last_split': lambda v: v.wg and v.stages == 28 and v.here == (10, 10, 8) and any(s * 16 % (v.H * v.W) for s in v.starts[1:]),
    'wgrad_ragged_column_tile': lambda v: v.wg and v.C * 9 % 128 != 0,
    'wgrad_k_128': lambda v: v.wg and v.K == 128 and v.bm == 128,
    'wgrad_k_256': lambda v: v.wg and v.K == 256 and v.bm == 256,
    'wgrad_accumulate': lambda v: v.wg and v.acc == 1,
    'wgrad_wave_copy': lambda v: v.wg and v.N * v.C >= 1024 and v.copy == 2,
    'wgrad_element_copy': lambda v: v.wg and v.copy == 1,
    # option
    'option_fwd': lambda v: v.fwd and v.opts['bsplit_halo'] == 0 and v.per_tap and halo_geometry(v.chan, v.rows, v.H, v.W) and v.pm == 1,
    'option_dgrad': lambda v: v.dg and v.opts['bsplit_halo'] == 0 and v.per_tap and halo_geometry(v.chan, v.rows, v.H, v.W),
}
# claims that bf16 tensors cannot meet in section A (the condition: see the docstring)
A_FP32_ONLY = {'nst_25_maxtap', 'reflect_5x5_pad_h_minus_1', 'option_fwd', 'option_dgrad'}


def claims_of(case):
    v = _View(case)
    return frozenset(k for k, f in CLAIMS.items() if f(v))


# ---- data, reference, bounds -----------------------------------------------------------------------------------------------------------------
def src_shape(case):
    N, C, H, W, K = case.geom[:5]
    return (N, K, H, W) if case.pass_ == 'dgrad' else (N, C, H, W)


def out_shape(case):
    N, C, H, W, K, Rr, S = case.geom[:7]
    pl = plan(case)
    return {'fwd': (N, K, pl.P, pl.Q), 'dgrad': (N, C, H, W), 'wgrad': (K, C, 3, 3)}[case.pass_]


def reference(case, src, w, b=None):
    """(float64 result before the activation and the base, the same call on absolute values)"""
    if case.pass_ == 'wgrad':
        return wgrad64(src, w, case.geom), wgrad64(src.abs(), w.abs(), case.geom)
    return split_arith.reference(case.pass_, case.geom, src, w, b)


def _grid5(t):
    return (t * 32).round() / 32


@functools.lru_cache(maxsize=None)
def data(c):
    """the operands of a case on the CPU, its float64 reference and A: made once, shared, never written to"""
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    g = torch.Generator().manual_seed(sum(v * (i + 1) * 7919 for i, v in enumerate(c.geom)) + 104729 * c.seed + 17 * ('fwd', 'dgrad', 'wgrad').index(c.pass_)
                                      + 1299709 * KINDS.index(c.kind) + 15485863 * PKS.index(c.pk) + (32452843 * (1 + FOLDS.index(c.fold)) if c.fold else 0))
    wg, half = c.pass_ == 'wgrad', c.pk == 'bf16'
    ss = src_shape(c)
    ws = (N, K, H, W) if wg else (K, C, Rr, S)
    nb = K if c.pass_ == 'fwd' else C
    b = base = None
    if c.kind == 'signed':
        src, w = _signed(g, *ss), _signed(g, *ws) * 2.0 ** c.wexp
        if half:
            src, w = (_grid5(src), _grid5(w)) if c.pass_ == 'dgrad' else (_bf16(src), _bf16(w))
        b = _signed(g, nb) if c.bias else None
        base = _signed(g, K, C, 3, 3) if c.acc else None
    elif c.kind == 'xlow':
        src = xlow(g, c.pk, ss, c.bits, c.wide)
        w = _ints(g, -1, 1, ws)
        b = _ints(g, -64, 64, (nb,)) if c.bias else None
        base = _ints(g, -4096, 4096, (K, C, 3, 3)) if c.acc else None
    elif c.kind == 'wlow':
        src = _ints(g, -1, 1, ss)
        w = wlow(g, ws, c.bits, c.wide)
        base = _ints(g, -4096, 4096, (K, C, 3, 3)) if c.acc else None
        assert not c.bias
    elif c.kind == 'mid':
        src, w = _ints(g, -511, 511, ss), _ints(g, -511, 511, ws)
        b = _ints(g, -64, 64, (nb,)) if c.bias else None
    elif c.kind == 'fold':
        assert c.pass_ == 'dgrad' and not c.bias
        src = fold(c.fold, *ss)
        w = _ints(g, -3, 3, ws)
    else:      # section C: randn under a range kind
        assert c.pk == 'bf16x3' and not c.bias and not c.acc
        src = torch.randn(ss, generator=g)
        w = torch.randn(ws, generator=g) * (1.0 if wg else 0.05)
        if c.kind == 'relu_normal':
            src = src.relu() if c.pass_ != 'dgrad' else src
            w = w * 0.05 if wg else w
        elif c.kind == 'tiny2':
            src, w = src * 1e-19, w * 1e-15
        else:
            src, w = range_scale(c.kind, g, src, w, (12, -9), (6, -3), (1e-10, 1e-10), (1e12, 1e8))
    assert not (c.bias and c.pass_ != 'fwd') and not (c.acc and not wg)
    ref, A = reference(c, src, w, b)
    if base is not None:
        A = A + base.double().abs()
    assert tuple(ref.shape) == out_shape(c)
    return Data(src, w, b, base, ref, A)


def slope_of(c):
    return split_arith.slope_of(c.kind)


def expected(c):
    """act(ref) (+ the base of accumulate = 1) in float64: what the call should produce"""
    d = data(c)
    out = R.activation(d.ref, c.act, slope_of(c))
    return out + d.base.double() if d.base is not None else out


def exact_expected(c):
    """section B: the result as the call stores it (bf16 forward / data gradient: rounded to nearest-even once)"""
    want = expected(c)
    assert bool((want.float().double() == want).all())
    return _bf16(want.float()).double() if c.pk == 'bf16' and c.pass_ != 'wgrad' else want


def bounds(c):
    """(E of the accumulation, the bound on |y - expected|, expected) per element"""
    d = data(c)
    want = expected(c)
    s = plan(c).splits if c.pass_ == 'wgrad' else 0
    if c.pk == 'bf16x3':
        E = (2 * (6 * kp(c) + s + 8) * U + 2.0 ** -24) * d.A
        return E, E + (2.0 ** -22 * want.abs() if c.act else 0.0), want
    if c.pass_ == 'wgrad':
        E = 2 * (kp(c) + s + 8) * U * d.A
        return E, E, want
    E = 2 * (kp(c) + 8) * U * d.A
    return E, 2.0 ** -8 * (want.abs() + E) + E + 2.0 ** -22 * want.abs() + 1e-30, want


def condition(c):
    """(largest bound of the case, what it has to stay under: half the smallest possible term)"""
    return float(bounds(c)[1].max()), TERM_MIN * 2.0 ** c.wexp / 2


def quanta(c):
    return float(data(c).A.max())


def gate(c, out):
    """(passes, max |err| / bound -- section B: the number of unequal elements; section C: the largest relative L2 of a produced channel)
    of a float64 result"""
    if not bool(torch.isfinite(out).all()):
        return False, float('inf')
    if c.sect == 'B':
        bad = int((out != exact_expected(c)).sum())
        return bad == 0, float(bad)
    if c.sect == 'C':
        e = float(channel_rel(c, out, data(c).ref).max())
        return e < 3e-6, e
    E, bound, want = bounds(c)
    err = (out - want).abs()
    return bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


def channel_rel(c, out, ref):
    """relative L2 of every produced channel (weight gradient: of every output channel k)"""
    return per_row_rel(out, ref) if c.pass_ != 'wgrad' else per_row_rel(out.transpose(0, 1), ref.transpose(0, 1))


# ---- the kernel's arithmetic, restated -------------------------------------------------------------------------------------------------------
PERTURBATIONS = (
    'drop_mm',                  # bf16x3: the (m, m) product dropped
    'drop_lh',                  # bf16x3: the (l, h) product (low piece of the packed operand) dropped
    'swap_row_classes',         # data gradient: row 1 takes the packed weights of row H-2 and the other way round
    'mirror_from_tap_0',        # data gradient: the column-mirror source of pixel 1 taken under tap s' = 0, not s' = 2
    'shift_tap',                # one high weight piece (one row, one channel) takes the value of the neighbouring tap
    'dead_stage_repeats',       # odd stage count: the rounded-up dead stage adds stage 0 once more
    'drop_last_stage',          # weight gradient: the last stage of the last split is not accumulated
    'zero_half_pixel',          # buffer 1 (stage 1): the 8-channel half 1 of one pixel is zero in every piece
)
PAIRS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # (packed piece, gathered piece): smallest terms first


def _pieces(t, pk):
    return split3(t) if pk == 'bf16x3' else [_bf16(t)]


def _windows(t, Rr, S):
    """[N][Cg][P][Q][R][S] of a padded tensor"""
    return t.unfold(2, Rr, 1).unfold(3, S, 1)


def _stage_major(win):
    """[N][Cg][P][Q][T] -> [stage = (chunk, tap)][16][N P Q]"""
    N, Cg, P, Q, T = win.shape
    return win.reshape(N, Cg // 16, 16, P * Q, T).permute(1, 4, 2, 0, 3).reshape(Cg // 16 * T, 16, N * P * Q)


def _weights_stage_major(wm):
    """[M][Cg][T] -> [M][stage][16]"""
    M, Cg, T = wm.shape
    return wm.reshape(M, Cg // 16, 16, T).permute(0, 1, 3, 2).reshape(M, Cg // 16 * T, 16)


def _accumulate(Ap, Bp, stages, pairs, perturb):
    """sum over `stages` (a list, in order) of the piece products of a stage in the order of `pairs`, in fp32: Ap[i] [M][nst][16],
    Bp[j] [nst][16][P]; every product of a stage is summed exactly and rounded to fp32 once, as a matrix instruction of exact products"""
    stages = list(stages)
    if perturb == 'dead_stage_repeats':
        assert len(stages) % 2 == 1
        stages = stages + stages[:1]
    idx = torch.tensor(stages)
    acc = torch.zeros(Ap[0].shape[0], Bp[0].shape[2])
    prods = [torch.bmm(Ap[a][:, idx].permute(1, 0, 2).double(), Bp[b][idx].double()).float() for a, b in pairs]
    for i in range(len(stages)):
        for p in prods:
            acc = acc + p[i]
    return acc


def _zero_half(Bp, stage):
    out = []
    for t in Bp:
        t = t.clone()
        t[stage, 8:, -1] = 0.0      # (the last pixel: its tap (0, 1) lies inside the plane)
        out.append(t)
    return out


def _shift_tap(Ap, T):
    """row M // 2, channel 8 of chunk 0: the first tap whose high piece differs from its neighbour's takes the neighbour's"""
    a = Ap[0].clone()
    m = a.shape[0] // 2
    for i in range(1, T):
        if float(a[m, i, 8]) != float(a[m, i - 1, 8]):
            a[m, i, 8] = a[m, i - 1, 8]
            return [a] + list(Ap[1:])
    return None


def emulate(c, perturb=None, d=None):
    """the call's result as float64 in the output's layout, or None where the perturbation has no place in this case"""
    d = d or data(c)
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    pl = plan(c)
    x3 = c.pk == 'bf16x3'
    if perturb in ('drop_mm', 'drop_lh') and not x3:
        return None
    if perturb in ('swap_row_classes', 'mirror_from_tap_0') and c.pass_ != 'dgrad':
        return None
    if perturb == 'drop_last_stage' and c.pass_ != 'wgrad':
        return None
    if perturb == 'dead_stage_repeats' and not any(h % 2 for h in pl.here):
        return None
    if perturb == 'zero_half_pixel' and pl.here[0] < 2:
        return None
    pairs = [p for p in PAIRS if not (perturb == 'drop_mm' and p == (1, 1)) and not (perturb == 'drop_lh' and p == (2, 0))] if x3 else [(0, 0)]
    acc_perturb = perturb if perturb == 'dead_stage_repeats' else None
    src, w = d.src.float(), d.w.float()
    if c.pass_ == 'wgrad':
        if perturb == 'shift_tap':
            return None
        xp = torch.nn.functional.pad(src, (1, 1, 1, 1), mode='reflect')
        Bm = _windows(xp, 3, 3).permute(0, 2, 3, 1, 4, 5).reshape(pl.stages, 16, C * 9)       # [stage][16 consecutive (n, y, x)][(c, r, s)]
        Am = w.permute(1, 0, 2, 3).reshape(K, pl.stages, 16)                               # dy [k][stage][16]
        Ap, Bp = _pieces(Am, c.pk), _pieces(Bm, c.pk)
        if perturb == 'zero_half_pixel':
            Bp = _zero_half(Bp, 1)
        parts = []
        for sp in range(pl.splits):
            stages = list(range(sp * pl.stages_per_split, sp * pl.stages_per_split + pl.here[sp]))
            if perturb == 'drop_last_stage' and sp == pl.splits - 1:
                stages = stages[:-1]
            parts.append(_accumulate(Ap, Bp, stages, pairs, acc_perturb if len(stages) % 2 else None))
        a0, a1 = torch.zeros_like(parts[0]), torch.zeros_like(parts[0])
        sp = 0
        while sp + 1 < pl.splits:
            a0, a1 = a0 + parts[sp], a1 + parts[sp + 1]
            sp += 2
        if sp < pl.splits:
            a0 = a0 + parts[sp]
        v = (a0 + a1).view(K, C, 3, 3)
        if d.base is not None:
            v = d.base.float() + v
        return v.double()
    if c.pass_ == 'fwd':
        xp = torch.nn.functional.pad(src, (pad, pad, pad, pad), mode='reflect' if pm == 1 else 'constant') if pad else src
        Bp = _pieces(_stage_major(_windows(xp, Rr, S).reshape(N, C, pl.P, pl.Q, Rr * S)), c.pk)
        Ap = _pieces(_weights_stage_major(w.reshape(K, C, Rr * S)), c.pk)
        if perturb == 'shift_tap':
            Ap = _shift_tap(Ap, Rr * S)
            if Ap is None:
                return None
        if perturb == 'zero_half_pixel':
            Bp = _zero_half(Bp, 1)
        y = _accumulate(Ap, Bp, range(pl.stages), pairs, acc_perturb).view(K, N, pl.P, pl.Q).permute(1, 0, 2, 3)
        if d.b is not None:
            y = y + d.b.view(1, -1, 1, 1)
        y = R.activation(y, c.act, slope_of(c))
        return (_bf16(y) if not x3 else y).double()
    # data gradient: rows = the C input channels, gathered = dy with a ring of zeros through the flipped weights; three row classes
    dyz = torch.nn.functional.pad(src, (1, 1, 1, 1))
    win = _windows(dyz, 3, 3).contiguous()                 # [N][K][H][W][r'][s']: dy[y - 1 + r'][x - 1 + s'] or 0
    rows3 = dyz.unfold(2, 3, 1)                            # [N][K][H][W + 2][r']
    b2 = torch.zeros_like(win)
    b2[:, :, :, 1, :, 0 if perturb == 'mirror_from_tap_0' else 2] = rows3[:, :, :, 1, :]         # column 1 also receives padded column -1: source column 0
    b2[:, :, :, W - 2, :, 0] = b2[:, :, :, W - 2, :, 0] + rows3[:, :, :, W, :]                  # column W-2: padded column W, source column W-1
    v = win + b2                                           # fp32; bf16 tensors: rounded once by _pieces
    wf = w.flip(2, 3).transpose(0, 1).contiguous()         # [C][K][r'][s']
    w1, w2 = wf.clone(), wf.clone()
    w1[:, :, 0] = wf[:, :, 0] + wf[:, :, 2]                # row 1 reads row 0 for itself and for padded row -1
    w2[:, :, 2] = wf[:, :, 2] + wf[:, :, 0]
    classes = [wf, w1, w2]
    if perturb == 'swap_row_classes':
        classes = [wf, w2, w1]
    rowsets = [[0] + list(range(2, H - 2)) + [H - 1], [1], [H - 2]]
    out = torch.zeros(N, C, H, W)
    for ph in range(3):
        rs = torch.tensor(rowsets[ph])
        Bp = _pieces(_stage_major(v[:, :, rs].reshape(N, K, len(rowsets[ph]), W, 9)), c.pk)
        Ap = _pieces(_weights_stage_major(classes[ph].reshape(C, K, 9)), c.pk)
        if ph == 0 and perturb == 'shift_tap':
            Ap = _shift_tap(Ap, 9)
            if Ap is None:
                return None
        if ph == 0 and perturb == 'zero_half_pixel':
            Bp = _zero_half(Bp, 1)
        y = _accumulate(Ap, Bp, range(pl.stages), pairs, acc_perturb)
        out[:, :, rs] = y.view(C, N, len(rowsets[ph]), W).permute(1, 0, 2, 3)
    return (_bf16(out) if not x3 else out).double()


def bf16_sums_exact(c):
    """bf16 data gradient: the column-mirror sums of dy and the folded row-class weights are bf16 numbers (both roundings exact)"""
    d = data(c)
    W = c.geom[3]
    s, w = d.src.float(), d.w.float()
    sums = [s[..., 0] + s[..., 2], s[..., W - 3] + s[..., W - 1], w[:, :, 0] + w[:, :, 2]]
    return all(bool((_bf16(t) == t).all()) for t in sums + [s, w])


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
Z, RF = 0, 1
HALO_OFF = (('bsplit_halo', 0),)


def G(N, C, H, W, K, k, pad, pm):
    return (N, C, H, W, K, k, k, 1, pad, pm)


# (name, pass, geometry, options, want without the storage type, forward only: (bias, act, wexp), accumulate, section A dtypes)
#   want: (kernel, mode, bm, row tiles, pixel | column tiles, stages, splits, stages per split, padded copy)
BOTH, FP32 = PKS, ('bf16x3',)
SHAPES = (
    # ---- forward: the pipeline, 1x1 filters on 16 .. 80 channels (15 pixels, 32 rows)
    ('f_pipe1', 'fwd', G(1, 16, 3, 5, 32, 1, 0, Z), (), (0, 0, 128, 1, 1, 1, 1, 1, 0), (False, 0, 0), 0, BOTH),
    ('f_pipe2', 'fwd', G(1, 32, 3, 5, 32, 1, 0, Z), (), (0, 0, 128, 1, 1, 2, 1, 2, 0), (True, 1, 0), 0, BOTH),
    ('f_pipe3', 'fwd', G(1, 48, 3, 5, 32, 1, 0, Z), (), (0, 0, 128, 1, 1, 3, 1, 3, 0), (True, 2, 0), 0, BOTH),
    ('f_pipe4', 'fwd', G(1, 64, 3, 5, 32, 1, 0, Z), (), (0, 0, 128, 1, 1, 4, 1, 4, 0), (True, 3, -5), 0, BOTH),
    ('f_pipe5', 'fwd', G(1, 80, 3, 5, 32, 1, 0, Z), (), (0, 0, 128, 1, 1, 5, 1, 5, 0), (True, 4, -5), 0, BOTH),
    # ---- forward: tiles and padding
    ('f_zero_m40', 'fwd', G(2, 16, 5, 7, 40, 3, 1, Z), (), (0, 0, 128, 1, 1, 9, 1, 9, 0), (True, 1, 0), 0, BOTH),          # 70 pixels, taps outside on four sides
    ('f_5x5_reflect', 'fwd', G(3, 16, 3, 5, 32, 5, 2, RF), (), (0, 1, 128, 1, 1, 25, 1, 25, 0), (True, 0, 0), 0, FP32),      # pad = H - 1, 25 taps
    ('f_reflect_2tiles', 'fwd', G(3, 16, 7, 9, 40, 3, 1, RF), (), (0, 1, 128, 1, 2, 9, 1, 9, 0), (True, 2, 0), 0, BOTH),     # 189 pixels, 63 per image
    ('f_one_tile', 'fwd', G(2, 16, 8, 8, 32, 3, 1, Z), (), (0, 0, 128, 1, 1, 9, 1, 9, 0), (False, 0, 0), 0, BOTH),
    ('f_valid_m256', 'fwd', G(1, 16, 6, 6, 256, 3, 0, Z), (), (0, 0, 256, 1, 1, 9, 1, 9, 0), (True, 0, 0), 0, BOTH),
    ('f_zero_m384', 'fwd', G(1, 16, 4, 4, 384, 3, 1, Z), (), (0, 0, 128, 3, 1, 9, 1, 9, 0), (False, 2, 0), 0, BOTH),
    ('f_reflect_m512', 'fwd', G(2, 16, 5, 7, 512, 3, 1, RF), (), (0, 1, 256, 2, 1, 9, 1, 9, 0), (True, 1, 0), 0, BOTH),
    ('f_option', 'fwd', G(1, 32, 4, 32, 256, 3, 1, RF), HALO_OFF, (0, 1, 256, 1, 1, 18, 1, 18, 0), (True, 0, 0), 0, FP32),
    # ---- data gradient (C = produced rows, K = gathered channels)
    ('d_4x4', 'dgrad', G(2, 32, 4, 4, 16, 3, 1, RF), (), (0, 2, 128, 1, 3, 9, 1, 9, 0), None, 0, BOTH),
    ('d_odd_3tiles', 'dgrad', G(1, 40, 13, 27, 16, 3, 1, RF), (), (0, 2, 128, 1, 5, 9, 1, 9, 0), None, 0, BOTH),            # phase 0: 297 pixels
    ('d_odd_small', 'dgrad', G(1, 40, 5, 7, 16, 3, 1, RF), (), (0, 2, 128, 1, 3, 9, 1, 9, 0), None, 0, BOTH),
    ('d_c256', 'dgrad', G(1, 256, 4, 6, 16, 3, 1, RF), (), (0, 2, 256, 1, 3, 9, 1, 9, 0), None, 0, BOTH),
    ('d_c512', 'dgrad', G(2, 512, 5, 5, 16, 3, 1, RF), (), (0, 2, 256, 2, 3, 9, 1, 9, 0), None, 0, BOTH),
    ('d_option', 'dgrad', G(1, 256, 4, 32, 32, 3, 1, RF), HALO_OFF, (0, 2, 256, 1, 3, 18, 1, 18, 0), None, 0, FP32),
    # ---- weight gradient
    ('w_one_split', 'wgrad', G(1, 16, 4, 16, 128, 3, 1, RF), (), (0, 3, 128, 1, 2, 4, 1, 4, 1), None, 0, BOTH),
    ('w_three_odd', 'wgrad', G(3, 16, 9, 16, 256, 3, 1, RF), (), (0, 3, 256, 1, 2, 27, 3, 9, 1), None, 0, BOTH),
    ('w_ragged_acc', 'wgrad', G(7, 16, 4, 16, 128, 3, 1, RF), (), (0, 3, 128, 1, 2, 28, 3, 10, 1), None, 1, BOTH),
    ('w_ragged_k256', 'wgrad', G(7, 16, 4, 16, 256, 3, 1, RF), (), (0, 3, 256, 1, 2, 28, 3, 10, 1), None, 0, BOTH),
    ('w_wave_copy', 'wgrad', G(4, 256, 4, 16, 128, 3, 1, RF), (), (0, 3, 128, 1, 18, 16, 2, 8, 2), None, 0, BOTH),
)
FOLD_SHAPES = ('d_4x4', 'd_odd_small', 'd_c256')
DGRAD_WLOW_BITS = {'bf16x3': 15, 'bf16': 7}      # (bf16: the folded weight w[2-r'] + w[r'] <= 254 stays a bf16 number)
# (pinned bits, wide bits) where halo_cases.XLOW_BITS leaves no room under 2^24: 5x5 taps over a 3x5 plane with pad = H - 1 gather one
# source element up to four times into one output element, and so do the mirrors of the data gradient on the 4x4 plane
XLOW_OVERRIDE = {('f_5x5_reflect', 'bf16x3'): (21, 18), ('d_4x4', 'bf16x3'): (21, 19)}
# section A seeds chosen on the reference alone: seed 0 of this case has |ref| = 72 somewhere (2^-8 |ref| over half a term)
SEEDS = {('d_c512', 'bf16'): 1}
# 'mid': both operands 9-bit integers (a non-zero middle piece on both sides: the (m, m) product carries bits), where Kp x 2^18 < 2^24
MID_SHAPES = ('f_pipe1', 'f_pipe2')


def xlow_bits(name, pass_, pk):
    return XLOW_OVERRIDE.get((name, pk), (XLOW_BITS[(pk, 'dgrad' if pass_ == 'dgrad' else 'fwd')], 20 if pk == 'bf16x3' else 0))


def _case(sect, name, pass_, geom, pk, opts, want9, act=0, bias=False, wexp=0, kind='signed', bits=0, wide=0, fold_='', acc=0, seed=0):
    want = want9[:3] + (PKS.index(pk),) + want9[3:]
    tag = '' if kind == 'signed' else '-%s%s' % (kind, ('_' + fold_) if fold_ else (str(bits) + ('w%d' % wide if wide else '')))
    full = '%s_%s_%s%s%s%s%s%s' % (sect, name, pk, '-bias' if bias else '', '-' + ACT_NAMES[act] if act else '', '-acc' if acc else '', tag,
                                   '-s%d' % seed if seed else '')
    c = Case(sect, full, pass_, geom, pk, act, bias, wexp, kind, bits, wide, fold_, acc, tuple(opts), want, None, seed)
    return c._replace(claims=claims_of(c))


def _table():
    cases = []
    flip = 0
    for name, pass_, geom, opts, want9, fwd, acc, a_pks in SHAPES:
        bias, act, wexp = fwd or (False, 0, 0)
        for pk in PKS:
            if pk in a_pks:
                cases.append(_case('A', name, pass_, geom, pk, opts, want9, act, bias, wexp, acc=acc, seed=SEEDS.get((name, pk), 0)))
            xb, xw = xlow_bits(name, pass_, pk)
            wb = DGRAD_WLOW_BITS[pk] if pass_ == 'dgrad' else WLOW_BITS[pk]
            bact = act if act in (0, 1, 2) else 0
            cases.append(_case('B', name, pass_, geom, pk, opts, want9, bact, bias, 0, 'xlow', xb, xw, acc=acc))
            # every other bf16x3 'wlow' case gives every 61st weight a third piece
            wide = 19 if pk == 'bf16x3' and flip % 2 == 0 else 0
            flip += pk == 'bf16x3'
            cases.append(_case('B', name, pass_, geom, pk, opts, want9, 0, False, 0, 'wlow', wb, wide, acc=acc))
            if name in MID_SHAPES and pk == 'bf16x3':
                cases.append(_case('B', name, pass_, geom, pk, opts, want9, bact, bias, 0, 'mid', 9))
            if name in FOLD_SHAPES:
                for f in FOLDS:
                    cases.append(_case('B', name, pass_, geom, pk, opts, want9, kind='fold', fold_=f))
    return tuple(cases)


CASES = _table()
BY_NAME = collections.OrderedDict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES), 'case names must be unique'

# section C (bf16x3): one forward, one data-gradient, one weight-gradient shape under every range kind; 'tiny2' is recorded, not gated
C_KINDS = ('relu_normal', 'wide_range', 'huge', 'tiny')
C_SHAPES = (('fwd', G(2, 32, 9, 7, 40, 3, 1, RF), (0, 1, 128, 1, 1, 18, 1, 18, 0)),
            ('dgrad', G(2, 40, 9, 7, 32, 3, 1, RF), (0, 2, 128, 1, 3, 18, 1, 18, 0)),
            ('wgrad', G(2, 16, 8, 16, 128, 3, 1, RF), (0, 3, 128, 1, 2, 16, 2, 8, 1)))
RANGE = collections.OrderedDict(((p, k), _case('C', 'range_%s' % p, p, g, 'bf16x3', (), w9, kind=k)) for p, g, w9 in C_SHAPES for k in C_KINDS + ('tiny2',))
