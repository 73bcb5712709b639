"""Case table, data makers, float64 reference, bounds, the host restated and an arithmetic emulation of the per-tap weight gradient
(csrc/hsplit_wgrad.hip: hsplit_wgrad_kernel<BM, STRIDE, TA, NC, GEN>, its padded copies and its split reduce in csrc/bsplit_pack.hip, the
host in csrc/bf16x6_conv.hip).  A plain module, no GPU and no library load at import: shared by tests/test_hsplit_wgrad_cases.py, which
checks the table and the emulation on the CPU, and tests/test_gpu_hsplit_wgrad_cases.py, which runs it.

A case is one direct call of pcgan_conv2d_bwd_weight_hsplit on the geometry (N, C, H, W, K, R, S, stride, pad, pad_mode) under the
library options of the case (`opts`: the OPTIONS keys, "hwgrad_ks" forces the number of splits).  `want` is the launch record
(pcgan_hwgrad_last_launch without the sequence number: RECORD) the case is there to hit; `plan` -- the host restated -- must reproduce
it, and `claims` are the predicates of CLAIMS the case is there for.

The host, restated (`supported`, `plan`): pcgan_conv2d_hsplit_wgrad_supported, hsplit_wgrad_gen (zero padding <= 1 applied in the gather,
option "wgrad_gen"), hsplit_wgrad_inline_reflect (3x3 stride 1 reflection padding 1, H >= 2, W >= 16, option "wgrad_padcopy" off),
hsplit_wgrad_bm (256 rows from K = 129 on), hsplit_wgrad_cw (256 columns with the 256-row tile and C R S >= 2048: bf16 tensors unless
"wgrad_cw" = 128, fp32 tensors under reflection padding with "wgrad_cw" = 256), hsplit_wgrad_splits (one round of resident workgroups,
at least 8 stages per split; "hwgrad_ks" > 0 replaces the wanted count, cut to [1, stages]; stages per split and the count re-derived),
launch_pad's choice of copy kernel (wave per plane: even padded width <= 128, padded plane <= 8192 elements, >= 1024 planes) and the
workspace (padded copy sized for 4-byte elements and rounded up to 256 bytes -- also where no copy is made, except under GEN -- then one
[K][C R S] fp32 partial sum per split).  `supported` refuses what pcgan_conv2d_bwd_weight_hsplit hands to the row-ring form (option
"wgrad_rowring" on and a shape pcgan_conv2d_wgrad_rowring_supported takes): such a call launches another kernel.

INSTANTIATIONS: the 22 of launch_tile, (BM, stride, storage type, NC = columns / 128, GEN).  UNREACHABLE under every option setting:
  (256, 2, fp32, 2, 0)   the wide fp32 form needs pad_mode 1 (hsplit_wgrad_cw), reflection padding needs stride 1
                         (pcgan_conv2d_hsplit_wgrad_supported).
No other: GEN never runs with 256 columns on fp32 tensors (GEN needs pad_mode 0, the wide fp32 form pad_mode 1), and launch_tile has no
such instantiation; every other one is reached by a case of each section below.

Section A, kind 'signed' (conv_f32_cases._signed, test_gpu_wgrad_generic._case): |x|, |dy| in [0.75, 1.25] with random signs, bf16 cases
rounded to bf16 first so the reference sees the rounded values.  Reference: float64 autograd of oracle.ops_ref.conv2d; the same call on
the absolute values gives A, the per-element sum of |terms|.  Per element, n = 16 x stages per split (from the record; the padded
columns of a ragged stage count, they cost nothing but loosen nothing either: A has no term there):
  fp32 tensors  |dw - ref| <= (2 (3 n + splits + 8) 2^-24 + 2^-20) A.  The derivation of tests/hgemm_cases.py, the kernel has the same
                two pieces per operand and the same three products: each operand, scaled by a power of two (exact), splits as h + l with
                relative error <= 2^-22; the dropped (l,l) product is <= 2^-22 of the term; second-order terms stay under 2^-20.  The
                three piece products per term are exact in fp32 (11 x 11 bits), accumulating them is 3 n additions bounded as
                conv_f32_cases bounds an fp32 sum of that depth in any order (factor 2 for the sum of |partial sums| against A); the
                reduce's adds over the splits and the scale-back (exact: powers of two) are inside splits + 8.
  bf16 tensors  |dw - ref| <= 2 (n + splits + 8) 2^-24 A: the products of bf16 values are exact in fp32, dw is stored as fp32.
Derived, not measured.  Condition (CPU for every case, and again before each launch): the largest bound of the case is under
0.75^2 / 2, half the smallest possible term -- one lost, doubled or misplaced-sign term in any element fails.  That caps a single-split
fp32 case at about 640 output pixels per element; deeper cases are split.

Section B, exact data: every partial sum is an integer multiple of one quantum and below 2^24 quanta (asserted per case on A, the sum of
|terms|), so every order of fp32 accumulation is exact and the gate is dw == ref in every element.  Both operands are split at run time
and (l,l) is dropped, so one operand has an empty low piece:
  'xlow'   x holds 15-bit integers with one element pinned to 2^15 - 1 (the scale is then 1/2: 11 bits in the high piece, 4 in the low
           one), dy in {-1, 0, 1};
  'dylow'  the mirror image;
  'int8'   bf16 tensors: 8-bit integers in both operands.
With 15-bit random values a mirrored, shifted or un-zeroed source element cannot coincide with the right one: every border form of the
table appears in this section too.

`emulate` restates the kernel's arithmetic in torch: which source element (or zero) every (stage, pixel, column) of the gather ends up
with and which dy values the `am` mask of a ragged row lets in, the scales from the maxima (split_arith.pow2_scale), split_arith.split2h of both operands, the three piece
products in the kernel's order (dy_l x_h) (dy_h x_l) (dy_h x_h) accumulated in fp32 stage by stage, split by split, (acc isx) isd, the
two-accumulator reduce of bsplit_wgrad_reduce_kernel.  A fault made on purpose is never run on a GPU: PERTURBATIONS are applied to
`emulate`, and tests/test_hsplit_wgrad_cases.py evaluates the gates of both sections on the result.
What `gather` does NOT restate is the kernel's per-thread mechanics of the borders -- the `lm` / `rmk` bit masks, the run loaded one
element late and rotated (`fix & 256`), the `fix` 1 / 2 register moves: it computes the source index those mechanics must arrive at,
and the border perturbations are faults of that index (what the element would hold had one of the mechanics failed).  That serves the
sensitivity study; the GPU gates do not lean on it, their reference is float64 autograd."""
import collections
import functools

import torch

from conv_f32_cases import _signed
from split_arith import U, cdiv, out_size, pow2_scale, split2h
from split_arith import wgrad64 as grad64      # (float64 autograd of oracle.ops_ref.conv2d)

TERM_MIN = 0.75 * 0.75
F32, BF16 = 0, 1
OPTIONS = {'wgrad_gen': 1, 'wgrad_padcopy': 0, 'wgrad_cw': 0, 'wgrad_rowring': 1, 'hwgrad_ks': 0}      # the library's defaults
RECORD = ('bm', 'stride', 'dtype', 'cw', 'form', 'copy', 'row_tiles', 'col_tiles', 'splits', 'stages_per_split', 'stages')
FORM_SEPARABLE, FORM_REFLECT, FORM_GEN = 0, 1, 2
COPY_NONE, COPY_ELEMENT, COPY_WAVE = 0, 1, 2
# how an fp32 case hands the operand maxima over: one slot, one per plane, ops.amax_of, and slot counts that walk thread_max_of_partials
# (strides by NT = 256 / 512 threads over 16-byte groups): 257 = 64 groups and a tail slot that holds the maximum, 300 = no multiple of
# NT, 6151 = enough groups for the four-in-flight loop of both workgroup sizes, and a 3-slot tail.  ONE slot (MAXIMA_SLOT) holds the true
# maximum, every other a decoy in (2^-7, 2^-6] of it (DECOY): a loop that skips the slot scales its operand >= 64 times too far, the
# largest element lands in [2^19, 2^20) and overflows the fp16 high piece (65504) -- inf / NaN in dw, which both gates refuse.  The
# perturbations 'x_maximum_slot_missed' / 'dy_maximum_slot_missed' show it on the emulation, in both sections.
MAXIMA = ('one', 'plane', 'amax_of', 'n6151', 'n257', 'n300')
MAXIMA_SLOT = {'n257': 256, 'n300': 299, 'n6151': 3073}
DECOY = 2.0 ** -6

INSTANTIATIONS = tuple((bm, st, dt, nc, gen) for gen in (1, 0) for bm in (128, 256) for st in (1, 2) for dt in (F32, BF16)
                       for nc in ((1, 2) if bm == 256 else (1,)) if not (gen and nc == 2 and dt == F32))
UNREACHABLE = ((256, 2, F32, 2, 0),)

Case = collections.namedtuple('Case', 'sect name geom half opts kind maxima want claims')
Data = collections.namedtuple('Data', 'x dy ref A')
Plan = collections.namedtuple('Plan', RECORD + ('ws_bytes', 'P', 'Q', 'Qs', 'nwg', 'here'))


def options(opts):
    o = dict(OPTIONS)
    o.update(opts)
    assert sorted(o) == sorted(OPTIONS), opts
    return o


# ---- the host, restated ----------------------------------------------------------------------------------------------------------------------
def _gen(geom, o):
    return bool(o['wgrad_gen']) and geom[9] == 0 and geom[8] <= 1


def _inline_reflect(geom, o):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    return st == 1 and pm == 1 and pad == 1 and Rr == 3 and S == 3 and H >= 2 and W >= 16 and not o['wgrad_padcopy']


def _rowring_takes(geom, half, o):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    if not o['wgrad_rowring'] or (half and o['wgrad_rowring'] == 3):
        return False
    return Rr == 3 and S == 3 and st == 1 and pad == 1 and pm == 1 and H >= 3 and W >= 16 and W % 16 == 0 and K % 128 == 0 and C % 32 == 0


def supported(geom, half=False, opts=()):
    """pcgan_conv2d_hsplit_wgrad_supported, and pcgan_conv2d_bwd_weight_hsplit launches the per-tap kernel itself"""
    o = options(dict(opts))
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    if st not in (1, 2) or (pm == 1 and (st != 1 or pad >= H or pad >= W)):
        return False
    if H + 2 * pad < Rr or W + 2 * pad < S:
        return False
    P, Q = out_size(H, Rr, st, pad), out_size(W, S, st, pad)
    if K < 32 or Rr * S > 49 or P < 1 or Q < 1:
        return False
    Qs = cdiv(Q, 16) * 16
    if not _gen(geom, o) and (Q % 16 != 0 or K > 256):
        return False
    if (Qs - Q) * 4 > Qs:
        return False
    if N * C * (H + 2 * pad) * (W + 2 * pad) * 4 >= 2 ** 31 or N * K * P * Q * 4 >= 2 ** 31 or N * C > 65535:
        return False
    return not _rowring_takes(geom, half, o)


def plan(geom, half=False, opts=()):
    """what pcgan_conv2d_bwd_weight_hsplit launches for a supported case: the record, the workspace size, and what the claims read"""
    o = options(dict(opts))
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    P, Q = out_size(H, Rr, st, pad), out_size(W, S, st, pad)
    Qs = cdiv(Q, 16) * 16
    CT = C * Rr * S
    gen, inline = _gen(geom, o), _inline_reflect(geom, o)
    bm = 256 if K > 128 else 128
    force = o['wgrad_cw']
    wide = (half and force != 128) or (not half and pm == 1 and force == 256)
    cw = 256 if wide and bm == 256 and CT >= 8 * 256 else 128
    nst = N * P * (Qs // 16)
    row_tiles, col_tiles = cdiv(K, bm), cdiv(CT, cw)
    want = max(1, (256 if bm == 256 else 512) // (row_tiles * col_tiles))
    if want > nst // 8:
        want = max(1, nst // 8)
    if o['hwgrad_ks'] > 0:
        want = min(o['hwgrad_ks'], nst)
    per = cdiv(nst, want)
    splits = cdiv(nst, per)
    Hp, Wp = H + 2 * pad, W + 2 * pad
    copy = COPY_NONE
    if not gen and not inline and pad > 0:
        copy = COPY_WAVE if Wp % 2 == 0 and Wp <= 128 and Hp * Wp <= 8192 and N * C >= 1024 else COPY_ELEMENT
    xpad = 0 if gen else cdiv(N * C * Hp * Wp * 4, 256) * 256
    form = FORM_GEN if gen else (FORM_REFLECT if inline else FORM_SEPARABLE)
    here = tuple(min(per, nst - s * per) for s in range(splits))
    return Plan(bm, st, BF16 if half else F32, cw, form, copy, row_tiles, col_tiles, splits, per, nst, xpad + splits * K * CT * 4, P, Q, Qs,
                row_tiles * col_tiles * splits, here)


def record(pl):
    return tuple(pl[:len(RECORD)])


def inst(case):
    w = dict(zip(RECORD, case.want))
    return (w['bm'], w['stride'], w['dtype'], w['cw'] // 128, int(w['form'] == FORM_GEN))


class _View(object):
    """a Plan plus the fields of the case that the claims read"""

    def __init__(self, case):
        self.__dict__.update(plan(case.geom, case.half, case.opts)._asdict())
        self.N, self.C, self.H, self.W, self.K, self.R, self.S, self.st, self.pad, self.pm = case.geom
        self.CT = self.C * self.R * self.S
        self.half, self.opts, self.maxima = case.half, options(dict(case.opts)), case.maxima
        self.spr = self.Qs // 16                       # stages per output row
        self.starts = tuple(s * self.stages_per_split for s in range(self.splits))


CLAIMS = {
    # rows
    'k_32': lambda v: v.K == 32 and v.bm == 128,
    'k_33': lambda v: v.K == 33 and v.bm == 128,
    'k_128': lambda v: v.K == 128 and v.bm == 128,
    'k_129': lambda v: v.K == 129 and v.bm == 256,
    'k_256': lambda v: v.K == 256,
    'k_257': lambda v: v.K == 257 and v.row_tiles == 2 and v.form == FORM_GEN,
    'k_320': lambda v: v.K == 320 and v.row_tiles == 2 and v.form == FORM_GEN,
    # columns
    'ct_27': lambda v: v.CT == 27 and v.C == 3,
    'ct_128': lambda v: v.CT == 128 and v.C == 8 and v.R * v.S == 16,
    'ct_129_plus': lambda v: 128 < v.CT < 256 and v.col_tiles == 2,
    'ct_196': lambda v: v.CT == 196 and v.C == 4,
    'ct_2048_wide': lambda v: v.CT == 2048 and v.cw == 256,
    'ct_2064_wide': lambda v: v.CT == 2064 and v.cw == 256,
    'wide_bf16_default': lambda v: v.half and v.cw == 256 and v.opts['wgrad_cw'] == 0,
    'wide_fp32_reflect': lambda v: not v.half and v.cw == 256 and v.opts['wgrad_cw'] == 256 and v.pm == 1,
    'bf16_forced_128': lambda v: v.half and v.cw == 128 and v.opts['wgrad_cw'] == 128 and v.bm == 256 and v.CT >= 2048,
    # grid
    'grid_under_8': lambda v: v.nwg < 8,
    'grid_ragged': lambda v: v.nwg >= 16 and v.nwg % 8 != 0,
    'grid_multiple_of_8': lambda v: v.nwg % 8 == 0,
    # output width, GEN masks
    'q_16': lambda v: v.Q == 16,
    'q_32': lambda v: v.Q == 32,
    'q_48': lambda v: v.Q == 48,
    'q_12': lambda v: v.Q == 12 and v.form == FORM_GEN,
    'q_13': lambda v: v.Q == 13 and v.form == FORM_GEN,
    'q_15': lambda v: v.Q == 15 and v.form == FORM_GEN,
    'q_24': lambda v: v.Q == 24 and v.form == FORM_GEN,
    'q_28': lambda v: v.Q == 28 and v.form == FORM_GEN,
    'odd_q_bf16': lambda v: v.half and v.Q % 2 == 1 and v.form == FORM_GEN,
    'masks_meet': lambda v: v.form == FORM_GEN and v.Qs == 16 and v.pad == 1,
    'stride2_last_tap_on_w': lambda v: v.form == FORM_GEN and v.st == 2 and v.pad == 1 and (v.Q - 1) * 2 + v.S - 1 - 1 == v.W,
    'pad_0': lambda v: v.form == FORM_GEN and v.pad == 0 and v.R > 1,
    'one_by_one': lambda v: v.R == 1 and v.S == 1,
    # rows of the image
    'p_1': lambda v: v.P == 1 and v.pad == 1 and v.form == FORM_GEN,
    'stride2_last_tap_on_h': lambda v: v.form == FORM_GEN and v.st == 2 and v.pad == 1 and (v.P - 1) * 2 + v.R - 1 - 1 == v.H,
    'reflect_h_2': lambda v: v.form == FORM_REFLECT and v.H == 2,
    'reflect_w_16': lambda v: v.form == FORM_REFLECT and v.W == 16,
    'reflect_w_32': lambda v: v.form == FORM_REFLECT and v.W == 32,
    # forms
    'copy_zero_2_s1': lambda v: v.copy and v.pm == 0 and v.pad == 2 and v.st == 1,
    'copy_zero_3_s1': lambda v: v.copy and v.pm == 0 and v.pad == 3 and v.st == 1,
    'copy_zero_2_s2': lambda v: v.copy and v.pm == 0 and v.pad == 2 and v.st == 2,
    'copy_zero_3_s2': lambda v: v.copy and v.pm == 0 and v.pad == 3 and v.st == 2,
    'copy_reflect_2': lambda v: v.copy and v.pm == 1 and v.pad == 2,
    'copy_reflect_3': lambda v: v.copy and v.pm == 1 and v.pad == 3,
    'copy_reflect_1_5x5': lambda v: v.copy and v.pm == 1 and v.pad == 1 and v.R == 5,
    'gen_off_3x3_s2': lambda v: v.opts['wgrad_gen'] == 0 and v.R == 3 and v.st == 2 and v.pad == 1 and v.copy,
    'unpadded_separable': lambda v: v.form == FORM_SEPARABLE and v.copy == COPY_NONE and v.pad == 0,
    'padcopy_residual_sibling': lambda v: v.opts['wgrad_padcopy'] == 1 and v.opts['wgrad_rowring'] == 0 and v.K == 256 and v.R == 3 and v.pm == 1
    and v.C % 32 == 0 and v.W % 16 == 0 and v.copy,
    'copy_wave': lambda v: v.copy == COPY_WAVE and v.N * v.C >= 1024 and (v.N * v.C) % 4 != 0,
    'copy_wave_zero': lambda v: v.copy == COPY_WAVE and v.pm == 0,
    'copy_element': lambda v: v.copy == COPY_ELEMENT,
    # pipeline
    'stages_1': lambda v: v.here == (1,),
    'stages_2': lambda v: v.here == (2,),
    'stages_3': lambda v: v.here == (3,),
    'stages_4': lambda v: v.here == (4,),
    'stages_5': lambda v: v.here == (5,),
    'stages_8': lambda v: v.here == (8,),
    'stages_9': lambda v: v.here == (9,),
    'split_starts_mid_row': lambda v: v.opts['hwgrad_ks'] > 0 and v.spr in (2, 3) and v.stages_per_split % 2 == 1 and any(s % v.spr for s in v.starts),
    'split_starts_mid_image': lambda v: v.opts['hwgrad_ks'] > 0 and v.N > 1 and any(s % (v.P * v.spr) for s in v.starts[1:]),
    'last_split_1': lambda v: v.splits > 1 and v.here[-1] == 1,
    'last_split_2': lambda v: v.splits > 1 and v.here[-1] == 2,
    'heuristic_nine_splits': lambda v: v.opts['hwgrad_ks'] == 0 and v.N * v.P * v.spr == 73 and v.splits == 9 and v.here[-1] == 1,
    # reduce
    'reduce_1': lambda v: v.stages == 64 and v.splits == 1,
    'reduce_2': lambda v: v.stages == 64 and v.splits == 2,
    'reduce_3': lambda v: v.stages == 64 and v.splits == 3,
    'reduce_7': lambda v: v.stages == 64 and v.splits == 7,
    'reduce_64': lambda v: v.stages == 64 and v.splits == 64,
    # maxima (fp32 tensors)
    'maxima_one': lambda v: not v.half and v.maxima == 'one',
    'maxima_plane': lambda v: not v.half and v.maxima == 'plane',
    'maxima_amax_of': lambda v: not v.half and v.maxima == 'amax_of',
    'maxima_n6151': lambda v: not v.half and v.maxima == 'n6151',
    'maxima_n257': lambda v: not v.half and v.maxima == 'n257',
    'maxima_n300': lambda v: not v.half and v.maxima == 'n300',
}
# what each section must claim at least once: everything, except that the reduce series runs where the condition of its section lets
# a 64-stage shape in (A: one fp32 split of 1024 pixels is over the bound's cap; B: 1024 products of 8-bit integers pass 2^24)
REQUIRED = {'A': set(CLAIMS), 'B': set(CLAIMS) - {'copy_wave_zero'}}


def claims_of(case):
    v = _View(case)
    return frozenset(k for k, f in CLAIMS.items() if f(v))


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
def G(N, C, H, W, K, k, st, pad, pm):
    return (N, C, H, W, K, k, k, st, pad, pm)


Z, RF = 0, 1
GEN_OFF, RING_OFF = {'wgrad_gen': 0}, {'wgrad_rowring': 0}


def KS(n, **more):
    return dict(more, hwgrad_ks=n)


# (name, geometry, options, {dtype: want}); want = RECORD.  fp32 = F32 (0), bf16 = BF16 (1).
#   want: (bm, stride, dtype, cw, form, copy, row tiles, column tiles, splits, stages per split, stages)
SHAPES = (
    # ---- GEN, 128 columns: rows and columns edges, 3x3 and 4x4 stride 2
    ('gen_s1_k32_c3', G(2, 3, 6, 16, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 12, 12), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 12, 12)}),
    ('gen_s2_k33', G(2, 8, 12, 32, 33, 3, 2, 1, Z), {}, {F32: (128, 2, 0, 128, 2, 0, 1, 1, 1, 12, 12), BF16: (128, 2, 1, 128, 2, 0, 1, 1, 1, 12, 12)}),
    ('gen_4x4s2_k128_ct128', G(1, 8, 12, 32, 128, 4, 2, 1, Z), {}, {F32: (128, 2, 0, 128, 2, 0, 1, 1, 1, 6, 6), BF16: (128, 2, 1, 128, 2, 0, 1, 1, 1, 6, 6)}),
    ('gen_s1_k129_ct144', G(1, 16, 8, 16, 129, 3, 1, 1, Z), {}, {F32: (256, 1, 0, 128, 2, 0, 1, 2, 1, 8, 8), BF16: (256, 1, 1, 128, 2, 0, 1, 2, 1, 8, 8)}),
    ('gen_s2_k256', G(1, 16, 16, 32, 256, 3, 2, 1, Z), {}, {F32: (256, 2, 0, 128, 2, 0, 1, 2, 1, 8, 8), BF16: (256, 2, 1, 128, 2, 0, 1, 2, 1, 8, 8)}),
    ('gen_4x4s2_k256', G(1, 8, 16, 32, 256, 4, 2, 1, Z), {}, {F32: (256, 2, 0, 128, 2, 0, 1, 1, 1, 8, 8), BF16: (256, 2, 1, 128, 2, 0, 1, 1, 1, 8, 8)}),
    ('gen_k257', G(1, 4, 4, 16, 257, 3, 1, 1, Z), {}, {F32: (256, 1, 0, 128, 2, 0, 2, 1, 1, 4, 4), BF16: (256, 1, 1, 128, 2, 0, 2, 1, 1, 4, 4)}),
    ('gen_k320_s2', G(1, 4, 8, 32, 320, 4, 2, 1, Z), {}, {F32: (256, 2, 0, 128, 2, 0, 2, 1, 1, 4, 4), BF16: (256, 2, 1, 128, 2, 0, 2, 1, 1, 4, 4)}),
    # ---- GEN, 2048+ columns: bf16 wide by default, forced to 128; fp32 narrow (16 / 17 column tiles: a grid that is a multiple of 8 / ragged)
    ('gen_4x4s1_c128_q15', G(1, 128, 5, 16, 256, 4, 1, 1, Z), {}, {F32: (256, 1, 0, 128, 2, 0, 1, 16, 1, 4, 4), BF16: (256, 1, 1, 256, 2, 0, 1, 8, 1, 4, 4)}),
    ('gen_3x3s1_c228', G(1, 228, 4, 16, 129, 3, 1, 1, Z), {}, {BF16: (256, 1, 1, 256, 2, 0, 1, 9, 1, 4, 4)}),
    ('gen_4x4s2_c128', G(1, 128, 8, 32, 129, 4, 2, 1, Z), {}, {F32: (256, 2, 0, 128, 2, 0, 1, 16, 1, 4, 4), BF16: (256, 2, 1, 256, 2, 0, 1, 8, 1, 4, 4)}),
    ('gen_4x4s2_c129', G(1, 129, 8, 32, 129, 4, 2, 1, Z), {}, {F32: (256, 2, 0, 128, 2, 0, 1, 17, 1, 4, 4), BF16: (256, 2, 1, 256, 2, 0, 1, 9, 1, 4, 4)}),
    ('gen_3x3s2_c228', G(1, 228, 8, 32, 129, 3, 2, 1, Z), {}, {BF16: (256, 2, 1, 256, 2, 0, 1, 9, 1, 4, 4)}),
    ('gen_4x4s2_c128_cw128', G(1, 128, 8, 32, 129, 4, 2, 1, Z), {'wgrad_cw': 128}, {BF16: (256, 2, 1, 128, 2, 0, 1, 16, 1, 4, 4)}),
    # ---- GEN: output widths (3 rows, K = 32, C = 4), pad 0, 1x1
    ('gen_q32', G(1, 4, 3, 32, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 6, 6), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 6, 6)}),
    ('gen_q48', G(1, 4, 3, 48, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 9, 9), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 9, 9)}),
    ('gen_q12', G(1, 4, 3, 12, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 3, 3), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 3, 3)}),
    ('gen_q13', G(2, 4, 3, 13, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 6, 6), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 6, 6)}),
    ('gen_q15_k129', G(1, 4, 3, 15, 129, 3, 1, 1, Z), {}, {F32: (256, 1, 0, 128, 2, 0, 1, 1, 1, 3, 3), BF16: (256, 1, 1, 128, 2, 0, 1, 1, 1, 3, 3)}),
    ('gen_q24', G(1, 4, 3, 24, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 6, 6), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 6, 6)}),
    ('gen_q28_s2', G(1, 4, 6, 56, 32, 4, 2, 1, Z), {}, {F32: (128, 2, 0, 128, 2, 0, 1, 1, 1, 6, 6), BF16: (128, 2, 1, 128, 2, 0, 1, 1, 1, 6, 6)}),
    ('gen_pad0', G(1, 4, 5, 18, 32, 3, 1, 0, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 3, 3), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 3, 3)}),
    ('gen_pad0_s2_q13', G(1, 4, 7, 27, 32, 3, 2, 0, Z), {}, {F32: (128, 2, 0, 128, 2, 0, 1, 1, 1, 3, 3), BF16: (128, 2, 1, 128, 2, 0, 1, 1, 1, 3, 3)}),
    ('gen_1x1', G(1, 32, 4, 16, 32, 1, 1, 0, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 4, 4), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 4, 4)}),
    # ---- pipeline: one split of 1, 2, 3, 4, 5, 8, 9 stages (P = stages, Q = 16; P = 1: both neighbouring rows outside)
    ('pipe_1', G(1, 3, 1, 16, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 1, 1), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 1, 1)}),
    ('pipe_2', G(1, 3, 2, 16, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 2, 2), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 2, 2)}),
    ('pipe_3', G(1, 3, 3, 16, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 3, 3), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 3, 3)}),
    ('pipe_4_k256', G(1, 3, 4, 16, 256, 3, 1, 1, Z), {}, {F32: (256, 1, 0, 128, 2, 0, 1, 1, 1, 4, 4), BF16: (256, 1, 1, 128, 2, 0, 1, 1, 1, 4, 4)}),
    ('pipe_5', G(1, 3, 5, 16, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 5, 5), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 5, 5)}),
    ('pipe_8', G(1, 3, 8, 16, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 8, 8), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 8, 8)}),
    ('pipe_9_k129', G(1, 3, 9, 16, 129, 3, 1, 1, Z), {}, {F32: (256, 1, 0, 128, 2, 0, 1, 1, 1, 9, 9), BF16: (256, 1, 1, 128, 2, 0, 1, 1, 1, 9, 9)}),
    ('pipe_1_s2_k129', G(1, 4, 2, 32, 129, 4, 2, 1, Z), {}, {F32: (256, 2, 0, 128, 2, 0, 1, 1, 1, 1, 1), BF16: (256, 2, 1, 128, 2, 0, 1, 1, 1, 1, 1)}),
    # ---- forced splits: mid-row, mid-image, short last split; the heuristic's nine splits
    ('split_q32_ks4', G(1, 4, 5, 32, 32, 3, 1, 1, Z), KS(4), {F32: (128, 1, 0, 128, 2, 0, 1, 1, 4, 3, 10), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 4, 3, 10)}),
    ('split_q32_ks3', G(1, 4, 5, 32, 32, 3, 1, 1, Z), KS(3), {F32: (128, 1, 0, 128, 2, 0, 1, 1, 3, 4, 10), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 3, 4, 10)}),
    ('split_q48_ks5', G(2, 4, 4, 48, 129, 3, 1, 1, Z), KS(5), {F32: (256, 1, 0, 128, 2, 0, 1, 1, 5, 5, 24), BF16: (256, 1, 1, 128, 2, 0, 1, 1, 5, 5, 24)}),
    ('split_reflect_ks4', G(2, 4, 3, 32, 32, 3, 1, 1, RF), KS(4), {F32: (128, 1, 0, 128, 1, 0, 1, 1, 4, 3, 12), BF16: (128, 1, 1, 128, 1, 0, 1, 1, 4, 3, 12)}),
    ('split_heuristic_73', G(1, 3, 73, 16, 32, 3, 1, 1, Z), {}, {F32: (128, 1, 0, 128, 2, 0, 1, 1, 9, 9, 73), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 9, 9, 73)}),
    # ---- the reduce: 64 stages in 1, 2, 3, 7, 64 splits
    ('reduce_1', G(4, 3, 16, 16, 32, 3, 1, 1, Z), KS(1), {F32: (128, 1, 0, 128, 2, 0, 1, 1, 1, 64, 64), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 1, 64, 64)}),
    ('reduce_2', G(4, 3, 16, 16, 32, 3, 1, 1, Z), KS(2), {F32: (128, 1, 0, 128, 2, 0, 1, 1, 2, 32, 64), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 2, 32, 64)}),
    ('reduce_3', G(4, 3, 16, 16, 32, 3, 1, 1, Z), KS(3), {F32: (128, 1, 0, 128, 2, 0, 1, 1, 3, 22, 64), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 3, 22, 64)}),
    ('reduce_7', G(4, 3, 16, 16, 32, 3, 1, 1, Z), KS(7), {F32: (128, 1, 0, 128, 2, 0, 1, 1, 7, 10, 64), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 7, 10, 64)}),
    ('reduce_64', G(4, 3, 16, 16, 32, 3, 1, 1, Z), KS(64), {F32: (128, 1, 0, 128, 2, 0, 1, 1, 64, 1, 64), BF16: (128, 1, 1, 128, 2, 0, 1, 1, 64, 1, 64)}),
    # ---- reflection in the gather
    ('reflect_h2_w16', G(2, 8, 2, 16, 32, 3, 1, 1, RF), {}, {F32: (128, 1, 0, 128, 1, 0, 1, 1, 1, 4, 4), BF16: (128, 1, 1, 128, 1, 0, 1, 1, 1, 4, 4)}),
    ('reflect_w32_k129', G(1, 8, 4, 32, 129, 3, 1, 1, RF), {}, {F32: (256, 1, 0, 128, 1, 0, 1, 1, 1, 8, 8), BF16: (256, 1, 1, 128, 1, 0, 1, 1, 1, 8, 8)}),
    ('reflect_c228_wide', G(1, 228, 2, 16, 129, 3, 1, 1, RF), {'wgrad_cw': 256}, {F32: (256, 1, 0, 256, 1, 0, 1, 9, 1, 2, 2), BF16: (256, 1, 1, 256, 1, 0, 1, 9, 1, 2, 2)}),
    ('reflect_c228_default', G(1, 228, 2, 16, 129, 3, 1, 1, RF), {}, {BF16: (256, 1, 1, 256, 1, 0, 1, 9, 1, 2, 2)}),
    # ---- the padded copy: element kernel
    ('copy_stem_7x7', G(1, 4, 16, 16, 64, 7, 1, 3, RF), {}, {F32: (128, 1, 0, 128, 0, 1, 1, 2, 2, 8, 16), BF16: (128, 1, 1, 128, 0, 1, 1, 2, 2, 8, 16)}),
    ('copy_reflect_2', G(1, 4, 6, 16, 32, 5, 1, 2, RF), {}, {F32: (128, 1, 0, 128, 0, 1, 1, 1, 1, 6, 6), BF16: (128, 1, 1, 128, 0, 1, 1, 1, 1, 6, 6)}),
    ('copy_reflect_1_5x5', G(1, 4, 8, 18, 129, 5, 1, 1, RF), {}, {F32: (256, 1, 0, 128, 0, 1, 1, 1, 1, 6, 6), BF16: (256, 1, 1, 128, 0, 1, 1, 1, 1, 6, 6)}),
    ('copy_zero_2_s1', G(1, 4, 6, 16, 40, 5, 1, 2, Z), {}, {F32: (128, 1, 0, 128, 0, 1, 1, 1, 1, 6, 6), BF16: (128, 1, 1, 128, 0, 1, 1, 1, 1, 6, 6)}),
    ('copy_zero_3_s1', G(1, 3, 5, 16, 256, 7, 1, 3, Z), {}, {F32: (256, 1, 0, 128, 0, 1, 1, 2, 1, 5, 5), BF16: (256, 1, 1, 128, 0, 1, 1, 2, 1, 5, 5)}),
    ('copy_zero_2_s2', G(1, 4, 16, 32, 32, 5, 2, 2, Z), {}, {F32: (128, 2, 0, 128, 0, 1, 1, 1, 1, 8, 8), BF16: (128, 2, 1, 128, 0, 1, 1, 1, 1, 8, 8)}),
    ('copy_zero_3_s2', G(1, 3, 8, 32, 129, 7, 2, 3, Z), {}, {F32: (256, 2, 0, 128, 0, 1, 1, 2, 1, 4, 4), BF16: (256, 2, 1, 128, 0, 1, 1, 2, 1, 4, 4)}),
    ('genoff_3x3_s2', G(1, 8, 12, 32, 32, 3, 2, 1, Z), GEN_OFF, {F32: (128, 2, 0, 128, 0, 1, 1, 1, 1, 6, 6), BF16: (128, 2, 1, 128, 0, 1, 1, 1, 1, 6, 6)}),
    ('genoff_4x4_s2', G(1, 8, 12, 32, 128, 4, 2, 1, Z), GEN_OFF, {F32: (128, 2, 0, 128, 0, 1, 1, 1, 1, 6, 6), BF16: (128, 2, 1, 128, 0, 1, 1, 1, 1, 6, 6)}),
    ('genoff_3x3_s2_k256', G(1, 8, 12, 32, 256, 3, 2, 1, Z), GEN_OFF, {F32: (256, 2, 0, 128, 0, 1, 1, 1, 1, 6, 6), BF16: (256, 2, 1, 128, 0, 1, 1, 1, 1, 6, 6)}),
    ('genoff_4x4_s2_k129', G(1, 8, 12, 32, 129, 4, 2, 1, Z), GEN_OFF, {F32: (256, 2, 0, 128, 0, 1, 1, 1, 1, 6, 6), BF16: (256, 2, 1, 128, 0, 1, 1, 1, 1, 6, 6)}),
    ('genoff_3x3_s2_c228', G(1, 228, 8, 32, 129, 3, 2, 1, Z), GEN_OFF, {BF16: (256, 2, 1, 256, 0, 1, 1, 9, 1, 4, 4)}),
    ('genoff_4x4_s2_c128', G(1, 128, 8, 32, 129, 4, 2, 1, Z), GEN_OFF, {BF16: (256, 2, 1, 256, 0, 1, 1, 8, 1, 4, 4)}),
    ('genoff_pad0', G(1, 4, 5, 18, 32, 3, 1, 0, Z), GEN_OFF, {F32: (128, 1, 0, 128, 0, 0, 1, 1, 1, 3, 3), BF16: (128, 1, 1, 128, 0, 0, 1, 1, 1, 3, 3)}),
    ('padcopy_residual', G(2, 32, 8, 32, 256, 3, 1, 1, RF), {'wgrad_padcopy': 1, 'wgrad_rowring': 0},
     {F32: (256, 1, 0, 128, 0, 1, 1, 3, 4, 8, 32), BF16: (256, 1, 1, 128, 0, 1, 1, 3, 4, 8, 32)}),
    ('padcopy_c228_wide', G(1, 228, 2, 16, 129, 3, 1, 1, RF), {'wgrad_padcopy': 1, 'wgrad_cw': 256},
     {F32: (256, 1, 0, 256, 0, 1, 1, 9, 1, 2, 2), BF16: (256, 1, 1, 256, 0, 1, 1, 9, 1, 2, 2)}),
    # ---- the padded copy: one wave per plane (1026 planes, padded width 18 / 20)
    ('wave_reflect', G(2, 513, 4, 16, 32, 3, 1, 1, RF), {'wgrad_padcopy': 1}, {F32: (128, 1, 0, 128, 0, 2, 1, 37, 1, 8, 8), BF16: (128, 1, 1, 128, 0, 2, 1, 37, 1, 8, 8)}),
    ('wave_zero_2', G(2, 513, 2, 16, 32, 5, 1, 2, Z), {}, {F32: (128, 1, 0, 128, 0, 2, 1, 101, 1, 4, 4)}),
)
B_SKIP = {('split_heuristic_73', BF16): '1168 products of 8-bit integers pass 2^24', ('wave_zero_2', F32): 'the zero branch of the wave copy moves no arithmetic',
          ('reduce_1', BF16): '1024 products of 8-bit integers pass 2^24', ('reduce_2', BF16): 'as reduce_1', ('reduce_3', BF16): 'as reduce_1',
          ('reduce_7', BF16): 'as reduce_1', ('reduce_64', BF16): 'as reduce_1'}
A_SKIP = {('reduce_1', F32): 'one fp32 split of 1024 pixels is over the cap of the condition', ('reduce_2', F32): '512 pixels per split at A = 1600: 0.296'}


def _table():
    cases = []
    nf = {'A': 0, 'B': 0}
    for name, geom, opts, wants in SHAPES:
        for dt in sorted(wants):
            for sect in 'AB':
                if (sect == 'A' and (name, dt) in A_SKIP) or (sect == 'B' and (name, dt) in B_SKIP):
                    continue
                half = dt == BF16
                if sect == 'A':
                    kind = 'signed'
                else:
                    kind = 'int8' if half else ('xlow', 'dylow')[nf[sect] % 2]
                # fp32 cases walk through the ways of handing the maxima over, in both sections
                maxima = None if half else MAXIMA[nf[sect] % 6]
                nf[sect] += 0 if half else 1
                c = Case(sect, '%s_%s_%s' % (sect, name, 'bf16' if half else 'fp32'), geom, half, tuple(sorted(opts.items())), kind, maxima,
                         wants[dt], None)
                cases.append(c._replace(claims=claims_of(c)))
    return tuple(cases)


CASES = _table()
BY_NAME = {c.name: c for c in CASES}

# section C (operand ranges, fp32 tensors, per element against the fp32 route): one GEN shape, one reflection-in-gather shape
C_KINDS = ('relu_normal', 'wide_range', 'tiny', 'huge')
C_SHAPES = (G(2, 16, 6, 16, 64, 3, 1, 1, Z), G(2, 16, 4, 32, 129, 3, 1, 1, RF))
# section D (host routing, ops.conv2d_bwd_weight with and without accumulate_into): GEN, reflection in the gather, padded copy
D_SHAPES = (('gen', G(2, 16, 12, 32, 128, 4, 2, 1, Z), False), ('reflect', G(2, 16, 4, 32, 129, 3, 1, 1, RF), False), ('copy', G(1, 16, 6, 16, 32, 5, 1, 2, RF), True))


# ---- data, reference, bounds ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(geom, half, kind):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    P, Q = out_size(H, Rr, st, pad), out_size(W, S, st, pad)
    g = torch.Generator().manual_seed(sum(v * (i + 1) * 7919 for i, v in enumerate(geom)) + int(half) + 17 * ('signed', 'xlow', 'dylow', 'int8').index(kind))

    def ints(bits, *shape):
        return torch.randint(-(2 ** bits - 1), 2 ** bits, shape, generator=g).float()

    def tern(*shape):
        return torch.randint(-1, 2, shape, generator=g).float()
    xs, ds = (N, C, H, W), (N, K, P, Q)
    if kind == 'signed':
        x, dy = _signed(g, *xs), _signed(g, *ds)
    elif kind == 'xlow':
        x, dy = ints(15, *xs), tern(*ds)
        x.view(-1)[x.numel() // 2] = 2.0 ** 15 - 1
    elif kind == 'dylow':
        x, dy = tern(*xs), ints(15, *ds)
        dy.view(-1)[dy.numel() // 2] = 2.0 ** 15 - 1
    else:
        x, dy = ints(8, *xs), ints(8, *ds)
    if half:
        x, dy = x.bfloat16(), dy.bfloat16()
    return Data(x, dy, grad64(x, dy, geom), grad64(x.abs(), dy.abs(), geom))


def data(case):
    """(x, dy, float64 reference, A) of one case on the CPU: made once, shared by the tests that use it, never written to"""
    assert (case.kind == 'int8') == (case.half and case.sect == 'B')
    return _data(case.geom, case.half, case.kind)


def bound(case, A, splits, stages_per_split):
    """section A, per element; n = 16 x stages per split"""
    n = 16 * stages_per_split
    if case.half:
        return 2 * (n + splits + 8) * U * A
    return (2 * (3 * n + splits + 8) * U + 2.0 ** -20) * A


def condition(case, d, splits, stages_per_split):
    """the condition of the case's section (asserted on the CPU for every case and again before each launch)"""
    if case.sect == 'A':
        mags = (d.x.float().abs(), d.dy.float().abs())
        assert all(0.75 <= float(m.min()) and float(m.max()) <= 1.25 for m in mags)
        worst = float(bound(case, d.A, splits, stages_per_split).max())
        assert worst < TERM_MIN / 2, '%s: the largest bound %.4f would not catch one lost term (%.4f)' % (case.name, worst, TERM_MIN / 2)
        return worst
    x, dy = d.x.float(), d.dy.float()
    assert bool((x == x.round()).all()) and bool((dy == dy.round()).all())
    if case.kind == 'int8':
        assert float(x.abs().max()) <= 255 and float(dy.abs().max()) <= 255
    else:
        big, small = (x, dy) if case.kind == 'xlow' else (dy, x)
        assert float(big.abs().max()) == 2.0 ** 15 - 1 and float(small.abs().max()) <= 1
    assert float(d.A.max()) < 2.0 ** 24, '%s: %g quanta' % (case.name, float(d.A.max()))
    return float(d.A.max()) / 2.0 ** 24


def gate(case, out, d, splits, stages_per_split):
    """(passes, max |err| / bound -- section B: the number of unequal elements) of a float64 result [K][C][R][S]"""
    if not bool(torch.isfinite(out).all()):
        return False, float('inf')
    if case.sect == 'B':
        bad = int((out != d.ref).sum())
        return bad == 0, float(bad)
    b = bound(case, d.A, splits, stages_per_split)
    err = (out - d.ref).abs()
    return bool((err <= b).all()), float((err / b.clamp_min(1e-300)).max())


# ---- the kernel's arithmetic, restated -------------------------------------------------------------------------------------------------------
PERTURBATIONS = (
    'left_not_zeroed',        # GEN: the element in front of column 0 is read as memory holds it (the element before, 0 in front of the tensor)
    'rotate_without_zero',    # GEN: the run loaded one element late is rotated but its element 0 keeps the first loaded value (column -1 + stride)
    'right_mask_short',       # GEN: the right mask starts one element late -- column W reads the element behind the row
    'mirror_w1',              # reflection in the gather, fix == 2: column W mirrors to W - 1 instead of W - 2
    'top_row0',               # reflection in the gather: row -1 taken as row 0 instead of row 1
    'am_off_by_one',          # GEN, ragged rows: one dy value behind column Q - 1 enters (the first of the next row)
    'drop_last_stage',        # the last stage of split 0 is not accumulated
    'double_first_stage',     # split 0 also accumulates the first stage of split 1
    'drop_lh',                # fp32 tensors: the (dy_l, x_h) product dropped
    'drop_hl',                # fp32 tensors: the (dy_h, x_l) product dropped
    'swap_rows',              # fp32 tensors: rows arow and arow + AR (= BM / 2) of the dy tile exchanged in the last stage of split 0
    'drop_odd_tail',          # the reduce without its odd last split
    'x_maximum_slot_missed',  # fp32 tensors, maxima in MAXIMA_SLOT: the slot with the maximum of |x| skipped, the scale comes from the largest decoy
    'dy_maximum_slot_missed',  # ... of |dy|
)


def _flat(t, idx, ok):
    """t.view(-1)[idx] where ok and idx inside the tensor, else 0 (the buffer load's range check)"""
    inside = ok & (idx >= 0) & (idx < t.numel())
    return torch.where(inside, t.reshape(-1)[idx.clamp(0, t.numel() - 1)], torch.zeros((), dtype=t.dtype))


def gather(case, d, perturb=None):
    """(dyg [K][stages * 16], xg [stages * 16][C R S]) as fp32: what the kernel's loaders hand to the split, stage by stage -- every stage is
    16 consecutive columns of one output row (the row width rounded up to 16 under GEN).  None where the perturbation has no place."""
    v = _View(case)
    N, C, H, W, K, Rr, S, st, pad, pm = case.geom
    P, Q = v.P, v.Q
    Qrow = v.Qs if v.form == FORM_GEN else Q
    x, dy = d.x.float(), d.dy.float()
    e = torch.arange(v.stages * 16)
    n, rem = e // (P * Qrow), e % (P * Qrow)
    y, q = rem // Qrow, rem % Qrow
    # dy: columns behind Q - 1 are masked (am)
    kk = torch.arange(K).view(-1, 1)
    didx = ((n * K + kk) * P + y) * Q + q
    dok = (q < Q).expand_as(didx)
    if perturb == 'am_off_by_one':
        if v.form != FORM_GEN or Q == v.Qs:
            return None
        dok = (q <= Q).expand_as(didx)
    dyg = _flat(dy, didx, dok)
    # x: column (c, r, s)
    col = torch.arange(v.CT)
    c, r, s = col // (Rr * S), (col // S) % Rr, col % S
    nn, yy, qq = n.view(-1, 1), y.view(-1, 1), q.view(-1, 1)
    if v.form == FORM_GEN:
        row, cc = yy * st - pad + r, qq * st + s - pad
        rowok = (row >= 0) & (row < H)
        ok = rowok & (cc >= 0) & (cc < W)
        idx = ((nn * C + c) * H + row) * W + cc
        if perturb == 'left_not_zeroed':
            if pad == 0:
                return None
            ok = rowok & (cc < W)
        elif perturb == 'rotate_without_zero':
            if pad == 0:
                return None
            idx = torch.where(cc < 0, idx + st, idx)
            ok = rowok & (cc < W)
        elif perturb == 'right_mask_short':
            if not bool(((cc == W) & (qq < Q)).any()):
                return None
            ok = rowok & (cc >= 0) & (cc <= W)
        elif perturb in ('mirror_w1', 'top_row0'):
            return None
        xg = _flat(x, idx, ok)
    elif v.form == FORM_REFLECT:
        if perturb in ('left_not_zeroed', 'rotate_without_zero', 'right_mask_short'):
            return None
        row, cc = yy + r - 1, qq + s - 1
        row = torch.where(row < 0, torch.full_like(row, 0 if perturb == 'top_row0' else 1), torch.where(row >= H, 2 * (H - 1) - row, row))
        cc = torch.where(cc < 0, -cc, torch.where(cc >= W, torch.full_like(cc, W - 1 if perturb == 'mirror_w1' else W - 2), cc))
        xg = x.reshape(-1)[((nn * C + c) * H + row) * W + cc]
    else:
        if perturb in ('left_not_zeroed', 'rotate_without_zero', 'right_mask_short', 'mirror_w1', 'top_row0'):
            return None
        xp = torch.nn.functional.pad(x, (pad, pad, pad, pad), mode='reflect' if pm == 1 else 'constant') if pad > 0 else x
        Hp, Wp = H + 2 * pad, W + 2 * pad
        assert tuple(xp.shape) == (N, C, Hp, Wp)
        xg = xp.reshape(-1)[((nn * C + c) * Hp + yy * st + r) * Wp + qq * st + s]
    return dyg, xg


def emulate(case, perturb=None):
    """the kernel's result [K][C][R][S] as float64, or None where the perturbation has no place in this case"""
    d = data(case)
    v = _View(case)
    g = gather(case, d, perturb)
    if g is None:
        return None
    dyg, xg = g
    K, CT = v.K, v.CT
    if perturb in ('drop_lh', 'drop_hl', 'swap_rows', 'x_maximum_slot_missed', 'dy_maximum_slot_missed') and case.half:
        return None
    if perturb == 'double_first_stage' and v.splits < 2:
        return None
    if perturb == 'drop_odd_tail' and v.splits % 2 == 0:
        return None
    if case.half:
        sx = sdy = 1.0
        prods = ((dyg, xg),)
    else:
        mx, md = float(d.x.abs().max()), float(d.dy.abs().max())
        if perturb in ('x_maximum_slot_missed', 'dy_maximum_slot_missed'):
            if case.maxima not in MAXIMA_SLOT:
                return None
            mx, md = (mx * DECOY, md) if perturb[0] == 'x' else (mx, md * DECOY)
        sx, sdy = pow2_scale(mx), pow2_scale(md)
        missed = perturb in ('x_maximum_slot_missed', 'dy_maximum_slot_missed')
        (dh, dl), (xh, xl) = split2h(dyg * sdy, may_overflow=missed), split2h(xg * sx, may_overflow=missed)
        prods = [(dl, xh), (dh, xl), (dh, xh)]
        if perturb == 'drop_lh':
            del prods[0]
        elif perturb == 'drop_hl':
            del prods[1]
    isx, isd = torch.tensor(1.0 / sx, dtype=torch.float32), torch.tensor(1.0 / sdy, dtype=torch.float32)
    parts = []
    for sp in range(v.splits):
        acc = torch.zeros(K, CT, dtype=torch.float32)
        stages = list(range(sp * v.stages_per_split, sp * v.stages_per_split + v.here[sp]))
        if sp == 0 and perturb == 'drop_last_stage':
            stages = stages[:-1]
        if sp == 0 and perturb == 'double_first_stage':
            stages = stages + [v.stages_per_split]
        for t in stages:
            sl = slice(t * 16, t * 16 + 16)
            for a, b in prods:
                at = a[:, sl]
                if perturb == 'swap_rows' and sp == 0 and t == stages[-1]:
                    tile = torch.zeros(v.bm, 16)
                    tile[:min(K, v.bm)] = at[:v.bm]
                    tile = torch.cat((tile[v.bm // 2:], tile[:v.bm // 2]))
                    at = torch.cat((tile[:min(K, v.bm)], at[v.bm:]))
                acc = acc + at @ b[sl]
        parts.append((acc * isx) * isd)
    a0, a1 = torch.zeros(K, CT), torch.zeros(K, CT)
    sp = 0
    while sp + 1 < v.splits:
        a0, a1 = a0 + parts[sp], a1 + parts[sp + 1]
        sp += 2
    if sp < v.splits and perturb != 'drop_odd_tail':
        a0 = a0 + parts[sp]
    return (a0 + a1).double().view(K, v.C, v.R, v.S)


def emulable(case):
    """small enough to emulate in a few seconds on the CPU"""
    v = _View(case)
    return v.stages * v.K * v.CT <= 40 * 256 * 2100


# which cases the sensitivity study names for each perturbation (shape names; each fails as A_<name> and as B_<name>, fp32 tensors and --
# where the perturbation has a place on bf16 tensors -- bf16 too).  Every perturbation but the two dropped products fails in EVERY case in
# which it has a place; a dropped low product passes the section-A gate of shallow cases (one piece's 2^-12 of sqrt(n) random-sign terms
# is inside a worst-case bound over 3 n additions) and is what section B is for: 'xlow' fails without (dy_h, x_l), 'dylow' without (dy_l, x_h).
PERTURBATION_FAILS = {
    'left_not_zeroed': ('gen_s1_k32_c3', 'gen_s2_k33', 'gen_4x4s2_k128_ct128'),       # GEN stride 1, stride 2 (3x3 and 4x4)
    'rotate_without_zero': ('gen_s1_k32_c3', 'gen_s2_k33', 'pipe_1'),
    'right_mask_short': ('gen_q13', 'gen_q15_k129', 'gen_q28_s2', 'gen_4x4s1_c128_q15'),      # ragged last stages
    'mirror_w1': ('reflect_h2_w16', 'reflect_w32_k129', 'reflect_c228_wide'),
    'top_row0': ('reflect_h2_w16', 'reflect_w32_k129', 'split_reflect_ks4'),
    'am_off_by_one': ('gen_q12', 'gen_q13', 'gen_q24', 'gen_q28_s2'),
    'drop_last_stage': ('pipe_1', 'pipe_9_k129', 'split_q32_ks4', 'copy_stem_7x7'),
    'double_first_stage': ('split_q32_ks4', 'split_q48_ks5', 'split_heuristic_73'),
    'drop_lh': ('gen_s1_k129_ct144', 'gen_4x4s2_k256'),
    'drop_hl': ('gen_4x4s2_k128_ct128', 'gen_s2_k256'),
    'swap_rows': ('gen_s1_k32_c3', 'gen_s1_k129_ct144', 'reflect_w32_k129'),
    'drop_odd_tail': ('pipe_3', 'reduce_3', 'reduce_7', 'split_q48_ks5'),
    'x_maximum_slot_missed': (),       # no shape named: EVERY fp32 case whose maxima come in 257, 300 or 6151 slots fails, in both sections
    'dy_maximum_slot_missed': (),
}
