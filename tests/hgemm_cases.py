"""Case table, data makers, float64 reference, bounds and an arithmetic emulation of the packed implicit GEMM on the f16 / bf16 matrix
pipe (csrc/hgemm.hip: hgemm_kernel<MODE, BM, BP, TA>, 3 modes x 4 tiles x 2 storage types = 24 instantiations, and hgemm_presplit_kernel).
A plain module, no GPU and no library load at import: shared by tests/test_hgemm_cases.py, which checks the table and the emulation on the
CPU, and tests/test_gpu_hgemm_cases.py, which runs it.

A case is one direct call of the C-ABI (fp32 tensors: pcgan_conv2d_hgemm_pack, then pcgan_conv2d_fwd_packed_hsplit /
pcgan_conv2d_bwd_data_packed_hsplit; bf16 descriptors: pcgan_conv2d_pack_weights, then pcgan_conv2d_fwd_packed / _bwd_data_packed) on the
geometry (N, C, H, W, K, R, S, stride, pad, pad_mode) of the CONVOLUTION (the data gradient gathers its K channels and produces its C)
under a forced tile / K split (library options "hgemm_tile" / "hgemm_ks").  `want` is the launch record (form, mode, bm, bp, ks, nphase)
the case is there to hit; conv_f32_cases.plan -- the host's routing restated -- must reproduce it with `form` mapped to hgemm_f16x2 /
hgemm_bf16 (the host launches the hgemm form of the same tiles, phases and K splits whenever the chunked-K kernel would run, the mode is
no fused reflect gradient and BM >= 64), and `claims` are the predicates of the plan that the case is there for (conv_f32_cases.CLAIMS and
CLAIMS below).  `supported` restates pcgan_conv2d_hgemm_supported.

Section A, kind 'signed' (conv_f32_cases._signed): |x|, |w|, |dy|, |bias| in [0.75, 1.25] with random signs; tanh / sigmoid cases multiply
the weights by 2^wexp so that |ref| stays near 1.  Reference: split_arith.reference in float64; the same call on absolute
values gives A.  Per element, Kp = the K length of the phase that owns it, ks = the K slices of the launch:
  fp32 tensors  |y - act(ref)| <= (2 (3 Kp + ks + 8) 2^-24 + 2^-20) A (+ 2^-22 |act(ref)|).  Each scaled operand splits as h + l with
                relative error <= 2^-22, the dropped (l,l) product is <= 2^-22 of the term, second-order terms under 2^-20 (the
                derivation of tests/thin_cases.py: same pieces, same products); the three piece products per term are exact in fp32 and
                accumulating them is 3 Kp additions, bounded as conv_f32_cases bounds a sum (factor 2); ks partial sums and the bias are
                inside ks + 8.  Scaling by powers of two is exact.  Pixels of a strided data gradient that no phase writes have A = 0:
                the bound there is 0 and the test asks for +0.
  bf16 tensors  operands are bf16 numbers (the weights rounded to bf16 first, as the kernel rounds them on their way to LDS), every
                product is exact, the stored result is one rounding to bf16: the _bf16_bound form of tests/test_gpu_hgemm.py and
                conv_f32_cases.py with E = 2 (Kp + ks + 8) 2^-24 A:  2^-8 (|act(ref)| + E) + E + 2^-22 |act(ref)| + 1e-30.
Condition (CPU, and again before each launch): the largest bound of the case on the linear result is under TERM_MIN 2^wexp / 2, half the
smallest possible term -- one lost, doubled or misplaced term in any element fails.  That caps fp32 cases at Kp <= 640 (the largest used,
16 channels x 25 taps, gives 0.09 of the 0.281 allowed) and bf16 cases at Kp <= 144 (|ref| < 72: conv_f32_cases.py explains).

Section B, exact data: every partial sum of the kernel is an integer multiple of one quantum and bounded by A quanta, so any order of
fp32 accumulation is exact when A < 2^24 quanta (asserted per case; at 15 bits Kp <= 511), and the gate is out == ref in every element.
  'xlow'  the activation tensor holds 15-bit integers with one element pinned to 2^15 - 1 (11 bits in the high piece, 4 in the low one),
          weights in {-1, 0, 1}, bias integers in [-64, 64], activation none / ReLU / LeakyReLU(0.25).
  'wlow'  15-bit integer weights, each row of the pass's weight matrix (the output channel forward, the input channel in the data
          gradient) times 2^j, j in [-20, 20], rows 0 and 1 at +20 and -20; the activation tensor in {-1, 0, 1}, no bias.
  bf16 tensors: 8-bit integers in both operands; the expected value is the exact integer rounded to bf16 to nearest even.
  'xlow16' (section C): 'xlow' with every magnitude but the pinned one <= 16: the maxima array is built by hand around it.

`emulate` restates the kernel's arithmetic in torch: the scale of x from the maxima, split_arith.split2h, the pre-split weights per row, the three
piece products in the kernel's order (l,h) (h,l) (h,h) accumulated in fp32 stage by stage in the kernel's K order (16-channel chunk, tap,
channel), slice by slice, the slice sum, (acc isx) isw, bias, activation.  A fault made on purpose is not run on a GPU: the sensitivity
study applies PERTURBATIONS to `emulate` and evaluates the gates of both sections on its result (tests/test_hgemm_cases.py)."""
import collections
import functools

import torch

from oracle import ops_ref as R
import conv_f32_cases as F
import split_arith
from conv_f32_cases import plan, record, _signed, TERM_MIN      # (record, SLOPE, per_row_rel: the tests reach them through this module)
from split_arith import U, SLOPE, cdiv, out_size, _ints, _bf16, _fwd64, _dgrad64, pow2_scale, split2h, per_row_rel, range_scale

NT = 256                        # threads of a workgroup (thread_max_of_partials strides by it)
ACT_NAMES = ('none', 'relu', 'lrelu', 'tanh', 'sigmoid')
KINDS = ('signed', 'xlow', 'wlow', 'xlow16')
MODES = ('fwd_zero', 'fwd_reflect', 'dgrad')
TILES = (128128, 128064, 64128, 64064)
INSTANTIATIONS = tuple((m, t // 1000, t % 1000, dt) for m in MODES for t in TILES for dt in ('fp32', 'bf16'))
FORMS = {False: 'hgemm_f16x2', True: 'hgemm_bf16'}

Case = collections.namedtuple('Case', 'sect name pass_ geom tile ks half act bias wexp kind want claims seed')
Data = collections.namedtuple('Data', 'src w b ref A rowexp')


# ---- the host, restated ----------------------------------------------------------------------------------------------------------------------
def supported(geom, pass_, half=False):
    """pcgan_conv2d_hgemm_supported (fp32 descriptors): the chunked K order (gathered channels a multiple of 16, <= 25 taps), more than
    32 produced channels, and no reflection padding in the data gradient"""
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    if half:
        return False
    if pass_ == 'fwd':
        return C % 16 == 0 and Rr * S <= F.NTAP_FWD and K > 32
    if pass_ == 'dgrad':
        return pm == 0 and K % 16 == 0 and Rr * S <= F.NTAP_FWD and C > 32
    return False


def hgemm_plan(case):
    """conv_f32_cases.plan with the form the host launches for it: the hgemm form wherever the chunked-K kernel would run with BM >= 64
    outside the fused reflect gradient"""
    pl = plan(case)
    if pl.form == 'igemm2_cg16' and pl.mode != 'dgrad_reflect' and pl.bm >= 64:
        pl = pl._replace(form=FORMS[case.half])
    return pl


def inst(case):
    return (case.want[1], case.want[2], case.want[3], 'bf16' if case.half else 'fp32')


def _stages(pl, p):
    """(stages, stages per slice, [(begin, end) per slice]) of phase p: hgemm_kernel's nst_all, nst_per, st_begin / st_end"""
    n = p.Kp // 16
    per = cdiv(n, pl.ks) if pl.ks > 1 else n
    return n, per, [(min(z * per, n), min(z * per + per, n)) for z in range(pl.ks)]


def _here(pl):
    return [e - b for p in pl.phases for b, e in _stages(pl, p)[2]]


CLAIMS = dict(F.CLAIMS)
CLAIMS.update({
    'stages_1': lambda pl: 1 in _here(pl),
    'stages_2': lambda pl: 2 in _here(pl),
    'stages_3': lambda pl: 3 in _here(pl),
    'odd_stages': lambda pl: any(n % 2 == 1 for n in _here(pl)),
    'slice_starts_in_chunk': lambda pl: any(b % (p.nR * p.nS) != 0 for p in pl.phases for b, e in _stages(pl, p)[2] if e > b),
    'tile_spans_images': lambda pl: pl.geom_n > 1 and any(p.Ptot // pl.geom_n % pl.bp != 0 for p in pl.phases),
    # (a tile holds pixels of ONE phase: the last tile of a phase is ragged and the next tile begins the next phase)
    'tile_spans_phases': lambda pl: pl.nphase > 1 and any(p.Ptot % pl.bp != 0 for p in pl.phases[:-1]),
    'phases_16': lambda pl: pl.nphase == 16,
    'nonsquare': lambda pl: pl.geom_rs[0] != pl.geom_rs[1],
    'm_33': lambda pl: pl.M == 33,
    'm_tile_plus_8': lambda pl: pl.M == pl.bm + 8,
    'plane_under_filter': lambda pl: pl.geom_hw[0] < pl.geom_rs[0] or pl.geom_hw[1] < pl.geom_rs[1],
    'all_mirror': lambda pl: pl.mode == 'fwd_reflect' and pl.geom_pad >= max(pl.geom_hw) - 1,
    'p_under_32': lambda pl: all(p.Ptot < 32 for p in pl.phases),
    'bias': lambda pl: pl.has_bias,
    'clamped_tile': lambda pl: pl.forced_tile and pl.forced_tile // 1000 != pl.bm,
})


class _PlanView(object):
    """a Plan plus the fields of the case that the claims above read (the namedtuple of conv_f32_cases is not edited)"""

    def __init__(self, case, pl):
        self.__dict__.update(pl._asdict())
        N, C, H, W, K, Rr, S, st, pad, pm = case.geom
        self.geom_rs, self.geom_hw, self.geom_pad, self.geom_n = (Rr, S), (H, W), pad, N
        self.has_bias, self.forced_tile = case.bias, case.tile


def holds(case, claim):
    return bool(CLAIMS[claim](_PlanView(case, hgemm_plan(case))))


# ---- data, reference, bound ------------------------------------------------------------------------------------------------------------------
def shapes(case):
    """(shape of the gathered tensor, shape of the produced tensor, rows of the pass's weight matrix)"""
    N, C, H, W, K, Rr, S, st, pad, pm = case.geom
    P, Q = out_size(H, Rr, st, pad), out_size(W, S, st, pad)
    if case.pass_ == 'fwd':
        return (N, C, H, W), (N, K, P, Q), K
    return (N, K, P, Q), (N, C, H, W), C


def reference(case, src, w, b):
    return split_arith.reference(case.pass_, case.geom, src, w, b)


@functools.lru_cache(maxsize=None)
def _data(pass_, geom, half, bias, wexp, kind, seed):
    c = Case('', '', pass_, geom, 0, 0, half, 0, bias, wexp, kind, (), (), seed)
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    sshape, oshape, M = shapes(c)
    fwd = pass_ == 'fwd'
    g = torch.Generator().manual_seed(sum(v * (i + 1) * 7919 for i, v in enumerate(geom)) + 104729 * seed + (17 if fwd else 0)
                                      + 1299709 * KINDS.index(kind) + 15485863 * int(half))
    rowexp, b = None, None
    if kind == 'signed':
        src, w = _signed(g, *sshape), _signed(g, K, C, Rr, S)
        if half:
            src, w = _bf16(src), _bf16(w)
        w = w * 2.0 ** wexp
        b = _signed(g, M) if bias else None
    elif kind in ('xlow', 'xlow16'):
        top = 2 ** (8 if half else 15) - 1
        src = _ints(g, -16, 16, sshape) if kind == 'xlow16' else _ints(g, -top, top, sshape)
        src.view(-1)[src.numel() // 2 + 3] = top
        w = _ints(g, -1, 1, (K, C, Rr, S))
        b = _ints(g, -64, 64, (M,)) if bias else None
    else:
        assert kind == 'wlow' and not bias
        top = 2 ** (8 if half else 15) - 1
        src = _ints(g, -1, 1, sshape)
        w = _ints(g, -top, top, (K, C, Rr, S))
        if not half:
            rowexp = torch.randint(-20, 21, (M,), generator=g)
            rowexp[0], rowexp[1] = 20, -20
            mag = torch.pow(2.0, rowexp.float())
            w = w * (mag.view(K, 1, 1, 1) if fwd else mag.view(1, C, 1, 1))
    ref, A = reference(c, src, w, b)
    assert tuple(ref.shape) == oshape
    return Data(src, w, b, ref, A, rowexp)


def data(case):
    """(src, w, bias, float64 reference BEFORE the activation, A, row exponents) of a case on the CPU: made once, shared, never written
    to.  w is the convolution's weight tensor [K][C][R][S] whatever the pass"""
    return _data(case.pass_, case.geom, case.half, case.bias, case.wexp, case.kind, case.seed)


def slope_of(case):
    return split_arith.slope_of(case.kind)


def expected(case, ref=None):
    d = data(case)
    return R.activation(d.ref if ref is None else ref, case.act, slope_of(case))


def kp_map(case, pl):
    """per element: Kp of the phase that owns it; 0 where no phase writes"""
    d = data(case)
    n = torch.zeros_like(d.ref)
    if case.pass_ == 'fwd' or pl.stride == 1:
        return n + pl.phases[0].Kp
    for p in pl.phases:
        n[:, :, p.fy::pl.stride, p.fx::pl.stride] = p.Kp
    return n


def bounds(case, A=None, ref=None):
    """(E of the accumulation, the bound on |y - expected|, expected) per element"""
    d = data(case)
    pl = hgemm_plan(case)
    A = d.A if A is None else A
    want = expected(case, ref)
    kp = kp_map(case, pl)
    if not case.half:
        E = (2 * (3 * kp + pl.ks + 8) * U + 2.0 ** -20) * A
        return E, E + (2.0 ** -22 * want.abs() if case.act else 0.0), want
    E = 2 * (kp + pl.ks + 8) * U * A
    return E, 2.0 ** -8 * (want.abs() + E) + E + 2.0 ** -22 * want.abs() + 1e-30, want


def condition(case):
    """(largest bound of the case on the LINEAR result, what it has to stay under: half the smallest possible term)"""
    return float(bounds(case._replace(act=0))[1].max()), TERM_MIN * 2.0 ** case.wexp / 2


def quanta(case):
    """exact kinds: the largest A of the case in units of its quantum (1, or 2^j of the row for 'wlow' on fp32 tensors)"""
    return split_arith.quanta(data(case))


def exact_expected(case):
    """section B: the float64 result as the call stores it (bf16 tensors: rounded to nearest-even once)"""
    want = expected(case)
    if case.half:
        assert bool((want.float().double() == want).all())
        return _bf16(want.float()).double()
    return want


# ---- the kernel's arithmetic in torch --------------------------------------------------------------------------------------------------------
def row_maxima(case, w):
    return w.abs().amax(dim=(1, 2, 3)) if case.pass_ == 'fwd' else w.abs().amax(dim=(0, 2, 3))


def _axis(fwd, reflect, p, tap, n, st, pad):
    """igemm.h axis_entry for every (tap, pixel): (index, in range)"""
    if not fwd:
        t = p.view(1, -1) + pad - tap.view(-1, 1)
        i = torch.div(t, st, rounding_mode='floor')
        return i, (t >= 0) & (i < n)
    i = p.view(1, -1) * st - pad + tap.view(-1, 1)
    if reflect:
        i = i.abs()
        i = torch.where(i >= n, 2 * (n - 1) - i, i)
        return i, torch.ones_like(i, dtype=torch.bool)
    return i, (i >= 0) & (i < n)


def phase_operands(case, p, src, w, swap=None):
    """one phase as the kernel walks it: (weights [M][stages][16], gathered pixels [Ptot][stages][16], (n, py, px) of the pixels); the
    stage index is chunk * T + tap.  swap = (pixel, t0, t1): that pixel's offset-table entries of taps t0 and t1 change places"""
    N, C, H, W, K, Rr, S, st, pad, pm = case.geom
    fwd = case.pass_ == 'fwd'
    Ng, Cg, Hg, Wg = src.shape
    T = p.nR * p.nS
    pg = torch.arange(p.Ptot)
    n, rem = pg // (p.Hs * p.Ws), pg % (p.Hs * p.Ws)
    ostep = 1 if fwd else st
    py, px = (rem // p.Ws) * ostep + p.fy, (rem % p.Ws) * ostep + p.fx
    r0, s0, tstep = (0, 0, 1) if fwd else ((p.fy + pad) % st, (p.fx + pad) % st, st)
    t = torch.arange(T)
    r, s = r0 + (t // p.nS) * tstep, s0 + (t % p.nS) * tstep
    y, yok = _axis(fwd, pm == 1, py, r, Hg, st, pad)
    x, xok = _axis(fwd, pm == 1, px, s, Wg, st, pad)
    flat = torch.where(yok & xok, n.view(1, -1) * (Hg * Wg) + y * Wg + x, torch.full_like(y, Ng * Hg * Wg))      # the zero row: OOB
    if swap is not None:
        q, t0, t1 = swap
        flat = flat.clone()
        flat[t0, q], flat[t1, q] = flat[t1, q].clone(), flat[t0, q].clone()
    rows = torch.cat([src.permute(0, 2, 3, 1).reshape(Ng * Hg * Wg, Cg), torch.zeros(1, Cg)])
    G = rows[flat].view(T, p.Ptot, Cg // 16, 16).permute(1, 2, 0, 3).reshape(p.Ptot, (Cg // 16) * T, 16)
    if fwd:
        Aw = w.reshape(K, C // 16, 16, Rr * S).permute(0, 1, 3, 2).reshape(K, (C // 16) * T, 16)
    else:
        ws = w[:, :, r0::st, s0::st]
        assert tuple(ws.shape[2:]) == (p.nR, p.nS)
        Aw = ws.permute(1, 0, 2, 3).reshape(C, K // 16, 16, T).permute(0, 1, 3, 2).reshape(C, (K // 16) * T, 16)
    return Aw.contiguous(), G.contiguous(), (n, py, px)


PERTURBATIONS = ('drop_lh', 'drop_hl', 'swap_taps', 'zero_4ch', 'last_stage_row_T', 'isw_next_row', 'dead_stage_repeats',
                 'slice_doubled', 'slice_lost', 'bias_every_slice')


def emulate(case, perturb=None, exact=None):
    """the call's result as float64 (bf16 tensors: rounded to bf16 once).  perturb, one of PERTURBATIONS:
      drop_lh / drop_hl      the (l,h) / (h,l) piece product is not accumulated
      swap_taps              two taps of one offset-table row change places for one pixel column
      zero_4ch               channels 4 .. 7 of one pixel are stored as zero in one stage (the BP = 64 store of one `ksub & 1` half)
      last_stage_row_T       the last live stage of the last slice gathers through the all-out-of-range table row T
      isw_next_row           iswS[ml] is taken from the next row of the tile
      dead_stage_repeats     the dead stage of an odd count runs the slice's first stage again
      slice_doubled / _lost  a slice boundary moved by one stage: the first slice runs one stage more / the second starts one stage late
      bias_every_slice       every slice of a K split adds the bias
    Returns None where the perturbation does not apply to the case (no split, no bias, one tap, bf16 tensors without low pieces)"""
    d = data(case)
    pl = hgemm_plan(case)
    sshape, oshape, M = shapes(case)
    exact = (case.kind != 'signed') if exact is None else exact
    if perturb in ('drop_lh', 'drop_hl', 'isw_next_row') and case.half:
        return None
    if perturb in ('slice_doubled', 'slice_lost', 'bias_every_slice') and (pl.ks == 1 or (perturb == 'bias_every_slice' and d.b is None)):
        return None
    if perturb == 'swap_taps' and all(p.nR * p.nS < 2 for p in pl.phases):
        return None
    if perturb == 'dead_stage_repeats' and not any(n % 2 == 1 for n in _here(pl)):
        return None
    out = torch.zeros(oshape)
    wr = d.w
    if case.half:
        sx, sw = 1.0, torch.ones(M)
    else:
        sx = pow2_scale(float(d.src.abs().max()))
        sw = torch.tensor([pow2_scale(float(v)) for v in row_maxima(case, wr)])
    isx, isw = 1.0 / sx, 1.0 / sw
    if perturb == 'isw_next_row':
        isw = torch.cat([isw[1:], isw[-1:]])

    def prod(a, b):      # [stages][M][Ptot]: the 16 products of every stage summed exactly, then ONE fp32 number
        r = torch.einsum('msk,psk->smp', a.double(), b.double())
        if exact:
            assert bool((r.float().double() == r).all()), 'a stage sum is no fp32 number'
        return r.float()

    for p in pl.phases:
        T = p.nR * p.nS
        swap = (p.Ptot // 2, 0, T - 1) if perturb == 'swap_taps' and T >= 2 else None
        Aw, G, (n, py, px) = phase_operands(case, p, d.src, wr, swap)
        nst, per, slices = _stages(pl, p)
        if case.half:
            xp, wp = [G], [_bf16(Aw)]
            pairs = ((0, 0),)
        else:
            xp, wp = list(split2h(G * sx)), list(split2h(Aw * sw.view(M, 1, 1)))
            pairs = ((1, 0), (0, 1), (0, 0))              # (weight piece, pixel piece): (l,h) (h,l) (h,h)
            if perturb == 'drop_lh':
                pairs = pairs[1:]
            elif perturb == 'drop_hl':
                pairs = (pairs[0], pairs[2])
        live = [z for z, (b, e) in enumerate(slices) if e > b]
        if perturb == 'zero_4ch':
            for t_ in xp:
                t_[p.Ptot // 2, nst // 2, 4:8] = 0.0
        if perturb == 'last_stage_row_T' and live:
            for t_ in xp:
                t_[:, slices[live[-1]][1] - 1, :] = 0.0
        prods = [prod(wp[a], xp[b]) for a, b in pairs]
        total = None
        for z, (b, e) in enumerate(slices):
            order = list(range(b, e))
            if perturb == 'dead_stage_repeats' and len(order) % 2 == 1:
                order.append(b)
            if perturb == 'slice_doubled' and z == 0 and e < nst:
                order.append(e)
            if perturb == 'slice_lost' and z == 1 and e > b:
                order = order[1:]
            acc = torch.zeros(M, p.Ptot)
            for s_ in order:
                for pr in prods:
                    acc = acc + pr[s_]
            part = (acc * isx) * isw.view(M, 1)
            if perturb == 'bias_every_slice':
                part = part + d.b.view(M, 1)
            total = part if total is None else total + part
        out[n, :, py, px] = total.t()
    if d.b is not None and perturb != 'bias_every_slice':
        out = out + d.b.view(1, -1, 1, 1)
    y = R.activation(out, case.act, slope_of(case))
    if case.half:
        y = _bf16(y)
    return y.double()


def gate(case, y):
    """does a result pass the gate of the case's section?  (section A: every element inside the bound; section B: every element exact)"""
    if case.kind == 'signed':
        E, bound, want = bounds(case)
        return bool(((y - want).abs() <= bound).all())
    return bool((y == exact_expected(case)).all())


# ---- the pack, restated -----------------------------------------------------------------------------------------------------------------------
def packed_fp32(case, w):
    """pcgan_conv2d_pack_weights' image of the A matrices, one after the other: float32 [sum over the phases of M x Kp]"""
    pl = hgemm_plan(case)
    src0 = torch.zeros(shapes(case)[0])
    return torch.cat([phase_operands(case, p, src0, w)[0].reshape(-1) for p in pl.phases])


def packed_presplit(case, w):
    """pcgan_conv2d_hgemm_pack's bytes (uint8): every aligned group of four floats of a row replaced by [4 high | 4 low] fp16 pieces of the
    values scaled by pow2_scale(rowmax) of the row; and the row maxima"""
    pl = hgemm_plan(case)
    M = shapes(case)[2]
    rowmax = row_maxima(case, w)
    sw = torch.tensor([pow2_scale(float(v)) for v in rowmax])
    src0 = torch.zeros(shapes(case)[0])
    parts = []
    for p in pl.phases:
        Aw = phase_operands(case, p, src0, w)[0].reshape(M, -1) * sw.view(M, 1)
        h = Aw.half()
        l = (Aw - h.float()).half()
        parts.append(torch.cat([h.view(M, -1, 1, 4), l.view(M, -1, 1, 4)], dim=2).reshape(-1))
    return torch.cat(parts).view(torch.uint8), rowmax


# ---- section C ---------------------------------------------------------------------------------------------------------------------------
RANGE_KINDS = ('wide_range', 'huge', 'tiny')


def range_data(case, kind):
    """randn operands under the kinds of tests/test_gpu_bf16x6.py; returns (src, w, float64 reference)"""
    sshape, oshape, M = shapes(case)
    N, C, H, W, K, Rr, S, st, pad, pm = case.geom
    g = torch.Generator().manual_seed(3000 + RANGE_KINDS.index(kind) + (17 if case.pass_ == 'fwd' else 0) + case.tile)
    src = torch.randn(*sshape, generator=g)
    w = torch.randn(K, C, Rr, S, generator=g) * 0.05
    # wide_range: magnitudes over twelve decades inside one tensor
    src, w = range_scale(kind, g, src, w, (12, -9), (6, -3), (1e-30, 1e-6), (1e12, 1e8))
    f = _fwd64 if case.pass_ == 'fwd' else _dgrad64
    return src, w, f(src.double(), w.double(), None, case.geom)


MAXPOS_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4096, 4104, 4107)


def maxima_slots(n):
    """split_arith.maxima_slots at NT = 256: from 4 NT = 1024 slots on the end of the first 4-in-flight round, from 16 NT = 4096 on the
    second and the third load in flight"""
    return split_arith.maxima_slots(n, NT)


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
CASES = []
BOTH, F32_ONLY = (False, True), (False,)


def _add(sect, name, pass_, geom, want, claims=(), tile=0, ks=0, halves=BOTH, act=0, bias=None, wexp=0, kind='signed', seed=0):
    """want = (mode, bm, bp, ks, nphase); the form follows the storage type"""
    if bias is None:
        bias = pass_ == 'fwd' and kind != 'wlow'
    for half in halves:
        CASES.append(Case(sect, '%s-%s%s-%s' % (name, kind, '-' + ACT_NAMES[act] if act else '', 'bf16' if half else 'fp32'), pass_, tuple(geom),
                          tile, ks, half, act, bias, wexp, kind, (FORMS[half],) + tuple(want), tuple(claims), seed))


# the base shape of each mode on M produced channels: 16 gathered channels x 3x3 = 144 terms, 9 stages (odd: a dead stage), both storage types
BASE = {
    'fwd_zero': ('fwd', lambda m: (2, 16, 11, 13, m, 3, 3, 1, 1, 0), 1),         # 143 pixels per image: tiles span the two images
    'fwd_reflect': ('fwd', lambda m: (3, 16, 7, 10, m, 3, 3, 1, 1, 1), 1),       # 70 pixels per image
    'dgrad': ('dgrad', lambda m: (2, m, 13, 11, 16, 3, 3, 1, 1, 0), 1),
}
M_OF = {64: (33, 64, 65, 128, 129, 136), 128: (65, 128, 129, 136)}
EXACT_ACT = {'fwd_zero': 1, 'fwd_reflect': 2, 'dgrad': 0}


def _m_claims(m, bm):
    return (('m_33',) if m == 33 else ()) + (('m_tile_plus_8',) if m == bm + 8 else ()) + (('m_ragged',) if m % bm else ()) + \
        (('m_blocks',) if m > bm else ())


for _mode in MODES:
    _pass, _gf, _nph = BASE[_mode]
    for _t in TILES:
        _bm, _bp = _t // 1000, _t % 1000
        # A: M in {33, 64, 65, 128, 129, 136} where the tile admits it (BM = 128 runs from 65 rows on), whole; the data gradient with a bias
        # on every other row count
        for _i, _m in enumerate(M_OF[_bm]):
            _add('A', '%s-3x3-m%d-%d' % (_mode, _m, _t), _pass, _gf(_m), (_mode, _bm, _bp, 1, _nph),
                 _m_claims(_m, _bm) + ('odd_stages', 'p_ragged', 'tile_spans_images') + (('bias',) if _pass == 'fwd' or _i % 2 == 0 else ()),
                 tile=_t, bias=_pass == 'fwd' or _i % 2 == 0)
        # A: the K split of every instantiation: 9 stages in slices of 5 + 4 (a short last slice)
        _add('A', '%s-3x3-m%d-%d-ks2' % (_mode, _bm + 8, _t), _pass, _gf(_bm + 8), (_mode, _bm, _bp, 2, _nph),
             ('split', 'short_slice', 'm_tile_plus_8', 'odd_stages'), tile=_t, ks=2, bias=True)
        # B: xlow and wlow on every instantiation, whole and split
        for _kind in ('xlow', 'wlow'):
            _add('B', '%s-3x3-m%d-%d' % (_mode, _bm + 8, _t), _pass, _gf(_bm + 8), (_mode, _bm, _bp, 1, _nph), ('m_tile_plus_8', 'odd_stages'),
                 tile=_t, kind=_kind, act=EXACT_ACT[_mode] if _kind == 'xlow' else 0, bias=_kind == 'xlow')
            _add('B', '%s-3x3-m%d-%d-ks2' % (_mode, 72, _t), _pass, _gf(72), (_mode, _bm, _bp, 2, _nph), ('split', 'short_slice'),
                 tile=_t, ks=2, kind=_kind, bias=_kind == 'xlow')

# A: Ptot in {BP - 1, BP, BP + 1} and under 32 pixels, for every instantiation.  1x1 on 32 channels (two stages, a chunk wrap at each);
# 127 is prime and 129 = 3 x 43, so these planes are one row
PIX = {127: (1, 1, 127), 128: (2, 8, 8), 129: (3, 1, 43), 63: (1, 7, 9), 64: (1, 8, 8), 65: (1, 5, 13), 25: (1, 5, 5)}
for _mode in MODES:
    _pm = 1 if _mode == 'fwd_reflect' else 0
    for _t in TILES:
        _bm, _bp = _t // 1000, _t % 1000
        for _px in (_bp - 1, _bp, _bp + 1, 25):
            _n, _h, _w = PIX[_px]
            _m = 72 if _bm == 128 else 40
            _g = (_n, 32, _h, _w, _m, 1, 1, 1, 0, _pm) if _mode != 'dgrad' else (_n, _m, _h, _w, 32, 1, 1, 1, 0, 0)
            _add('A', '%s-1x1-p%d-%d' % (_mode, _px, _t), 'fwd' if _mode != 'dgrad' else 'dgrad', _g, (_mode, _bm, _bp, 1, 1),
                 ('stages_2',) + (('p_under_32',) if _px == 25 else ()) + (('p_ragged',) if _px % _bp else ()) + (('p_blocks',) if _px > _bp else ()),
                 tile=_t, bias=_px != _bp)

# What follows runs on EVERY mode x tile (and both storage types where the condition allows: bf16 tensors need Kp <= 144, so 4x4 / 5x5 / 3x5
# on 16 channels run on fp32 tensors only)
FILTERS = ((1, 1, 0), (1, 2, 0), (1, 3, 1), (2, 2, 1), (1, 5, 2), (3, 3, 1), (4, 4, 1), (5, 5, 2), (3, 5, 2), (2, 3, 0))      # (R, S, pad)


def _geom(mode, n, cg, h, w, m, r, s, st, pad):
    """the convolution that gathers cg channels of an h x w plane (forward: its input; data gradient: the CONVOLUTION's input plane, the
    gathered dy is smaller) and produces m"""
    return (n, cg, h, w, m, r, s, st, pad, 1 if mode == 'fwd_reflect' else 0) if mode != 'dgrad' else (n, m, h, w, cg, r, s, st, pad, 0)


for _mode in MODES:
    _ps = 'fwd' if _mode != 'dgrad' else 'dgrad'
    for _t in TILES:
        _bm, _bp = _t // 1000, _t % 1000
        _m = 72 if _bm == 128 else 40
        # A: filters 1x1, 1x2, 1x3, 2x2, 1x5, 3x3, 4x4, 5x5, 3x5, 2x3 on 16 channels
        for _r, _s, _pad in FILTERS:
            _add('A', '%s-%dx%d-%d' % (_mode, _r, _s, _t), _ps, _geom(_mode, 2, 16, 9, 10, _m, _r, _s, 1, _pad), (_mode, _bm, _bp, 1, 1),
                 (('nonsquare',) if _r != _s else ()) + (('stages_1',) if _r * _s == 1 else ()) + (('stages_2',) if _r * _s == 2 else ())
                 + (('stages_3',) if _r * _s == 3 else ()), tile=_t, halves=BOTH if _r * _s <= 9 else F32_ONLY, bias=True)
        # A + B: C = 32 and 48 at 1x1 (16: above): two and three stages per workgroup with a chunk wrap at every stage; B: 16 too
        for _ci, _c in enumerate((16, 32, 48)):
            _cl = ('stages_%d' % (_ci + 1),) + (('odd_stages',) if _ci != 1 else ())
            if _c != 16:
                _add('A', '%s-1x1-c%d-%d' % (_mode, _c, _t), _ps, _geom(_mode, 2, _c, 9, 10, _m, 1, 1, 1, 0), (_mode, _bm, _bp, 1, 1), _cl, tile=_t, bias=True)
            for _kind in ('xlow', 'wlow'):
                _add('B', '%s-1x1-c%d-%d' % (_mode, _c, _t), _ps, _geom(_mode, 2, _c, 9, 10, _m, 1, 1, 1, 0), (_mode, _bm, _bp, 1, 1), _cl, tile=_t,
                     kind=_kind, bias=_kind == 'xlow')
        # A: zero padding 0 .. R - 1: 0 and 2 at 3x3 (1: the base shape), 0 at 2x2 (1: the filter list); fp32 tensors: 0, 1, 3, 4 at 5x5 and
        # 0, 2, 3 at 4x4 (the filter list runs 5x5 at pad 2 and 4x4 at pad 1)
        if _mode != 'fwd_reflect':
            for _pad in (0, 2):
                _add('A', '%s-3x3p%d-%d' % (_mode, _pad, _t), _ps, _geom(_mode, 2, 16, 9, 10, _m, 3, 3, 1, _pad), (_mode, _bm, _bp, 1, 1), (), tile=_t,
                     bias=True)
            _add('A', '%s-2x2p0-%d' % (_mode, _t), _ps, _geom(_mode, 2, 16, 9, 10, _m, 2, 2, 1, 0), (_mode, _bm, _bp, 1, 1), (), tile=_t, bias=True)
            for _pad, _h, _w in ((0, 9, 8), (1, 9, 8), (3, 6, 7), (4, 6, 7)):
                _add('A', '%s-5x5p%d-%d' % (_mode, _pad, _t), _ps, _geom(_mode, 2, 16, _h, _w, _m, 5, 5, 1, _pad), (_mode, _bm, _bp, 1, 1), (), tile=_t,
                     halves=F32_ONLY, bias=True)
            for _pad, _h, _w in ((0, 9, 8), (2, 8, 7), (3, 6, 7)):
                _add('A', '%s-4x4p%d-%d' % (_mode, _pad, _t), _ps, _geom(_mode, 2, 16, _h, _w, _m, 4, 4, 1, _pad), (_mode, _bm, _bp, 1, 1), (), tile=_t,
                     halves=F32_ONLY, bias=True)
        # A: strides 2 and 4 forward (3x3; fp32 tensors also 4x4 stride 4: 24 pixels)
        if _mode != 'dgrad':
            _add('A', '%s-3x3s2-%d' % (_mode, _t), 'fwd', _geom(_mode, 2, 16, 13, 11, _m, 3, 3, 2, 1), (_mode, _bm, _bp, 1, 1), ('p_ragged',), tile=_t)
            _add('A', '%s-3x3s4-%d' % (_mode, _t), 'fwd', _geom(_mode, 3, 16, 15, 13, _m, 3, 3, 4, 1), (_mode, _bm, _bp, 1, 1), ('p_ragged',), tile=_t)
            _add('A', '%s-4x4s4-%d' % (_mode, _t), 'fwd', _geom(_mode, 2, 16, 15, 10, _m, 4, 4, 4, 1), (_mode, _bm, _bp, 1, 1), ('p_under_32',), tile=_t,
                 halves=F32_ONLY)
        # A: a bias with each of the five activations forward (tanh and sigmoid: weights times 2^-3, |ref| of a few units)
        if _mode != 'dgrad':
            for _a in range(1, 5):      # (none: the base shape)
                _add('A', 'act-%s-%d' % (_mode, _t), 'fwd', BASE[_mode][1](_m), (_mode, _bm, _bp, 1, 1), ('bias',), tile=_t, act=_a,
                     wexp=-3 if _a >= 3 else 0, seed=1)
        # A: reflection with pad up to H - 1 (every row and column has a mirror image) and planes smaller than the filter
        if _mode == 'fwd_reflect':
            _add('A', 'fwd_reflect-3x3p2-h3-%d' % _t, 'fwd', (3, 16, 3, 3, _m, 3, 3, 1, 2, 1), (_mode, _bm, _bp, 1, 1), ('all_mirror',), tile=_t)
            _add('A', 'fwd_reflect-3x3p1-h2-%d' % _t, 'fwd', (3, 16, 2, 2, _m, 3, 3, 1, 1, 1), (_mode, _bm, _bp, 1, 1),
                 ('all_mirror', 'plane_under_filter', 'p_under_32'), tile=_t)
            _add('A', 'fwd_reflect-5x5p2-h3-%d' % _t, 'fwd', (3, 16, 3, 3, _m, 5, 5, 1, 2, 1), (_mode, _bm, _bp, 1, 1),
                 ('all_mirror', 'plane_under_filter', 'p_under_32'), tile=_t, halves=F32_ONLY)
            _add('A', 'fwd_reflect-5x5p4-h5-%d' % _t, 'fwd', (2, 16, 5, 6, _m, 5, 5, 1, 4, 1), (_mode, _bm, _bp, 1, 1), (), tile=_t, halves=F32_ONLY)
        # A + B: the data gradient of 3x3 stride 2 (phases of 1, 2, 2, 4 taps and 42, 35, 36, 30 pixels per image: the last tile of a phase
        # is ragged and the next begins the next phase), of 4x4 stride 2 (four phases of 4 taps) and of 5x5 stride 4 with pad 2: 16 phases of
        # 1, 2 or 4 taps and at most 24 pixels -- each with a bias
        if _mode == 'dgrad':
            _add('A', 'dgrad-3x3s2-%d' % _t, 'dgrad', (2, _m, 13, 11, 16, 3, 3, 2, 1, 0), ('dgrad', _bm, _bp, 1, 4),
                 ('phases_differ', 'tile_spans_phases', 'stages_1', 'stages_2', 'bias'), tile=_t, bias=True)
            _add('B', 'dgrad-3x3s2-%d' % _t, 'dgrad', (2, _m, 13, 11, 16, 3, 3, 2, 1, 0), ('dgrad', _bm, _bp, 1, 4),
                 ('phases_differ', 'tile_spans_phases'), tile=_t, kind='xlow', bias=True)
            _add('A', 'dgrad-4x4s2-%d' % _t, 'dgrad', (2, _m, 11, 9, 16, 4, 4, 2, 1, 0), ('dgrad', _bm, _bp, 1, 4), ('tile_spans_phases', 'bias'), tile=_t, bias=True)
            for _kind in ('signed', 'xlow', 'wlow'):
                _add('A' if _kind == 'signed' else 'B', 'dgrad-5x5s4p2-%d' % _t, 'dgrad', (2, _m, 13, 11, 16, 5, 5, 4, 2, 0), ('dgrad', _bm, _bp, 1, 16),
                     ('phases_16', 'phases_differ', 'tile_spans_phases', 'p_under_32') + (('bias',) if _kind != 'wlow' else ()), tile=_t, kind=_kind,
                     bias=_kind != 'wlow')

# the activations through the split-K reduce (fp32 and bf16 stores)
for _a in range(5):
    _add('A', 'act-fwd_reflect-128128-ks2', 'fwd', (3, 16, 7, 10, 72, 3, 3, 1, 1, 1), ('fwd_reflect', 128, 128, 2, 1), ('bias', 'split'), tile=128128, ks=2,
         act=_a, wexp=-3 if _a >= 3 else 0, seed=1)
    _add('A', 'act-fwd_zero-64064-ks2', 'fwd', (2, 16, 11, 13, 40, 3, 3, 1, 1, 0), ('fwd_zero', 64, 64, 2, 1), ('bias', 'split'), tile=64064, ks=2,
         act=_a, wexp=-3 if _a >= 3 else 0, seed=1)
_add('A', 'dgrad-4x4s2-k32-128128-ks2', 'dgrad', (2, 72, 11, 9, 32, 4, 4, 2, 1, 0), ('dgrad', 128, 128, 2, 4), ('split', 'tile_spans_phases'),
     tile=128128, ks=2, bias=True)
_add('B', 'fwd_reflect-3x3p2-h3-64064', 'fwd', (3, 16, 3, 3, 40, 3, 3, 1, 2, 1), ('fwd_reflect', 64, 64, 1, 1), ('all_mirror',), tile=64064, kind='xlow')
# pixels that no phase writes: 1x1 stride 2 (three of four) and 3x3 stride 4 (7 of 16 phases): no bias (the call with one is refused:
# NEED_ZERO_REFUSED below), those pixels exactly +0, no split workspace whatever is forced
_add('A', 'dgrad-1x1s2-64128', 'dgrad', (2, 40, 15, 9, 32, 1, 1, 2, 0, 0), ('dgrad', 64, 128, 1, 1), ('need_zero', 'stages_2'), tile=64128, ks=4, bias=False)
_add('A', 'dgrad-1x1s2-128128', 'dgrad', (2, 72, 15, 9, 16, 1, 1, 2, 0, 0), ('dgrad', 128, 128, 1, 1), ('need_zero', 'stages_1'), tile=128128, bias=False)
_add('A', 'dgrad-3x3s4-128064', 'dgrad', (2, 72, 14, 13, 16, 3, 3, 4, 1, 0), ('dgrad', 128, 64, 1, 9), ('need_zero', 'stages_1'), tile=128064, bias=False)
_add('A', 'dgrad-3x3s4-64064', 'dgrad', (2, 40, 14, 13, 16, 3, 3, 4, 1, 0), ('dgrad', 64, 64, 1, 9), ('need_zero', 'stages_1'), tile=64064, bias=False)
_add('B', 'dgrad-3x3s4-64064', 'dgrad', (2, 40, 14, 13, 16, 3, 3, 4, 1, 0), ('dgrad', 64, 64, 1, 9), ('need_zero',), tile=64064, kind='xlow', bias=False)
_add('B', 'dgrad-1x1s2-64128', 'dgrad', (2, 40, 15, 9, 32, 1, 1, 2, 0, 0), ('dgrad', 64, 128, 1, 1), ('need_zero',), tile=64128, kind='wlow', bias=False)

# A + B (fp32 tensors: more than 144 terms): the split with an empty last slice (25 stages, 6 slices of 5), slices that begin inside a
# chunk (C = 32, 3x3, ks 4: 18 stages, slices begin at stages 0, 5, 10, 15 of chunks of 9)
for _kind in ('signed', 'xlow', 'wlow'):
    _sect = 'A' if _kind == 'signed' else 'B'
    _b = _kind != 'wlow'
    _add(_sect, 'fwd_zero-5x5-128128-ks6', 'fwd', (2, 16, 9, 9, 72, 5, 5, 1, 2, 0), ('fwd_zero', 128, 128, 6, 1), ('split', 'empty_slice', 'odd_stages'),
         tile=128128, ks=6, halves=F32_ONLY, kind=_kind, bias=_b)
    _add(_sect, 'fwd_reflect-5x5-64064-ks6', 'fwd', (2, 16, 7, 9, 40, 5, 5, 1, 2, 1), ('fwd_reflect', 64, 64, 6, 1), ('split', 'empty_slice'),
         tile=64064, ks=6, halves=F32_ONLY, kind=_kind, bias=_b)
    _add(_sect, 'dgrad-5x5-128064-ks6', 'dgrad', (2, 72, 9, 8, 16, 5, 5, 1, 2, 0), ('dgrad', 128, 64, 6, 1), ('split', 'empty_slice'),
         tile=128064, ks=6, halves=F32_ONLY, kind=_kind, bias=_b)
    _add(_sect, 'fwd_zero-3x3-c32-64128-ks4', 'fwd', (2, 32, 9, 10, 40, 3, 3, 1, 1, 0), ('fwd_zero', 64, 128, 4, 1),
         ('split', 'slice_starts_in_chunk', 'short_slice', 'odd_stages', 'stages_3'), tile=64128, ks=4, halves=F32_ONLY, kind=_kind, bias=_b)
    _add(_sect, 'dgrad-3x3-k32-128128-ks4', 'dgrad', (2, 72, 9, 10, 32, 3, 3, 1, 1, 0), ('dgrad', 128, 128, 4, 1),
         ('split', 'slice_starts_in_chunk', 'short_slice'), tile=128128, ks=4, halves=F32_ONLY, kind=_kind, bias=_b)

# what the contract refuses: a forced 128-row tile on <= 64 rows runs as 64 rows; a forced split is cut to stages / 4
_add('A', 'clamp-fwd_zero-m33-128128', 'fwd', (2, 16, 11, 13, 33, 3, 3, 1, 1, 0), ('fwd_zero', 64, 128, 1, 1), ('clamped_tile', 'm_33'), tile=128128)
_add('A', 'clamp-dgrad-m64-128064', 'dgrad', (2, 64, 13, 11, 16, 3, 3, 1, 1, 0), ('dgrad', 64, 64, 1, 1), ('clamped_tile',), tile=128064, bias=True)
_add('A', 'clamp-fwd_reflect-ks8-64064', 'fwd', (3, 16, 7, 10, 40, 3, 3, 1, 1, 1), ('fwd_reflect', 64, 64, 2, 1), ('split',), tile=64064, ks=8)

BY_NAME = collections.OrderedDict(('%s.%s' % (c.sect, c.name), c) for c in CASES)
assert len(BY_NAME) == len(CASES), 'case names must be unique'

# data gradients with pixels that no phase writes take no bias: the call is refused (conv2d_bwd_data: bias with uncovered phases)
NEED_ZERO_REFUSED = (BY_NAME['A.dgrad-1x1s2-64128-signed-fp32']._replace(bias=True), BY_NAME['A.dgrad-3x3s4-128064-signed-bf16']._replace(bias=True))

# section C (fp32 tensors)
MAXPOS = {'fwd': Case('C', 'maxpos-fwd', 'fwd', (2, 16, 9, 10, 40, 3, 3, 1, 1, 0), 64064, 0, False, 1, True, 0, 'xlow16', (FORMS[False], 'fwd_zero', 64, 64, 1, 1), (), 0),
          'dgrad': Case('C', 'maxpos-dgrad', 'dgrad', (2, 72, 9, 10, 16, 3, 3, 1, 1, 0), 128128, 0, False, 0, True, 0, 'xlow16',
                        (FORMS[False], 'dgrad', 128, 128, 1, 1), (), 0)}
RANGE = {(p, t): Case('C', 'range-%s-%d' % (p, t), p, (2, 32, 12, 12, 96, 3, 3, 1, 1, 0) if p == 'fwd' else (2, 96, 12, 12, 32, 3, 3, 1, 1, 0), t, 0, False, 0,
                      False, 0, 'signed', (FORMS[False], 'fwd_zero' if p == 'fwd' else 'dgrad', t // 1000, t % 1000, 1, 1), (), 0)
         for p in ('fwd', 'dgrad') for t in (64128, 128064)}
ZERO = {'fwd': BY_NAME['A.fwd_zero-3x3-m65-64128-signed-fp32'],
        'dgrad': BY_NAME['A.dgrad-3x3s2-128064-signed-fp32']}
# one all-zero weight row on exact data ('xlow' with a bias, no activation): each pass on a 64 x 128 and a 128 x 64 tile
ZERO_ROW = {(p, t): BY_NAME['B.%s-3x3-m%d-%d-xlow%s-fp32' % ('fwd_zero' if p == 'fwd' else 'dgrad', t // 1000 + 8, t, '-relu' if p == 'fwd' else '')]._replace(act=0)
            for p in ('fwd', 'dgrad') for t in (64128, 128064)}
# section D: the pack (forward; a stride-2 data gradient whose phases have 1, 2, 2, 4 taps), M in {33, 136}
PACK = [Case('D', 'pack-%s-m%d' % (p, m), p, (1, 16, 9, 10, m, 3, 3, 1, 1, 0) if p == 'fwd' else (1, m, 13, 11, 32, 3, 3, 2, 1, 0), 0, 0, False, 0, False, 0, k,
             (), (), 0) for p in ('fwd', 'dgrad') for m in (33, 136) for k in ('xlow', 'wlow')]
