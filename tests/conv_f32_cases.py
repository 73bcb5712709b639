"""Case table, data maker, float64 reference and error bound of the fp32-MFMA / small-M convolution tests (a plain module: shared by
tests/test_conv_f32_cases.py, which checks the table on the CPU, and tests/test_gpu_conv_f32.py, which runs it on the GPU).

A case is one direct call of pcgan_conv2d_fwd / pcgan_conv2d_bwd_data: geometry (N, C, H, W, K, R, S, stride, pad, pad_mode) of the
CONVOLUTION (the data gradient gathers its K channels and produces its C), a forced tile / K split (library options "hgemm_tile" /
"hgemm_ks"; they act on layers of more than 32 rows only), the storage type, a fused activation, and `want`: the launch record
(form, mode, bm, bp, ks, nphase) the case is there to hit.  `plan()` restates the host's routing (csrc/igemm_conv.hip: bwd_plan,
choose_tile, launch_igemm; csrc/smallm_conv.hip: launch_smallm) in Python so that the CPU test can hold `want` and the raggedness each
case claims against it without a GPU; the GPU test holds `want` against what the library recorded.

Data: |x|, |w|, |dy|, |bias| uniform in [0.75, 1.25] with independent random signs, so every term of every sum has a magnitude in
[0.5625, 1.5625]; bf16 cases round the activation tensor to bf16 first and the reference sees the stored values (the weights stay fp32:
these kernels take them as fp32).
Reference: split_arith.reference -- oracle.ops_ref.conv2d in float64, its autograd for the data gradient (reflection padding included); the
same call on absolute values gives A, the per-element sum of |terms|.

Bound, fp32 storage, per element:  |y - ref| <= 2 n_eff 2^-24 A,  n_eff = Kp of the element's phase + K slices + 8: the standard bound
of an fp32 sum of that many terms in any order, with a factor 2 for the product rounded before it is added (the fp32 MFMA and the fused
multiply-add round once per term, so this is generous, not tight).  The 8 is the depth of the additions behind the K loop that one term
can pass through, and its parts do not all meet in one element: the bias (1); the three cross-wave adds of the small-M kernels (3); the
mirror gather of the fused reflect gradient, which adds up to four images before the product (3); reflect_fold_kernel, which adds up to
three column images into a value and up to three such values into the result (2 + 3: up to 9 images when a plane is smaller than
2 pad + 2).  The MFMA kernels reach at most 3 + 1 (fused) or 5 + 1 (padded fallback, which never gathers mirrors).  Only a small-M kernel
on the padded grid reaches 3 + 5 + 1 = 9, and there Kp over-counts the K loop by far more than one: each wave sums a quarter of the
channels, and with fewer than four channels Kp counts the padding channels.  Fused activations (1-Lipschitz):  |y - act(ref)| <= bound + 2^-22 |act(ref)|.
Bound, bf16 storage (the form of _bf16_bound in tests/test_gpu_hgemm.py): with E = 2 n_eff 2^-24 A the accumulation term,
    |y - act(ref)| <= 2^-8 (|act(ref)| + E) + E + 2^-22 |act(ref)| + 1e-30
-- half an ulp of the stored bf16 result (2^-8 of its magnitude) plus what was accumulated before the store.
The padded reflect fallback (conv2d_bwd_data_impl: reflection padding without K % 16 == 0, or a plane under 2 pad + 2) computes the
gradient t of the PADDED tensor, stores it in the storage type, and reflect_fold_kernel reads the up to 9 images t_i of an element back,
adds them in fp32 and stores once more.  For bf16 each stored image carries its own half ulp, 2^-8 (|t_i| + E_i), and sum E_i = E
because A is the sum over all images; the fold's adds (and the bias it adds at the end) cost at most 16 * 2^-24 (T + |bias|) with
T = sum |t_i|.  So E above becomes
    E' = E + 2^-8 (T + E) + 2^-20 (T + |bias|)
(T from the float64 gradient of the padded tensor, folded as absolute values).  In fp32 the images are stored exactly and the fold's adds
are inside the 8.

Condition, asserted for every case and every element on the reference alone (tests/test_conv_f32_cases.py, and again before each launch):
bound < 0.5625 / 2, half the smallest possible term -- one lost, doubled or misplaced term in any element fails.  For fp32 that caps a
sum at about 1100 terms; for bf16 storage the half ulp of the result must stay under it too, |ref| < 72, which caps a sum of random signs
at about 200 terms.  That is why the bf16 cases use 16 gathered channels x 9 taps and fewer, why the channel-split strip cases (>= 64
channels), the 7x7 / 11x11 filters on 8 .. 16 channels and the split with an empty last slice (25 stages of 16: 400 terms) run in fp32
only, and why no case holds the 512 -> 1 layer itself (8192 terms): C = 64 / 67 / 115 reach the same code."""
import collections
import functools

import torch
import torch.nn.functional as F

from oracle import ops_ref as R
from split_arith import U, SLOPE, cdiv, out_size, reference

TERM_MIN = 0.75 * 0.75      # the smallest possible |term|; the largest is 1.25 * 1.25
NTAP_FWD, NTAP_MIR, NTAP_CG4 = 25, 9, 49
ACT_NAMES = ('none', 'relu', 'lrelu', 'tanh', 'sigmoid')

Case = collections.namedtuple('Case', 'sect name pass_ geom tile ks half act bias want claims seed')
Plan = collections.namedtuple('Plan', 'form mode bm bp ks nphase M Cg Cgp phases padded need_zero stride kernel small_plane')
Phase = collections.namedtuple('Phase', 'fy fx nR nS Hs Ws Kp Ptot')


def round4(v):
    return (v + 3) & ~3


# ---- the host's routing, restated ------------------------------------------------------------------------------------------------------------
def _chunked_k(Cg, M, Rr, S):
    return Cg % 16 == 0 and M > 4 and Rr * S <= NTAP_FWD


def _cg4_k(Cg, M, Rr, S):
    return round4(Cg) == 4 and M > 4 and Rr * S <= NTAP_CG4


def _tile_blocks(M, pmax, nphase, mm, pp):
    return cdiv(M, mm) * cdiv(pmax, pp) * nphase


def _may_split(M, pmax, nphase, fk):
    if fk > 1:
        return M > 4
    m = 128 if M > 64 else (64 if M > 32 else 32)
    return M > 4 and _tile_blocks(M, pmax, nphase, m, 128) < 192


def _choose_tile(M, pmax, nphase, nst, allow_split, ft, fk):
    m = 128 if M > 64 else (64 if M > 32 else 32)
    p = 128
    if (ft or fk) and M > 32:
        if ft:
            m, p = ft // 1000, ft % 1000
        else:
            if _tile_blocks(M, pmax, nphase, m, p) < 384:
                p = 64
            if m == 128 and _tile_blocks(M, pmax, nphase, m, p) < 384:
                m = 64
        if M <= 64 and m == 128:
            m = 64
        k = fk if fk > 0 else 1
        if not allow_split:
            k = 1
        if k > nst // 4:
            k = max(nst // 4, 1)
        return m, p, k
    if allow_split and _may_split(M, pmax, nphase, fk) and nst >= 32:
        k = min(512 // _tile_blocks(M, pmax, nphase, m, 128), 8, nst // 8)
        if k >= 2:
            return m, 128, k
    if m >= 64 and _tile_blocks(M, pmax, nphase, m, p) < 384:
        p = 64
    if m == 128 and _tile_blocks(M, pmax, nphase, m, p) < 384:
        m = 64
    return m, p, 1


def _bwd_phases(geom):
    """csrc/igemm_conv.hip bwd_plan: (phases, fused, rowfold, padded, need_zero)"""
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    fused = pm == 1 and _chunked_k(K, C, Rr, S) and Rr * S <= NTAP_MIR and H >= 2 * pad + 2 and W >= 2 * pad + 2
    rowfold = fused and pad == 1 and Rr == 3 and st == 1
    padded = pm == 1 and not fused
    Hh, Ww, p = (H + 2 * pad, W + 2 * pad, 0) if padded else (H, W, pad)
    Kgp = round4(K)
    ph, need_zero = [], False
    if rowfold:
        for f in range(3):
            Hs = H - 2 if f == 0 else 1
            ph.append(Phase(0 if f == 0 else (1 if f == 1 else H - 2), 0, Rr, S, Hs, W, Rr * S * Kgp, N * Hs * W))
        return ph, fused, rowfold, padded, need_zero
    for fy in range(st):
        for fx in range(st):
            r0, s0 = (fy + p) % st, (fx + p) % st
            nR = cdiv(Rr - r0, st) if r0 < Rr else 0
            nS = cdiv(S - s0, st) if s0 < S else 0
            Hs = cdiv(Hh - fy, st) if fy < Hh else 0
            Ws = cdiv(Ww - fx, st) if fx < Ww else 0
            if Hs * Ws == 0:
                continue
            if nR * nS == 0:
                need_zero = True
                continue
            ph.append(Phase(fy, fx, nR, nS, Hs, Ws, nR * nS * Kgp, N * Hs * Ws))
    return ph, fused, rowfold, padded, need_zero


def plan(case):
    """what the library launches for `case` (the record's fields and what the bound and the claims need)"""
    N, C, H, W, K, Rr, S, st, pad, pm = case.geom
    P, Q = out_size(H, Rr, st, pad), out_size(W, S, st, pad)
    ft, fk = case.tile, case.ks
    if case.pass_ == 'fwd':
        M, Cg = K, C
        ph = [Phase(0, 0, Rr, S, P, Q, Rr * S * round4(C), N * P * Q)]
        mode, padded, need_zero, rowfold = ('fwd_reflect' if pm == 1 else 'fwd_zero'), False, False, False
        part = (N * P * Q <= 65536 and C >= 64) if K <= 4 else _may_split(K, N * P * Q, 1, fk)
        unit = st == 1
    else:
        M, Cg = C, K
        ph, fused, rowfold, padded, need_zero = _bwd_phases(case.geom)
        mode = 'dgrad_reflect' if fused else 'dgrad'
        part = (_may_split(C, N * cdiv(H, st) * cdiv(W, st), st * st, fk) and not padded and not need_zero and not rowfold)
        unit = True
    Cgp = round4(Cg)
    small = pm == 1 and (H < 2 * pad + 2 or W < 2 * pad + 2)
    pmax = max(p.Ptot for p in ph)
    if M <= 4:
        maxR, minH = max(p.nR for p in ph), min(p.Hs for p in ph)
        maxstrips = max(N * cdiv(p.Hs, 8) * p.Ws for p in ph)
        maxtaps = max(p.nR * p.nS for p in ph)
        if unit and 3 <= maxR <= 7 and minH >= 8:
            wgs, ks = cdiv(maxstrips, 64) * len(ph), 1
            if part and len(ph) == 1 and wgs < 128 and Cg >= 64:
                ks = min(256 // wgs, 8, Cg // 16)
            return Plan('smallm', mode, 1, (40 if maxR <= 4 else 70) + (3 if M <= 3 else 4), ks, len(ph), M, Cg, Cgp, ph, padded, need_zero, st, 'strip', small)
        return Plan('smallm', mode, 2 if maxtaps <= 9 else 3, 0, 1, len(ph), M, Cg, Cgp, ph, padded, need_zero, st,
                    'fewtaps' if maxtaps <= 9 else 'generic', small)
    nst = min(cdiv(p.Kp, 16) for p in ph)
    bm, bp, ks = _choose_tile(M, pmax, len(ph), nst, part, ft, fk)
    form = 'igemm2_cg16' if _chunked_k(Cg, M, Rr, S) else ('igemm2_cg4' if _cg4_k(Cg, M, Rr, S) else 'igemm')
    return Plan(form, mode, bm, bp, ks, len(ph), M, Cg, Cgp, ph, padded, need_zero, st, form, small)


def record(pl):
    return (pl.form, pl.mode, pl.bm, pl.bp, pl.ks, pl.nphase)


def instantiation(case, rec):
    """the kernel instantiation a launch record (form, mode, bm, bp, ks, nphase) of `case` names"""
    form, mode, bm, bp = rec[:4]
    dt = 'bf16' if case.half else 'fp32'
    if form == 'smallm':
        kmode = 'dgrad' if mode == 'dgrad_reflect' else mode
        if bm == 1:
            return 'smallm_strip<%s, %d, %d, %s>' % (kmode, bp // 10, bp % 10, dt)
        return '%s<%s, %s>' % ('smallm_fewtaps' if bm == 2 else 'smallm_conv', kmode, dt)
    kern = {'igemm2_cg16': 'igemm2<%s, %d, %d, 16, %s>', 'igemm2_cg4': 'igemm2<%s, %d, %d, 4, %s>', 'igemm': 'igemm<%s, %d, %d, %s>'}[form]
    return kern % (mode, bm, bp, dt)


def all_instantiations():
    tiles = ((128, 128), (128, 64), (64, 128), (64, 64), (32, 128))
    three, four = ('fwd_zero', 'fwd_reflect', 'dgrad'), ('fwd_zero', 'fwd_reflect', 'dgrad', 'dgrad_reflect')
    out = []
    for dt in ('fp32', 'bf16'):
        for bm, bp in tiles:
            out += ['igemm2<%s, %d, %d, 16, %s>' % (m, bm, bp, dt) for m in four]
            out += ['igemm2<%s, %d, %d, 4, %s>' % (m, bm, bp, dt) for m in three]
            out += ['igemm<%s, %d, %d, %s>' % (m, bm, bp, dt) for m in three]
        for m in three:
            out += ['smallm_strip<%s, %d, %d, %s>' % (m, nr, mo, dt) for nr in (4, 7) for mo in (3, 4)]
            out += ['smallm_fewtaps<%s, %s>' % (m, dt), 'smallm_conv<%s, %s>' % (m, dt)]
    return out


# ---- what a case may claim about itself (each a predicate of the plan) ----------------------------------------------------------------------
def _slices(pl, p):
    """(stages, stages per slice) of phase p under the K split; the strip kernel splits channels"""
    n = pl.Cg if pl.kernel == 'strip' else cdiv(p.Kp, 16)
    return n, cdiv(n, pl.ks)


CLAIMS = {
    'm_ragged': lambda pl: pl.M % pl.bm != 0,
    'm_blocks': lambda pl: pl.M > pl.bm,
    'p_ragged': lambda pl: any(p.Ptot % pl.bp != 0 for p in pl.phases),
    'p_blocks': lambda pl: any(p.Ptot > pl.bp for p in pl.phases),
    'kp16': lambda pl: any(p.Kp % 16 != 0 for p in pl.phases),                          # a short last K stage (igemm_kernel)
    'tap_in_slice': lambda pl: pl.Cgp % (pl.bp // 16) != 0,                              # the tap changes inside a thread's BP / 16 K slots
    'tap_at_slice': lambda pl: pl.Cgp % (pl.bp // 16) == 0 and pl.Cgp % 16 != 0,         # ... only at their start, not at every stage
    'split': lambda pl: pl.ks > 1,
    'empty_slice': lambda pl: pl.ks > 1 and any((pl.ks - 1) * _slices(pl, p)[1] >= _slices(pl, p)[0] for p in pl.phases),
    'short_slice': lambda pl: pl.ks > 1 and any(0 < _slices(pl, p)[0] - (pl.ks - 1) * _slices(pl, p)[1] < _slices(pl, p)[1] for p in pl.phases),
    'phases_differ': lambda pl: len({(p.nR * p.nS, p.Ptot) for p in pl.phases}) > 2,
    'stage4_partial': lambda pl: pl.form == 'igemm2_cg4' and any((p.nR * p.nS) % 4 != 0 for p in pl.phases),
    'cg3': lambda pl: pl.Cg == 3,
    'cg4': lambda pl: pl.Cg == 4,
    'padded_fold': lambda pl: pl.padded,
    'need_zero': lambda pl: pl.need_zero,
    'fold_both_sides': lambda pl: pl.padded and pl.small_plane,                          # H or W under 2 pad + 2: three images along that axis
    'strip_tail': lambda pl: any(p.Hs % 8 != 0 for p in pl.phases),
    'strip_blocks': lambda pl: any(p.Ptot // p.Hs * cdiv(p.Hs, 8) > 64 for p in pl.phases),                # more than one workgroup of 64 strips
    'pix256': lambda pl: any(p.Ptot % 256 != 0 and p.Ptot > 256 for p in pl.phases),
    'pix64': lambda pl: any(p.Ptot % 64 != 0 and p.Ptot > 64 for p in pl.phases),
    'c8': lambda pl: pl.Cg % 8 == 0,
    'c8rem': lambda pl: pl.Cg % 8 != 0 and pl.Cg > 8,
    'taps12': lambda pl: any(p.nR > 8 and p.nS > 8 for p in pl.phases),                  # entries 8 .. 11 of the 12-entry offset tables
}


# ---- data, reference, bound --------------------------------------------------------------------------------------------------------------------
def _signed(g, *shape):
    mag = 0.75 + 0.5 * torch.rand(*shape, generator=g)
    return mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def _fold_images(dy, w, geom):
    """T = sum over the mirror images of |gradient of the reflection-padded tensor| (the padded fallback stores each image before the fold)"""
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    xp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad, dtype=torch.float64, requires_grad=True)
    F.conv2d(xp, w, None, stride=st).backward(dy)
    t = xp.grad.detach().abs()
    xz = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    (F.pad(xz, (pad, pad, pad, pad), mode='reflect') * t).sum().backward()
    return xz.grad.detach()


Data = collections.namedtuple('Data', 'src w b ref A T')


@functools.lru_cache(maxsize=None)
def _data(pass_, geom, half, bias, seed):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    g = torch.Generator().manual_seed(sum(v * (i + 1) * 7919 for i, v in enumerate(geom)) + 2 * seed * 104729 + int(half) + (17 if pass_ == 'fwd' else 0))
    P, Q = out_size(H, Rr, st, pad), out_size(W, S, st, pad)
    src = _signed(g, N, C, H, W) if pass_ == 'fwd' else _signed(g, N, K, P, Q)
    w = _signed(g, K, C, Rr, S)
    b = _signed(g, K if pass_ == 'fwd' else C) if bias else None
    if half:
        src = src.bfloat16()
    for t in (src.float(), w) + ((b,) if bias else ()):
        assert 0.75 <= float(t.abs().min()) and float(t.abs().max()) <= 1.25
    ref, A = reference(pass_, geom, src, w, b)
    T = None
    if pass_ == 'dgrad' and pm == 1:
        T = _fold_images(src.double(), w.double(), geom)
    return Data(src, w, b, ref, A, T)


def data(case):
    """(src, w, bias, float64 reference BEFORE the activation, A, T) of a case on the CPU: made once, shared, never written to"""
    return _data(case.pass_, case.geom, case.half, case.bias, case.seed)


def n_eff(case, pl):
    """per element: Kp of the phase that owns it + K slices + 8 (a tensor of the output's shape)"""
    N, C, H, W, K = case.geom[:5]
    d = data(case)
    n = torch.zeros_like(d.ref)
    if case.pass_ == 'fwd' or pl.padded or pl.mode == 'dgrad_reflect' or pl.stride == 1:
        n += max(p.Kp for p in pl.phases)
    else:
        for p in pl.phases:
            n[:, :, p.fy::pl.stride, p.fx::pl.stride] = p.Kp
    return n + pl.ks + 8


def bounds(case, pl):
    """(linear accumulation bound E, the bound on |y - act(ref)|, act(ref)) per element"""
    d = data(case)
    E = 2 * n_eff(case, pl) * U * d.A
    aref = R.activation(d.ref, case.act, SLOPE)
    if not case.half:
        return E, E + (2.0 ** -22 * aref.abs() if case.act else 0.0), aref
    if pl.padded:
        E = E + 2.0 ** -8 * (d.T + E) + 2.0 ** -20 * (d.T + (d.b.abs().double().view(1, -1, 1, 1) if d.b is not None else 0.0))
    return E, 2.0 ** -8 * (aref.abs() + E) + E + 2.0 ** -22 * aref.abs() + 1e-30, aref


def condition(case, pl):
    """the largest bound of the case on the LINEAR result, to be held under TERM_MIN / 2 (for bf16: including the half ulp of the result)"""
    d = data(case)
    E, _, _ = bounds(case._replace(act=0), pl)
    if case.half:
        E = 2.0 ** -8 * (d.ref.abs() + E) + E
    return float(E.max())


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
CASES = []
TILE_M = {32128: 24, 64128: 40, 64064: 40, 128128: 72, 128064: 72}      # rows that give the tile (forced from 33 rows on): all ragged
TILES = tuple(TILE_M)
BOTH, F32_ONLY = (False, True), (False,)


def _add(sect, name, pass_, geom, want, claims=(), tile=0, ks=0, halves=BOTH, act=0, bias=None, seed=0):
    if bias is None:      # forward: always; data gradient: the transposed convolutions (stride 2, zero padding) and every reflect gradient
        bias = pass_ == 'fwd' or (geom[7] == 2 and geom[5] >= 2 and geom[9] == 0) or geom[9] == 1
    for half in halves:
        CASES.append(Case(sect, '%s-%s' % (name, 'bf16' if half else 'fp32'), pass_, tuple(geom), tile, ks, half, act, bias, tuple(want),
                          tuple(claims), seed))


def _tiles(sect, name, pass_, geomf, form, mode, nphase, claims=(), halves=BOTH, tiles=TILES, ks=0, want_ks=1, M=None, **kw):
    """one case per tile: geomf(M) with the row count that gives the tile"""
    for t in tiles:
        m = (M or TILE_M)[t]
        _add(sect, '%s-%d%s' % (name, t, '-ks%d' % ks if ks else ''), pass_, geomf(m), (form, mode, t // 1000, t % 1000, want_ks, nphase),
             claims, tile=0 if m <= 32 else t, ks=ks, halves=halves, **kw)


# A. igemm2_kernel<.., 16>: gathered channels a multiple of 16.  144 terms (16 channels x 3x3) for both storage types.
_tiles('A', 'fwd_zero-3x3', 'fwd', lambda m: (2, 16, 11, 13, m, 3, 3, 1, 1, 0), 'igemm2_cg16', 'fwd_zero', 1, ('m_ragged', 'p_ragged', 'p_blocks'))
_tiles('A', 'fwd_reflect-3x3', 'fwd', lambda m: (3, 16, 7, 10, m, 3, 3, 1, 1, 1), 'igemm2_cg16', 'fwd_reflect', 1, ('m_ragged', 'p_ragged', 'p_blocks'))
_tiles('A', 'dgrad_s1-3x3', 'dgrad', lambda m: (2, m, 13, 11, 16, 3, 3, 1, 1, 0), 'igemm2_cg16', 'dgrad', 1, ('m_ragged', 'p_ragged', 'p_blocks'))
# stride 2, odd H / W: phases of 1, 2, 2, 4 taps and 42, 35, 36, 30 pixels per image
_tiles('A', 'dgrad_s2-3x3', 'dgrad', lambda m: (2, m, 13, 11, 32, 3, 3, 2, 1, 0), 'igemm2_cg16', 'dgrad', 4, ('m_ragged', 'p_ragged', 'phases_differ'))
# reflect, pad 1, 3 rows: the three row classes with folded weights (rows without a mirror | row 1 | row H - 2)
_tiles('A', 'rowfold-7x12', 'dgrad', lambda m: (2, m, 7, 12, 16, 3, 3, 1, 1, 1), 'igemm2_cg16', 'dgrad_reflect', 3, ('m_ragged', 'p_ragged'))
_tiles('A', 'rowfold-4x4', 'dgrad', lambda m: (3, m, 4, 4, 16, 3, 3, 1, 1, 1), 'igemm2_cg16', 'dgrad_reflect', 3, ('m_ragged', 'p_ragged'),
       tiles=(32128, 64064, 128128))      # the smallest legal plane: every row and column is a border
# fused mirror gather without the row fold (<= 9 taps and not 3 rows at pad 1): 3x3 at pad 2 (two mirror rows / columns a side), 2x3 at pad 1
_tiles('A', 'fused-3x3p2', 'dgrad', lambda m: (2, m, 9, 7, 16, 3, 3, 1, 2, 1), 'igemm2_cg16', 'dgrad_reflect', 1, ('m_ragged', 'p_ragged'))
_tiles('A', 'fused-2x3p1', 'dgrad', lambda m: (2, m, 6, 11, 16, 2, 3, 1, 1, 1), 'igemm2_cg16', 'dgrad_reflect', 1, ('m_ragged', 'p_ragged'),
       tiles=(32128, 64128))
# K split, forced: 9 stages in 2 slices (5 + 4); two M tiles
_tiles('A', 'fwd_zero-3x3', 'fwd', lambda m: (2, 16, 11, 13, m, 3, 3, 1, 1, 0), 'igemm2_cg16', 'fwd_zero', 1, ('split', 'short_slice', 'm_blocks', 'm_ragged'),
       tiles=(64128, 64064, 128128, 128064), ks=2, want_ks=2, M={64128: 80, 64064: 80, 128128: 136, 128064: 136})
_tiles('A', 'dgrad_s1-3x3', 'dgrad', lambda m: (2, m, 13, 11, 16, 3, 3, 1, 1, 0), 'igemm2_cg16', 'dgrad', 1, ('split', 'short_slice'),
       tiles=(64128, 128064), ks=2, want_ks=2)
_tiles('A', 'fused-3x3p2', 'dgrad', lambda m: (2, m, 9, 7, 16, 3, 3, 1, 2, 1), 'igemm2_cg16', 'dgrad_reflect', 1, ('split', 'short_slice'),
       tiles=(64064, 128128), ks=2, want_ks=2)
# fp32 only (more than 200 terms): other filters, longer K, the split with an empty last slice (25 stages, 6 slices of 5), the heuristic's
# own split on the 32-row tile (50 stages: 6 slices of 9, the last of 5), stride-2 phases of 9, 6, 6, 4 taps split in two
_tiles('A', 'fwd_zero-5x5', 'fwd', lambda m: (2, 16, 13, 13, m, 5, 5, 1, 2, 0), 'igemm2_cg16', 'fwd_zero', 1, ('split', 'empty_slice'),
       tiles=(64128, 128128), ks=6, want_ks=6, halves=F32_ONLY)
_tiles('A', 'fwd_reflect-5x5', 'fwd', lambda m: (2, 16, 9, 14, m, 5, 5, 1, 2, 1), 'igemm2_cg16', 'fwd_reflect', 1, ('split', 'empty_slice'),
       tiles=(64064, 128064), ks=6, want_ks=6, halves=F32_ONLY)
_tiles('A', 'dgrad_s1-5x5', 'dgrad', lambda m: (2, m, 12, 12, 16, 5, 5, 1, 2, 0), 'igemm2_cg16', 'dgrad', 1, ('split', 'empty_slice'),
       tiles=(64128, 128064), ks=6, want_ks=6, halves=F32_ONLY)
_add('A', 'fwd_zero-1x1-c128', 'fwd', (2, 128, 15, 9, 72, 1, 1, 1, 0, 0), ('igemm2_cg16', 'fwd_zero', 128, 64, 2, 1), ('split', 'm_ragged', 'p_ragged'),
     tile=128064, ks=2, halves=F32_ONLY)
_add('A', 'fwd_zero-4x4s2-c32', 'fwd', (3, 32, 11, 13, 40, 4, 4, 2, 1, 0), ('igemm2_cg16', 'fwd_zero', 64, 64, 8, 1), ('split', 'm_ragged', 'p_ragged'),
     tile=64064, ks=8, halves=F32_ONLY)
_add('A', 'fwd_reflect-4x4s2-c64', 'fwd', (2, 64, 11, 11, 24, 4, 4, 2, 1, 1), ('igemm2_cg16', 'fwd_reflect', 32, 128, 8, 1), ('split', 'p_ragged'), halves=F32_ONLY)
_add('A', 'fwd_zero-5x5-c32-heuristic', 'fwd', (2, 32, 9, 9, 24, 5, 5, 1, 2, 0), ('igemm2_cg16', 'fwd_zero', 32, 128, 6, 1), ('split', 'short_slice', 'p_ragged'),
     halves=F32_ONLY)
_add('A', 'dgrad_s1-4x4-k48', 'dgrad', (2, 40, 10, 9, 48, 4, 4, 1, 1, 0), ('igemm2_cg16', 'dgrad', 64, 128, 3, 1), ('split', 'm_ragged', 'p_ragged'),
     tile=64128, ks=3, halves=F32_ONLY)
_add('A', 'dgrad_s2-5x5-k32', 'dgrad', (2, 72, 13, 13, 32, 5, 5, 2, 2, 0), ('igemm2_cg16', 'dgrad', 128, 128, 2, 4), ('split', 'phases_differ', 'm_ragged'),
     tile=128128, ks=2, halves=F32_ONLY)
_add('A', 'dgrad_s2-4x4-k64', 'dgrad', (2, 40, 11, 9, 64, 4, 4, 2, 1, 0), ('igemm2_cg16', 'dgrad', 64, 64, 4, 4), ('split', 'm_ragged', 'p_ragged'),
     tile=64064, ks=4, halves=F32_ONLY)

# B. igemm2_kernel<.., 4>: a gathered tensor of 3 or 4 channels; 49 taps = 12 stages of 4 taps and a partial one
_tiles('B', 'fwd_zero-7x7s2-c3', 'fwd', lambda m: (2, 3, 19, 17, m, 7, 7, 2, 3, 0), 'igemm2_cg4', 'fwd_zero', 1, ('cg3', 'stage4_partial', 'm_ragged', 'p_ragged'))
_tiles('B', 'fwd_reflect-7x7-c3', 'fwd', lambda m: (2, 3, 9, 10, m, 7, 7, 1, 3, 1), 'igemm2_cg4', 'fwd_reflect', 1, ('cg3', 'stage4_partial', 'm_ragged', 'p_ragged'))
_tiles('B', 'fwd_zero-4x4s2-c4', 'fwd', lambda m: (3, 4, 18, 14, m, 4, 4, 2, 1, 0), 'igemm2_cg4', 'fwd_zero', 1, ('cg4', 'm_ragged', 'p_ragged'))
_tiles('B', 'fwd_reflect-7x7-c4', 'fwd', lambda m: (2, 4, 9, 10, m, 7, 7, 1, 3, 1), 'igemm2_cg4', 'fwd_reflect', 1, ('cg4', 'stage4_partial'),
       tiles=(32128, 128128))
# the data gradient of a convolution that produces 3 / 4 channels from more than 4: the head's weights (zero padding; reflection: section C)
_tiles('B', 'dgrad-7x7-k3', 'dgrad', lambda m: (2, m, 9, 10, 3, 7, 7, 1, 3, 0), 'igemm2_cg4', 'dgrad', 1, ('cg3', 'stage4_partial', 'm_ragged', 'p_ragged'))
_tiles('B', 'dgrad-4x4s2-k4', 'dgrad', lambda m: (2, m, 13, 11, 4, 4, 4, 2, 1, 0), 'igemm2_cg4', 'dgrad', 4, ('cg4', 'm_ragged', 'p_ragged'),
       tiles=(32128, 64064, 128064))
_tiles('B', 'dgrad-3x3s2-k3', 'dgrad', lambda m: (2, m, 13, 11, 3, 3, 3, 2, 1, 0), 'igemm2_cg4', 'dgrad', 4, ('cg3', 'phases_differ', 'stage4_partial'),
       tiles=(64128, 128128))
_tiles('B', 'fwd_zero-7x7s2-c3', 'fwd', lambda m: (2, 3, 19, 17, m, 7, 7, 2, 3, 0), 'igemm2_cg4', 'fwd_zero', 1, ('split', 'short_slice', 'stage4_partial'),
       tiles=(64128, 128064), ks=3, want_ks=3)      # 13 stages: 5 + 5 + 3
_add('B', 'dgrad-7x7-k3-ks2', 'dgrad', (2, 40, 9, 10, 3, 7, 7, 1, 3, 0), ('igemm2_cg4', 'dgrad', 64, 64, 2, 1), ('split', 'short_slice', 'cg3'), tile=64064, ks=2)

# C. igemm_kernel: generic K order.  Cgp = 8, 12, 20, 24 (gathered channels 5, 8, 12, 20, 24) against a thread's 8 (BP 128) / 4 (BP 64) K slots
_GEN_C = {32128: 5, 64128: 12, 64064: 20, 128128: 20, 128064: 12}
for _t in TILES:
    _cg = _GEN_C[_t]
    _cl = ('kp16', 'm_ragged', 'p_ragged') + (('tap_in_slice',) if round4(_cg) % (_t % 1000 // 16) else ('tap_at_slice',))
    _tiles('C', 'fwd_zero-3x3-c%d' % _cg, 'fwd', lambda m, c=_cg: (2, c, 11, 13, m, 3, 3, 1, 1, 0), 'igemm', 'fwd_zero', 1, _cl, tiles=(_t,))
    _tiles('C', 'fwd_reflect-3x3-c%d' % _cg, 'fwd', lambda m, c=_cg: (3, c, 7, 10, m, 3, 3, 1, 1, 1), 'igemm', 'fwd_reflect', 1, _cl, tiles=(_t,))
    _tiles('C', 'dgrad_s1-3x3-k%d' % _cg, 'dgrad', lambda m, c=_cg: (2, m, 13, 11, c, 3, 3, 1, 1, 0), 'igemm', 'dgrad', 1, _cl, tiles=(_t,))
_tiles('C', 'fwd_zero-3x3-c8', 'fwd', lambda m: (2, 8, 11, 13, m, 3, 3, 1, 1, 0), 'igemm', 'fwd_zero', 1, ('kp16', 'tap_at_slice'), tiles=(32128, 64128))
_tiles('C', 'fwd_zero-3x3-c8', 'fwd', lambda m: (2, 8, 11, 13, m, 3, 3, 1, 1, 0), 'igemm', 'fwd_zero', 1, ('kp16',), tiles=(64064,))
_tiles('C', 'fwd_zero-3x3-c20', 'fwd', lambda m: (2, 20, 11, 13, m, 3, 3, 1, 1, 0), 'igemm', 'fwd_zero', 1, ('kp16', 'tap_in_slice'), tiles=(32128,))
_tiles('C', 'dgrad_s1-3x3-k24', 'dgrad', lambda m: (2, m, 13, 11, 24, 3, 3, 1, 1, 0), 'igemm', 'dgrad', 1, ('kp16', 'tap_at_slice'), tiles=(128128,), halves=F32_ONLY)
_tiles('C', 'dgrad_s2-4x4-k12', 'dgrad', lambda m: (2, m, 13, 11, 12, 4, 4, 2, 1, 0), 'igemm', 'dgrad', 4, ('tap_in_slice', 'phases_differ'),
       tiles=(64128, 128128))
_tiles('C', 'dgrad_s2-3x3-k24', 'dgrad', lambda m: (2, m, 13, 11, 24, 3, 3, 2, 1, 0), 'igemm', 'dgrad', 4, ('kp16', 'phases_differ'), tiles=(32128, 128064))
# more than 25 taps on 16 channels (7x7: 784 terms, fp32 only), whole and split 5 ways (49 stages: 4 x 10 + 9)
_tiles('C', 'fwd_zero-7x7-c16', 'fwd', lambda m: (2, 16, 9, 10, m, 7, 7, 1, 3, 0), 'igemm', 'fwd_zero', 1, ('m_ragged', 'p_ragged'), tiles=(128064,), halves=F32_ONLY)
_add('C', 'fwd_zero-7x7-c16-32128-heuristic', 'fwd', (2, 16, 9, 10, 24, 7, 7, 1, 3, 0), ('igemm', 'fwd_zero', 32, 128, 6, 1), ('split', 'short_slice'), halves=F32_ONLY)
_tiles('C', 'fwd_reflect-7x7-c16', 'fwd', lambda m: (2, 16, 9, 10, m, 7, 7, 1, 3, 1), 'igemm', 'fwd_reflect', 1, ('split', 'short_slice'),
       tiles=(64064, 128128), ks=5, want_ks=5, halves=F32_ONLY)
_tiles('C', 'dgrad-7x7-k16', 'dgrad', lambda m: (2, m, 9, 10, 16, 7, 7, 1, 3, 0), 'igemm', 'dgrad', 1, ('split', 'short_slice'),
       tiles=(64128,), ks=5, want_ks=5, halves=F32_ONLY)
# 11x11 stride 4: forward on 8 channels (968 terms; 16 channels would be 1936), the heuristic's split of its 61 stages (7 slices of 9, the
# last of 7, the last stage of 8 slots); data gradient on 16 channels: 16 phases of 9, 6, 6, 4 taps, generic because the FILTER has 121
_add('C', 'fwd_zero-11x11s4-c8', 'fwd', (2, 8, 35, 31, 24, 11, 11, 4, 5, 0), ('igemm', 'fwd_zero', 32, 128, 7, 1), ('split', 'short_slice', 'kp16'), halves=F32_ONLY)
_add('C', 'dgrad-11x11s4-k16', 'dgrad', (2, 24, 23, 19, 16, 11, 11, 4, 5, 0), ('igemm', 'dgrad', 32, 128, 1, 16), ('phases_differ',), bias=False)
_add('C', 'dgrad-11x11s4-k16-64064', 'dgrad', (2, 40, 23, 19, 16, 11, 11, 4, 5, 0), ('igemm', 'dgrad', 64, 64, 1, 16), ('phases_differ',), tile=64064, bias=False)
# reflect data gradients the fused kernel refuses: the gradient of the PADDED tensor (zero-padding kernels at pad 0 on the larger grid),
# then reflect_fold_kernel -- K % 16 != 0; a plane under 2 pad + 2 (rows fold from both sides: up to 9 images); the head (3 gathered channels)
_add('C', 'padded-3x3-k5', 'dgrad', (2, 24, 9, 10, 5, 3, 3, 1, 1, 1), ('igemm', 'dgrad', 32, 128, 1, 1), ('padded_fold', 'kp16'))
_add('C', 'padded-3x3-k12-w11', 'dgrad', (2, 40, 6, 11, 12, 3, 3, 1, 1, 1), ('igemm', 'dgrad', 64, 128, 1, 1), ('padded_fold', 'tap_in_slice'), tile=64128, ks=2, halves=F32_ONLY)
_add('C', 'padded-5x5-k5-h5', 'dgrad', (2, 24, 5, 8, 5, 5, 5, 1, 2, 1), ('igemm', 'dgrad', 32, 128, 1, 1), ('padded_fold',), halves=F32_ONLY)
_add('C', 'padded-3x3-k16-h3', 'dgrad', (2, 24, 3, 9, 16, 3, 3, 1, 1, 1), ('igemm2_cg16', 'dgrad', 32, 128, 1, 1), ('padded_fold',), halves=F32_ONLY)
_add('C', 'padded-5x5-k3-h4', 'dgrad', (3, 24, 4, 5, 3, 5, 5, 1, 2, 1), ('igemm2_cg4', 'dgrad', 32, 128, 1, 1), ('padded_fold', 'cg3'), halves=F32_ONLY)
_add('C', 'padded-7x7-k3-head', 'dgrad', (2, 40, 9, 10, 3, 7, 7, 1, 3, 1), ('igemm2_cg4', 'dgrad', 64, 128, 1, 1), ('padded_fold', 'cg3'), tile=64128, halves=F32_ONLY)
_add('C', 'padded-3x3-k3', 'dgrad', (2, 24, 9, 10, 3, 3, 3, 1, 1, 1), ('igemm2_cg4', 'dgrad', 32, 128, 1, 1), ('padded_fold', 'cg3'))
# planes under 2 pad + 2 in both storage types (3 rows at pad 1: the middle row receives images from both sides, 9 at its inner pixels)
_add('C', 'padded-3x3-k5-h3', 'dgrad', (2, 24, 3, 9, 5, 3, 3, 1, 1, 1), ('igemm', 'dgrad', 32, 128, 1, 1), ('padded_fold', 'fold_both_sides', 'kp16'))
_add('C', 'padded-3x3-k3-h3', 'dgrad', (2, 24, 3, 9, 3, 3, 3, 1, 1, 1), ('igemm2_cg4', 'dgrad', 32, 128, 1, 1), ('padded_fold', 'fold_both_sides', 'cg3'))
_add('C', 'padded-3x3-k2-w3', 'dgrad', (2, 40, 9, 3, 2, 3, 3, 1, 1, 1), ('igemm2_cg4', 'dgrad', 64, 64, 1, 1), ('padded_fold', 'fold_both_sides'), tile=64064)
# the same gradients WITHOUT a bias (every other reflect gradient of the table carries one, added once behind the fold)
_add('C', 'padded-3x3-k5-nobias', 'dgrad', (2, 24, 9, 10, 5, 3, 3, 1, 1, 1), ('igemm', 'dgrad', 32, 128, 1, 1), ('padded_fold',), bias=False)
# 1x1 stride 2: three of four pixels belong to no phase (memset first), and no split workspace whatever is forced
_add('C', 'need_zero-1x1s2-k24', 'dgrad', (2, 40, 15, 9, 24, 1, 1, 2, 0, 0), ('igemm', 'dgrad', 64, 128, 1, 1), ('need_zero', 'kp16'), tile=64128, ks=4)
_add('C', 'need_zero-1x1s2-k16', 'dgrad', (2, 24, 15, 9, 16, 1, 1, 2, 0, 0), ('igemm2_cg16', 'dgrad', 32, 128, 1, 1), ('need_zero',))

# D. small-M (<= 4 output channels).  want = (smallm, mode, bm = 1 strip | 2 few taps | 3 generic, bp = NR * 10 + MO, channel split, phases)
# strip kernel: heights 8 (whole strips), 9 and 19 (tails of 1 and 3 rows)
_add('D', 'strip-fwd_zero-3x3-m3', 'fwd', (2, 16, 19, 13, 3, 3, 3, 1, 1, 0), ('smallm', 'fwd_zero', 1, 43, 1, 1), ('strip_tail', 'strip_blocks'))
_add('D', 'strip-fwd_zero-4x4-m1', 'fwd', (3, 8, 10, 9, 1, 4, 4, 1, 1, 0), ('smallm', 'fwd_zero', 1, 43, 1, 1), ('strip_tail',))
_add('D', 'strip-fwd_zero-4x4-m4', 'fwd', (2, 8, 9, 10, 4, 4, 4, 1, 1, 0), ('smallm', 'fwd_zero', 1, 44, 1, 1), ())
_add('D', 'strip-fwd_zero-5x5-m3', 'fwd', (2, 6, 9, 11, 3, 5, 5, 1, 2, 0), ('smallm', 'fwd_zero', 1, 73, 1, 1), ('strip_tail',))
_add('D', 'strip-fwd_zero-7x7-m4', 'fwd', (2, 3, 19, 9, 4, 7, 7, 1, 3, 0), ('smallm', 'fwd_zero', 1, 74, 1, 1), ('strip_tail',))
_add('D', 'strip-fwd_reflect-3x3-m3', 'fwd', (2, 13, 9, 13, 3, 3, 3, 1, 1, 1), ('smallm', 'fwd_reflect', 1, 43, 1, 1), ('strip_tail',))
_add('D', 'strip-fwd_reflect-3x3-m4', 'fwd', (2, 16, 8, 11, 4, 3, 3, 1, 1, 1), ('smallm', 'fwd_reflect', 1, 44, 1, 1), ())
_add('D', 'strip-fwd_reflect-7x7-m3-head', 'fwd', (2, 3, 19, 13, 3, 7, 7, 1, 3, 1), ('smallm', 'fwd_reflect', 1, 73, 1, 1), ('strip_tail', 'strip_blocks'))
_add('D', 'strip-fwd_reflect-7x7-m3-c16', 'fwd', (2, 16, 9, 10, 3, 7, 7, 1, 3, 1), ('smallm', 'fwd_reflect', 1, 73, 1, 1), ('strip_tail',), halves=F32_ONLY)
_add('D', 'strip-fwd_reflect-5x5-m4', 'fwd', (2, 7, 9, 9, 4, 5, 5, 1, 2, 1), ('smallm', 'fwd_reflect', 1, 74, 1, 1), ('strip_tail',))
_add('D', 'strip-dgrad-3x3-m3', 'dgrad', (2, 3, 19, 11, 16, 3, 3, 1, 1, 0), ('smallm', 'dgrad', 1, 43, 1, 1), ('strip_tail',))
_add('D', 'strip-dgrad-4x4-m4', 'dgrad', (2, 4, 9, 10, 8, 4, 4, 1, 1, 0), ('smallm', 'dgrad', 1, 44, 1, 1), ('strip_tail',))
_add('D', 'strip-dgrad-5x5-m1', 'dgrad', (3, 1, 8, 9, 6, 5, 5, 1, 2, 0), ('smallm', 'dgrad', 1, 73, 1, 1), ())
_add('D', 'strip-dgrad-7x7-m4', 'dgrad', (2, 4, 9, 10, 3, 7, 7, 1, 3, 0), ('smallm', 'dgrad', 1, 74, 1, 1), ('strip_tail',))
_add('D', 'strip-dgrad-7x7-m3-k16', 'dgrad', (2, 3, 9, 10, 16, 7, 7, 1, 3, 0), ('smallm', 'dgrad', 1, 73, 1, 1), ('strip_tail',), halves=F32_ONLY)
# stride-2 phases on the strip kernel: 7x7 stride 2 (4 or 3 row taps, 10 / 9 rows per phase), 11x11 stride 2 (6 or 5)
_add('D', 'strip-dgrad_s2-7x7-m3', 'dgrad', (2, 3, 19, 17, 8, 7, 7, 2, 3, 0), ('smallm', 'dgrad', 1, 43, 1, 4), ('strip_tail', 'phases_differ'))
_add('D', 'strip-dgrad_s2-7x7-m4', 'dgrad', (2, 4, 19, 17, 4, 7, 7, 2, 3, 0), ('smallm', 'dgrad', 1, 44, 1, 4), ('strip_tail', 'phases_differ'))
_add('D', 'strip-dgrad_s2-11x11-m3', 'dgrad', (2, 3, 19, 17, 4, 11, 11, 2, 5, 0), ('smallm', 'dgrad', 1, 73, 1, 4), ('strip_tail', 'phases_differ'))
_add('D', 'strip-dgrad_s2-11x11-m4', 'dgrad', (2, 4, 17, 19, 4, 11, 11, 2, 5, 0), ('smallm', 'dgrad', 1, 74, 1, 4), ('strip_tail', 'phases_differ'))
# the reflect gradient that lands on an image: padded grid, strip kernel, then the fold
_add('D', 'strip-padded-7x7-m3', 'dgrad', (2, 3, 9, 10, 8, 7, 7, 1, 3, 1), ('smallm', 'dgrad', 1, 73, 1, 1), ('padded_fold', 'strip_tail'), halves=F32_ONLY)
_add('D', 'strip-padded-3x3-m3', 'dgrad', (2, 3, 9, 10, 4, 3, 3, 1, 1, 1), ('smallm', 'dgrad', 1, 43, 1, 1), ('padded_fold', 'strip_tail'))
_add('D', 'fewtaps-padded-3x3-m3-h3', 'dgrad', (2, 3, 3, 9, 4, 3, 3, 1, 1, 1), ('smallm', 'dgrad', 2, 0, 1, 1), ('padded_fold', 'fold_both_sides'))
# channel split (one phase, few strips, >= 64 channels): 64 = 4 x 16; 67 = 3 x 17 + 16; 115 = 6 x 17 + 13 (the 512 -> 1 layer's code)
_add('D', 'strip-split-4x4-c64-m1', 'fwd', (2, 64, 15, 15, 1, 4, 4, 1, 1, 0), ('smallm', 'fwd_zero', 1, 43, 4, 1), ('split', 'strip_tail'), halves=F32_ONLY)
_add('D', 'strip-split-4x4-c67-m1', 'fwd', (2, 67, 15, 15, 1, 4, 4, 1, 1, 0), ('smallm', 'fwd_zero', 1, 43, 4, 1), ('split', 'short_slice', 'strip_tail'), halves=F32_ONLY)
_add('D', 'strip-split-3x3-c115-m3', 'fwd', (2, 115, 9, 9, 3, 3, 3, 1, 1, 1), ('smallm', 'fwd_reflect', 1, 43, 7, 1), ('split', 'short_slice', 'strip_tail'), halves=F32_ONLY)
_add('D', 'strip-split-5x5-c40-nosplit', 'fwd', (2, 40, 9, 9, 4, 5, 5, 1, 2, 0), ('smallm', 'fwd_zero', 1, 74, 1, 1), ('strip_tail',), halves=F32_ONLY)
# few-taps kernel (phases of <= 9 taps the strip kernel does not take): 8-channel blocks with and without a remainder, > 256 pixels
_add('D', 'fewtaps-fwd_zero-3x3s2-c16', 'fwd', (3, 16, 21, 19, 3, 3, 3, 2, 1, 0), ('smallm', 'fwd_zero', 2, 0, 1, 1), ('c8', 'pix256'))
_add('D', 'fewtaps-fwd_zero-3x3-c13-h7', 'fwd', (3, 13, 7, 15, 4, 3, 3, 1, 1, 0), ('smallm', 'fwd_zero', 2, 0, 1, 1), ('c8rem', 'pix256'))
_add('D', 'fewtaps-fwd_reflect-3x3s2-c13', 'fwd', (3, 13, 21, 19, 1, 3, 3, 2, 1, 1), ('smallm', 'fwd_reflect', 2, 0, 1, 1), ('c8rem', 'pix256'))
_add('D', 'fewtaps-fwd_reflect-1x1-c16', 'fwd', (2, 16, 13, 11, 3, 1, 1, 1, 0, 1), ('smallm', 'fwd_reflect', 2, 0, 1, 1), ('c8', 'pix256'))
_add('D', 'fewtaps-dgrad_s2-4x4-k12', 'dgrad', (3, 3, 21, 19, 12, 4, 4, 2, 1, 0), ('smallm', 'dgrad', 2, 0, 1, 4), ('c8rem', 'pix256'))
_add('D', 'fewtaps-dgrad_s2-4x4-k16', 'dgrad', (3, 4, 22, 18, 16, 4, 4, 2, 1, 0), ('smallm', 'dgrad', 2, 0, 1, 4), ('c8', 'pix256'))
_add('D', 'fewtaps-dgrad-2x2-k9', 'dgrad', (3, 1, 11, 10, 9, 2, 2, 1, 0, 0), ('smallm', 'dgrad', 2, 0, 1, 1), ('c8rem', 'pix256'))
# generic small-M kernel: more than 9 taps and a plane under 8 rows, 1-2 row taps, a strided forward, more than 7 row taps (11x11: table
# entries 8 .. 10 of 12)
_add('D', 'generic-fwd_zero-7x7s2-m1', 'fwd', (2, 3, 19, 17, 1, 7, 7, 2, 3, 0), ('smallm', 'fwd_zero', 3, 0, 1, 1), ('pix64',))
_add('D', 'generic-fwd_zero-2x5-m3', 'fwd', (2, 9, 11, 13, 3, 2, 5, 1, 1, 0), ('smallm', 'fwd_zero', 3, 0, 1, 1), ('pix64',))
_add('D', 'generic-fwd_zero-11x11-m1', 'fwd', (2, 8, 13, 12, 1, 11, 11, 1, 5, 0), ('smallm', 'fwd_zero', 3, 0, 1, 1), ('taps12', 'pix64'), halves=F32_ONLY)
_add('D', 'generic-fwd_zero-11x11-m2-c1', 'fwd', (2, 1, 13, 12, 2, 11, 11, 1, 5, 0), ('smallm', 'fwd_zero', 3, 0, 1, 1), ('taps12', 'pix64'))
_add('D', 'generic-fwd_reflect-5x5-h7-m2', 'fwd', (2, 7, 7, 9, 2, 5, 5, 1, 2, 1), ('smallm', 'fwd_reflect', 3, 0, 1, 1), ('pix64',))
_add('D', 'generic-fwd_reflect-7x7s2-m4', 'fwd', (2, 3, 19, 17, 4, 7, 7, 2, 3, 1), ('smallm', 'fwd_reflect', 3, 0, 1, 1), ('pix64',))
_add('D', 'generic-dgrad-5x5-h7-m3', 'dgrad', (2, 3, 7, 12, 6, 5, 5, 1, 2, 0), ('smallm', 'dgrad', 3, 0, 1, 1), ('pix64',))
_add('D', 'generic-dgrad-11x11-m1', 'dgrad', (2, 1, 13, 12, 1, 11, 11, 1, 5, 0), ('smallm', 'dgrad', 3, 0, 1, 1), ('taps12', 'pix64'))
_add('D', 'generic-dgrad_s2-7x7-h13-m3', 'dgrad', (2, 3, 13, 17, 4, 7, 7, 2, 3, 0), ('smallm', 'dgrad', 3, 0, 1, 4), ('phases_differ',))

# E. fused activations: the tile epilogue of each MFMA kernel, the small-M epilogues, splitk_reduce_kernel (fp32 and bf16 stores)
for _a in range(5):
    _n = ACT_NAMES[_a]
    _add('E', 'cg16-%s' % _n, 'fwd', (2, 16, 11, 13, 40, 3, 3, 1, 1, 0), ('igemm2_cg16', 'fwd_zero', 64, 64, 1, 1), (), tile=64064, act=_a)
    _add('E', 'cg4-%s' % _n, 'fwd', (2, 3, 9, 10, 24, 7, 7, 1, 3, 1), ('igemm2_cg4', 'fwd_reflect', 32, 128, 1, 1), (), act=_a)
    _add('E', 'igemm-%s' % _n, 'fwd', (2, 12, 11, 13, 72, 3, 3, 1, 1, 0), ('igemm', 'fwd_zero', 128, 128, 1, 1), (), tile=128128, act=_a)
    _add('E', 'strip-%s' % _n, 'fwd', (2, 3, 19, 13, 3, 7, 7, 1, 3, 1), ('smallm', 'fwd_reflect', 1, 73, 1, 1), (), act=_a)
    _add('E', 'fewtaps-%s' % _n, 'fwd', (3, 13, 7, 15, 4, 3, 3, 1, 1, 0), ('smallm', 'fwd_zero', 2, 0, 1, 1), (), act=_a)
    _add('E', 'smallm_generic-%s' % _n, 'fwd', (2, 9, 11, 13, 3, 2, 5, 1, 1, 0), ('smallm', 'fwd_zero', 3, 0, 1, 1), (), act=_a)
    _add('E', 'reduce-%s' % _n, 'fwd', (2, 16, 11, 13, 40, 3, 3, 1, 1, 0), ('igemm2_cg16', 'fwd_zero', 64, 128, 2, 1), ('split',), tile=64128, ks=2, act=_a)
    # 3 x 41 x 11 x 13 = 17589 outputs: no multiple of 4, the reduce's scalar path
    _add('E', 'reduce_scalar-%s' % _n, 'fwd', (3, 16, 11, 13, 41, 3, 3, 1, 1, 0), ('igemm2_cg16', 'fwd_zero', 64, 128, 2, 1), ('split',), tile=64128, ks=2, act=_a)
    _add('E', 'reduce_strip-%s' % _n, 'fwd', (2, 64, 15, 15, 1, 4, 4, 1, 1, 0), ('smallm', 'fwd_zero', 1, 43, 4, 1), ('split',), act=_a, halves=F32_ONLY)

BY_NAME = collections.OrderedDict(('%s.%s' % (c.sect, c.name), c) for c in CASES)
assert len(BY_NAME) == len(CASES), 'case names must be unique'
