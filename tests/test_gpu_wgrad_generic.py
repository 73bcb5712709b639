"""GPU: the generic weight gradient (csrc/wgrad_igemm.hip: wgrad2_kernel, wgrad_kernel, smallm_wgrad_kernel, smallm_wgrad_strip_kernel and
wgrad_reduce_kernel) held to float64 element by element, instantiation by instantiation.

Every layer the matrix-pipe routes do not take lands here, and the row-ring / hsplit tests measure those routes against this one.  Each
case calls pcgan_conv2d_bwd_weight directly (the host's routing cannot divert it) and reads pcgan_wgrad_last_launch back: kernel family,
padding mode, BM, VECA, variant, storage type, splits and units per split must be what the case is there to hit, so a case that lands on
another instantiation fails.  The library option "wgrad_ks" forces the number of splits where a case needs one.

Per case (_run): workspace and a 4 KiB tail behind the queried size filled with 0xFF bytes (NaN partial sums; the tail must not change),
accumulate = 0 into a NaN-filled dw, then accumulate = 1 into a random base scaled to max|ref|, which must be BIT-equal to base + dw
(same partial sums, same order, one more add).
Data: |x|, |dy| uniform in [0.75, 1.25] with independent random signs (bf16 cases: rounded to bf16 first, the reference sees the rounded
values), so every term of every sum has a magnitude in [0.5625, 1.5625].
Reference: float64 autograd of oracle.ops_ref.conv2d; the same call on (|x|, |dy|) gives A, the per-element sum of |terms|.
Gate, per element:  |dw - ref| <= 2 n_eff 2^-24 A,  n_eff = (most output pixels one split sums, from the record) + ceil(splits / 4) + 4:
the standard bound of an fp32 sum of that depth in any order (partial sum, the reduce's four-way tree over the splits, the final adds),
with a factor 2 for a product rounded before it is added.  Derived, not measured.
Condition, asserted per case before the launch:  2 n_eff 2^-24 1.5625 (terms per element) < 0.5625 / 2  -- the bound is under half the
smallest possible term, so one missing, doubled or misplaced term in any element fails.

A. every tile instantiation: {wgrad2 NT 2 | 1, wgrad_kernel KMODE 0 | 1 | 2} x padding mode x BM {32, 64, 128} x VECA x {fp32, bf16},
   3x3 stride 1, ragged rows / K tiles / last chunk; the five forms again at 4x4 stride 2.
B. pipeline length of wgrad2_kernel (1 .. 33 stages in one split: each side of every refill of the 16-slot offset ring, a wrapped ring),
   a short last split, two M tiles with a ragged second, wgrad_reduce_kernel at 1 .. 64 splits (its four-accumulator loop needs 14),
   one un-forced case with several splits.
C. the small-M kernels: smallm_wgrad_kernel, the <= 4-row shapes that fall to the tile kernel, smallm_wgrad_strip_kernel NT 4 / 7 with
   strip tails, column groups, several splits; bf16 tensors against the same values up-cast to fp32 (bit-equal, ops.conv2d_bwd_weight
   relies on it).
D. ops.conv2d_bwd_weight(accumulate_into=...) on the generic route against base + ops.conv2d_bwd_weight(...), bit-equal.

Measured on an MI355X (256 CUs), max(|err| / bound) and relative L2 error per section (recorded, not gated):
  fp32 tensors                    cases   max |err| / bound    relative L2
    A  tile instantiations           70   0.005 .. 0.024       1.3e-7 .. 2.5e-7
    B  pipeline stages 1 .. 33      120   0.001 .. 0.048       6.8e-8 .. 5.9e-7   (the largest of both at 33 stages)
    B  short last split              24   0.001 .. 0.003       2.4e-7 .. 3.1e-7
    B  two M tiles                    8   0.008 .. 0.013       1.6e-7 .. 2.4e-7
    B  reduce, 1 .. 64 splits        32   0.001 .. 0.023       7.4e-8 .. 1.6e-7
    B  heuristic: 5 splits of 10      1   0.001                3.0e-7
    C  smallm_wgrad_kernel           14   <= 0.001             7.7e-8 .. 1.1e-7
    C  few rows on the tile kernel    8   0.002 .. 0.003       1.6e-7 .. 3.6e-7
    C  strip kernel                 120   <= 0.001             7.4e-8 .. 9.7e-8
  bf16 tensors (365 cases): every element equal to the float64 reference -- the products are exact in fp32 and so are these short
  sums of them; the strip kernel on bf16 tensors and on their fp32 up-cast gave the same bits in all 120 cases.
  The errors sit far inside the bound because it is a worst case over all orders and sign patterns, while rounding errors of random
  signs grow with the square root of the depth; what the gate buys is the condition above: any lost or doubled term is >= 2 x the bound."""
import ctypes
import functools

import pytest
import torch

from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TERM_MAX, TERM_MIN = 1.25 * 1.25, 0.75 * 0.75


@pytest.fixture
def force_ks():
    """sets the library's "wgrad_ks" option (cached launch plans hold workspace sizes that depend on it: dropped on every change) and
    restores the heuristic afterwards"""
    from pcgan_amd.hip import lib as L, ops

    def force(ks):
        L.set_option('wgrad_ks', ks)
        ops.clear_plans()
    try:
        yield force
    finally:
        L.set_option('wgrad_ks', 0)
        ops.clear_plans()


def _cdiv(a, b):
    return -(-a // b)


def _out(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


def _grad(x, dy, geom):
    N, C, H, W, K, Rr, S, stride, pad, pad_mode = geom
    w = torch.zeros(K, C, Rr, S, dtype=torch.float64, requires_grad=True)
    R.conv2d(x.double(), w, None, stride, pad, pad_mode).backward(dy.double())
    return w.grad.detach()


@functools.lru_cache(maxsize=None)
def _case(geom, half):
    """(x, dy, float64 reference, A = sum of |terms|) of one case on the CPU: made once, shared by the tests that use it, never written to"""
    N, C, H, W, K, Rr, S, stride, pad, pad_mode = geom
    g = torch.Generator().manual_seed(sum(v * (i + 1) * 7919 for i, v in enumerate(geom)) + int(half))

    def signed(*shape):
        mag = 0.75 + 0.5 * torch.rand(*shape, generator=g)
        return mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    x, dy = signed(N, C, H, W), signed(N, K, _out(H, Rr, stride, pad), _out(W, S, stride, pad))
    if half:
        x, dy = x.bfloat16(), dy.bfloat16()
    assert 0.75 <= float(x.float().abs().min()) and float(x.float().abs().max()) <= 1.25
    assert 0.75 <= float(dy.float().abs().min()) and float(dy.float().abs().max()) <= 1.25
    return x, dy, _grad(x, dy, geom), _grad(x.abs(), dy.abs(), geom)


def _forced(units, ks):
    """(splits, units per split) the option "wgrad_ks" = ks > 0 gives over `units` chunks (strips): cut to [1, units], then re-derived"""
    s = max(1, min(ks, units))
    per = _cdiv(units, s)
    return _cdiv(units, per), per


def _split_pixels(geom, rec):
    """the most output pixels one split sums: chunks of 32 pixels; strips are 8 rows of one column, ordered image, strip row, column"""
    N, C, H, W, K, Rr, S, stride, pad, _ = geom
    P, Q = _out(H, Rr, stride, pad), _out(W, S, stride, pad)
    if rec['family'] != 'strip':
        return min(rec['units'] * 32, N * P * Q)
    spc = _cdiv(P, 8)
    best = 0
    for sp in range(rec['splits']):
        strips = range(sp * rec['units'], min((sp + 1) * rec['units'], N * spc * Q))
        best = max(best, sum(min(8, P - 8 * ((sg % (spc * Q)) // Q)) for sg in strips))
    return best


def _launch(dev, geom, x, dy, base, half):
    """pcgan_conv2d_bwd_weight twice (accumulate 0 into NaN, accumulate 1 into base); returns (dw, accumulated, record) on the device"""
    from pcgan_amd.hip import lib as L, ops
    lib = L.load()
    N, C, H, W, K, Rr, S, stride, pad, pad_mode = geom
    d = ops.make_desc(N, C, H, W, K, Rr, S, stride, pad, pad_mode, ops.BF16 if half else ops.F32)
    nb = int(lib.pcgan_conv2d_workspace_bytes(ctypes.byref(d), L.PASS_BWD_WEIGHT))
    ws = torch.full((nb + 4096,), 0xFF, dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    xd, dyd = x.to(dev).contiguous(), dy.to(dev).contiguous()
    out = []
    seq0 = ops.wgrad_last_launch()['seq']
    for acc, dw in ((0, torch.full((K, C, Rr, S), float('nan'), device=dev)), (1, base.to(dev).clone())):
        L.check(lib.pcgan_conv2d_bwd_weight(ctypes.byref(d), vp(xd.data_ptr()), vp(dyd.data_ptr()), vp(dw.data_ptr()), acc, vp(ws.data_ptr()), nb,
                                            vp(torch.cuda.current_stream().cuda_stream)), 'conv2d_bwd_weight')
        rec = ops.wgrad_last_launch()
        assert rec['seq'] == seq0 + 1 + acc, 'one recorded launch per call: %r after %d' % (rec, seq0)
        out.append(dw)
    torch.cuda.synchronize()
    assert bool((ws[nb:] == 0xFF).all()), 'the kernel wrote behind the workspace it asked for (%d bytes)' % nb
    assert nb == _cdiv(rec['splits'] * K * Rr * S * _cdiv(C, 4) * 4 * 4, 256) * 256, 'workspace %d bytes does not hold %d splits' % (nb, rec['splits'])
    return out[0], out[1], rec


def _run(dev, sect, geom, half, expect):
    """one case: launch, record against `expect` (a dict of record fields), gate, accumulate"""
    N, C, H, W, K, Rr, S, stride, pad, pad_mode = geom
    x, dy, ref, A = _case(geom, half)
    g = torch.Generator().manual_seed(N + C + K + H + W)
    base = torch.randn(K, C, Rr, S, generator=g) * float(ref.abs().max())
    terms = N * _out(H, Rr, stride, pad) * _out(W, S, stride, pad)
    # the condition, before the launch, from the split the case expects
    n_pre = _split_pixels(geom, expect) + _cdiv(expect['splits'], 4) + 4
    assert 2 * n_pre * U * TERM_MAX * terms < TERM_MIN / 2, 'the bound (n_eff %d, %d terms) would not catch one lost term' % (n_pre, terms)
    dw, acc, rec = _launch(dev, geom, x, dy, base, half)
    want = dict(expect, mode=pad_mode, dtype=int(half))
    got = {k: rec[k] for k in want}
    assert got == want, 'the case ran another instantiation: %r, wanted %r' % (rec, want)
    n_eff = _split_pixels(geom, rec) + _cdiv(rec['splits'], 4) + 4
    assert n_eff <= n_pre, (n_eff, n_pre)
    bound = 2 * n_eff * U * A
    dwc = dw.double().cpu()
    err = (dwc - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    rel = float((dwc - ref).norm() / ref.norm())
    print('WGRAD %s %s %s: %s %s BM %d VECA %d variant %d mode %d, %d split(s) of %d; n_eff %d; max |err| / bound %.4f; relative L2 %.3e' % (
        sect, geom, 'bf16' if half else 'fp32', rec['family'], 'bf16' if rec['dtype'] else 'fp32', rec['bm'], rec['veca'], rec['variant'],
        rec['mode'], rec['splits'], rec['units'], n_eff, ratio, rel))
    assert bool(torch.isfinite(dwc).all()), 'elements nobody wrote (or NaN partial sums read): %d' % int((~torch.isfinite(dwc)).sum())
    assert bool((err <= bound).all()), '%d element(s) outside 2 n_eff 2^-24 A, worst %.3g x the bound at %r' % (
        int((err > bound).sum()), ratio, tuple(int(v) for v in torch.unravel_index((err / bound.clamp_min(1e-300)).argmax(), err.shape)))
    want_acc = base.to(dw.device) + dw
    assert torch.equal(acc, want_acc), 'accumulate = 1 is not base + dw bit for bit: %d element(s) differ' % int((acc != want_acc).sum())
    return dw, rec


def _plane(chunks, veca, ragged, N=1):
    """H x W (as square as it gets) with ceil(N H W / 32) == chunks, dY planes a multiple of 4 pixels or not, last chunk ragged or full"""
    cands = [(abs(H - W), H, W) for H in range(3, 64) for W in range(5, 64)
             if _cdiv(N * H * W, 32) == chunks and ((H * W) % 4 == 0) == veca and ((N * H * W) % 32 != 0) == ragged]
    assert cands, (chunks, veca, ragged, N)
    return min(cands)[1:]


# ---- A. every tile instantiation ----------------------------------------------------------------------------------------------------------
FORMS = {64: ('tile2', 2), 128: ('tile2', 1), 24: ('tile', 0), 10: ('tile', 1), 126: ('tile', 2)}      # C -> (family, variant)
BMS = {24: 32, 40: 64, 72: 128}                                                                          # K -> BM (ragged rows)
HALVES = pytest.mark.parametrize('half', [False, True], ids=['fp32', 'bf16'])
PAD_MODES = pytest.mark.parametrize('pad_mode', [0, 1], ids=['zero', 'reflect'])


@HALVES
@PAD_MODES
@pytest.mark.parametrize('hw,veca', [((6, 10), 1), ((5, 7), 0)], ids=['6x10', '5x7'])
@pytest.mark.parametrize('K', sorted(BMS))
@pytest.mark.parametrize('C', sorted(FORMS))
def test_tile_instantiation(dev, C, K, hw, veca, pad_mode, half):
    """3x3, stride 1, pad 1, N = 3, the heuristic's one split: 6 chunks with the last of 20 pixels (VECA) / 4 with the last of 9"""
    fam, var = FORMS[C]
    geom = (3, C, hw[0], hw[1], K, 3, 3, 1, 1, pad_mode)
    _run(dev, 'A', geom, half, dict(family=fam, variant=var, bm=BMS[K], veca=veca, splits=1, units=_cdiv(3 * hw[0] * hw[1], 32)))


@HALVES
@pytest.mark.parametrize('hw,veca', [((12, 10), 0), ((11, 9), 1)], ids=['12x10', '11x9'])
@pytest.mark.parametrize('C', sorted(FORMS))
def test_tile_forms_strided(dev, C, hw, veca, half):
    """4x4, stride 2, zero padding 1 (the strided tap offset): outputs 6x5 and 5x4"""
    fam, var = FORMS[C]
    P, Q = _out(hw[0], 4, 2, 1), _out(hw[1], 4, 2, 1)
    _run(dev, 'A', (3, C, hw[0], hw[1], 40, 4, 4, 2, 1, 0), half, dict(family=fam, variant=var, bm=64, veca=veca, splits=1, units=_cdiv(3 * P * Q, 32)))


# ---- B. pipeline length, split ranges, the reduce -----------------------------------------------------------------------------------------
STAGES2 = (1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 33)
STAGE_CASES = [(C, st) for C in (128, 64) for st in STAGES2] + [(24, st) for st in (1, 2, 9, 33)]


@HALVES
@PAD_MODES
@pytest.mark.parametrize('veca', [1, 0], ids=['veca', 'scalar'])
@pytest.mark.parametrize('C,stages', STAGE_CASES)
def test_pipeline_stages(dev, force_ks, C, stages, veca, pad_mode, half):
    """one split of `stages` chunks (wgrad_ks = 1), K = 8, 3x3 pad 1, N = 1: odd and even counts, each side of every refill of
    wgrad2_kernel's 16-slot offset ring (stages 8, 16, 24 issue the next), a wrapped ring from 17 on; the last chunk ragged in every
    scalar case and in the VECA cases with an odd count"""
    fam, var = FORMS[C]
    H, W = _plane(stages, bool(veca), not veca or stages % 2 == 1)
    force_ks(1)
    _run(dev, 'B.stages', (1, C, H, W, 8, 3, 3, 1, 1, pad_mode), half, dict(family=fam, variant=var, bm=32, veca=veca, splits=1, units=stages))


SHORT = {    # (chunks, wgrad_ks) -> (N, VECA plane, scalar plane, splits, chunks per split)
    (20, 3): (2, (14, 22), (18, 17), 3, 7),      # 7 + 7 + 6
    (33, 4): (3, (8, 43), (15, 23), 4, 9),       # 9 + 9 + 9 + 6
}


@HALVES
@PAD_MODES
@pytest.mark.parametrize('veca', [1, 0], ids=['veca', 'scalar'])
@pytest.mark.parametrize('chunks,ks', sorted(SHORT))
@pytest.mark.parametrize('C', [128, 64, 24])
def test_short_last_split(dev, force_ks, C, chunks, ks, veca, pad_mode, half):
    """several splits, the last one short (the c_end clamp), splits that start inside one image and end in the next"""
    fam, var = FORMS[C]
    N, pv, ps, splits, per = SHORT[(chunks, ks)]
    H, W = pv if veca else ps
    assert _cdiv(N * H * W, 32) == chunks and chunks - (splits - 1) * per < per
    force_ks(ks)
    _run(dev, 'B.short', (N, C, H, W, 8, 3, 3, 1, 1, pad_mode), half, dict(family=fam, variant=var, bm=32, veca=veca, splits=splits, units=per))


@HALVES
@PAD_MODES
@pytest.mark.parametrize('hw,veca', [((6, 10), 1), ((5, 7), 0)], ids=['6x10', '5x7'])
@pytest.mark.parametrize('C', [128, 24])
def test_two_m_tiles(dev, C, hw, veca, pad_mode, half):
    """K = 136: two M tiles of 128 rows, the second with 8"""
    fam, var = FORMS[C]
    _run(dev, 'B.mtiles', (3, C, hw[0], hw[1], 136, 3, 3, 1, 1, pad_mode), half,
         dict(family=fam, variant=var, bm=128, veca=veca, splits=1, units=_cdiv(3 * hw[0] * hw[1], 32)))


@pytest.mark.parametrize('splits', [1, 2, 3, 4, 5, 8, 12, 13, 14, 16, 17, 20, 29, 32, 33, 64])
@pytest.mark.parametrize('C,K,pad_mode', [(16, 8, 0), (10, 5, 1)], ids=['1152_columns', '540_columns'])
def test_reduce_splits(dev, force_ks, C, K, pad_mode, splits):
    """wgrad_reduce_kernel: every remainder of its loops (four waves take the splits round-robin, four accumulators each from 14 splits
    on), whole workgroups (C = 16, K = 8: 1152 partial-sum columns) and a ragged last one with padded channels that must not reach dw
    (C = 10, K = 5: 540 columns of 12 channels); up to 17 splits of two chunks with a last one of one, beyond that one chunk per split"""
    chunks = 1 if splits == 1 else (2 * splits - 1 if splits <= 17 else splits)
    veca = splits % 2 == 0
    H, W = _plane(chunks, veca, True, N=2)
    force_ks(splits)
    _run(dev, 'B.reduce', (2, C, H, W, K, 3, 3, 1, 1, pad_mode), False,
         dict(family='tile', variant=0 if C == 16 else 1, bm=32, veca=int(veca), splits=splits, units=_cdiv(chunks, splits)))


@HALVES
def test_heuristic_multi_split(dev, half):
    """the heuristic's own path with several splits and a short last one: N = 2, 64 -> 32, 5x5 pad 2 at 27x27 is 46 chunks (256 CUs: 5
    splits of 10, the last of 6); what the record says is asserted, not those numbers"""
    from pcgan_amd.hip import lib as L, ops
    geom = (2, 64, 27, 27, 32, 5, 5, 1, 2, 0)
    d = ops.make_desc(*geom, ops.BF16 if half else ops.F32)
    splits = int(L.load().pcgan_conv2d_workspace_bytes(ctypes.byref(d), L.PASS_BWD_WEIGHT)) // (32 * 25 * 64 * 4)      # (whole partial sums)
    _, rec = _run(dev, 'B.heuristic', geom, half, dict(family='tile2', variant=2, bm=32, veca=0, splits=splits, units=_cdiv(46, splits)))
    assert rec['splits'] >= 2 and rec['splits'] == _cdiv(46, rec['units']) and 46 % rec['units'] != 0, rec


# ---- C. the small-M kernels ---------------------------------------------------------------------------------------------------------------
SMALLM = {    # name: (geometry without the padding mode, padding modes)
    'k4_c32_3x3': ((3, 32, 13, 11, 4, 3, 3, 1, 1), (0, 1)),          # 429 pixels
    'k1_c16_4x4_s2': ((3, 16, 22, 18, 1, 4, 4, 2, 1), (0, 1)),       # 11 x 9 outputs: 297 pixels
    'k3_c16_p10': ((3, 16, 10, 13, 3, 3, 3, 1, 1), (0, 1)),          # 10 output rows: below the strip kernel's 16; 390 pixels
    'k2_c14_1x1': ((3, 14, 11, 13, 2, 1, 1, 1, 0), (0,)),            # 16 padded channels, two of them padding; 429 pixels
}
SMALLM_CASES = [(name, pm) for name in sorted(SMALLM) for pm in SMALLM[name][1]]
KS03 = pytest.mark.parametrize('ks', [0, 3])


@HALVES
@KS03
@pytest.mark.parametrize('name,pad_mode', SMALLM_CASES)
def test_smallm_kernel(dev, force_ks, name, pad_mode, ks, half):
    """smallm_wgrad_kernel: one split (a thread walks its pixels 256 apart: pixel counts that are no multiple of 256) and three"""
    geom = SMALLM[name][0] + (pad_mode,)
    N, C, H, W, K, Rr, S, stride, pad, _ = geom
    chunks = _cdiv(N * _out(H, Rr, stride, pad) * _out(W, S, stride, pad), 32)
    assert (N * _out(H, Rr, stride, pad) * _out(W, S, stride, pad)) % 256 != 0
    splits, per = _forced(chunks, ks) if ks else (1, chunks)
    force_ks(ks)
    _run(dev, 'C.smallm', geom, half, dict(family='smallm', variant=0, bm=0, veca=0, splits=splits, units=per))


@HALVES
@KS03
@PAD_MODES
@pytest.mark.parametrize('C,K,k,pad,hw,variant,veca', [(24, 2, 3, 1, (10, 13), 0, 0), (3, 1, 7, 3, (10, 12), 1, 1)], ids=['k2_c24_3x3', 'k1_c3_7x7'])
def test_few_rows_on_the_tile_kernel(dev, force_ks, C, K, k, pad, hw, variant, veca, pad_mode, ks, half):
    """K <= 4 with a padded channel count that is no multiple of 16: the tile kernel at BM 32, 30 / 31 of 32 rows masked"""
    geom = (3, C, hw[0], hw[1], K, k, k, 1, pad, pad_mode)
    chunks = _cdiv(3 * hw[0] * hw[1], 32)
    splits, per = _forced(chunks, ks) if ks else (1, chunks)
    force_ks(ks)
    _run(dev, 'C.fewrows', geom, half, dict(family='tile', variant=variant, bm=32, veca=veca, splits=splits, units=per))


STRIP_FILTERS = [(3, 3, 1, 4), (4, 4, 1, 4), (5, 5, 2, 7), (7, 7, 3, 7), (3, 5, 1, 7), (5, 3, 1, 7)]       # R, S, pad, NT
STRIP_SHAPES = [(1, 16, 17), (2, 18, 19), (3, 16, 16), (3, 18, 19)]                                        # M, C, P
STRIP_CASES = [(Rr, S, pad, nt, M, C, P, ks) for Rr, S, pad, nt in STRIP_FILTERS for M, C, P in STRIP_SHAPES for ks in ((0, 3, 4) if P == 19 else (0, 3))]


@HALVES
@PAD_MODES
@pytest.mark.parametrize('Rr,S,pad,nt,M,C,P,ks', STRIP_CASES)
def test_strip_kernel(dev, force_ks, Rr, S, pad, nt, M, C, P, ks, pad_mode, half):
    """smallm_wgrad_strip_kernel, N = 2, 13 output columns: NT 4 (3x3, 4x4) and NT 7 (5x5: the second column group holds one column;
    7x7: groups of 4 + 3; 3x5 / 5x3: rows and columns masked differently); 16, 17, 19 output rows (whole strips, tails of 1 and 3 rows);
    one split, three (P = 19: 78 strips, 26 + 26 + 26; P = 16: 52 strips, 18 + 18 + 16) and four (P = 19: 20 + 20 + 20 + 18).
    bf16 tensors: the same values up-cast to fp32 must give the same bits (ops.conv2d_bwd_weight sends bf16 tensors that way)."""
    geom = (2, C, P - 2 * pad + Rr - 1, 13 - 2 * pad + S - 1, M, Rr, S, 1, pad, pad_mode)
    strips = 2 * _cdiv(P, 8) * 13
    splits, per = _forced(strips, ks) if ks else (1, strips)
    if P == 19 and ks:
        assert (splits, per) == ((3, 26) if ks == 3 else (4, 20))
    force_ks(ks)
    dw, _ = _run(dev, 'C.strip', geom, half, dict(family='strip', variant=nt, bm=0, veca=0, splits=splits, units=per))
    if half:
        x, dy, ref, _ = _case(geom, True)
        dw32, _, rec = _launch(dev, geom, x.float(), dy.float(), torch.zeros_like(ref, dtype=torch.float32), False)
        assert (rec['family'], rec['variant'], rec['dtype'], rec['splits'], rec['units']) == ('strip', nt, 0, splits, per), rec
        assert torch.equal(dw, dw32), 'bf16 tensors and their fp32 up-cast differ in %d element(s)' % int((dw != dw32).sum())


# ---- D. the Python wrapper ------------------------------------------------------------------------------------------------------------------
@HALVES
@pytest.mark.parametrize('geom,family', [((3, 24, 6, 10, 40, 3, 3, 1, 1, 0), 'tile'), ((2, 16, 19, 13, 3, 7, 7, 1, 3, 1), 'strip')], ids=['tile', 'strip'])
def test_wrapper_accumulates_bit_equal(dev, geom, family, half):
    """ops.conv2d_bwd_weight(accumulate_into = base) == base + ops.conv2d_bwd_weight(...), bit for bit, on the generic route"""
    from pcgan_amd.hip import ops
    N, C, H, W, K, Rr, S, stride, pad, pad_mode = geom
    x, dy, ref, _ = _case(geom, half)
    xd, dyd = x.to(dev), dy.to(dev)
    for dt in {ops.BF16 if half else ops.F32, ops.F32}:        # (bf16 strip shapes are sent to the fp32 kernel)
        assert ops._plan(ops._L.PASS_BWD_WEIGHT, N, C, H, W, K, Rr, S, stride, pad, pad_mode, dt).route == 'generic'
    g = torch.Generator().manual_seed(N + C + K)
    base = (torch.randn(K, C, Rr, S, generator=g) * float(ref.abs().max())).to(dev)
    seq0 = ops.wgrad_last_launch()['seq']
    dw = ops.conv2d_bwd_weight(xd, dyd, (K, C, Rr, S), stride, pad, pad_mode)
    acc = ops.conv2d_bwd_weight(xd, dyd, (K, C, Rr, S), stride, pad, pad_mode, accumulate_into=base.clone())
    torch.cuda.synchronize()
    rec = ops.wgrad_last_launch()
    assert rec['seq'] == seq0 + 2 and rec['family'] == family, rec
    assert float((dw.double().cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    assert torch.equal(acc, base + dw), '%d element(s) differ' % int((acc != base + dw).sum())
