"""The case table of tests/test_gpu_thin_cases.py (tests/thin_cases.py), checked without a GPU: every case is a thin-kernel shape for the
kernel and host form it names, reaches the tile edge it claims, and satisfies the condition that makes its gate bite (section A: the
largest bound under half the smallest term; section B: every partial sum under 2^24 quanta).  The arithmetic of the kernel, restated in
torch (thin_cases.emulate), is exact on the section B data and stops being exact when one low piece is zeroed or one tap is shifted -- so an
exact comparison on the GPU sees such a fault.  Section D: the library's predicates (pcgan_conv2d_thin_supported, _packed_bytes,
_workspace_bytes; the library loads without a GPU) on both sides of every limit of thin_geometry."""
import ctypes

import pytest
import torch

import thin_cases as T

NAMES = list(T.BY_NAME)
EXACT = [n for n in NAMES if T.BY_NAME[n].kind != 'signed']


@pytest.mark.parametrize('name', NAMES)
def test_case(name):
    c = T.BY_NAME[name]
    assert T.accepts(c.pass_, c.geom) and T.classify(c.pass_, c.geom) == c.want and c.want in T.ACCEPTED
    assert T.rows_of(c) in (64, 128, 192, 256) and 1 <= T.gathered(c) <= 4
    for claim in c.claims:
        assert T.CLAIMS[claim](c), 'the case claims %r: grid %r' % (claim, T.grid(c))
    d = T.data(c)
    assert d.ref.shape == d.A.shape and bool((d.A >= d.ref.abs() - 1e-9 * d.A).all())
    if c.pass_ == 'dgrad':
        assert not c.bias and c.act == 0, 'the thin data gradient takes no bias and no activation'
    if c.kind == 'signed':
        for t, s in ((d.src, 1.0), (d.w, 2.0 ** c.wexp)) + (((d.b, 1.0),) if c.bias else ()):
            assert 0.75 * s <= float(t.abs().min()) and float(t.abs().max()) <= 1.25 * s
        worst, allowed = T.condition(c)
        assert worst < allowed, 'the largest bound %.4f would not catch one lost term (%.4f allowed)' % (worst, allowed)
        assert c.act in (0, 1, 2) or (c.wexp == -4 and c.want[0] == '<4,4,2>' and float(d.ref.abs().max()) < 8)
        assert float(d.A.min()) >= T.TERM_MIN * 2.0 ** c.wexp, 'every element sums at least one term'
    else:
        assert T.quanta(c) < 2.0 ** 24, 'partial sums of up to %.3g quanta: fp32 accumulation would not be exact' % T.quanta(c)
        assert c.act in (0, 1, 2) and T.slope_of(c) == 0.25
        top = 2 ** c.bits - 1
        if c.kind == 'xlow':
            assert bool((d.src == d.src.round()).all()) and float(d.src.abs().max()) == top and set(d.w.unique().tolist()) == {-1.0, 0.0, 1.0}
            assert d.b is None or (bool((d.b == d.b.round()).all()) and float(d.b.abs().max()) <= 64)
        else:
            ints = d.w / torch.pow(2.0, d.rowexp.float()).view((-1, 1, 1, 1) if c.pass_ == 'fwd' else (1, -1, 1, 1))
            assert bool((ints == ints.round()).all()) and float(ints.abs().max()) <= top
            assert int(d.rowexp[0]) == 20 and int(d.rowexp[1]) == -20 and set(d.src.unique().tolist()) == {-1.0, 0.0, 1.0}


def test_worst_shape_condition():
    """7x7 on 4 channels: the issue's figure, max E about 0.016 against the 0.281 allowed"""
    worst = max(T.condition(c)[0] for c in T.CASES if c.kind == 'signed' and c.geom[5] == 7 and T.gathered(c) == 4 and c.geom[9] == 0)
    assert 0.008 < worst < 0.03, worst


def test_table_covers_every_kernel_form_and_width():
    for sect in ('A', 'B'):
        cs = [c for c in T.CASES if c.sect == sect]
        assert {c.want for c in cs} == set(T.ACCEPTED)
    A = [c for c in T.CASES if c.sect == 'A']
    for pair in T.ACCEPTED:
        assert any(T.CLAIMS['ragged'](c) or T.CLAIMS['tile_plus_one'](c) for c in A if c.want == pair)
    assert {T.rows_of(c) // 64 for c in A} == {1, 2, 3, 4} and {T.gathered(c) for c in A} == {1, 2, 3, 4}
    for k in T.KERNELS:      # every kernel: 1 .. 4 gathered channels, a bias at least twice, an exact tile and one row and column more
        ks = [c for c in A if c.want[0] == k]
        assert {T.gathered(c) for c in ks} == {1, 2, 3, 4}
        assert sum(1 for c in ks if c.bias) >= 2
        assert any(T.CLAIMS['one_tile'](c) for c in ks) and any(T.CLAIMS['tile_plus_one'](c) for c in ks)
    assert {c.act for c in A if c.bias} == {0, 1, 2, 3, 4}
    assert {c.geom[8] for c in A if c.want[1] == 'dgrad_zero'} >= {0, 1, 3, 5, 6}
    assert {c.geom[8] for c in A if c.want[1] == 'fwd_reflect'} >= {1, 3, 5} and {c.geom[8] for c in A if c.want[1] == 'dgrad_reflect'} >= {1, 3, 5}
    B = [c for c in T.CASES if c.sect == 'B']
    assert 12 <= len(B) <= 14
    for pair in T.ACCEPTED:
        assert {c.kind for c in B if c.want == pair} == {'xlow', 'wlow'}


@pytest.mark.parametrize('name', EXACT + ['C.maxpos'])
def test_emulation_is_exact_and_notices_one_piece(name):
    """scale, split to fp16, three products accumulated in fp32, scale back: equal to float64 in every element; not equal once one low
    piece is zeroed or one tap is shifted"""
    c = T.MAXPOS if name == 'C.maxpos' else T.BY_NAME[name]
    d = T.data(c)
    ref = T.bounds(c)[2]
    y, (xl, wl) = T.emulate(c)
    assert bool((y == ref).all()), '%d element(s) differ' % int((y != ref).sum())
    low = xl if c.kind != 'wlow' else wl
    frac = float((low != 0).float().mean())
    print('THIN-EMU %s: %.0f %% of the low pieces are non-zero' % (name, 100 * frac))
    if c.kind == 'xlow':
        assert frac > (0.5 if c.bits >= 14 else 0.3)      # b bits leave b - 11 to the low piece: 81 % non-zero at 15, 36 % at 12
        assert not bool((wl != 0).any()), 'weights in {-1, 0, 1} have no low piece: the (Al, Bh) product is held by the wlow cases'
    elif c.kind == 'wlow':
        assert frac > 0.5 and not bool((xl != 0).any())
    else:
        assert int((low != 0).sum()) == 1      # only the pinned element has one
    if c.act == 0:      # (a ReLU may hide the one element: the perturbed runs compare the linear result)
        for perturb in ('zero_wl' if c.kind == 'wlow' else 'zero_xl', 'shift_tap'):
            bad, _ = T.emulate(c, perturb)
            n = int((bad != ref).sum())
            print('THIN-EMU %s: %s changes %d element(s)' % (name, perturb, n))
            assert n > 0, perturb
    else:
        lin = c._replace(act=0)
        for perturb in ('zero_xl', 'shift_tap'):
            assert int((T.emulate(lin, perturb)[0] != T.bounds(lin)[2]).sum()) > 0, perturb
    assert d.src.dtype == torch.float32


def test_maxima_slots():
    assert T.maxima_slots(1) == [0] and T.maxima_slots(5) == [0, 4] and T.maxima_slots(1023) == [0, 1022]
    assert T.maxima_slots(1024) == [0, 1023] and T.maxima_slots(1025) == [0, 1023, 1024]
    mid = [4 * T.NT + 1, 4 * (2 * T.NT + 77) + 2]      # float4 NT (thread 0's second load) and 2 NT + 77 (thread 77's third load)
    assert T.maxima_slots(4096) == [0] + mid + [4095] and T.maxima_slots(4100) == [0] + mid + [4095, 4099]
    assert T.maxima_slots(4103) == [0] + mid + [4095, 4099, 4102]
    assert mid == [1025, 2358] and mid[0] // 4 == T.NT and mid[1] // 4 == 2 * T.NT + 77 and 77 + 3 * T.NT < 4096 // 4


# ---- section D: the predicates ---------------------------------------------------------------------------------------------------------------
def _desc(lib, geom, dt=None):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    d = lib.ConvDesc(N, C, H, W, K, Rr, S, st, pad, pm, T.out_size(H, Rr, st, pad), T.out_size(W, S, st, pad))
    d.dtype = lib.F32 if dt is None else dt
    return d


def test_predicates_on_both_sides_of_every_limit():
    from pcgan_amd.hip import lib
    h = lib.load()
    FWD, BWD = lib.PASS_FWD, lib.PASS_BWD_DATA

    def ok(pass_, geom, dt=None):
        d = _desc(lib, geom, dt)
        p = FWD if pass_ == 'fwd' else BWD
        s = h.pcgan_conv2d_thin_supported(ctypes.byref(d), p)
        nb, ws = h.pcgan_conv2d_thin_packed_bytes(ctypes.byref(d), p), h.pcgan_conv2d_thin_workspace_bytes(ctypes.byref(d), p)
        assert s in (0, 1) and (nb > 0) == bool(s) and (s or ws == 0)
        assert bool(s) == T.accepts(pass_, geom, dt in (None, lib.F32)), (pass_, geom)
        return bool(s), nb, ws

    yes = lambda *a: ok(*a)[0]
    # forward: gathered channels
    for C in (1, 2, 3, 4):
        assert yes('fwd', (2, C, 16, 16, 64, 7, 7, 1, 3, 0))
    assert not yes('fwd', (2, 5, 16, 16, 64, 7, 7, 1, 3, 0))
    # produced channels
    for K in (64, 128, 192, 256):
        assert yes('fwd', (2, 4, 16, 16, K, 7, 7, 1, 3, 0))
    for K in (48, 65, 320):
        assert not yes('fwd', (2, 4, 16, 16, K, 7, 7, 1, 3, 0))
    # filters and strides
    assert yes('fwd', (2, 4, 16, 16, 64, 7, 7, 1, 3, 0)) and yes('fwd', (2, 4, 16, 16, 64, 7, 7, 2, 3, 0))
    assert yes('fwd', (2, 4, 16, 16, 64, 4, 4, 2, 1, 0)) and not yes('fwd', (2, 4, 16, 16, 64, 4, 4, 1, 1, 0))
    assert not yes('fwd', (2, 4, 16, 16, 64, 3, 3, 1, 1, 0)) and not yes('fwd', (2, 4, 16, 16, 64, 7, 4, 2, 1, 0))
    # reflection: stride 1 only, pad < H and pad < W
    assert yes('fwd', (2, 4, 16, 16, 64, 7, 7, 1, 3, 1)) and not yes('fwd', (2, 4, 16, 16, 64, 7, 7, 2, 3, 1))
    assert not yes('fwd', (2, 4, 16, 16, 64, 4, 4, 2, 1, 1))
    assert yes('fwd', (1, 4, 6, 9, 64, 7, 7, 1, 5, 1)) and not yes('fwd', (1, 4, 6, 9, 64, 7, 7, 1, 6, 1))
    assert yes('fwd', (1, 4, 9, 6, 64, 7, 7, 1, 5, 1)) and not yes('fwd', (1, 4, 9, 6, 64, 7, 7, 1, 6, 1))
    assert yes('fwd', (1, 4, 3, 5, 64, 7, 7, 1, 6, 0))          # zero padding: any
    # storage type
    assert not yes('fwd', (2, 4, 16, 16, 64, 7, 7, 1, 3, 0), lib.BF16) and not yes('dgrad', (2, 64, 16, 16, 3, 7, 7, 1, 3, 0), lib.BF16)
    # data gradient: gathered K, produced C, stride, zero padding 0 .. 6, reflection of any pad
    for K in (1, 2, 3, 4):
        assert yes('dgrad', (2, 64, 16, 16, K, 7, 7, 1, 3, 0))
    assert not yes('dgrad', (2, 64, 16, 16, 5, 7, 7, 1, 3, 0))
    for C in (64, 128, 192, 256):
        assert yes('dgrad', (2, C, 16, 16, 3, 7, 7, 1, 3, 0))
    for C in (48, 65, 320):
        assert not yes('dgrad', (2, C, 16, 16, 3, 7, 7, 1, 3, 0))
    assert not yes('dgrad', (2, 64, 16, 16, 3, 7, 7, 2, 3, 0)) and not yes('dgrad', (2, 64, 16, 16, 3, 4, 4, 2, 1, 0))
    assert not yes('dgrad', (2, 64, 16, 16, 3, 7, 7, 2, 3, 1))
    assert yes('dgrad', (2, 64, 16, 16, 3, 7, 7, 1, 0, 0)) and yes('dgrad', (2, 64, 16, 16, 3, 7, 7, 1, 6, 0))
    assert not yes('dgrad', (2, 64, 16, 16, 3, 7, 7, 1, 7, 0))
    assert yes('dgrad', (2, 64, 16, 16, 3, 7, 7, 1, 7, 1))
    # a forward shape is no data-gradient shape and the other way round
    assert not yes('dgrad', (2, 4, 16, 16, 64, 7, 7, 1, 3, 0)) and not yes('fwd', (2, 64, 16, 16, 3, 7, 7, 1, 3, 0))
    # sizes
    for M, nst_, R_, st_, pad_ in ((64, 13, 7, 1, 3), (128, 13, 7, 2, 3), (192, 4, 4, 2, 1), (256, 4, 4, 2, 1)):
        _, nb, ws = ok('fwd', (2, 4, 16, 16, M, R_, R_, st_, pad_, 0))
        assert nb == (M // 32) * nst_ * 2 * 64 * 16 + 4 * M and ws == 0
    for N, C, H, W, K, pad in ((2, 64, 9, 33, 3, 3), (1, 256, 4, 4, 4, 3), (3, 128, 12, 40, 1, 1)):
        _, nb, ws = ok('dgrad', (N, C, H, W, K, 7, 7, 1, pad, 1))
        assert nb == (C // 32) * 13 * 2 * 64 * 16 + 4 * C and ws == 4 * N * C * (H + 2 * pad) * (W + 2 * pad)
        _, nb, ws = ok('dgrad', (N, C, H, W, K, 7, 7, 1, pad, 0))
        assert nb == (C // 32) * 13 * 2 * 64 * 16 + 4 * C and ws == 0
    # null descriptor, unknown pass
    assert h.pcgan_conv2d_thin_supported(None, FWD) == 0
    assert h.pcgan_conv2d_thin_supported(ctypes.byref(_desc(lib, (2, 4, 16, 16, 64, 7, 7, 1, 3, 0))), lib.PASS_BWD_WEIGHT) == 0


@pytest.mark.parametrize('name', NAMES + ['C.maxpos'])
def test_library_accepts_every_case_and_sizes_match(name):
    """a case the library refused at the descriptor check would be no thin-kernel case; the sizes the GPU test allocates by are the formulas"""
    from pcgan_amd.hip import lib
    h = lib.load()
    c = T.MAXPOS if name == 'C.maxpos' else T.BY_NAME[name]
    d = _desc(lib, c.geom)
    p = lib.PASS_FWD if c.pass_ == 'fwd' else lib.PASS_BWD_DATA
    assert h.pcgan_conv2d_thin_supported(ctypes.byref(d), p) == 1
    assert h.pcgan_conv2d_thin_packed_bytes(ctypes.byref(d), p) == T.packed_bytes(c)
    assert h.pcgan_conv2d_thin_workspace_bytes(ctypes.byref(d), p) == T.workspace_bytes(c)
