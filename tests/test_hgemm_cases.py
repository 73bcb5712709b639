"""The case table of tests/test_gpu_hgemm_cases.py (tests/hgemm_cases.py), checked without a GPU: every case's launch record and claims
hold under the restated host routing (conv_f32_cases.plan), satisfies the condition that makes its gate bite (section A: the largest
bound under half the smallest term; section B: every partial sum under 2^24 quanta), all 24 instantiations of hgemm_kernel are hit in
both sections and every claim is made by some case.  The kernel's arithmetic restated in torch (hgemm_cases.emulate) equals the float64
reference on the section B data and stays inside the bound on the section A data; each perturbation of it -- a fault of the kind a rewrite
of the kernel can make -- fails the gates of at least one case (the sensitivity study: a kernel made wrong on purpose is not run on a
GPU).  The restated `supported` predicate is held against the library, which loads without a GPU."""
import collections
import ctypes

import pytest
import torch

import hgemm_cases as T

NAMES = list(T.BY_NAME)
EXACT = [n for n in NAMES if T.BY_NAME[n].kind != 'signed']
SIGNED = [n for n in NAMES if T.BY_NAME[n].kind == 'signed']
NEW_CLAIMS = ('stages_1', 'stages_2', 'stages_3', 'odd_stages', 'slice_starts_in_chunk', 'tile_spans_images', 'tile_spans_phases', 'phases_16',
              'nonsquare', 'm_33', 'm_tile_plus_8', 'plane_under_filter', 'all_mirror', 'p_under_32', 'bias', 'clamped_tile',
              'split', 'empty_slice', 'short_slice', 'need_zero', 'phases_differ', 'm_ragged', 'm_blocks', 'p_ragged', 'p_blocks')


@pytest.mark.parametrize('name', NAMES)
def test_case(name):
    c = T.BY_NAME[name]
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    pl = T.hgemm_plan(c)
    assert T.record(pl) == c.want, 'the plan launches %r' % (T.record(pl),)
    assert c.want[0] == T.FORMS[c.half] and T.inst(c) in T.INSTANTIATIONS
    assert T.supported(c.geom, c.pass_), 'no shape of the packed implicit GEMM'
    for claim in c.claims:
        assert T.holds(c, claim), claim
    sshape, oshape, M = T.shapes(c)
    assert N <= 3 and C <= 136 and K <= 136 and M > 32 and 16 <= (C if c.pass_ == 'fwd' else K) <= 48
    assert (H <= 15 and W <= 15) or (H == 1 and Rr * S == 1), 'planes of at most 15 x 15 (one-row planes for the prime pixel counts)'
    d = T.data(c)
    assert tuple(d.src.shape) == sshape and tuple(d.ref.shape) == oshape
    if c.pass_ == 'dgrad':
        assert c.act == 0 and pm == 0, 'the data gradient takes no activation and no reflection'
        assert not (c.bias and pl.need_zero), 'a bias with uncovered phases is refused'
    if c.half:
        assert bool((T._bf16(d.src) == d.src).all()) and bool((T._bf16(d.w) == d.w).all()), 'operands of bf16 tensors are bf16 numbers'
    if c.kind == 'signed':
        for t, s in ((d.src, 1.0), (d.w, 2.0 ** c.wexp)) + (((d.b, 1.0),) if c.bias else ()):
            assert 0.75 * s <= float(t.abs().min()) and float(t.abs().max()) <= 1.25 * s
        worst, allowed = T.condition(c)
        assert worst < allowed, 'the largest bound %.4f would not catch one lost term (%.4f allowed)' % (worst, allowed)
        kp = max(p.Kp for p in pl.phases)
        assert kp <= (144 if c.half else 640)
        assert c.act in (0, 1, 2) or c.wexp == -3
        if pl.need_zero:
            assert bool((d.A == 0).any()) and bool((T.bounds(c)[1][d.A == 0] <= 1e-30).all()), 'pixels no phase writes: bound 0'
    else:
        assert T.quanta(c) < 2.0 ** 24, 'partial sums of up to %.3g quanta: fp32 accumulation would not be exact' % T.quanta(c)
        assert max(p.Kp for p in pl.phases) <= 511 and c.act in (0, 1, 2) and T.slope_of(c) == 0.25
        top = 2 ** (8 if c.half else 15) - 1
        for t in (d.src, d.b):
            assert t is None or bool((t == t.round()).all())
        if c.kind == 'xlow':
            assert float(d.src.abs().max()) == top and set(d.w.unique().tolist()) == {-1.0, 0.0, 1.0}
            assert d.b is None or float(d.b.abs().max()) <= 64
        else:
            ints = d.w if d.rowexp is None else d.w / torch.pow(2.0, d.rowexp.float()).view((-1, 1, 1, 1) if c.pass_ == 'fwd' else (1, -1, 1, 1))
            assert bool((ints == ints.round()).all()) and float(ints.abs().max()) <= top and not c.bias
            assert (d.rowexp is not None) == (not c.half) and set(d.src.unique().tolist()) == {-1.0, 0.0, 1.0}
            assert d.rowexp is None or (int(d.rowexp[0]) == 20 and int(d.rowexp[1]) == -20)


def test_worst_conditions():
    """fp32 tensors: the coefficient at 16 channels x 25 taps, and the largest condition of the table well inside the 0.281 allowed;
    bf16 tensors: half an ulp at |ref| < 72 is what the condition allows, which 144 terms respect and 288 do not"""
    assert abs((2 * (3 * 400 + 1 + 8) * T.U + 2.0 ** -20) - 1.451e-4) < 1e-6
    w32 = max(T.condition(c)[0] for c in T.CASES if c.kind == 'signed' and not c.half and c.wexp == 0)
    w16 = max(T.condition(c)[0] for c in T.CASES if c.kind == 'signed' and c.half and c.wexp == 0)
    print('HGEMM-CPU largest condition: fp32 tensors %.4f, bf16 tensors %.4f of %.4f allowed' % (w32, w16, T.TERM_MIN / 2))
    assert 0.03 < w32 < 0.1 and w16 < T.TERM_MIN / 2
    probe = T.BY_NAME['A.fwd_zero-3x3-c32-64128-ks4-signed-fp32']._replace(half=True, want=())
    worst, allowed = T.condition(probe)
    assert worst > 0.7 * allowed, '288 terms leave bf16 tensors next to no room: %.4f of %.4f' % (worst, allowed)


def test_table_covers_every_instantiation_and_claim():
    for sect in 'AB':
        got = {T.inst(c) for c in T.CASES if c.sect == sect}
        assert got == set(T.INSTANTIATIONS), 'section %s misses %r' % (sect, set(T.INSTANTIATIONS) - got)
        for i in T.INSTANTIATIONS:      # a whole launch and a split launch for each instantiation
            assert {c.want[4] > 1 for c in T.CASES if c.sect == sect and T.inst(c) == i} == {False, True}, (sect, i)
    for i in T.INSTANTIATIONS:
        mine = [c for c in T.CASES if c.sect == 'A' and T.inst(c) == i]
        rows = {T.shapes(c)[2] for c in mine}
        assert rows >= set(T.M_OF[i[1]]), (i, rows)
        bp = i[2]
        tot = {p.Ptot for c in mine for p in T.hgemm_plan(c).phases}
        assert {bp - 1, bp, bp + 1} <= tot and min(tot) < 32, (i, sorted(tot))
        assert any('tile_spans_images' in c.claims for c in mine), i
    made = {cl for c in T.CASES for cl in c.claims}
    assert made >= set(NEW_CLAIMS), set(NEW_CLAIMS) - made
    A = [c for c in T.CASES if c.sect == 'A']
    B = [c for c in T.CASES if c.sect == 'B']
    for i in T.INSTANTIATIONS:      # what every mode x tile x storage type covers
        mode, bm, bp, dt = i
        mine = [c for c in A if T.inst(c) == i]
        filt = {(c.geom[5], c.geom[6]) for c in mine}
        need = {(1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (3, 3), (2, 3)} | (set() if dt == 'bf16' else {(4, 4), (5, 5), (3, 5)})
        assert filt >= need, (i, need - filt)
        assert {c.geom[1] if c.pass_ == 'fwd' else c.geom[4] for c in mine if c.geom[5] * c.geom[6] == 1} >= {16, 32, 48}, i
        assert {c.geom[7] for c in mine} >= {1, 2, 4}, i
        assert {c.want[5] for c in mine} >= ({1, 4, 16} if mode == 'dgrad' else {1}), i
        if mode != 'fwd_reflect':
            assert {c.geom[8] for c in mine if (c.geom[5], c.geom[6], c.geom[7]) == (3, 3, 1)} >= {0, 1, 2}, i
            assert {c.geom[8] for c in mine if (c.geom[5], c.geom[6], c.geom[7]) == (2, 2, 1)} >= {0, 1}, i
            assert dt == 'bf16' or {c.geom[8] for c in mine if (c.geom[5], c.geom[7]) == (5, 1)} >= {0, 1, 2, 3, 4}, i
            assert dt == 'bf16' or {c.geom[8] for c in mine if (c.geom[5], c.geom[7]) == (4, 1)} >= {0, 1, 2, 3}, i
        else:
            assert all(any(cl in c.claims for c in mine) for cl in ('all_mirror', 'plane_under_filter')), i
        if mode == 'dgrad':
            assert any(c.bias for c in mine) and any(not c.bias for c in mine), i
        else:
            assert {c.act for c in mine if c.bias} == {0, 1, 2, 3, 4}, i
        assert {c.kind for c in B if T.inst(c) == i} == {'xlow', 'wlow'}, i
    for half in (False, True):      # the activations through the split-K reduce, both stores
        assert {c.act for c in A if c.half == half and c.bias and c.want[4] > 1 and c.pass_ == 'fwd'} == {0, 1, 2, 3, 4}
    for claim in ('stages_1', 'stages_2', 'stages_3', 'odd_stages', 'empty_slice', 'short_slice', 'slice_starts_in_chunk', 'phases_16'):
        assert {c.kind for c in B if claim in c.claims} >= {'xlow', 'wlow'}, claim
    for c in T.NEED_ZERO_REFUSED:
        assert c.bias and T.hgemm_plan(c).need_zero


@pytest.mark.parametrize('name', EXACT + ['C.' + c.name for c in T.MAXPOS.values()])
def test_emulation_is_exact(name):
    c = T.BY_NAME[name] if name in T.BY_NAME else {('C.' + v.name): v for v in T.MAXPOS.values()}[name]
    assert T.quanta(c) < 2.0 ** 24
    y = T.emulate(c)
    want = T.exact_expected(c)
    assert bool((y == want).all()), '%d element(s) differ' % int((y != want).sum())


@pytest.mark.parametrize('name', SIGNED)
def test_emulation_stays_inside_the_bound(name):
    c = T.BY_NAME[name]
    y = T.emulate(c)
    E, bound, want = T.bounds(c)
    err = (y - want).abs()
    assert bool((err <= bound).all()), '%d element(s) outside, worst %.3g x the bound' % (int((err > bound).sum()), float((err / bound.clamp_min(1e-300)).max()))
    pl = T.hgemm_plan(c)
    if pl.need_zero:
        un = T.data(c).A == 0
        assert bool((y[un] == 0).all()) and not bool(torch.signbit(y[un]).any())


# the study runs on the cases that reach an edge (every case that makes a claim of the pipeline or the split) and on one plain case per
# instantiation and section
_EDGE = ('stages_1', 'stages_2', 'stages_3', 'odd_stages', 'slice_starts_in_chunk', 'split', 'empty_slice', 'short_slice', 'phases_16', 'need_zero')


def _study_cases():
    seen, out = set(), []
    for c in T.CASES:
        key = (c.sect, T.inst(c), c.kind, tuple(cl for cl in c.claims if cl in _EDGE))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_each_perturbation_fails_some_gate():
    """drop one piece product, swap two taps for one pixel, zero four channels of one pixel in one stage, read the last live stage through
    row T, take iswS from the next row, repeat a stage in the dead slot, move a slice boundary either way, add the bias in every slice:
    each fails the gate of at least one case; which sections fail it is printed (and recorded in tests/test_gpu_hgemm_cases.py)"""
    cases = _study_cases()
    for perturb in T.PERTURBATIONS:
        fails, applies = collections.Counter(), collections.Counter()
        for c in cases:
            lin = c._replace(act=0)      # (a ReLU may hide the one element)
            y = T.emulate(lin, perturb, exact=False)
            if y is None:
                continue
            applies[(c.sect, c.kind)] += 1
            if not T.gate(lin, y):
                fails[(c.sect, c.kind)] += 1
        print('HGEMM-PERTURB %-18s fails %s' % (perturb, ', '.join('%s %s %d of %d' % (k + (fails[k], applies[k])) for k in sorted(applies))))
        assert sum(fails.values()) > 0, 'no case catches %s: a case is missing' % perturb
        if perturb not in ('drop_lh', 'drop_hl', 'isw_next_row'):      # a lost or misplaced TERM fails section A too
            assert any(k[0] == 'A' for k in fails), perturb


def test_maxima_slots():
    assert T.maxima_slots(1) == [0] and T.maxima_slots(5) == [0, 4] and T.maxima_slots(1023) == [0, 1022]
    assert T.maxima_slots(1024) == [0, 1023] and T.maxima_slots(1025) == [0, 1023, 1024]
    mid = [4 * T.NT + 1, 4 * (2 * T.NT + 77) + 2]      # float4 NT (thread 0's second load) and 2 NT + 77 (thread 77's third load)
    assert T.maxima_slots(4096) == [0] + mid + [4095] and T.maxima_slots(4104) == [0] + mid + [4095, 4103]
    assert T.maxima_slots(4107) == [0] + mid + [4095, 4103, 4106]
    assert mid[0] // 4 == T.NT and mid[1] // 4 == 2 * T.NT + 77 and 0 + 3 * T.NT < 4096 // 4 and 77 + 3 * T.NT < 4096 // 4
    # 4096 slots = 1024 float4: every thread of 256 runs the 4-in-flight loop once (i + 3 * 256 < 1024) and float4 1023 is its last load;
    # 4104: float4 1024 and 1025 fall to the remainder loop; 4107: three elements to the scalar tail
    assert 1024 // 4 == T.NT and (4104 // 4) - 4 * T.NT == 2 and 4107 - 4 * (4107 // 4) == 3


def test_pack_restatement_splits_exactly():
    """the restated pre-split of section D: high + low pieces give the scaled weights back exactly on the integer kinds"""
    for c in T.PACK:
        d = T.data(c)
        raw, rowmax = T.packed_presplit(c, d.w)
        f32 = T.packed_fp32(c, d.w)
        assert raw.numel() == 4 * f32.numel() and rowmax.numel() == T.shapes(c)[2]
        pieces = raw.view(torch.float16).view(-1, 2, 4).float()
        pl = T.hgemm_plan(c)
        M = T.shapes(c)[2]
        sw = torch.tensor([T.pow2_scale(float(v)) for v in rowmax])
        off = 0
        for p in pl.phases:
            n = M * p.Kp
            got = (pieces[off // 4:(off + n) // 4, 0] + pieces[off // 4:(off + n) // 4, 1]).reshape(M, p.Kp)
            assert bool((got == f32[off:off + n].view(M, p.Kp) * sw.view(M, 1)).all())
            off += n


# ---- the predicate -----------------------------------------------------------------------------------------------------------------------
def _desc(lib, geom, dt=None):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    d = lib.ConvDesc(N, C, H, W, K, Rr, S, st, pad, pm, (H + 2 * pad - Rr) // st + 1, (W + 2 * pad - S) // st + 1)
    d.dtype = lib.F32 if dt is None else dt
    return d


def test_predicate_agrees_with_the_library():
    from pcgan_amd.hip import lib
    h = lib.load()
    geoms = {c.geom for c in T.CASES}
    base = (2, 16, 9, 10, 40, 3, 3, 1, 1, 0)
    for i, vals in ((1, (8, 15, 16, 17, 32, 33, 48)), (4, (16, 32, 33, 40, 47, 48)), (5, (1, 3, 5, 6)), (6, (1, 5, 6)), (9, (0, 1)), (7, (1, 2, 4))):
        for v in vals:
            g = list(base)
            g[i] = v
            if i == 5:
                g[8] = 0
            geoms.add(tuple(g))
    for g in sorted(geoms):
        for pass_, code in (('fwd', lib.PASS_FWD), ('dgrad', lib.PASS_BWD_DATA)):
            for half in (False, True):
                d = _desc(lib, g, lib.BF16 if half else lib.F32)
                got = h.pcgan_conv2d_hgemm_supported(ctypes.byref(d), code)
                assert bool(got) == T.supported(g, pass_, half), (g, pass_, half, got)
    d = _desc(lib, base)
    assert h.pcgan_conv2d_hgemm_supported(None, lib.PASS_FWD) == 0 and h.pcgan_conv2d_hgemm_supported(ctypes.byref(d), lib.PASS_BWD_WEIGHT) == 0
