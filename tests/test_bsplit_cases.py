"""The case table of tests/test_gpu_bsplit_cases.py (tests/bsplit_cases.py), checked without a GPU: every case is the edge its claims name
(predicates over the restated host), reproduces the launch record it wants, and satisfies the condition that makes its gate bite (section
A: the largest bound under half the smallest term, bf16 mirror sums and folded weights exact; section B: every partial sum under 2^24,
every value -- the column-mirror sums and the folded weights included -- a number of the piece form).  The kernel's arithmetic restated
in torch (bsplit_cases.emulate) equals the float64 reference on section B data and stays inside the bound on section A data.  The restated
predicates and sizes are held equal to the library's over a sweep of descriptors (host code: the library loads without a GPU).

Sensitivity study (test_sensitivity): each fault of bsplit_cases.PERTURBATIONS is applied to `emulate` only -- a kernel made wrong on
purpose is never run on a GPU -- and every gate evaluated on its result.  Cases failed of the cases in which the fault has a place,
sections A | B | C (C: the 3e-6 clause alone, the fp32 route runs on the GPU only):
  drop_mm             A  0 of 24 | B   2 of  74 | C 12 of 12   a middle piece is 2^-9 of a value, (m,m) 2^-18 of a term: inside the worst-case
                                                             bound of A; B: the two 'mid' cases, where both operands have a middle piece
  drop_lh             A  0 of 24 | B  12 of  74 | C 12 of 12   B: the 'wlow' cases whose packed operand has a third piece (every 61st: 19 bits)
  swap_row_classes    A 11 of 11 | B  72 of  72 | C  4 of  4   every data-gradient case
  mirror_from_tap_0   A 11 of 11 | B  54 of  72 | C  4 of  4   B: not the 'fold' classes that leave column 0 empty
  shift_tap           A 22 of 25 | B  82 of 104 | C  8 of  8   A: a neighbour of the same sign and nearly the same magnitude stays inside the
                                                             bound; B: an unchanged result where the shifted weight meets zeros only
  dead_stage_repeats  A 31 of 31 | B 113 of 113 | C  0 of  0   every odd stage count: 1, 3, 5, 9, 25, and the 9-stage splits (C: even counts)
  drop_last_stage     A 10 of 10 | B  20 of  20 | C  4 of  4   every weight-gradient case
  zero_half_pixel     A 43 of 43 | B 107 of 141 | C 12 of 12   B: not where the 'fold' data is zero in that pixel anyway
Every perturbation fails at least one gate; the two dropped products are what section B's pieces and section C are for.
The faults that are whole terms fail EVERY section A case in which they have a place (asserted)."""
import ctypes

import pytest
import torch

import bsplit_cases as T

NAMES = list(T.BY_NAME)
EXACT = [n for n in NAMES if T.BY_NAME[n].sect == 'B']
SIGNED = [n for n in NAMES if T.BY_NAME[n].sect == 'A']


@pytest.mark.parametrize('name', NAMES)
def test_case(name):
    c = T.BY_NAME[name]
    pl = T.plan(c)
    d = T.data(c)
    assert T.supported(c.pass_, c.geom) and T.record(pl) == c.want, (T.record(pl), c.want)
    assert c.want[0] == T.PER_TAP, 'every case of this table runs the per-tap kernel'
    assert T.inst(c) in T.INSTANTIATIONS and c.claims == T.claims_of(c) and c.claims, 'a case without a claim'
    assert max(d.src.numel(), d.w.numel(), d.ref.numel()) * 4 <= 4 << 20 and pl.ws_bytes <= 8 << 20
    assert d.ref.shape == d.A.shape and bool((d.A >= T.expected(c).abs() - 1e-9 * d.A).all())
    if c.pass_ != 'fwd':
        assert not c.bias and c.act == 0
    if c.pk == 'bf16':
        assert bool((T._bf16(d.src) == d.src).all()) and bool((T._bf16(d.w) == d.w).all()), 'operands of bf16 tensors are bf16 numbers'
        if c.pass_ == 'dgrad':
            assert T.bf16_sums_exact(c), 'a mirror sum or a folded weight that is no bf16 number: its rounding is not in the gate'
    if c.sect == 'A':
        for t, s in ((d.src, 1.0), (d.w, 2.0 ** c.wexp)) + (((d.b, 1.0),) if c.bias else ()) + (((d.base, 1.0),) if c.acc else ()):
            assert 0.75 * s <= float(t.abs().min()) and float(t.abs().max()) <= 1.25 * s
        worst, allowed = T.condition(c)
        assert worst < allowed, 'the largest bound %.4f would not catch one lost term (%.4f allowed)' % (worst, allowed)
        assert c.act in (0, 1, 2) or (c.wexp == -5 and float(d.ref.abs().max()) < 8)
        assert float(d.A.min()) >= T.TERM_MIN * 2.0 ** c.wexp, 'every element sums at least one term'
        if c.pk == 'bf16x3':
            assert T.kp(c) <= 448
        elif c.pass_ != 'wgrad':
            assert T.kp(c) <= 144 and float(T.expected(c).abs().max()) < 72
        if c.pk == 'bf16' and c.pass_ == 'dgrad':      # the grid 2^-5
            assert bool((d.src * 32 == (d.src * 32).round()).all()) and bool((d.w * 32 == (d.w * 32).round()).all())
    else:
        assert T.quanta(c) < 2.0 ** 24, 'partial sums of up to %.3g: fp32 accumulation would not be exact' % T.quanta(c)
        assert c.act in (0, 1, 2) and T.slope_of(c) == 0.25
        for t in (d.src, d.w, d.b, d.base):
            assert t is None or bool((t == t.round()).all())
        low, other = (d.src, d.w) if c.kind == 'xlow' else (d.w, d.src)
        if c.kind == 'xlow':
            assert float(low.abs().max()) == 2 ** c.bits - 1 and set(other.unique().tolist()) == {-1.0, 0.0, 1.0}
            assert (c.bits, c.wide) == T.xlow_bits(c.name[2:c.name.index('_' + c.pk)], c.pass_, c.pk)
        elif c.kind == 'mid':
            assert c.pk == 'bf16x3' and all(bool((t3[1] != 0).any()) for t3 in (T.split3(d.src), T.split3(d.w))) and T.kp(c) * 2 ** 18 < 2 ** 24
        elif c.kind == 'wlow':
            assert float(low.abs().max()) <= 2 ** max(c.bits, c.wide) - 1 and set(other.unique().tolist()) == {-1.0, 0.0, 1.0}
        else:
            assert float(d.src.abs().max()) <= 59 and float(d.w.abs().max()) <= 3
        # every value the kernel splits is a number of the piece form: the operands, the mirror sums, the folded weights
        vals = [d.src, d.w]
        if c.pass_ == 'dgrad':
            W = c.geom[3]
            vals += [d.src[..., 0] + d.src[..., 2], d.src[..., W - 3] + d.src[..., W - 1], d.w[:, :, 0] + d.w[:, :, 2]]
        for t in vals:
            t = t.float()
            assert bool((sum(T.split3(t)) == t).all()) if c.pk == 'bf16x3' else bool((T._bf16(t) == t).all())


def test_names_instantiations_and_claims():
    assert len(set(NAMES)) == len(T.CASES) and len(T.INSTANTIATIONS) == 16
    for sect in 'AB':
        assert {T.inst(c) for c in T.CASES if c.sect == sect} == set(T.INSTANTIATIONS), sect
    for claim in T.CLAIMS:
        for pk in T.PKS:
            for sect in 'AB':
                if sect == 'A' and pk == 'bf16' and claim in T.A_FP32_ONLY:
                    assert not any(claim in c.claims for c in T.CASES if c.sect == 'A' and c.pk == pk)
                    continue
                assert any(claim in c.claims for c in T.CASES if c.sect == sect and c.pk == pk), (claim, pk, sect)
    for pk in T.PKS:      # the exact kinds of every pass, the eight source classes on the three fold shapes
        B = [c for c in T.CASES if c.sect == 'B' and c.pk == pk]
        for i in T.INSTANTIATIONS:
            assert {c.kind for c in B if T.inst(c) == i} >= {'xlow', 'wlow'} or i[2] != pk, i
        assert {(c.fold, c.geom) for c in B if c.kind == 'fold'} == {(f, dict((n, g) for n, p, g, *_ in T.SHAPES)[s]) for f in T.FOLDS for s in T.FOLD_SHAPES}
    assert any(c.wide and c.kind == 'wlow' for c in T.CASES if c.pass_ == 'wgrad') and any(c.wide and c.kind == 'wlow' for c in T.CASES if c.pass_ == 'fwd')
    assert any(c.wide and c.kind == 'wlow' for c in T.CASES if c.pass_ == 'dgrad')
    fa = [c for c in T.CASES if c.sect == 'A' and c.pass_ == 'fwd' and c.bias]
    assert {c.act for c in fa} == {0, 1, 2, 3, 4}
    for c in T.RANGE.values():
        assert T.record(T.plan(c)) == c.want and c.pk == 'bf16x3'


def test_bf16_caps_of_the_condition():
    """why the 5x5 case and the option cases have no bf16 case in section A: at 288 and 400 terms |ref| passes 72 somewhere, so 2^-8 |ref|
    alone is over half a term"""
    for name in ('f_5x5_reflect', 'f_option', 'd_option'):
        c = [c for c in T.CASES if c.name.startswith('A_%s_bf16x3' % name)][0]
        probe = c._replace(pk='bf16', want=c.want[:3] + (1,) + c.want[4:], name='probe_' + name, claims=None)
        worst, allowed = T.condition(probe)
        assert worst > allowed, (name, worst, allowed)


@pytest.mark.parametrize('name', EXACT)
def test_emulation_is_exact(name):
    c = T.BY_NAME[name]
    y = T.emulate(c)
    want = T.exact_expected(c)
    assert tuple(y.shape) == T.out_shape(c) and bool((y == want).all()), '%d element(s) differ' % int((y != want).sum())


@pytest.mark.parametrize('name', SIGNED)
def test_emulation_is_inside_the_bound(name):
    c = T.BY_NAME[name]
    ok, ratio = T.gate(c, T.emulate(c))
    assert ok and ratio <= 1.0, ratio


@pytest.mark.parametrize('key', list(T.RANGE), ids=lambda k: '%s-%s' % k)
def test_emulation_on_range_data(key):
    c = T.RANGE[key]
    d = T.data(c)
    assert bool(torch.isfinite(d.src).all()) and float(d.ref.abs().max()) > 1e-37
    if c.kind == 'tiny':      # the smallest kept product, 2^-18 of a typical term and 2^-9 x 2^-9 of it for (m, m), stays a normal fp32 number
        typical = float(d.src.abs().median() * d.w.abs().median())
        assert typical * 2.0 ** -18 > 2.0 ** -126 * 1e3
    if c.kind == 'tiny2':
        typical = float(d.src.abs().median() * d.w.abs().median())
        assert typical * 2.0 ** -18 < 2.0 ** -126 < typical
        return
    ok, e = T.gate(c, T.emulate(c))
    assert ok, e


def test_sensitivity():
    """every perturbation of the emulation fails at least one gate; the counts are the ones of the module docstring"""
    lines = []
    for p in T.PERTURBATIONS:
        tally = {s: [0, 0] for s in 'ABC'}
        for c in list(T.CASES) + [c for c in T.RANGE.values() if c.kind != 'tiny2']:
            y = T.emulate(c, p)
            if y is None:
                continue
            # (a ReLU may hide the one element: the perturbed runs compare the linear result)
            ok, _ = T.gate(c, y)
            tally[c.sect][1] += 1
            tally[c.sect][0] += 0 if ok else 1
        lines.append('BSPLIT-SENS %-20s A %3d of %3d | B %3d of %3d | C %2d of %2d' % ((p,) + tuple(v for s in 'ABC' for v in tally[s])))
        print(lines[-1])
        assert sum(tally[s][0] for s in 'ABC') > 0, '%s fails no gate' % p
        assert all(tally[s][1] > 0 for s in 'AB'), p
        if p in ('swap_row_classes', 'mirror_from_tap_0', 'dead_stage_repeats', 'drop_last_stage', 'zero_half_pixel'):
            assert tally['A'][0] == tally['A'][1], 'a fault of whole terms fails EVERY section A case in which it has a place: %s' % lines[-1]


# ---- the restated host against the library ---------------------------------------------------------------------------------------------------
def _desc(lib, geom, pk='bf16x3'):
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    d = lib.ConvDesc(N, C, H, W, K, Rr, S, st, pad, pm, (H + 2 * pad - Rr) // st + 1, (W + 2 * pad - S) // st + 1)
    d.dtype = lib.BF16 if pk == 'bf16' else lib.F32
    return d


def test_predicates_and_sizes_over_a_sweep_of_descriptors():
    from pcgan_amd.hip import lib
    h = lib.load()
    n = 0
    for pk in T.PKS:
        for N in (1, 3):
            for C in (8, 16, 32, 40, 256):
                for K in (16, 24, 31, 32, 40, 64, 128, 256, 384, 512):
                    for H, W in ((3, 5), (4, 4), (4, 16), (5, 7), (4, 32), (6, 64), (9, 48)):
                        for k, pad, pm, st in ((3, 1, 1, 1), (3, 1, 0, 1), (3, 0, 0, 1), (1, 0, 0, 1), (5, 2, 1, 1), (5, 4, 1, 1), (7, 3, 0, 1), (3, 1, 1, 2)):
                            if H + 2 * pad < k or W + 2 * pad < k:
                                continue
                            geom = (N, C, H, W, K, k, k, st, pad, pm)
                            ref = ctypes.byref(_desc(lib, geom, pk))
                            got = (h.pcgan_conv2d_bsplit_supported(ref), h.pcgan_conv2d_bsplit_dgrad_supported(ref), h.pcgan_conv2d_bsplit_wgrad_supported(ref))
                            want = tuple(int(T.supported(p, geom)) for p in ('fwd', 'dgrad', 'wgrad'))
                            assert got == want, (geom, got, want)
                            sizes = (h.pcgan_conv2d_bsplit_packed_bytes(ref), h.pcgan_conv2d_bsplit_dgrad_packed_bytes(ref),
                                     h.pcgan_conv2d_bsplit_wgrad_workspace_bytes(ref))
                            plans = [T.plan_of(p, geom, pk) if s else None for p, s in zip(('fwd', 'dgrad', 'wgrad'), want)]
                            assert sizes == tuple((pl.ws_bytes if p == 2 else pl.packed_bytes) if pl else 0 for p, pl in enumerate(plans)), (geom, sizes)
                            n += 1
    assert n > 3000
    assert h.pcgan_conv2d_bsplit_supported(None) == 0 and h.pcgan_conv2d_bsplit_dgrad_supported(None) == 0 and h.pcgan_conv2d_bsplit_wgrad_supported(None) == 0
    big = (64, 256, 182, 182, 256, 3, 3, 1, 1, 1)      # beyond 2 GiB
    assert T.refusal(big) == 4 and h.pcgan_conv2d_bsplit_supported(ctypes.byref(_desc(lib, big))) == 0


def test_weight_gradient_predicate_answers_what_the_call_accepts():
    """K = 64, 384 and 512 used to be answered 1 (and a workspace size named) while pcgan_conv2d_bwd_weight_bsplit refuses them: the
    predicate, and hence the workspace size, is the call's own rule now -- one full row tile, K = 128 or 256"""
    from pcgan_amd.hip import lib
    h = lib.load()
    for K in (32, 64, 127, 128, 129, 192, 255, 256, 257, 384, 512):
        ref = ctypes.byref(_desc(lib, (2, 16, 4, 16, K, 3, 3, 1, 1, 1)))
        yes = h.pcgan_conv2d_bsplit_wgrad_supported(ref)
        assert yes == int(K in (128, 256)) and (h.pcgan_conv2d_bsplit_wgrad_workspace_bytes(ref) > 0) == bool(yes), K


@pytest.mark.parametrize('name', NAMES + ['C:%s-%s' % k for k in T.RANGE])
def test_library_accepts_every_case_and_sizes_match(name):
    from pcgan_amd.hip import lib
    h = lib.load()
    c = T.RANGE[tuple(name[2:].split('-'))] if name.startswith('C:') else T.BY_NAME[name]
    ref = ctypes.byref(_desc(lib, c.geom, c.pk))
    pl = T.plan(c)
    if c.pass_ == 'fwd':
        assert h.pcgan_conv2d_bsplit_supported(ref) == 1 and h.pcgan_conv2d_bsplit_packed_bytes(ref) == pl.packed_bytes
    elif c.pass_ == 'dgrad':
        assert h.pcgan_conv2d_bsplit_dgrad_supported(ref) == 1 and h.pcgan_conv2d_bsplit_dgrad_packed_bytes(ref) == pl.packed_bytes
    else:
        assert h.pcgan_conv2d_bsplit_wgrad_supported(ref) == 1 and h.pcgan_conv2d_bsplit_wgrad_workspace_bytes(ref) == pl.ws_bytes
    assert lib.get_option('bsplit_halo') == 1
