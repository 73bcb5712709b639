"""CPU: the case table of the per-tap weight gradient (tests/hsplit_wgrad_cases.py) is well-formed and complete, the host restated
reproduces every wanted launch record, the conditions of both sections hold, the emulation of the kernel's arithmetic passes both gates
and every fault applied to it is caught -- no GPU, and no fault is ever made on one.

The restated host is checked against the library where that needs no GPU: pcgan_conv2d_hsplit_wgrad_supported and
pcgan_conv2d_hsplit_wgrad_workspace_bytes under the options of every case (host arithmetic only).

Sensitivity study (test_every_perturbation_is_caught): hsplit_wgrad_cases.PERTURBATION_FAILS names, per perturbation, shapes whose
section-A and section-B cases both fail under it; beyond those, every perturbation except the two dropped piece products fails the gate
of EVERY case in which it has a place -- among them a skipped maximum slot of either operand in every fp32 case that hands its maxima
over in 257, 300 or 6151 slots (the decoy slots sit at most 2^-6 under the maximum: the mis-scaled operand overflows fp16).  Measured with the emulation (max |err| / bound, section A, fp32 tensors): 0.018 unperturbed;
section B and the bf16 cases of section A reproduce the float64 reference exactly."""
import ctypes
import functools

import pytest
import torch

import hsplit_wgrad_cases as H


def _want(case):
    return dict(zip(H.RECORD, case.want))


@functools.lru_cache(maxsize=None)
def _emulated(name, perturb=None):
    c = H.BY_NAME[name]
    out = H.emulate(c, perturb)
    if out is None:
        return None
    w = _want(c)
    return H.gate(c, out, H.data(c), w['splits'], w['stages_per_split'])


def test_table_is_well_formed():
    assert len(H.INSTANTIATIONS) == 22 and len(set(H.INSTANTIATIONS)) == 22 and set(H.UNREACHABLE) <= set(H.INSTANTIATIONS)
    assert len(H.BY_NAME) == len(H.CASES) and len({s[0] for s in H.SHAPES}) == len(H.SHAPES)
    for c in H.CASES:
        assert c.sect in 'AB' and len(c.want) == len(H.RECORD) and len(c.geom) == 10
        assert c.kind == ('signed' if c.sect == 'A' else ('int8' if c.half else c.kind)) and c.kind in ('signed', 'xlow', 'dylow', 'int8')
        assert (c.maxima is None) == c.half and (c.half or c.maxima in H.MAXIMA)
        assert set(dict(c.opts)) <= set(H.OPTIONS)
        assert c.claims, '%s claims nothing' % c.name
        N, C, Hh, W, K, Rr, S, st, pad, pm = c.geom
        pl = H.plan(c.geom, c.half, c.opts)
        assert N * pl.P * pl.Q <= 1200 and K * C * Rr * S * 4 <= 4 << 20, '%s is larger than a case needs to be' % c.name
    for skip in list(H.A_SKIP) + list(H.B_SKIP):
        assert skip[0] in {s[0] for s in H.SHAPES} and skip[1] in dict((s[0], s[3]) for s in H.SHAPES)[skip[0]]


@pytest.mark.parametrize('case', H.CASES, ids=lambda c: c.name)
def test_case_is_supported_and_planned(case):
    assert H.supported(case.geom, case.half, case.opts)
    pl = H.plan(case.geom, case.half, case.opts)
    assert H.record(pl) == case.want, 'the host restated gives %r' % (dict(zip(H.RECORD, H.record(pl))),)
    assert H.inst(case) in H.INSTANTIATIONS and H.inst(case) not in H.UNREACHABLE
    assert sum(pl.here) == pl.stages and len(pl.here) == pl.splits and min(pl.here) >= 1


def test_unreachable_instantiations():
    """(256, 2, fp32, 2, 0): 256 columns on fp32 tensors need reflection padding, which needs stride 1 -- for every option setting and a
    sweep of geometries the restated host never plans it, and plans no instantiation launch_tile does not have"""
    seen = set()
    for gen in (0, 1):
        for cw in (0, 128, 256):
            for padcopy in (0, 1):
                opts = {'wgrad_gen': gen, 'wgrad_cw': cw, 'wgrad_padcopy': padcopy, 'wgrad_rowring': 0}
                for half in (False, True):
                    for K in (32, 129):
                        for C in (8, 256):
                            for k, st, pad in ((3, 1, 1), (3, 2, 1), (4, 2, 1), (5, 1, 2), (5, 2, 2), (1, 1, 0)):
                                for pm in (0, 1):
                                    W = {1: 16 + k - 1 - 2 * pad, 2: 2 * 15 + k - 2 * pad}[st]
                                    geom = (1, C, W, W, K, k, k, st, pad, pm)
                                    if H.supported(geom, half, opts):
                                        pl = H.plan(geom, half, opts)
                                        seen.add((pl.bm, pl.stride, pl.dtype, pl.cw // 128, int(pl.form == H.FORM_GEN)))
    assert seen <= set(H.INSTANTIATIONS) and not seen & set(H.UNREACHABLE)
    assert seen == set(H.INSTANTIATIONS) - set(H.UNREACHABLE)


@pytest.mark.parametrize('sect', ['A', 'B'])
def test_every_instantiation_and_edge_is_claimed(sect):
    cases = [c for c in H.CASES if c.sect == sect]
    assert {H.inst(c) for c in cases} == set(H.INSTANTIATIONS) - set(H.UNREACHABLE)
    claimed = set().union(*[c.claims for c in cases])
    assert H.REQUIRED[sect] <= claimed, 'section %s: nobody claims %r' % (sect, sorted(H.REQUIRED[sect] - claimed))
    assert H.REQUIRED['A'] | H.REQUIRED['B'] == set(H.CLAIMS)
    # each reachable instantiation at 3x3 and, where it is a stride-2 one, again at 4x4
    for i in set(H.INSTANTIATIONS) - set(H.UNREACHABLE):
        taps = {c.geom[5] for c in cases if H.inst(c) == i}
        assert 3 in taps and (i[1] == 1 or 4 in taps), (sect, i, taps)


@pytest.mark.parametrize('case', H.CASES, ids=lambda c: c.name)
def test_conditions_hold(case):
    w = _want(case)
    H.condition(case, H.data(case), w['splits'], w['stages_per_split'])


def test_library_agrees_with_the_host_restated():
    """pcgan_conv2d_hsplit_wgrad_supported and _workspace_bytes (host arithmetic, no GPU) under the options of every case"""
    from pcgan_amd.hip import lib as L
    h = L.load()
    saved = {k: L.get_option(k) for k in H.OPTIONS}
    try:
        for c in H.CASES:
            o = H.options(dict(c.opts))
            for k, v in o.items():
                L.set_option(k, v)
            N, C, Hh, W, K, Rr, S, st, pad, pm = c.geom
            pl = H.plan(c.geom, c.half, c.opts)
            d = L.ConvDesc(N, C, Hh, W, K, Rr, S, st, pad, pm, pl.P, pl.Q)
            d.dtype = L.BF16 if c.half else L.F32
            assert h.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(d)) == 1, c.name
            assert int(h.pcgan_conv2d_hsplit_wgrad_workspace_bytes(ctypes.byref(d))) == pl.ws_bytes, c.name
            assert h.pcgan_conv2d_hsplit_wgrad_inline(ctypes.byref(d)) == int(pl.copy == H.COPY_NONE), c.name
        # what the restated host refuses, the library refuses (ragged rows / K > 256 outside GEN, a stage under three quarters full)
        for geom, opts in (((1, 4, 5, 15, 32, 3, 3, 1, 1, 1), {}), ((1, 4, 4, 16, 257, 3, 3, 1, 1, 0), {'wgrad_gen': 0}), ((1, 4, 4, 11, 32, 3, 3, 1, 1, 0), {}),
                           ((1, 4, 8, 32, 32, 3, 3, 2, 1, 1), {}), ((1, 4, 4, 16, 31, 3, 3, 1, 1, 0), {})):
            for k, v in H.options(opts).items():
                L.set_option(k, v)
            N, C, Hh, W, K, Rr, S, st, pad, pm = geom
            d = L.ConvDesc(N, C, Hh, W, K, Rr, S, st, pad, pm, H.out_size(Hh, Rr, st, pad), H.out_size(W, S, st, pad))
            assert not H.supported(geom, False, opts) and h.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(d)) == 0, geom
    finally:
        for k, v in saved.items():
            L.set_option(k, v)


@pytest.mark.parametrize('case', [c for c in H.CASES if H.emulable(c)], ids=lambda c: c.name)
def test_emulation_passes_the_gate(case):
    ok, ratio = _emulated(case.name)
    assert ok, '%s: the emulation misses its own gate (%g)' % (case.name, ratio)


def test_every_case_is_emulated():
    assert all(H.emulable(c) for c in H.CASES)


@pytest.mark.parametrize('perturb', H.PERTURBATIONS)
def test_every_perturbation_is_caught(perturb):
    assert set(H.PERTURBATION_FAILS) == set(H.PERTURBATIONS)
    for shape in H.PERTURBATION_FAILS[perturb]:
        hit = {'A': 0, 'B': 0}
        for c in H.CASES:
            if c.name[2:].rsplit('_', 1)[0] != shape:
                continue
            res = _emulated(c.name, perturb)
            if res is None:
                continue
            assert not res[0], '%s survives %s (%g)' % (c.name, perturb, res[1])
            hit[c.sect] += 1
        assert hit['A'] and hit['B'], '%s under %s: %r' % (shape, perturb, hit)
    if perturb in ('drop_lh', 'drop_hl'):
        # section B decides: every 'dylow' case fails without (dy_l, x_h), every 'xlow' case without (dy_h, x_l)
        kind = 'dylow' if perturb == 'drop_lh' else 'xlow'
        mine = [c for c in H.CASES if c.kind == kind]
        assert len(mine) >= 20 and all(not _emulated(c.name, perturb)[0] for c in mine)
        return
    placed = [(c, _emulated(c.name, perturb)) for c in H.CASES]
    placed = [(c, r) for c, r in placed if r is not None]
    assert {c.sect for c, r in placed} == {'A', 'B'}
    if perturb.endswith('maximum_slot_missed'):      # every slot count, in both sections, and not by a near miss: the result is not finite
        assert {(c.sect, c.maxima) for c, r in placed} == {(s, m) for s in 'AB' for m in H.MAXIMA_SLOT}
        assert all(r[1] == float('inf') for c, r in placed)
    assert all(not r[0] for c, r in placed), 'survive %s: %r' % (perturb, [c.name for c, r in placed if r[0]])
