"""GPU: the per-tap weight gradient (csrc/hsplit_wgrad.hip hsplit_wgrad_kernel, the padded copies and the split reduce of
csrc/bsplit_pack.hip) held to float64 element by element, instantiation by instantiation: the table of tests/hsplit_wgrad_cases.py.

Every case calls pcgan_conv2d_bwd_weight_hsplit directly under its library options (fixture `library_options`: restored afterwards, cached
launch plans dropped on every change) and reads pcgan_hwgrad_last_launch back: BM, stride, storage type, columns per workgroup, form,
copy kernel, row and column tiles, splits, stages per split and stages must be what the case is there to hit, and the sequence number
advances by exactly one per call -- a case that lands on another instantiation, form, split count or copy kernel fails.
Per case (_launch): before each of its two calls the workspace and a 4 KiB tail behind the queried size are filled with 0xFF bytes (NaN
partial sums and a NaN padded copy; the tail must not change in either), accumulate = 0 into a NaN-filled dw, then accumulate = 1 into a
random base scaled to max|ref|, which must be BIT-equal to base + dw.  fp32 cases hand the operand maxima over as the case says (hsplit_wgrad_cases.MAXIMA).

A. signed data, gate per element: fp32 (2 (3 n + splits + 8) 2^-24 + 2^-20) A, bf16 2 (n + splits + 8) 2^-24 A, n = 16 x stages per
   split from the record; the condition (bound under half the smallest term) asserted again before the launch.
B. exact data ('xlow' / 'dylow' / 'int8'): dw == ref in every element.
C. operand ranges (relu_normal, wide_range, tiny, huge of tests/test_gpu_wgrad_rowring.py) on one GEN and one reflection-in-gather shape,
   against the fp32 route of the product on the same inputs: e < 3e-6 and e <= 2 e32 + 5e-7; per element max|dw - ref| <=
   2 max|dw32 - ref| + 5e-7 max|ref| and <= 1e-4 max|ref| (the project's split-route tolerances).
D. host routing: ops.conv2d_bwd_weight and accumulate_into=... reach the same record and give the bits of the direct call; a call the
   host unit hands to the row-ring form leaves the record where it was.

Measured on an MI355X (256 CUs), max(|err| / bound) and relative L2 error per group of cases (recorded, not gated):
  fp32 tensors, section A            cases   max |err| / bound    relative L2
    GEN rows / columns / widths         21   0.0009 .. 0.0062     9.5e-8 .. 1.7e-7
    pipeline, 1 .. 9 stages              8   0.0015 .. 0.0109     7.2e-8 .. 1.5e-7   (the largest ratio at one stage, stride 2, K = 129)
    forced / heuristic splits            5   0.0003 .. 0.0018     1.1e-7 .. 1.5e-7
    reduce, 3 / 7 / 64 splits            3   0.0003 .. 0.0012     1.5e-7 .. 2.2e-7
    reflection in the gather             3   0.0017 .. 0.0078     9.2e-8 .. 1.5e-7
    padded copy (both kernels)          16   0.0010 .. 0.0078     9.2e-8 .. 1.5e-7
  bf16 tensors, section A (63 cases): every element equal to the float64 reference -- the products are exact in fp32 and so are
  these short sums of them.  Section B (57 fp32, 57 bf16 cases): every element equal, as gated.
  Section C (16 cases; one slot per plane and ops.amax_of give the same bits): relative L2 (e, e32) from (1.20e-7, 1.46e-7) to
  (1.62e-7, 2.30e-7), closest to the 2 x clause (1.311e-7, 1.271e-7) at the GEN shape, wide_range; per element, of max|ref|,
  (1.59e-7, 1.76e-7) .. (3.82e-7, 4.59e-7): in all 16 cases at or under the fp32 route's own error.
  The errors sit far inside the bound because it is a worst case over all orders and sign patterns; what the gate buys is the condition:
  any lost, doubled or misplaced term is >= 2 x the bound.
  Wall time of the module: 2.5 s for its 253 tests (the slowest 1.1 s: the first, which loads the library; every other under 0.1 s)."""
import ctypes

import pytest
import torch

import gpu_direct as D
import hsplit_wgrad_cases as H

pytestmark = pytest.mark.gpu

@pytest.fixture
def library_options():
    """sets library options (cached launch plans hold workspace sizes that depend on them: dropped on every change) and restores what
    was there afterwards"""
    from pcgan_amd.hip import lib as L, ops
    saved = {k: L.get_option(k) for k in H.OPTIONS}

    def apply(opts):
        for k, v in H.options(dict(opts)).items():
            L.set_option(k, v)
        ops.clear_plans()
    try:
        yield apply
    finally:
        for k, v in saved.items():
            L.set_option(k, v)
        ops.clear_plans()


def _desc(geom, half):
    from pcgan_amd.hip import ops
    N, C, Hh, W, K, Rr, S, st, pad, pm = geom
    return ops.make_desc(N, C, Hh, W, K, Rr, S, st, pad, pm, ops.BF16 if half else ops.F32)


def _maxima(t, how, seed):
    """the partial maxima of |t| (device, fp32) in the form `how`"""
    from pcgan_amd.hip import ops
    if how == 'amax_of':
        return ops.amax_of(t)
    if how == 'plane':
        return t.abs().amax(dim=(2, 3)).reshape(-1).contiguous()
    m = t.abs().max().reshape(1)
    if how == 'one':
        return m.contiguous()
    n = int(how[1:])
    g = torch.Generator().manual_seed(seed)
    # every other slot: a decoy in (2^-7, 2^-6] of the maximum -- a skipped slot overflows the fp16 high piece (hsplit_wgrad_cases.MAXIMA)
    out = ((torch.rand(n, generator=g) * 0.5 + 0.5) * H.DECOY).to(t.device) * m
    out[H.MAXIMA_SLOT[how]] = m[0]
    return out.contiguous()


def _launch(dev, geom, half, x, dy, base, maxima, seed=0):
    """pcgan_conv2d_bwd_weight_hsplit twice (accumulate 0 into NaN, accumulate 1 into base); returns (dw, accumulated, record)"""
    from pcgan_amd.hip import lib as L, ops
    lib = L.load()
    N, C, Hh, W, K, Rr, S, st, pad, pm = geom
    d = _desc(geom, half)
    assert lib.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(d))
    nb = int(lib.pcgan_conv2d_hsplit_wgrad_workspace_bytes(ctypes.byref(d)))
    ws = D.guarded(dev, nb)
    vp = D.VP
    xd, dyd = x.to(dev).contiguous(), dy.to(dev).contiguous()
    if half:
        mx = (None, 0, None, 0)
        keep = ()
    else:
        xm, dm = _maxima(xd, maxima, seed), _maxima(dyd, maxima, seed + 1)
        assert xm.dtype == torch.float32 and xm.data_ptr() % 16 == 0
        mx = (vp(xm.data_ptr()), xm.numel(), vp(dm.data_ptr()), dm.numel())
        keep = (xm, dm)
    out = []
    seq0 = ops.hwgrad_last_launch()['seq']
    for acc, dw in ((0, torch.full((K, C, Rr, S), float('nan'), device=dev)), (1, base.to(dev).clone())):
        ws.fill_(0xFF)       # before EACH call: NaN partial sums and a NaN padded copy, so an element left unwritten by either call shows
        L.check(lib.pcgan_conv2d_bwd_weight_hsplit(ctypes.byref(d), vp(xd.data_ptr()), mx[0], mx[1], vp(dyd.data_ptr()), mx[2], mx[3], vp(dw.data_ptr()),
                                                   acc, vp(ws.data_ptr()), nb, vp(torch.cuda.current_stream().cuda_stream)), 'conv2d_bwd_weight_hsplit')
        rec = ops.hwgrad_last_launch()
        assert rec['seq'] == seq0 + 1 + acc, 'one recorded launch per call: %r after %d' % (rec, seq0)
        out.append(dw)
        torch.cuda.synchronize()
        assert bool((ws[nb:] == 0xFF).all()), 'call %d wrote behind the workspace it asked for (%d bytes)' % (acc, nb)
    del keep
    return out[0], out[1], rec, nb


def _run(dev, case, library_options):
    d = H.data(case)
    want = dict(zip(H.RECORD, case.want))
    N, C, Hh, W, K, Rr, S, st, pad, pm = case.geom
    worst = H.condition(case, d, want['splits'], want['stages_per_split'])      # before the launch, from the split the case expects
    library_options(case.opts)
    g = torch.Generator().manual_seed(N + C + K + Hh + W)
    base = torch.randn(K, C, Rr, S, generator=g) * float(d.ref.abs().max())
    dw, acc, rec, nb = _launch(dev, case.geom, case.half, d.x, d.dy, base, case.maxima, seed=K + C)
    got = {k: rec[k] for k in H.RECORD}
    assert got == want, 'the case ran another launch: %r, wanted %r' % (got, want)
    assert nb == H.plan(case.geom, case.half, case.opts).ws_bytes
    out = dw.double().cpu()
    ok, ratio = H.gate(case, out, d, rec['splits'], rec['stages_per_split'])
    rel = float((out - d.ref).norm() / d.ref.norm()) if bool(torch.isfinite(out).all()) else float('nan')
    print('HWGRAD %s: BM %d stride %d %s cw %d form %d copy %d, tiles %d x %d, %d split(s) of %d / %d stages; maxima %s; condition %.3f; '
          '%s %.4g; relative L2 %.3e' % (case.name, rec['bm'], rec['stride'], 'bf16' if rec['dtype'] else 'fp32', rec['cw'], rec['form'], rec['copy'],
                                         rec['row_tiles'], rec['col_tiles'], rec['splits'], rec['stages_per_split'], rec['stages'], case.maxima, worst,
                                         'max |err| / bound' if case.sect == 'A' else 'unequal elements', ratio, rel))
    assert bool(torch.isfinite(out).all()), 'elements nobody wrote (or NaN partial sums / padded copy read): %d' % int((~torch.isfinite(out)).sum())
    if not ok:
        bad = (out != d.ref) if case.sect == 'B' else ((out - d.ref).abs() > H.bound(case, d.A, rec['splits'], rec['stages_per_split']))
        where = [tuple(int(v) for v in i) for i in bad.nonzero()[:8]]
        raise AssertionError('%s: %d element(s) outside the gate (%.4g), first (k, c, r, s) %r' % (case.name, int(bad.sum()), ratio, where))
    want_acc = base.to(dw.device) + dw
    assert torch.equal(acc, want_acc), 'accumulate = 1 is not base + dw bit for bit: %d element(s) differ' % int((acc != want_acc).sum())


# ---- A, B: the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in H.CASES if c.sect == 'A'], ids=lambda c: c.name)
def test_signed(dev, case, library_options):
    _run(dev, case, library_options)


@pytest.mark.parametrize('case', [c for c in H.CASES if c.sect == 'B'], ids=lambda c: c.name)
def test_exact(dev, case, library_options):
    _run(dev, case, library_options)


# ---- C: operand ranges ------------------------------------------------------------------------------------------------------------------------------
def _fp32_route(x, dy, geom):
    """the project's fp32 route (the fp32-MFMA weight gradient) on the same device tensors"""
    from pcgan_amd.hip import ops
    N, C, Hh, W, K, Rr, S, st, pad, pm = geom
    old = (ops.HSPLIT, ops.BF16X6)
    ops.HSPLIT = False
    ops.BF16X6 = False
    ops.clear_plans()
    try:
        route = ops._plan(ops._L.PASS_BWD_WEIGHT, N, C, Hh, W, K, Rr, S, st, pad, pm, ops.F32).route
        seq = ops.hwgrad_last_launch()['seq']
        dw32 = ops.conv2d_bwd_weight(x, dy, (K, C, Rr, S), st, pad, pm)
        torch.cuda.synchronize()
        after = ops.hwgrad_last_launch()['seq']
    finally:
        ops.HSPLIT, ops.BF16X6 = old
        ops.clear_plans()
    assert route == 'generic' and after == seq, 'the comparison kernel was not the fp32 weight gradient: %s %r %r' % (route, seq, after)
    return dw32.double().cpu()


@pytest.mark.parametrize('maxima', ['plane', 'amax_of'])
@pytest.mark.parametrize('kind', H.C_KINDS)
@pytest.mark.parametrize('geom', H.C_SHAPES, ids=['gen', 'reflect'])
def test_operand_ranges(dev, geom, kind, maxima, library_options):
    x, dy, ref = D.range_case(kind, geom, H.grad64)
    library_options({})
    pl = H.plan(geom, False, {})
    K, C, Rr, S = geom[4], geom[1], geom[5], geom[6]
    g = torch.Generator().manual_seed(K + C)
    base = torch.randn(K, C, Rr, S, generator=g) * float(ref.abs().max())
    dw, acc, rec, nb = _launch(dev, geom, False, x, dy, base, maxima)
    assert tuple(rec[k] for k in H.RECORD) == H.record(pl), rec
    dw32 = _fp32_route(x.to(dev), dy.to(dev), geom)
    out = dw.double().cpu()
    (e, m), (e32, m32) = D.errors(out, ref), D.errors(dw32, ref)
    print('HWGRAD C %s %s %s: relative L2 (e, e32) = (%.3e, %.3e); max|err| / max|ref| (per-tap, fp32 route) = (%.3e, %.3e)' % (geom, kind, maxima, e, e32, m, m32))
    assert bool(torch.isfinite(out).all())
    assert e < 3e-6 and e <= 2 * e32 + 5e-7, 'relative L2 %.3e (fp32 route %.3e)' % (e, e32)
    assert m <= 2 * m32 + 5e-7 and m <= 1e-4, 'max |error| %.3e of the largest magnitude (fp32 route %.3e)' % (m, m32)
    assert torch.equal(acc, base.to(dev) + dw)


# ---- D: host routing --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,geom,half', H.D_SHAPES, ids=[s[0] for s in H.D_SHAPES])
def test_host_routing_reaches_the_same_launch(dev, name, geom, half, library_options, monkeypatch):
    """ops.conv2d_bwd_weight(...) and (..., accumulate_into=base) against the direct call: same record, same bits; with "hwgrad_ks" = 0
    the workspace is the heuristic's"""
    from pcgan_amd.hip import ops
    monkeypatch.setattr(ops, 'BSPLIT_MIN_PIXELS', 0)
    library_options({})
    N, C, Hh, W, K, Rr, S, st, pad, pm = geom
    d = H._data(geom, half, 'signed')
    pl = H.plan(geom, half, {})
    g = torch.Generator().manual_seed(N + C + K)
    base = torch.randn(K, C, Rr, S, generator=g) * float(d.ref.abs().max())
    dw, acc, rec, nb = _launch(dev, geom, half, d.x, d.dy, base, 'amax_of')
    assert tuple(rec[k] for k in H.RECORD) == H.record(pl) and nb == pl.ws_bytes
    xd, dyd = d.x.to(dev), d.dy.to(dev)
    assert ops._plan(ops._L.PASS_BWD_WEIGHT, N, C, Hh, W, K, Rr, S, st, pad, pm, ops.BF16 if half else ops.F32).route == 'hsplit'
    dw2 = ops.conv2d_bwd_weight(xd, dyd, (K, C, Rr, S), st, pad, pm)
    rec2 = ops.hwgrad_last_launch()
    into = base.to(dev).clone()
    ops.conv2d_bwd_weight(xd, dyd, (K, C, Rr, S), st, pad, pm, accumulate_into=into)
    rec3 = ops.hwgrad_last_launch()
    torch.cuda.synchronize()
    for r, k in ((rec2, 1), (rec3, 2)):
        assert r['seq'] == rec['seq'] + k and {f: r[f] for f in H.RECORD} == {f: rec[f] for f in H.RECORD}, (r, rec)
    assert torch.equal(dw2, dw) and torch.equal(into, acc)


def test_row_ring_call_leaves_the_record(dev, library_options):
    """a shape the host unit hands to the row-ring form: the per-tap kernel is not launched and its record does not move; with
    "wgrad_rowring" = 0 the same call launches it"""
    from pcgan_amd.hip import lib as L, ops
    geom = H.G(1, 32, 4, 16, 128, 3, 1, 1, 1)
    assert not H.supported(geom, False, {}) and H.supported(geom, False, {'wgrad_rowring': 0})
    d = H._data(geom, False, 'signed')
    lib = L.load()
    for ring, moves in ((1, 0), (0, 1)):
        library_options({'wgrad_rowring': ring})
        desc = _desc(geom, False)
        nb = int(lib.pcgan_conv2d_hsplit_wgrad_workspace_bytes(ctypes.byref(desc)))
        ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
        xd, dyd = d.x.to(dev), d.dy.to(dev)
        xm, dm = ops.amax_of(xd), ops.amax_of(dyd)
        dw = torch.full((128, 32, 3, 3), float('nan'), device=dev)
        vp = ctypes.c_void_p
        seq0 = ops.hwgrad_last_launch()['seq']
        L.check(lib.pcgan_conv2d_bwd_weight_hsplit(ctypes.byref(desc), vp(xd.data_ptr()), vp(xm.data_ptr()), xm.numel(), vp(dyd.data_ptr()), vp(dm.data_ptr()),
                                                   dm.numel(), vp(dw.data_ptr()), 0, vp(ws.data_ptr()), nb, vp(torch.cuda.current_stream().cuda_stream)), 'hsplit')
        torch.cuda.synchronize()
        assert ops.hwgrad_last_launch()['seq'] == seq0 + moves
        err = (dw.double().cpu() - d.ref).abs()
        assert bool((err <= 1e-4 * d.ref.abs().max()).all())
