"""GPU: the per-tap bf16-piece convolution (csrc/bsplit_conv.hip: bsplit_conv_fwd_kernel, 4 modes x 2 tiles x 2 piece forms) held to float64
element by element, instantiation by instantiation.

tests/test_gpu_bf16x6.py judges it by one relative L2 per tensor on randn data with fp32 descriptors, tests/test_gpu_bf16.py reaches it
through the routing of ops under a bf16-sized tolerance: one wrong low piece, a swapped row class, a column-mirror source from the wrong
tap, a dead stage that adds something or a dropped stage of the last weight-gradient split passes both.  Here (tests/bsplit_cases.py:
table, data, reference, bounds, the host restated, the conditions that make the gates bite; tests/test_bsplit_cases.py checks all of that,
the emulation and the sensitivity study on the CPU) each case calls the C-ABI directly -- pcgan_conv2d_bsplit_pack / _fwd_bsplit,
_bsplit_dgrad_pack / _bwd_data_bsplit, _bwd_weight_bsplit with an fp32 or a bf16 descriptor -- with a packed buffer of exactly the size
the library names plus a 0xFF tail, the output a NaN-filled view between two 4 KiB guards, the weight-gradient workspace of exactly the
named size (0xFF-filled: NaN partial sums and padded copy) with a guard behind it.  After each call every output element is finite, no
guard byte has changed, the launch record (pcgan_bsplit_last_launch) equals the case's `want` -- the per-tap kernel, not the window
kernel, in the instantiation the case names -- and the packed / workspace sizes equal the restated host's.

A. lost, doubled or misplaced terms: signed data of magnitudes [0.75, 1.25], per element inside the bound of the piece form, the largest
   bound of every case under half the smallest term.
B. every piece on the right pair, every fold source in the right element, exactly: integer data whose every partial sum is an fp32
   number ('xlow', 'wlow', 'mid', and per source class of the data gradient 'fold'), out == ref in every element.
C. operand ranges (bf16x3): relu_normal, wide_range, huge, tiny per produced channel against float64 and against the fp32 route on the
   same inputs (the gate of tests/test_gpu_bf16x6.py: relative L2 < 3e-6 and < 2 x the fp32 route's + 5e-7); 'tiny2', one step further
   down, is recorded only.

Measured on an MI355X (256 CUs), recorded and not gated beyond the clauses above:
  section  cases  max |err| / bound            relative L2            what
    A       45    bf16x3 fwd    0.0003 .. 0.0031   3.3e-8 .. 2.9e-7    every case inside its bound; largest condition 0.151 of the 0.281 allowed
                  bf16x3 dgrad  0.0005 .. 0.0010   1.4e-7 .. 2.3e-7    (bf16x3 weight gradient over 448 pixels), 0.262 for bf16 tensors (a data
                  bf16x3 wgrad  0.0002 .. 0.0025   1.1e-7 .. 1.8e-7    gradient), where 2^-8 |ref| is most of it and the rounding of
                  bf16   fwd    0.85   .. 0.97     1.5e-3 .. 1.7e-3    the store reaches it; the bf16 weight gradient stores fp32: 5 cases, at least
                  bf16   dgrad  0.92   .. 0.96     1.6e-3 .. 1.7e-3    one with every element equal to float64
                  bf16   wgrad  0      .. 0.0002   0      .. 2.6e-8
    B      146    0                            0                      every element exact: 48 'xlow', 48 'wlow', 2 'mid', 48 'fold' (8 source classes
                                                                      x 3 shapes x 2 piece forms); the largest partial sum 0.75 of 2^24
    C       15    12 gated cases, relative L2 per produced channel 8.3e-8 .. 3.7e-7 against 1.1e-7 .. 3.9e-7 on the fp32 route:
                  fwd    relu_normal 1.7e-7 .. 3.7e-7 | 1.7e-7 .. 2.8e-7, wide_range 1.1e-7 .. 2.8e-7 | 1.1e-7 .. 3.4e-7, huge 2.1e-7 .. 2.9e-7 |
                         2.4e-7 .. 3.9e-7, tiny 2.0e-7 .. 3.4e-7 | 2.1e-7 .. 3.7e-7
                  dgrad  relu_normal 1.9e-7 .. 3.1e-7 | 2.5e-7 .. 3.5e-7, wide_range 1.2e-7 .. 2.5e-7 | 1.1e-7 .. 2.8e-7, huge 1.8e-7 .. 3.3e-7 |
                         2.2e-7 .. 3.8e-7, tiny 1.9e-7 .. 2.9e-7 | 2.3e-7 .. 3.7e-7
                  wgrad  relu_normal 1.0e-7 .. 2.6e-7 | 1.4e-7 .. 2.9e-7, wide_range 8.3e-8 .. 2.0e-7 | 1.1e-7 .. 3.1e-7, huge 1.2e-7 .. 2.2e-7 |
                         2.4e-7 .. 3.7e-7, tiny 1.3e-7 .. 2.1e-7 | 2.3e-7 .. 3.7e-7
                  'tiny2' (factors 1e-19 and 1e-15: typical terms near 1e-36, so the (h,m) / (m,h) products sit around 2^-126 and the four
                  smaller ones below it), recorded only: fwd 2.0e-7 .. 3.2e-7, dgrad 1.9e-7 .. 2.9e-7, wgrad 1.3e-7 .. 2.1e-7 -- the same as
                  'tiny', no zero written.  At this depth the matrix pipe did not lose the subnormal piece products (a flushed (h,m) product
                  would be 2^-9 of a term, four decades above what was measured), so there is no limit of the form to add to DESIGN.md
                  section 8 from this measurement.
  Coverage, from the cases that ran (cases in A, in B):
    fwd_zero    128 bf16x3: 8, 18   fwd_zero    128 bf16: 8, 16   fwd_zero    256 bf16x3: 1,  2   fwd_zero    256 bf16: 1,  2
    fwd_reflect 128 bf16x3: 2,  4   fwd_reflect 128 bf16: 1,  4   fwd_reflect 256 bf16x3: 2,  4   fwd_reflect 256 bf16: 1,  4
    dgrad       128 bf16x3: 3, 22   dgrad       128 bf16: 3, 22   dgrad       256 bf16x3: 3, 14   dgrad       256 bf16: 2, 14
    wgrad       128 bf16x3: 3,  6   wgrad       128 bf16: 3,  6   wgrad       256 bf16x3: 2,  4   wgrad       256 bf16: 2,  4
  Found with this work: no fault of the kernel -- all 208 tests passed on the kernel as it was.  One inconsistency of the host, seen while
  restating it and held by tests/test_bsplit_cases.py (2 CPU tests: the sweep of descriptors and the K series): pcgan_conv2d_bsplit_wgrad_
  supported answered 1, and the workspace query a size, for every K >= 32, while pcgan_conv2d_bwd_weight_bsplit refuses all but one full
  row tile.  The change: the predicate holds K = 128 | 256 itself, and the `c.K in (128, 256)` clause of ops.py, which kept callers away
  from the difference, is gone.  What it moves: no launch -- the route table reaches the same decision from the same two values, the
  route-count tests of the suite pass unchanged, and no kernel, pack or shared header is touched.
  Sensitivity (tests/test_bsplit_cases.py: the eight faults applied to the torch restatement of the kernel's arithmetic, never to a kernel
  on a GPU; cases failed of the cases in which the fault has a place, A | B | C): (m,m) dropped 0 of 24 | 2 of 74 | 12 of 12; (l,h) dropped
  0 of 24 | 12 of 74 | 12 of 12; row classes 1 and 2 swapped 11 of 11 | 72 of 72 | 4 of 4; the column-mirror source of pixel 1 from tap 0
  11 of 11 | 54 of 72 | 4 of 4; one tap shifted 22 of 25 | 82 of 104 | 8 of 8; the dead stage of an odd count repeating stage 0 31 of 31 |
  113 of 113 | none (even counts); the last stage of the last weight-gradient split dropped 10 of 10 | 20 of 20 | 4 of 4; one 8-channel
  half of one pixel zero in buffer 1 43 of 43 | 107 of 141 | 12 of 12.
  Wall time of the file: 208 tests in 2.2 s, the slowest 0.8 s (the first data-gradient case: its float64 autograd reference on the CPU).
"""
import ctypes

import pytest
import torch

import bsplit_cases as T
from gpu_direct import VP, GUARD, ptr, guarded, where, coverage_gate

pytestmark = pytest.mark.gpu

NAMES = list(T.BY_NAME)
SEEN = {}      # case name -> (section, (mode, BM, piece form)) of the cases that ran in this process


@pytest.fixture
def library_options():
    """sets library options (cached launch plans depend on them: dropped on every change) and restores what was there afterwards"""
    from pcgan_amd.hip import lib as L, ops
    saved = {k: L.get_option(k) for k in T.OPTIONS}

    def apply(opts):
        for k, v in T.options(opts).items():
            L.set_option(k, v)
        ops.clear_plans()
    try:
        yield apply
    finally:
        for k, v in saved.items():
            L.set_option(k, v)
        ops.clear_plans()


def _view(dev, shape, dt, fill=None):
    """a NaN-filled (or `fill`) view of `shape` between two guards of 0xFF; returns (whole buffer, view, bytes)"""
    n = 1
    for v in shape:
        n *= v
    nbytes = n * (2 if dt == torch.bfloat16 else 4)
    big = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    y = big[GUARD:GUARD + nbytes].view(dt).view(shape)
    if fill is None:
        y.fill_(float('nan'))
    else:
        y.copy_(fill)
    return big, y, nbytes


def _guards_intact(big, nbytes):
    return bool((big[:GUARD] == 0xFF).all()) and bool((big[GUARD + nbytes:] == 0xFF).all())


def _launch(dev, c, d):
    """one direct call of the case's entry point; returns (result as float64 on the CPU, record)"""
    from pcgan_amd.hip import lib as L, ops
    lib = L.load()
    half = c.pk == 'bf16'
    dt = torch.bfloat16 if half else torch.float32
    desc = ops.make_desc(*c.geom, dtype=L.BF16 if half else L.F32)
    ref = ctypes.byref(desc)
    pl = T.plan(c)
    st = VP(torch.cuda.current_stream().cuda_stream)
    src = d.src.to(dev).to(dt).contiguous()
    assert bool((src.double().cpu() == d.src.double()).all()), 'the operand is no number of the storage type'
    assert tuple(src.shape) == T.src_shape(c)
    seq0 = ops.bsplit_last_launch()['seq']
    if c.pass_ == 'wgrad':
        dy = d.w.to(dev).to(dt).contiguous()
        assert bool((dy.double().cpu() == d.w.double()).all())
        assert lib.pcgan_conv2d_bsplit_wgrad_supported(ref) == 1
        nb = int(lib.pcgan_conv2d_bsplit_wgrad_workspace_bytes(ref))
        assert nb == pl.ws_bytes, (nb, pl.ws_bytes)
        ws = guarded(dev, nb)
        big, y, nbytes = _view(dev, T.out_shape(c), torch.float32, d.base.to(dev) if d.base is not None else None)
        L.check(lib.pcgan_conv2d_bwd_weight_bsplit(ref, ptr(src), ptr(dy), ptr(y), int(c.acc), ptr(ws), nb, st), 'conv2d_bwd_weight_bsplit')
        rec = ops.bsplit_last_launch()
        torch.cuda.synchronize()
        assert bool((ws[nb:] == 0xFF).all()), 'the call wrote behind the %d bytes of workspace it asked for' % nb
    else:
        w = d.w.to(dev).contiguous()
        assert w.dtype == torch.float32
        fwd = c.pass_ == 'fwd'
        if fwd:
            assert lib.pcgan_conv2d_bsplit_supported(ref) == 1
            nb = int(lib.pcgan_conv2d_bsplit_packed_bytes(ref))
        else:
            assert lib.pcgan_conv2d_bsplit_dgrad_supported(ref) == 1
            nb = int(lib.pcgan_conv2d_bsplit_dgrad_packed_bytes(ref))
        assert nb == pl.packed_bytes, (nb, pl.packed_bytes)
        pk = guarded(dev, nb)
        big, y, nbytes = _view(dev, T.out_shape(c), dt)
        if fwd:
            b = d.b.to(dev).contiguous() if d.b is not None else None
            L.check(lib.pcgan_conv2d_bsplit_pack(ref, ptr(w), ptr(pk), st), 'conv2d_bsplit_pack')
            L.check(lib.pcgan_conv2d_fwd_bsplit(ref, ptr(src), ptr(pk), ptr(b), ptr(y), c.act, T.slope_of(c), st), 'conv2d_fwd_bsplit')
        else:
            L.check(lib.pcgan_conv2d_bsplit_dgrad_pack(ref, ptr(w), ptr(pk), st), 'conv2d_bsplit_dgrad_pack')
            L.check(lib.pcgan_conv2d_bwd_data_bsplit(ref, ptr(src), ptr(pk), ptr(y), st), 'conv2d_bwd_data_bsplit')
        rec = ops.bsplit_last_launch()
        torch.cuda.synchronize()
        assert bool((pk[nb:] == 0xFF).all()), 'the pack wrote behind the %d bytes it asked for' % nb
    assert rec['seq'] == seq0 + 1, 'one recorded launch per call: %r after %d' % (rec, seq0)
    got = tuple(rec[k] for k in T.RECORD)
    assert got == c.want, 'the case ran another launch: %r, wanted %r' % (dict(zip(T.RECORD, got)), dict(zip(T.RECORD, c.want)))
    assert _guards_intact(big, nbytes), 'the call wrote outside its output'
    yc = y.double().cpu()
    assert bool(torch.isfinite(yc).all()), 'elements nobody wrote, or not finite: %d' % int((~torch.isfinite(yc)).sum())
    return yc, rec


@pytest.mark.parametrize('name', NAMES)
def test_case(dev, name, library_options):
    from pcgan_amd.hip import lib as L
    c = T.BY_NAME[name]
    d = T.data(c)
    if c.sect == 'A':
        worst, allowed = T.condition(c)
        assert worst < allowed, 'the largest bound %.4f would not catch one lost term' % worst
        E, bound, want = T.bounds(c)
    else:
        worst = T.quanta(c) / 2.0 ** 24
        assert worst < 1.0
        want = T.exact_expected(c)
        bound = torch.ones_like(want)
    library_options(c.opts)
    yc, rec = _launch(dev, c, d)
    SEEN[name] = (c.sect, T.inst(c))
    err = (yc - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    rel = float((yc - want).norm() / want.norm())
    print('BSPLIT %s: %s BM %d %s; tiles %d x %d, %d stage(s) in %d split(s); condition %.3f; max |err| / bound %.4f; relative L2 %.3e; '
          'elements != reference %d' % ((name,) + T.inst(c) + (rec['row_tiles'], rec['tiles'], rec['stages'], rec['splits'], worst, ratio, rel,
                                                               int((yc != want).sum()))))
    if c.sect == 'A':
        assert bool((err <= bound).all()), '%d element(s) outside the bound, worst %.3g x the bound at %r' % (
            int((err > bound).sum()), ratio, where(err / bound.clamp_min(1e-300)))
    else:
        assert bool((yc == want).all()), '%d element(s) not exact, the first worst at %r: %r, reference %r' % (
            int((yc != want).sum()), where(err), float(yc[where(err)]), float(want[where(err)]))
    if c.opts:
        assert L.get_option('bsplit_halo') == 0      # (the case ran under the option; the fixture restores it)


def test_option_is_back_at_its_default():
    """after the option cases above: bsplit_halo is 1 again, and the same geometry goes to the window kernel"""
    from pcgan_amd.hip import lib as L
    assert L.get_option('bsplit_halo') == 1
    for name in ('f_option', 'd_option'):
        c = [c for c in T.CASES if c.name.startswith('B_%s_bf16x3' % name)][0]
        assert T.plan(c._replace(opts=())).kernel == T.WINDOW and T.plan(c).kernel == T.PER_TAP


# ---- C. operand ranges (bf16x3) ---------------------------------------------------------------------------------------------------------
def _fp32_route(c, src, w):
    """the project's fp32 route (fp32-MFMA kernels) on the same device tensors"""
    from pcgan_amd.hip import ops
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    old = (ops.HSPLIT, ops.BF16X6)
    ops.HSPLIT = False
    ops.BF16X6 = False
    ops.clear_plans()
    try:
        p = {'fwd': ops._L.PASS_FWD, 'dgrad': ops._L.PASS_BWD_DATA, 'wgrad': ops._L.PASS_BWD_WEIGHT}[c.pass_]
        route = ops._plan(p, N, C, H, W, K, Rr, S, st, pad, pm, ops.F32).route
        seq = ops.bsplit_last_launch()['seq']
        if c.pass_ == 'fwd':
            y = ops.conv2d_fwd(src, w, None, st, pad, pm, pack_cache={})
        elif c.pass_ == 'dgrad':
            y = ops.conv2d_bwd_data(src, w, (H, W), st, pad, pm, pack_cache={})
        else:
            y = ops.conv2d_bwd_weight(src, w, (K, C, Rr, S), st, pad, pm)
        torch.cuda.synchronize()
        after = ops.bsplit_last_launch()['seq']
    finally:
        ops.HSPLIT, ops.BF16X6 = old
        ops.clear_plans()
    assert route in ('packed', 'generic') and after == seq, 'the comparison did not run on the fp32 route: %s' % route
    return y.double().cpu()


@pytest.mark.parametrize('key', list(T.RANGE), ids=lambda k: '%s-%s' % k)
def test_operand_ranges(dev, key, library_options):
    c = T.RANGE[key]
    d = T.data(c)
    assert bool(torch.isfinite(d.src).all()) and float(d.ref.abs().max()) > 1e-37      # (the true values are fp32 numbers)
    library_options(())
    yc, rec = _launch(dev, c, d)
    y32 = _fp32_route(c, d.src.to(dev).contiguous(), d.w.to(dev).contiguous())
    e6, e32 = T.channel_rel(c, yc, d.ref), T.channel_rel(c, y32, d.ref)
    print('BSPLIT C %s %s: relative L2 per channel %.3e .. %.3e (fp32 route %.3e .. %.3e); zeros written %d of %d' % (
        c.pass_, c.kind, float(e6.min()), float(e6.max()), float(e32.min()), float(e32.max()), int((yc == 0).sum()), yc.numel()))
    if c.kind == 'tiny2':      # recorded only: piece products below 2^-126
        return
    worst = int((e6 - 2 * e32).argmax())
    assert bool((e6 < 3e-6).all()), 'channel %d: %.3e' % (int(e6.argmax()), float(e6.max()))
    assert bool((e6 < 2 * e32 + 5e-7).all()), 'channel %d: %.3e against %.3e on the fp32 route' % (worst, float(e6[worst]), float(e32[worst]))


def test_zz_every_instantiation_ran():
    """from the cases that ran in this process: all sixteen instantiations in section A and in section B, when the whole file ran.  A
    selection (-k, one worker of several) is held to its own cases only; a process in which no case ran has nothing to check and says so"""
    coverage_gate(SEEN, NAMES, T.INSTANTIATIONS, 'AB', T.BY_NAME, T.inst, 'COVERAGE %-11s BM %d %-6s: A %2d case(s), B %2d')
