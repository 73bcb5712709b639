"""GPU: the fp32-MFMA implicit GEMM (csrc/igemm_mfma.hip: igemm_kernel, igemm2_kernel<.., 16>, igemm2_kernel<.., 4>), the small-M kernels
(csrc/smallm_conv.hip: smallm_strip_kernel, smallm_conv_fewtaps_kernel, smallm_conv_kernel) and their helpers (csrc/igemm_conv.hip:
splitk_reduce_kernel, reflect_fold_kernel, the repack kernels; transpose4 / pack_strip) held to float64 element by element, instantiation
by instantiation.

These kernels run every forward and data gradient the fast routes refuse, and the fast routes' tests gate against their error.  Each case
(tests/conv_f32_cases.py: table, data, reference, bound and the condition that makes the bound bite; tests/test_conv_f32_cases.py checks
the table on the CPU) calls pcgan_conv2d_fwd / pcgan_conv2d_bwd_data directly -- the host's routing cannot divert it -- with the output
NaN-filled and the workspace plus a 4 KiB tail behind the queried size filled with 0xFF bytes (the tail must not change), and reads
pcgan_igemm_last_launch back: one launch, and form, mode, bm, bp, ks and phases must be what the case is there to hit, so a case that lands
on another instantiation fails.  "hgemm_tile" / "hgemm_ks" force tile and K split from 33 rows on; "hgemm_bf16" = 0 keeps bf16 tensors on
these kernels.  Every case then runs again through ops.conv2d_fwd / ops.conv2d_bwd_data with a pack cache (pcgan_conv2d_pack_weights +
the _packed entry points; ops.HSPLIT / ops.BF16X6 off so that the route is 'packed'), which must give the same record and the same bits.

A. igemm2_kernel<.., 16>: five tiles x {fwd_zero, fwd_reflect, dgrad stride 1, dgrad stride 2 with odd H / W, dgrad_reflect row-folded
   (7x12 and the smallest legal plane 4x4), dgrad_reflect fused without the fold}, whole and K-split (short and empty last slice, the
   heuristic's own split on the 32-row tile), 1x1 / 2x3 / 3x3 / 4x4 / 5x5 filters.  The mirror-gather form holds at most 9 taps
   (NTAP_MIR), so a 5x5 reflect gradient never reaches it (it takes the padded fallback, section C); the fused form without the row fold
   is reached with 3x3 at pad 2 and 2x3 at pad 1.
B. igemm2_kernel<.., 4>: 3 and 4 gathered channels, 7x7 (49 taps: a partial last stage of 4), 4x4 / 3x3 stride 2, forward and the data
   gradient of a convolution that produces 3 / 4 channels, all five tiles, K-split.
C. igemm_kernel: gathered channels 5, 8, 12, 20, 24 (the tap changes inside a thread's 8 K slots on the 128-pixel tiles for Cgp 12 and 20,
   at their start for 8 and 24; on the 64-pixel tiles a thread's 4 slots never straddle a tap because Cgp is a multiple of 4), 7x7 on 16
   channels, 11x11 stride 4, three modes x five tiles, forced and heuristic splits; the padded reflect fallback + reflect_fold_kernel for
   K % 16 != 0 and for planes under 2 pad + 2, where an axis folds from both sides (both storage types, on igemm_kernel, igemm2<.., 4> and
   the few-taps kernel), with the bias that the fold adds and without one; 1x1 stride 2 (memset, no split workspace).
D. small-M: strip kernel NR 4 / 7 x MO 3 / 4 x three modes, stride-2 phases, heights 8 / 9 / 19, M = 1, 3, 4, the channel split (64, 67,
   115 channels); few-taps kernel with and without an 8-channel remainder, more than 256 pixels; generic kernel (plane under 8 rows, two
   row taps, strided forward, 11x11).
E. fused activations (none, ReLU, LeakyReLU(0.2), tanh, sigmoid) in each kernel's epilogue and in splitk_reduce_kernel (vector and scalar
   path, fp32 and bf16 stores, behind the MFMA kernels and behind the strip kernel's channel split).

Instantiations reached, ticked from the records read back on an MI355X (256 CUs), not from the table:
  kernel             modes x tiles / variants                                    fp32          bf16
  igemm2<.., 16>     4 modes x 5 tiles                                           20 of 20 ran  20 of 20 ran
  igemm2<.., 4>      3 modes x 5 tiles                                           15 of 15 ran  15 of 15 ran
  igemm_kernel       3 modes x 5 tiles                                           15 of 15 ran  15 of 15 ran
  smallm_strip       3 modes x NR 4 / 7 x MO 3 / 4                               12 of 12 ran  12 of 12 ran
  smallm_fewtaps     3 modes                                                      3 of  3 ran   3 of  3 ran
  smallm_conv        3 modes                                                      3 of  3 ran   3 of  3 ran
  136 of 136 ran (the last test of this file asserts it from the records when the whole file ran in one process; a selection is held to
  the instantiations of its own cases, and a process in which no case ran fails that test).  K splits recorded: 1 .. 8 on the MFMA kernels (forced 2, 3,
  4, 5, 6, 8; the heuristic's 6, 7, 8 on the 32-row tile), channel splits 4 and 7 on the strip kernel; 1, 3, 4 and 16 phases.
  Not reachable through the C-ABI, by construction of the host: the small-M kernels have no dgrad_reflect form (launch_kernel maps the
  mode to dgrad, and bwd_fused_reflect needs more than 4 output rows anyway); igemm_kernel and igemm2<.., 4> have none either
  (static_assert; launch_igemm refuses); the forcing options do not reach layers of <= 32 rows, so the 32x128 tile splits by the
  heuristic alone.  splitk_reduce_kernel, reflect_fold_kernel, repack_fwd / repack_bwd / repack_bwd_multi (plain, chunked, folded),
  transpose4 and pack_strip run under the cases that need them; the tests name no instantiation of theirs beyond fp32 / bf16.

Measured there per section, recorded and not gated (max |err| / bound over the section's cases; relative L2 error):
  section  storage  cases   max |err| / bound    relative L2
    A      fp32       56    < 0.001 .. 0.025     1.4e-7 .. 2.5e-7
    A      bf16       43    0.900 .. 0.985       1.6e-3 .. 1.7e-3
    B      fp32       30    0.003 .. 0.074       5.6e-8 .. 2.5e-7
    B      bf16       30    0.901 .. 0.991       1.6e-3 .. 1.7e-3
    C      fp32       45    < 0.001 .. 0.041     7.4e-8 .. 4.3e-7
    C      bf16       33    0.780 .. 0.986       1.6e-3 .. 2.4e-3
    D      fp32       42    < 0.001 .. 0.048     7.2e-8 .. 2.7e-7
    D      bf16       34    0.710 .. 0.977       1.6e-3 .. 2.3e-3
    E      fp32       45    < 0.001 .. 0.013     1.0e-7 .. 6.3e-7
    E      bf16       40    0.317 .. 0.975       5.6e-4 .. 1.7e-3
  fp32: the errors sit far inside the bound because it is a worst case over all orders and sign patterns; what the gate buys is the
  condition (largest bound of any case 0.143 against the 0.28 allowed): a lost or doubled term is >= 2 x the bound.  bf16: the half ulp of
  the stored result is attained (results just above a power of two), the accumulation term is the margin; largest condition 0.272.
  Found and fixed with these cases: the padded reflect fallback wrote the bias onto the padded grid, so reflect_fold_kernel added it once
  per mirror image (up to 9 times); the grid is now written without it and the fold adds it once.  Every reflect data gradient of the
  table carries a bias.  No net of the project passes a bias there.  Everything else passes on the kernels as they were.
  Wall time of the file: 399 tests in 2.4 s."""
import ctypes

import pytest
import torch

import conv_f32_cases as T
from gpu_direct import VP, ptr, guarded

pytestmark = pytest.mark.gpu

NAMES = list(T.BY_NAME)
SEEN = {}      # case name -> record read back (printed by the last test: the coverage table above is filled from it)


@pytest.fixture
def force():
    """sets "hgemm_tile" / "hgemm_ks" and "hgemm_bf16" = 0 (cached launch plans hold workspace sizes that depend on them: dropped on every
    change) and restores what was set before"""
    from pcgan_amd.hip import lib as L, ops
    before = {k: L.get_option(k) for k in ('hgemm_tile', 'hgemm_ks', 'hgemm_bf16')}

    def set_(tile, ks):
        L.set_option('hgemm_tile', tile)
        L.set_option('hgemm_ks', ks)
        L.set_option('hgemm_bf16', 0)
        ops.clear_plans()
    try:
        yield set_
    finally:
        for k, v in before.items():
            L.set_option(k, v)
        ops.clear_plans()


def _record():
    from pcgan_amd.hip import ops
    r = ops.igemm_last_launch()
    return r['seq'], (r['form'], r['mode'], r['bm'], r['bp'], r['ks'], r['nphase'])


def _direct(dev, c, src, w, b):
    """the C-ABI call of the case; returns (output, record)"""
    from pcgan_amd.hip import lib as L, ops
    lib = L.load()
    N, C, H, W, K, Rr, S, stride, pad, pm = c.geom
    d = ops.make_desc(*c.geom, ops.BF16 if c.half else ops.F32)
    fwd = c.pass_ == 'fwd'
    nb = int(lib.pcgan_conv2d_workspace_bytes(ctypes.byref(d), L.PASS_FWD if fwd else L.PASS_BWD_DATA))
    ws = guarded(dev, nb)
    shape = (N, K, d.P, d.Q) if fwd else (N, C, H, W)
    y = torch.full(shape, float('nan'), dtype=src.dtype, device=dev)
    st = VP(torch.cuda.current_stream().cuda_stream)
    seq0, _ = _record()
    if fwd:
        L.check(lib.pcgan_conv2d_fwd(ctypes.byref(d), ptr(src), ptr(w), ptr(b), ptr(y), c.act, T.SLOPE, ptr(ws), nb, st), 'conv2d_fwd')
    else:
        L.check(lib.pcgan_conv2d_bwd_data(ctypes.byref(d), ptr(src), ptr(w), ptr(b), ptr(y), ptr(ws), nb, st), 'conv2d_bwd_data')
    seq, rec = _record()
    assert seq == seq0 + 1, 'one recorded launch per call: %d after %d' % (seq, seq0)
    torch.cuda.synchronize()
    assert bool((ws[nb:] == 0xFF).all()), 'the call wrote behind the workspace it asked for (%d bytes)' % nb
    return y, rec


def _packed(dev, monkeypatch, c, src, w, b):
    """the same case through the pack cache: pcgan_conv2d_pack_weights and the _packed entry point"""
    from pcgan_amd.hip import ops
    N, C, H, W, K, Rr, S, stride, pad, pm = c.geom
    what = 'fwd' if c.pass_ == 'fwd' else 'dgrad'
    with monkeypatch.context() as mp:
        mp.setattr(ops, 'HSPLIT', False)
        mp.setattr(ops, 'BF16X6', False)
        r0 = ops.ROUTE_STATS.get((what, 'packed'), 0)
        seq0, _ = _record()
        if c.pass_ == 'fwd':
            y = ops.conv2d_fwd(src, w, b, stride, pad, pm, c.act, T.SLOPE, pack_cache={})
        else:
            y = ops.conv2d_bwd_data(src, w, (H, W), stride, pad, pm, bias=b, pack_cache={})
        seq, rec = _record()
        torch.cuda.synchronize()
        assert ops.ROUTE_STATS.get((what, 'packed'), 0) == r0 + 1, 'the pack-cache call took another route: %r' % (ops.ROUTE_STATS,)
        assert seq == seq0 + 1
    return y, rec


@pytest.mark.parametrize('name', NAMES)
def test_case(dev, force, monkeypatch, name):
    c = T.BY_NAME[name]
    pl = T.plan(c)
    assert T.record(pl) == c.want
    dat = T.data(c)
    E, bound, aref = T.bounds(c, pl)
    worst = T.condition(c, pl)
    assert worst < T.TERM_MIN / 2, 'the largest bound %.4f would not catch one lost term' % worst
    force(c.tile, c.ks)
    src, w = dat.src.to(dev).contiguous(), dat.w.to(dev).contiguous()
    b = dat.b.to(dev).contiguous() if dat.b is not None else None
    y, rec = _direct(dev, c, src, w, b)
    SEEN[name] = rec
    assert rec == c.want, 'the case ran another instantiation: %r, wanted %r' % (rec, c.want)
    yc = y.double().cpu()
    err = (yc - aref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool(torch.isfinite(yc).all()) else float('nan')
    rel = float((yc - aref).norm() / aref.norm())
    print('CONVF32 %s %s: %s %r; max |err| / bound %.4f; relative L2 %.3e; condition %.3f' % (c.sect, name, T.instantiation(c, rec), rec, ratio, rel, worst))
    assert bool(torch.isfinite(yc).all()), 'elements nobody wrote (or NaN partial sums read): %d' % int((~torch.isfinite(yc)).sum())
    assert bool((err <= bound).all()), '%d element(s) outside the bound, worst %.3g x the bound at %r (%.6g, reference %.6g)' % (
        int((err > bound).sum()), ratio, tuple(int(v) for v in torch.unravel_index((err / bound.clamp_min(1e-300)).argmax(), err.shape)),
        float(yc.flatten()[int((err / bound.clamp_min(1e-300)).argmax())]), float(aref.flatten()[int((err / bound.clamp_min(1e-300)).argmax())]))
    y2, rec2 = _packed(dev, monkeypatch, c, src, w, b)
    assert rec2 == c.want, 'the pack-cache call ran another instantiation: %r, wanted %r' % (rec2, c.want)
    assert torch.equal(y2, y), 'packed and unpacked calls differ in %d element(s)' % int((y2 != y).sum())


def test_zz_every_instantiation_ran():
    """the records read back by the cases that ran in this process name every instantiation those cases are there for -- all 136 when the
    whole file ran.  A selection (-k, one worker of several) is held to its own cases only; a process in which no case ran has nothing
    to check and says so"""
    assert SEEN, 'no case of this file ran in this process before this test: nothing was checked (run the whole file in one process)'
    ran = {T.instantiation(T.BY_NAME[n], r) for n, r in SEEN.items()}
    want = {T.instantiation(T.BY_NAME[n], T.BY_NAME[n].want) for n in SEEN}
    every = T.all_instantiations()
    fams = (('igemm2<.., 16>', lambda i: i.startswith('igemm2<') and ', 16, ' in i), ('igemm2<.., 4>', lambda i: i.startswith('igemm2<') and ', 4, ' in i),
            ('igemm_kernel', lambda i: i.startswith('igemm<')), ('smallm_strip', lambda i: i.startswith('smallm_strip<')),
            ('smallm_fewtaps', lambda i: i.startswith('smallm_fewtaps<')), ('smallm_conv', lambda i: i.startswith('smallm_conv<')))
    for fam, sel_ in fams:
        for dt in ('fp32', 'bf16'):
            sel = [i for i in every if sel_(i) and i.endswith(dt + '>')]
            print('COVERAGE %-16s %s: %d of %d ran' % (fam, dt, len([i for i in sel if i in ran]), len(sel)))
    assert sorted(want - ran) == [], 'instantiations the cases that ran should have reached and did not'
    if len(SEEN) == len(NAMES):
        assert sorted(set(every) - ran) == [], 'instantiations no case reached'
