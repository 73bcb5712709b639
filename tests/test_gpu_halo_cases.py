"""GPU: the window ("halo") kernel (csrc/halo_conv.hip: bsplit_halo_kernel, 2 modes x 3 piece forms x 2 widths) held to float64 element by
element, instantiation by instantiation.

tests/test_gpu_bf16x6.py judges it by one relative L2 per tensor on randn data: one wrong low piece, one misplaced window entry or one
wrong corner source is about 1e-6 of the norm and passes.  Here (tests/halo_cases.py: table, data, reference, bounds, the conditions that
make them bite; tests/test_halo_cases.py checks all of that and the library's predicate on the CPU) each case calls the C-ABI directly --
pcgan_conv2d_hsplit_pack / _fwd_hsplit / _bwd_data_hsplit / _bwd_data_hsplit_add for the two fp16 pieces, pcgan_conv2d_bsplit_pack /
_fwd_bsplit / _bsplit_dgrad_pack / _bwd_data_bsplit with an fp32 or a bf16 descriptor for the bf16 forms (option bsplit_halo is 1: asserted)
-- into a NaN-filled view between two 4 KiB guards of 0xFF, with a packed buffer of the size the library names plus a 0xFF tail; afterwards
every output element is finite, no guard byte has changed and the non-finite counter is 0.

A. lost, doubled or misplaced terms: signed data of magnitudes [0.75, 1.25], per element inside the bound of the piece form, the largest
   bound of every case under half the smallest term.  All twelve instantiations at one tile per image, two tiles (width 64), three tiles
   on both widths; f16x2 also two chunk pairs with two weight tiles, bias with each activation, the data gradient plain and with an addend.
B. every piece on the right pair, every fold source in the right entry, exactly: integer data whose every partial sum is an fp32 number
   ('xlow', 'wlow', and per source class of the sum entries 'fold'), out == ref in every element; three chunk pairs run here.
C. scales and ranges (f16x2): the true maximum in every slot class of thread_max_of_partials at 512 threads and four pointer alignments;
   all-zero input; one all-zero weight row; operands over twelve decades, times 1e12 / 1e8, times 1e-30 / 1e-6 per produced channel
   against float64 and against the fp32 route; the four-corner sums of the data gradient at the top of the fp16 range.

Measured on an MI355X (256 CUs), recorded and not gated beyond the clauses above:
  section  cases  max |err| / bound      relative L2            what
    A       33    f16x2   0.0002 .. 0.0013   5.4e-8 .. 2.7e-7   every case inside its bound; largest condition 0.22 of the 0.281 allowed (f16x2 data
                  bf16x3  0.0005 .. 0.0008   2.3e-7 .. 2.4e-7   gradient at 64 gathered channels), 0.11 for bf16x3, 0.27 for bf16 tensors, where half a
                  bf16    0.92   .. 0.96     1.7e-3             bf16 ulp at |ref| in [64, 128) is 0.25 on its own and the rounding reaches it
    B      140    0                      0                      every element exact: 24 'xlow', 20 'wlow', 96 'fold' (8 source classes x 4 shapes x 3
                                                                piece forms); v_mfma_f32_32x32x16_f16 and _bf16 add exactly when every partial sum is
                                                                an fp32 number
    C      180 launches of the maximum-slot cases (33 slot placements over 12 array lengths forward, 12 over 4 in the data gradient, x 4 alignments;
           from 8192 slots on also in the second and third of the four loads in flight): exact every time, counter at 0;
           4 all-zero inputs and the 2 all-zero weight rows: exact; 12 range cases, relative L2 per channel
           7.0e-8 .. 3.1e-7 against 9.3e-8 .. 4.2e-7 on the fp32 route (wide_range 7.0e-8 .. 3.1e-7 | 9.3e-8 .. 3.0e-7, huge 1.3e-7 .. 2.9e-7 |
           2.1e-7 .. 4.1e-7, tiny 1.3e-7 .. 3.0e-7 | 2.1e-7 .. 4.2e-7); 4 four-corner cases: max |err| / bound 0.0008 .. 0.0028, relative L2
           1.5e-7 .. 1.8e-7
  Coverage, from the cases that ran (cases in A, in B):
    fwd   f16x2  W 32: 4,  5     fwd   bf16x3 W 32: 2,  6     fwd   bf16 W 32: 2,  5
    fwd   f16x2  W 64: 3,  2     fwd   bf16x3 W 64: 2,  2     fwd   bf16 W 64: 2,  2
    dgrad f16x2  W 32: 6, 21     dgrad bf16x3 W 32: 2, 21     dgrad bf16 W 32: 2, 21
    dgrad f16x2  W 64: 4, 18     dgrad bf16x3 W 64: 2, 19     dgrad bf16 W 64: 2, 18
  Found and fixed with these cases: the f16x2 data gradient scaled dy by pow2_scale(max |dy|), which puts the maximum into [2^13, 2^14), and
  split the corner sum entries -- four dy elements -- AFTER the sum.  Four sources of 16382 make 65528, past fp16's 65504: with dy = 1 - 2^-13
  everywhere, and with only the sixteen corner sources of one plane at the maximum, the kernel as it was wrote NaN into the four pixels
  (1 | H-2, 1 | W-2) of every produced plane (1024 of 32768 | 98304 elements in all four cases; the counter fired, so a training run would have
  stopped, not gone wrong silently).  Now the high piece of a sum entry below 2^16 -- all that four true sources reach -- saturates at
  65504 and the low piece takes the rest (under 32, to 2^-7: the split keeps its 2^-22); a sum from 2^16 on, which only a maximum that
  was none can make, still overflows into the counter.  The 208 other tests of this file passed on the kernel as it was.  The forward
  mode mirrors without adding, and every other split2h call site of the library (hgemm, thin, the three weight-gradient kernels, the packs)
  splits one loaded element times its scale: no other kernel sums before the split.
  What the fix moves: nothing that was finite before.  Every value the plain cast kept finite splits into the same two pieces, so forward
  and data-gradient results of the fp16 route on randn dy and on dy spanning twelve decades (three shapes, two builds in two processes)
  differ in 0 elements, and fake_B, rec_A, the nine losses and the sampled G / D / E state that the benchmark dumps after its last step
  are the same bits under both builds.  The whole GPU suite passes after it; the benchmark's step rate, three interleaved pairs of both
  builds on one MI355X: 1197.6, 1195.8, 1189.8 images/s before, 1196.7, 1197.9, 1199.4 after.
  Sensitivity: a kernel made wrong on purpose is not run on the shared GPU machines, so the four faults were applied to the torch
  restatement of the kernel's arithmetic (halo_cases.emulate with fp32 piece sums) and every gate evaluated on its result.  Dropping the
  (l,h) product fails no case of A (a low piece is 2^-11 of a term), 8 'wlow' cases of B (the six f16x2 ones and the two bf16x3 ones whose
  weights have a third piece), 2 corner and all 12 range cases; the two sum rows swapped fails 18 of the 18 data-gradient cases of A, 12
  'xlow', 10 'wlow' and all 96 'fold' cases of B, 2 corner and the 6 data-gradient range cases; a corner entry of three sources fails the same
  cases and all 4 corner cases; one window entry (four channels of one pixel) of the second buffer written as zero fails all 33 cases of A,
  all 'xlow' and 'wlow' cases, the 12 'fold' cases whose source class holds the pixel, the corner and the range cases.
  Wall time of the file: 213 tests in 3.0 s, the slowest 0.7 s (the first launch of a process)."""
import ctypes

import pytest
import torch

import halo_cases as T
from gpu_direct import VP, GUARD, ptr, guarded, where, coverage_gate

pytestmark = pytest.mark.gpu

NAMES = list(T.BY_NAME)
SEEN = {}      # case name -> (section, (pass, piece form, width)) of the cases that ran in this process


class _Call(object):
    """one packed weight tensor and the buffers of a direct call, guards included"""

    def __init__(self, dev, c, w):
        from pcgan_amd.hip import lib as L, ops
        self.lib, self.L, self.c, self.dev = L.load(), L, c, dev
        self.half = c.pk == 'bf16'
        self.d = ops.make_desc(*T.geom(c), dtype=L.BF16 if self.half else L.F32)
        self.pass_ = L.PASS_FWD if c.pass_ == 'fwd' else L.PASS_BWD_DATA
        ops._sentinel()      # (registers the non-finite counter with the library, once)
        ref = ctypes.byref(self.d)
        N, G, H, W, M = c.shape
        assert T.accepts(G, H, W, M) and L.get_option('bsplit_halo') == 1
        if c.pk == 'f16x2':
            assert self.lib.pcgan_conv2d_hsplit_supported(ref, self.pass_) == 1, 'not a window-kernel shape: %r' % (c.shape,)
            self.nb = int(self.lib.pcgan_conv2d_hsplit_packed_bytes(ref, self.pass_))
        elif c.pass_ == 'fwd':
            assert self.lib.pcgan_conv2d_bsplit_supported(ref) == 1
            self.nb = int(self.lib.pcgan_conv2d_bsplit_packed_bytes(ref))
        else:
            assert self.lib.pcgan_conv2d_bsplit_dgrad_supported(ref) == 1
            self.nb = int(self.lib.pcgan_conv2d_bsplit_dgrad_packed_bytes(ref))
        assert self.nb == T.packed_bytes(c), (self.nb, T.packed_bytes(c))
        self.pk = guarded(dev, self.nb)
        self.st = VP(torch.cuda.current_stream().cuda_stream)
        assert w.dtype == torch.float32 and w.is_contiguous()
        if c.pk == 'f16x2':
            L.check(self.lib.pcgan_conv2d_hsplit_pack(ref, self.pass_, ptr(w), ptr(self.pk), self.st), 'conv2d_hsplit_pack')
        elif c.pass_ == 'fwd':
            L.check(self.lib.pcgan_conv2d_bsplit_pack(ref, ptr(w), ptr(self.pk), self.st), 'conv2d_bsplit_pack')
        else:
            L.check(self.lib.pcgan_conv2d_bsplit_dgrad_pack(ref, ptr(w), ptr(self.pk), self.st), 'conv2d_bsplit_dgrad_pack')

    def run(self, src, b=None, add=None, maxima=None, act=0, slope=0.0):
        """the call into a NaN-filled view between two guards; returns the view (as float64 on the CPU too) after checking the guards"""
        from pcgan_amd.hip import ops
        c, lib, L = self.c, self.lib, self.L
        shape = T.out_shape(c)
        dt = torch.bfloat16 if self.half else torch.float32
        nbytes = (2 if self.half else 4) * shape[0] * shape[1] * shape[2] * shape[3]
        big = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=self.dev)
        y = big[GUARD:GUARD + nbytes].view(dt).view(shape)
        y.fill_(float('nan'))
        assert src.dtype == dt and src.is_contiguous() and tuple(src.shape) == T.src_shape(c)
        ref = ctypes.byref(self.d)
        if c.pk == 'f16x2':
            if maxima is None:
                slots = int(lib.pcgan_absmax_slots(src.numel()))
                maxima = torch.full((slots,), float('nan'), device=self.dev)
                L.check(lib.pcgan_absmax(ptr(src), src.numel(), 0, ptr(maxima), slots, self.st), 'absmax')
            assert maxima.dtype == torch.float32 and maxima.is_contiguous()
            if c.pass_ == 'fwd':
                assert add is None
                L.check(lib.pcgan_conv2d_fwd_hsplit(ref, ptr(src), ptr(maxima), maxima.numel(), ptr(self.pk), ptr(b), ptr(y), act, slope,
                                                    self.st), 'conv2d_fwd_hsplit')
            elif add is None:
                assert b is None and act == 0
                L.check(lib.pcgan_conv2d_bwd_data_hsplit(ref, ptr(src), ptr(maxima), maxima.numel(), ptr(self.pk), ptr(y), self.st),
                        'conv2d_bwd_data_hsplit')
            else:
                assert b is None and act == 0 and add.is_contiguous() and tuple(add.shape) == shape
                L.check(lib.pcgan_conv2d_bwd_data_hsplit_add(ref, ptr(src), ptr(maxima), maxima.numel(), ptr(self.pk), ptr(add), ptr(y),
                                                             self.st), 'conv2d_bwd_data_hsplit_add')
        elif c.pass_ == 'fwd':
            assert add is None and maxima is None
            L.check(lib.pcgan_conv2d_fwd_bsplit(ref, ptr(src), ptr(self.pk), ptr(b), ptr(y), act, slope, self.st), 'conv2d_fwd_bsplit')
        else:
            assert add is None and maxima is None and b is None and act == 0
            L.check(lib.pcgan_conv2d_bwd_data_bsplit(ref, ptr(src), ptr(self.pk), ptr(y), self.st), 'conv2d_bwd_data_bsplit')
        if c.pk != 'f16x2':      # the launch record of the bsplit entries: the window kernel, not the per-tap one
            rec = ops.bsplit_last_launch()
            assert (rec['kernel'], rec['mode'], rec['bm']) == (1, 0 if c.pass_ == 'fwd' else 1, 256), rec
        torch.cuda.synchronize()
        assert bool((big[:GUARD] == 0xFF).all()) and bool((big[GUARD + nbytes:] == 0xFF).all()), 'the call wrote outside its output'
        assert bool((self.pk[self.nb:] == 0xFF).all()), 'the pack wrote behind the %d bytes it asked for' % self.nb
        yc = y.double().cpu()
        assert bool(torch.isfinite(yc).all()), 'elements nobody wrote, or not finite: %d' % int((~torch.isfinite(yc)).sum())
        assert ops.nonfinite_count(reset=False) == 0, 'the non-finite counter moved'
        return y, yc


def _to(dev, c, t):
    if t is None:
        return None
    return t.to(dev).to(torch.bfloat16 if c.pk == 'bf16' else torch.float32).contiguous()


def _dev(dev, c, d):
    f32 = lambda t: t.to(dev).contiguous() if t is not None else None
    return _to(dev, c, d.src), f32(d.w), f32(d.b), _to(dev, c, d.add)


def test_window_kernel_is_the_default_of_the_bsplit_entries():
    from pcgan_amd.hip import lib as L
    assert L.get_option('bsplit_halo') == 1


@pytest.mark.parametrize('name', NAMES)
def test_case(dev, name):
    c = T.BY_NAME[name]
    d = T.data(c)
    E, bound, want = T.bounds(c)
    if c.kind == 'signed':
        worst, allowed = T.condition(c)
        assert worst < allowed, 'the largest bound %.4f would not catch one lost term' % worst
    else:
        assert T.quanta(c) < 2.0 ** 24
        want = T.exact_expected(c)
    src, w, b, add = _dev(dev, c, d)
    assert bool((src.double().cpu() == d.src.double()).all()), 'the operand is no number of the storage type'
    y, yc = _Call(dev, c, w).run(src, b, add, None, c.act, T.slope_of(c))
    SEEN[name] = (c.sect, T.inst(c))
    err = (yc - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    rel = float((yc - want).norm() / want.norm())
    print('HALO %s %s: %s %s W %d; max |err| / bound %.4f; relative L2 %.3e; elements != reference %d' % (
        (c.sect, name) + T.inst(c) + (ratio, rel, int((yc != want).sum()))))
    if c.kind == 'signed':
        assert bool((err <= bound).all()), '%d element(s) outside the bound, worst %.3g x the bound at %r' % (
            int((err > bound).sum()), ratio, where(err / bound.clamp_min(1e-300)))
    else:
        assert bool((yc == want).all()), '%d element(s) not exact, the first worst at %r: %r, reference %r' % (
            int((yc != want).sum()), where(err), float(yc[where(err)]), float(want[where(err)]))


# ---- C. scales and ranges (f16x2) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pass_,n', [('fwd', n) for n in T.MAXPOS_N] + [('dgrad', n) for n in (1, 5, 2049, 8203)])
def test_maximum_in_every_slot(dev, pass_, n):
    """sx comes from thread_max_of_partials (512 threads) over a maxima array of the caller's making: the true maximum (2^15 - 1 forward,
    2^13 - 1 in the data gradient; every other magnitude and every other slot is 16) in the first slot, the last, the last lane of the
    first 4-in-flight round, the second and the third load in flight and the last float4 (split_arith.maxima_slots), with the array 0, 4, 8
    and 12 bytes off a 16-byte boundary.  A missed slot scales the
    pinned element past fp16: the result is not the exact one and the non-finite counter moves.  (The data gradient shares the code:
    four lengths.)"""
    c = T.MAXPOS[pass_]
    d = T.data(c)
    want = T.exact_expected(c)
    top = 2.0 ** c.bits - 1
    assert float(d.src.abs().max()) == top and float(d.src.abs().flatten().topk(2).values[1]) <= 16.0 and T.quanta(c) < 2.0 ** 24
    src, w, b, _ = _dev(dev, c, d)
    call = _Call(dev, c, w)
    base = torch.empty(n + 4, dtype=torch.float32, device=dev)
    assert base.data_ptr() % 16 == 0
    for off in range(4):
        for slot in T.maxima_slots(n):
            base.fill_(16.0)
            m = base[off:off + n]
            m[slot] = top
            assert m.data_ptr() % 16 == 4 * off and m.numel() == n
            y, yc = call.run(src, b, None, m, c.act, T.slope_of(c))
            assert bool((yc == want).all()), 'n %d, slot %d, %d bytes off: %d element(s) wrong' % (n, slot, 4 * off, int((yc != want).sum()))


@pytest.mark.parametrize('pass_,width', [('fwd', 32), ('fwd', 64), ('dgrad', 32), ('dgrad', 64)])
def test_all_zero_input(dev, pass_, width):
    """pow2_scale(0) = 1: an all-zero input gives act(bias) exactly in every element (the addend, or zeros, in the data gradient)"""
    c = T.BY_NAME['A.%s-f16x2-%s' % (pass_, {('fwd', 32): '1x32x4x32-m256-bias-relu', ('fwd', 64): '2x32x4x64-m256-bias-lrelu',
                                           ('dgrad', 32): '1x32x4x32-m256-add', ('dgrad', 64): '2x32x4x64-m256-add'}[(pass_, width)])]
    d = T.data(c)
    src, w, b, add = _dev(dev, c, d)
    src = torch.zeros_like(src)
    call = _Call(dev, c, w)
    zeros = torch.zeros(3, dtype=torch.float32, device=dev)
    if pass_ == 'fwd':
        for act in (0, 1, 2):
            y, yc = call.run(src, b, None, zeros, act, T.SLOPE)
            want = T.R.activation(d.b, act, T.SLOPE).view(1, -1, 1, 1).expand(T.out_shape(c)).double()
            assert bool((yc == want).all()), 'act %d: %d element(s) differ from act(bias)' % (act, int((yc != want).sum()))
    else:
        assert bool((call.run(src, None, add, zeros)[1] == d.add.double()).all())
        assert bool((call.run(src, None, None, zeros)[1] == 0).all())


@pytest.mark.parametrize('pass_', ['fwd', 'dgrad'])
def test_one_all_zero_weight_row(dev, pass_):
    """an all-zero row of the pass's weight matrix (row maximum 0, scale 1): that channel equals its bias (forward) or zero (data gradient)
    exactly, the others stay inside the section A bound"""
    c = T.BY_NAME['A.fwd-f16x2-1x32x4x32-m256-bias-relu']._replace(act=0) if pass_ == 'fwd' else T.BY_NAME['A.dgrad-f16x2-1x32x4x32-m256']
    d = T.data(c)
    w0 = d.w.clone()
    row = 37
    if pass_ == 'fwd':
        w0[row] = 0.0
    else:
        w0[:, row] = 0.0
    ref, A = T.reference(c, d.src, w0, d.b)
    E, bound, want = T.bounds(c, A, ref)
    y, yc = _Call(dev, c, w0.to(dev).contiguous()).run(d.src.to(dev), d.b.to(dev) if d.b is not None else None)
    assert bool((yc[:, row] == (float(d.b[row]) if d.b is not None else 0.0)).all())
    assert bool(((yc - want).abs() <= bound).all())


@pytest.mark.parametrize('kind', T.RANGE_KINDS)
@pytest.mark.parametrize('pass_,width', [('fwd', 32), ('fwd', 64), ('dgrad', 32), ('dgrad', 64)])
def test_operand_ranges(dev, monkeypatch, pass_, width, kind):
    """randn operands over twelve decades inside one tensor, times 1e12 / 1e8, and times 1e-30 / 1e-6: per produced channel the rule of
    tests/test_gpu_bf16x6.py, relative L2 against float64 < 3e-6 and < 2 x the fp32 route's own error on the same inputs + 5e-7"""
    from pcgan_amd.hip import ops
    c = T.RANGE[(pass_, width)]
    N, G, H, W, M = c.shape
    src, w, ref = T.range_data(c, kind)
    assert bool(torch.isfinite(src).all()) and float(ref.abs().max()) > 1e-37      # (the true values are fp32 numbers)
    sd, wd = src.to(dev).contiguous(), w.to(dev).contiguous()
    y, yc = _Call(dev, c, wd).run(sd)
    e16 = T.per_row_rel(yc, ref)
    monkeypatch.setattr(ops, 'HSPLIT', False)
    monkeypatch.setattr(ops, 'BF16X6', False)      # the fp32 MFMA kernels on the same data
    key = ('fwd' if pass_ == 'fwd' else 'dgrad', 'packed')
    n0 = ops.ROUTE_STATS.get(key, 0)
    if pass_ == 'fwd':
        y32 = ops.conv2d_fwd(sd, wd, None, 1, 1, 1, pack_cache={})
    else:
        y32 = ops.conv2d_bwd_data(sd, wd, (H, W), 1, 1, 1, pack_cache={})
    assert ops.ROUTE_STATS.get(key, 0) == n0 + 1, 'the comparison did not run on the fp32 route: %r' % (ops.ROUTE_STATS,)
    e32 = T.per_row_rel(y32.double().cpu(), ref)
    print('HALO C range %s %d %s: relative L2 per channel %.3e .. %.3e (fp32 route %.3e .. %.3e); zeros written %d of %d' % (
        pass_, width, kind, float(e16.min()), float(e16.max()), float(e32.min()), float(e32.max()), int((yc == 0).sum()), yc.numel()))
    worst = int((e16 - 2 * e32).argmax())
    assert bool((e16 < 3e-6).all()), 'channel %d: %.3e' % (int(e16.argmax()), float(e16.max()))
    assert bool((e16 < 2 * e32 + 5e-7).all()), 'channel %d: %.3e against %.3e on the fp32 route' % (worst, float(e16[worst]), float(e32[worst]))
    assert ops.nonfinite_count(reset=False) == 0


@pytest.mark.parametrize('which', ['constant', 'one_plane'])
@pytest.mark.parametrize('width', [32, 64])
def test_four_corner_sums_stay_in_fp16(dev, width, which):
    """a corner sum entry adds four dy elements BEFORE the split: with dy = 1 - 2^-13 everywhere (or just in the sixteen corner sources of
    one plane) the sum scales to 4 x 16382 under pow2_scale(max |dy|), past fp16's 65504, so the high piece of a sum entry saturates there.
    Finite output inside the section A bound, counter at 0"""
    c = T.CORNER[width]
    dy, w, ref, A = T.corner_data(c, which)
    E, bound, want = T.bounds(c, A, ref)
    assert float(dy.abs().max()) == 1.0 - 2.0 ** -13
    y, yc = _Call(dev, c, w.to(dev).contiguous()).run(dy.to(dev).contiguous())
    err = (yc - want).abs()
    print('HALO C corner %d %s: max |err| / bound %.4f, relative L2 %.3e' % (width, which, float((err / bound).max()), float((yc - want).norm() / want.norm())))
    assert bool((err <= bound).all()), '%d element(s) outside the bound, the worst at %r' % (int((err > bound).sum()), where(err / bound))


def test_zz_every_instantiation_ran():
    """from the cases that ran in this process: all twelve instantiations in section A and in section B, when the whole file ran.  A
    selection (-k, one worker of several) is held to its own cases only; a process in which no case ran has nothing to check and says so"""
    coverage_gate(SEEN, NAMES, T.INSTANTIATIONS, 'AB', T.BY_NAME, T.inst, 'COVERAGE %-5s %-6s W %d: A %2d case(s), B %2d')
