"""GPU: the thin convolutions (csrc/thin_conv.hip: thin_conv_kernel<7,7,1>, <7,7,2>, <4,4,2>, thin_pack_kernel, and reflect_fold_kernel
behind the reflect data gradient) held to float64 element by element, kernel by kernel and host form by host form.

tests/test_gpu_thin.py judges ten layer-shaped cases by relative L2 and by max |err| against max |ref|: one wrong low piece in one window
position or one misplaced weight fragment is about 1e-6 of the norm and passes.  Here (tests/thin_cases.py: table, data, reference, bounds,
the conditions that make them bite; tests/test_thin_cases.py checks all of that and the library's predicates on the CPU) each case calls
pcgan_conv2d_thin_pack and pcgan_conv2d_fwd_thin / pcgan_conv2d_bwd_data_thin directly: the output is a NaN-filled view inside a larger
buffer with 4 KiB of 0xFF bytes in front and behind, the packed buffer and the workspace are the sizes the library names plus a 4 KiB 0xFF
tail; afterwards every output element is finite (ragged tiles included) and no guard byte has changed.  The case then runs again through
ops.conv2d_fwd / ops.conv2d_bwd_data with a pack cache: the route counter ('fwd' | 'dgrad', 'thin') goes up by one and the bits are the same.

A. lost, doubled or misplaced terms: signed data of magnitudes [0.75, 1.25], |y - ref| <= (2 (3 Kp + 8) 2^-24 + 2^-20) A per element with
   the largest bound of every case under half the smallest term.  Every accepted (kernel, form) pair, 1 .. 4 gathered channels, 64 .. 256
   produced channels, exact tiles, one row and column more, planes under a tile and under the filter, pads 0 .. 6, reflection where
   everything mirrors, folds from both sides, bias with each activation.
B. every piece on the right pair, exactly: integer data whose every partial sum is an fp32 number ('xlow': low pieces in the activation
   tensor; 'wlow': in the weights, rows spanning 2^-20 .. 2^20), out == ref in every element.
C. scales and ranges: the true maximum in every slot class of thread_max_of_partials (misaligned scalar path, 4-in-flight float4 loop,
   float4 remainder, scalar tail) at four pointer alignments; all-zero input; all-zero filter rows; operands spanning many decades, times
   1e12 / 1e8, times 1e-30 / 1e-4.

Measured on an MI355X (256 CUs), recorded and not gated beyond the clauses above:
  section  cases  max |err| / bound     relative L2            what
    A       31    0.0005 .. 0.0053      4.1e-8 .. 1.8e-7       every case inside its bound; largest condition 0.043 of the 0.281 allowed
                                                               (reflect gradient 1x64x6x7 at pad 5: up to 9 mirror images)
    B       14    0                     0                      every element exact, 'xlow' and 'wlow', all six (kernel, form) pairs: the
                                                               premise that v_mfma_f32_32x32x16_f16 adds exactly when every partial sum is an
                                                               fp32 number holds on this chip
    C      132 launches of the maximum-slot case (33 slot placements x 4 alignments, 12 array lengths; from 4096 slots on also in the second
           and third of the four loads in flight): exact every time, sentinel at 0;
           4 all-zero inputs and the two all-zero filter rows: exact; 6 range cases: relative L2 per channel 8.4e-8 .. 2.0e-7 against
           5.8e-8 .. 2.8e-7 on the fp32-MFMA route (wide_range 8.4e-8 .. 2.0e-7, huge 1.3e-7 .. 2.0e-7, tiny 1.3e-7 .. 1.9e-7)
  The bound of section A is a worst case over orders and signs, so the errors sit far inside it; what the gate buys is the condition: a
  lost, doubled or misplaced term is >= 2 x the bound in the element it belongs to.  A single wrong LOW piece is 2^-11 of a term and only
  section B (and the per-channel gates of C) sees it.
  Coverage, from the cases that ran (cases; M / 64; gathered channels):
    <7,7,1> fwd_zero       5   1, 2         3, 4
    <7,7,1> fwd_reflect    8   1, 2, 3, 4   1, 2, 3, 4
    <7,7,2> fwd_zero       6   1, 2, 3, 4   1, 2, 3, 4
    <4,4,2> fwd_zero       9   1, 2, 3, 4   1, 2, 3, 4
    <7,7,1> dgrad_zero     8   1, 2, 3, 4   1, 2, 3, 4
    <7,7,1> dgrad_reflect  9   1, 2         1, 2, 3, 4
  Found and fixed with these cases: the epilogue scaled back by 1 / (pow2_scale(rowmax) * sx).  With x near 1e-30 (sx at the 2^100 clamp)
  and filter rows near 1e-5 (2^30) the product is 2^130 = inf in fp32, the reciprocal 0, and the kernel wrote exact zeros (38016 of 38016
  elements in both `tiny` cases, relative L2 1.0, sentinel silent) where the true values, near 1e-34, are normal fp32 numbers.  The two
  reciprocals are now applied one after the other; no other result of the suite moved.  Everything else passes on the kernel as it was.
  Sensitivity, each edit on a scratch copy of the kernel, run once: dropping the (Al, Bh) product fails 21 cases of A, the 6 'wlow' cases
  of B and the 6 range cases; a zero stored to Wl[NPOS - 1] fails 3 'xlow' cases of B (the cases whose last window position is a real
  pixel with a live tap) and the 6 range cases, nothing in A; o0 and o1 swapped in the last stage fails 29 cases of A, 13 of B, all of
  the maximum-slot cases, the zero-row case and the range cases.
  Wall time of the file: 69 tests in 1.9 s, the slowest 0.7 s (the first launch of a process)."""
import ctypes

import pytest
import torch

import thin_cases as T
from gpu_direct import VP, GUARD, ptr, guarded, where

pytestmark = pytest.mark.gpu

NAMES = list(T.BY_NAME)
SEEN = {}      # case name -> (kernel, form, M / 64, gathered channels) of the cases that ran in this process


class _Call(object):
    """one packed weight tensor and the buffers of a direct call, guards included"""

    def __init__(self, dev, c, w):
        from pcgan_amd.hip import lib as L, ops
        self.lib, self.L, self.c, self.dev = L.load(), L, c, dev
        self.d = ops.make_desc(*c.geom)
        self.pass_ = L.PASS_FWD if c.pass_ == 'fwd' else L.PASS_BWD_DATA
        ref = ctypes.byref(self.d)
        assert self.lib.pcgan_conv2d_thin_supported(ref, self.pass_) == 1, 'not a thin-kernel shape: %r' % (c.geom,)
        self.nb = int(self.lib.pcgan_conv2d_thin_packed_bytes(ref, self.pass_))
        self.nws = int(self.lib.pcgan_conv2d_thin_workspace_bytes(ref, self.pass_))
        assert self.nb == T.packed_bytes(c) and self.nws == T.workspace_bytes(c)
        self.pk, self.ws = guarded(dev, self.nb), guarded(dev, self.nws)
        self.st = VP(torch.cuda.current_stream().cuda_stream)
        L.check(self.lib.pcgan_conv2d_thin_pack(ref, self.pass_, ptr(w), ptr(self.pk), self.st), 'conv2d_thin_pack')

    def run(self, src, b, maxima, act, slope):
        """the call into a NaN-filled view between two guards; returns the view after checking every guard"""
        c = self.c
        shape = T.out_shape(c)
        nbytes = 4 * shape[0] * shape[1] * shape[2] * shape[3]
        big = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=self.dev)
        y = big[GUARD:GUARD + nbytes].view(torch.float32).view(shape)
        y.fill_(float('nan'))
        assert maxima.dtype == torch.float32 and maxima.is_contiguous() and src.is_contiguous()
        ref = ctypes.byref(self.d)
        if c.pass_ == 'fwd':
            self.L.check(self.lib.pcgan_conv2d_fwd_thin(ref, ptr(src), ptr(maxima), maxima.numel(), ptr(self.pk), ptr(b), ptr(y), act, slope, self.st),
                         'conv2d_fwd_thin')
        else:
            assert b is None and act == 0
            self.L.check(self.lib.pcgan_conv2d_bwd_data_thin(ref, ptr(src), ptr(maxima), maxima.numel(), ptr(self.pk), ptr(y), ptr(self.ws), self.nws,
                                                             self.st), 'conv2d_bwd_data_thin')
        torch.cuda.synchronize()
        assert bool((big[:GUARD] == 0xFF).all()) and bool((big[GUARD + nbytes:] == 0xFF).all()), 'the call wrote outside its output'
        assert bool((self.pk[self.nb:] == 0xFF).all()), 'the pack wrote behind the %d bytes it asked for' % self.nb
        assert bool((self.ws[self.nws:] == 0xFF).all()), 'the call wrote behind the workspace it asked for (%d bytes)' % self.nws
        return y


def _amax1(src):
    return src.abs().amax().reshape(1).float().contiguous()


def _through_ops(c, src, w, b):
    """the same call through the host's routing with a pack cache; the thin route must be the one that runs"""
    from pcgan_amd.hip import ops
    N, C, H, W, K, Rr, S, stride, pad, pm = c.geom
    key = ('fwd' if c.pass_ == 'fwd' else 'dgrad', 'thin')
    n0 = ops.ROUTE_STATS.get(key, 0)
    if c.pass_ == 'fwd':
        y = ops.conv2d_fwd(src, w, b, stride, pad, pm, c.act, T.slope_of(c), pack_cache={})
    else:
        y = ops.conv2d_bwd_data(src, w, (H, W), stride, pad, pm, pack_cache={})
    torch.cuda.synchronize()
    assert ops.ROUTE_STATS.get(key, 0) == n0 + 1, 'the pack-cache call took another route: %r' % (ops.ROUTE_STATS,)
    return y


def _dev(dev, d):
    return d.src.to(dev).contiguous(), d.w.to(dev).contiguous(), (d.b.to(dev).contiguous() if d.b is not None else None)


@pytest.mark.parametrize('name', NAMES)
def test_case(dev, name):
    c = T.BY_NAME[name]
    assert T.classify(c.pass_, c.geom) == c.want
    d = T.data(c)
    E, bound, aref = T.bounds(c)
    if c.kind == 'signed':
        worst, allowed = T.condition(c)
        assert worst < allowed, 'the largest bound %.4f would not catch one lost term' % worst
    else:
        assert T.quanta(c) < 2.0 ** 24
    src, w, b = _dev(dev, d)
    y = _Call(dev, c, w).run(src, b, _amax1(src), c.act, T.slope_of(c))
    SEEN[name] = c.want + (T.rows_of(c) // 64, T.gathered(c))
    yc = y.double().cpu()
    finite = bool(torch.isfinite(yc).all())
    err = (yc - aref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if finite else float('nan')
    rel = float((yc - aref).norm() / aref.norm())
    print('THIN %s %s: %s %s M/64 %d G %d; max |err| / bound %.4f; relative L2 %.3e; elements != reference %d' % (
        (c.sect, name) + SEEN[name] + (ratio, rel, int((yc != aref).sum()))))
    assert finite, 'elements nobody wrote: %d' % int((~torch.isfinite(yc)).sum())
    if c.kind == 'signed':
        assert bool((err <= bound).all()), '%d element(s) outside the bound, worst %.3g x the bound at %r' % (
            int((err > bound).sum()), ratio, where(err / bound.clamp_min(1e-300)))
    else:
        assert bool((yc == aref).all()), '%d element(s) not exact, the first worst at %r: %r, reference %r' % (
            int((yc != aref).sum()), where(err), float(yc[where(err)]), float(aref[where(err)]))
    y2 = _through_ops(c, src, w, b)
    assert torch.equal(y2, y), 'direct and pack-cache calls differ in %d element(s)' % int((y2 != y).sum())


# ---- C. scales and ranges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', T.MAXPOS_N)
def test_maximum_in_every_slot(dev, n):
    """sx comes from thread_max_of_partials over a maxima array of the caller's making: the true maximum (2^15 - 1; every other magnitude and
    every other slot is 16) in the first slot, the last, the last lane of the 4-in-flight float4 loop, its second and third load and the last
    float4 (split_arith.maxima_slots), with the array 0,
    4, 8 and 12 bytes off a 16-byte boundary.  A missed slot scales 32767 by 2^9: fp16 overflows, the result is not the exact one and the
    non-finite sentinel counts it"""
    from pcgan_amd.hip import ops
    c = T.MAXPOS
    d = T.data(c)
    aref = T.bounds(c)[2]
    assert float(d.src.abs().max()) == 32767.0 and float(d.src.abs().flatten().topk(2).values[1]) <= 16.0 and T.quanta(c) < 2.0 ** 24
    src, w, b = _dev(dev, d)
    want = aref.float().to(dev)
    assert bool((want.double().cpu() == aref).all())
    y0 = _through_ops(c, src, w, b)          # (registers the non-finite sentinel with the library)
    assert torch.equal(y0, want)
    assert ops.nonfinite_count(reset=False) == 0
    call = _Call(dev, c, w)
    base = torch.empty(n + 4, dtype=torch.float32, device=dev)
    assert base.data_ptr() % 16 == 0
    for off in range(4):
        for slot in T.maxima_slots(n):
            base.fill_(16.0)
            m = base[off:off + n]
            m[slot] = 32767.0
            assert m.data_ptr() % 16 == 4 * off and m.numel() == n
            y = call.run(src, b, m, c.act, T.slope_of(c))
            assert torch.equal(y, want), 'n %d, slot %d, %d bytes off: %d element(s) wrong' % (n, slot, 4 * off, int((y != want).sum()))
    assert ops.nonfinite_count(reset=False) == 0


_ZERO_CASES = ['A.fwd_reflect-771-2x4x9x33-k64-p3-bias-relu', 'A.fwd_zero-772-2x3x17x65-k64-p3-bias-lrelu', 'A.fwd_zero-442-2x4x18x66-k64-p1-bias-lrelu',
               'A.dgrad_reflect-771-2x64x9x33-k3-p3']


@pytest.mark.parametrize('name', _ZERO_CASES)
def test_all_zero_input(dev, name):
    """pow2_scale(0) = 1: an all-zero input gives act(bias) exactly in every element (zeros for the data gradient, which has no bias)"""
    from oracle import ops_ref as R
    c = T.BY_NAME[name]
    d = T.data(c)
    src, w, b = _dev(dev, d)
    src = torch.zeros_like(src)
    call = _Call(dev, c, w)
    for act in ((0, 1, 2) if c.pass_ == 'fwd' else (0,)):
        y = call.run(src, b, torch.zeros(3, dtype=torch.float32, device=dev), act, T.SLOPE)
        want = R.activation(d.b, act, T.SLOPE).view(1, -1, 1, 1).expand(T.out_shape(c)) if b is not None else torch.zeros(T.out_shape(c))
        assert torch.equal(y.cpu(), want.contiguous()), 'act %d: %d element(s) differ from act(bias)' % (act, int((y.cpu() != want).sum()))


def test_all_zero_filter_rows(dev):
    """two all-zero rows of the weight matrix (row maximum 0, scale 1): those channels equal their bias exactly, the others stay inside
    the section A bound"""
    c = T.BY_NAME['A.fwd_reflect-771-2x4x9x33-k64-p3-bias-relu']._replace(act=0)
    d = T.data(c)
    w0 = d.w.clone()
    w0[5] = 0.0
    w0[40] = 0.0
    ref, A = T.reference(c, d.src, w0, d.b)
    E, bound, aref = T.bounds(c, A, ref)
    src, w, b = d.src.to(dev), w0.to(dev), d.b.to(dev)
    y = _Call(dev, c, w).run(src, b, _amax1(src), 0, 0.0)
    yc = y.cpu()
    for row in (5, 40):
        assert bool((yc[:, row] == d.b[row]).all())
    assert bool(((yc.double() - aref).abs() <= bound).all())
    assert torch.equal(_through_ops(c, src, w, b), y)


@pytest.mark.parametrize('kind', T.RANGE_KINDS)
@pytest.mark.parametrize('which', ['fwd_reflect', 'dgrad_reflect'])
def test_operand_ranges(dev, monkeypatch, which, kind):
    """randn operands spanning many decades, times 1e12 / 1e8, and times 1e-30 / 1e-4 (true values near 1e-34: normal fp32 numbers, the
    input's scale at the 2^100 clamp, the filter rows' at 2^30): per produced channel the route's gates, relative L2 < 3e-6 and <= 2 x the
    fp32-MFMA kernels' own error + 5e-7"""
    from pcgan_amd.hip import ops
    c = T.RANGE_FWD if which == 'fwd_reflect' else T.RANGE_DGRAD
    src, w, ref = T.range_data(c, kind)
    assert bool(torch.isfinite(src).all()) and float(ref.abs().max()) > 1e-37      # (the true values are fp32 numbers)
    sd, wd = src.to(dev).contiguous(), w.to(dev).contiguous()
    y = _Call(dev, c, wd).run(sd, None, _amax1(sd), 0, 0.0)
    yc = y.double().cpu()
    assert bool(torch.isfinite(yc).all())
    e16 = T.per_row_rel(yc, ref)
    assert torch.equal(_through_ops(c, sd, wd, None), y)
    N, C, H, W, K, Rr, S, stride, pad, pm = c.geom
    monkeypatch.setattr(ops, 'THIN', False)
    y32 = ops.conv2d_fwd(sd, wd, None, stride, pad, pm, 0, 0.0, pack_cache={}) if c.pass_ == 'fwd' else \
        ops.conv2d_bwd_data(sd, wd, (H, W), stride, pad, pm, pack_cache={})
    e32 = T.per_row_rel(y32.double().cpu(), ref)
    print('THIN C range %s %s: relative L2 per channel %.3e .. %.3e (fp32-MFMA route %.3e .. %.3e); zeros written %d of %d' % (
        which, kind, float(e16.min()), float(e16.max()), float(e32.min()), float(e32.max()), int((yc == 0).sum()), yc.numel()))
    worst = int((e16 - 2 * e32).argmax())
    assert bool((e16 < 3e-6).all()), 'channel %d: %.3e' % (int(e16.argmax()), float(e16.max()))
    assert bool((e16 <= 2 * e32 + 5e-7).all()), 'channel %d: %.3e against %.3e on the fp32-MFMA route' % (worst, float(e16[worst]), float(e32[worst]))
    assert ops.nonfinite_count(reset=False) == 0


def test_zz_every_kernel_and_form_ran():
    """from the cases that ran in this process: every (kernel, host form) pair the library accepts, with every M / 64 in 1 .. 4 and every
    gathered channel count in 1 .. 4, when the whole file ran.  A selection (-k, one worker of several) is held to its own cases only; a
    process in which no case ran has nothing to check and says so"""
    assert SEEN, 'no case of this file ran in this process before this test: nothing was checked (run the whole file in one process)'
    for pair in T.ACCEPTED:
        rows = sorted({s[2] for s in SEEN.values() if s[:2] == pair})
        chans = sorted({s[3] for s in SEEN.values() if s[:2] == pair})
        print('COVERAGE %-8s %-14s %2d case(s); M / 64 %r; gathered channels %r' % (pair + (sum(1 for s in SEEN.values() if s[:2] == pair), rows, chans)))
    want = {T.BY_NAME[n].want for n in SEEN}
    assert {s[:2] for s in SEEN.values()} == want
    if len(SEEN) == len(NAMES):
        assert {s[:2] for s in SEEN.values()} == set(T.ACCEPTED), 'a (kernel, form) pair no case reached'
        assert {s[2] for s in SEEN.values()} == {1, 2, 3, 4} and {s[3] for s in SEEN.values()} == {1, 2, 3, 4}
        for k in T.KERNELS:
            assert {s[3] for s in SEEN.values() if s[0] == k} == {1, 2, 3, 4}, 'kernel %s: a gathered channel count never ran' % k
