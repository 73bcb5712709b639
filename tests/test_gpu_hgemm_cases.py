"""GPU: the packed implicit GEMM on the f16 / bf16 matrix pipe (csrc/hgemm.hip: hgemm_kernel, 3 modes x 4 tiles x 2 storage types, and
hgemm_presplit_kernel) held to float64 element by element, instantiation by instantiation.

tests/test_gpu_hgemm.py judges its fp32 tensors by norms on randn data: one wrong low piece, one misplaced weight fragment or one tap
read from the wrong table row is about 1e-6 of the norm and passes.  Here (tests/hgemm_cases.py: table, data, reference, bounds, the
conditions that make them bite, the arithmetic restated; tests/test_hgemm_cases.py checks all of that on the CPU) each case calls the C-ABI
directly -- pcgan_conv2d_hgemm_pack, then pcgan_conv2d_fwd_packed_hsplit / pcgan_conv2d_bwd_data_packed_hsplit for fp32 tensors;
pcgan_conv2d_pack_weights, then pcgan_conv2d_fwd_packed / pcgan_conv2d_bwd_data_packed with a bf16 descriptor -- under a forced tile and
K split, into a NaN-filled view between two 4 KiB guards of 0xFF, with a packed buffer, a workspace and a row-maxima array of the sizes
the library names under the forced options plus a 0xFF tail.  Afterwards every output element is finite, no guard byte has changed, the
non-finite counter has not moved and pcgan_igemm_last_launch equals the record the case names, one sequence number on.  The same case
then runs through ops.conv2d_fwd / ops.conv2d_bwd_data with a fresh pack cache: the route counter moves by one and the bits equal the
direct call's.

A. lost, doubled or misplaced terms: signed data of magnitudes [0.75, 1.25], per element inside the bound of the storage type, the largest
   bound of every case under half the smallest term.  Every instantiation at M in {33, 64, 65, 128, 129, 136} (BM = 128: from 65 on), at
   BP - 1, BP, BP + 1 and 25 pixels, whole and split; filters 1x1 .. 5x5 and 3x5 / 2x3; 16, 32, 48 channels at 1x1 (one, two, three stages);
   strides 1, 2, 4 (the data gradient of 5x5 stride 4: 16 phases); zero padding 0 .. R - 1 at 2x2, 3x3, 4x4, 5x5; reflection up to pad H - 1 and planes under the
   filter; a bias with each activation forward and a bias in the data gradient; the split with an empty last slice, a short one and slices
   that begin inside a chunk; pixels no phase writes exactly +0 (and the call with a bias refused); a forced 128-row tile on <= 64 rows and
   a forced split past stages / 4 run clamped and say so in the record.
B. every piece on the right pair, every stage and slice exactly once: integer data whose every partial sum is an fp32 number ('xlow',
   'wlow'), out == ref in every element, on all 24 instantiations whole and split and again on the 1-, 2-, 3-stage, odd-stage, split and
   16-phase shapes.
C. scales and ranges (fp32 tensors): the true maximum in every slot class of thread_max_of_partials at 256 threads and four pointer
   alignments; all-zero input; one all-zero weight row, on exact data exact in every element; operands over twelve decades, times 1e12 / 1e8, times 1e-30 / 1e-6 per produced
   channel against float64 and against the fp32 route.
D. the bytes pcgan_conv2d_hgemm_pack writes against the restatement, the row maxima, the tail.

Measured on an MI355X (256 CUs), recorded and not gated beyond the clauses above:
  section  cases  max |err| / bound         relative L2            what
    A       451   fp32  0.0002 .. 0.0136    6.1e-8 .. 2.4e-7    every case inside its bound; largest condition 0.061 of the 0.281 allowed (16
            338   bf16  0.83   .. 0.992     1.3e-3 .. 1.7e-3    channels x 5x5), 0.234 for bf16 tensors, where half a bf16 ulp of the result is
                                                                nearly all of the bound and the rounding reaches it
    B       145   fp32  0                   0                   every element exact: 145 'xlow', 135 'wlow'; v_mfma_f32_32x32x16_f16 and _bf16
            135   bf16  0                   0                   add exactly when every partial sum is an fp32 number
    C       180 launches of the maximum-slot cases (33 slot placements over 12 array lengths forward, 12 over 4 in the data gradient, x 4
            alignments; from 4096 slots on also in the second and third of the four loads in flight): exact every time, counter at 0;
            4 launches on all-zero input: exact; one all-zero weight row: on exact data (4 cases: each pass on a 64 x 128 and a 128 x 64
            tile) every element exact, on signed data (2 cases) the row exact and the rest inside the section A bound; 12 range
            cases, relative L2 per channel 9.4e-8 .. 2.7e-7 against 1.1e-7 .. 3.8e-7 on the fp32 route (wide_range 9.4e-8 .. 2.7e-7 |
            1.1e-7 .. 3.0e-7, huge 1.6e-7 .. 2.5e-7 | 2.3e-7 .. 3.8e-7, tiny 1.6e-7 .. 2.4e-7 | 2.3e-7 .. 3.7e-7), no zero written
    D       10 packs (4 integer, 4 'wlow', 2 randn): every byte as restated, the row maxima equal, nothing behind the image
    the two calls with a bias over uncovered phases: refused with the library's message
  Coverage, from the cases that ran (cases in A, in B), BM x BP:
                    128 x 128   128 x 64    64 x 128    64 x 64
    fwd_zero    fp32  39, 12     38, 10     42, 12     45, 10
                bf16  27, 10     27, 10     30, 10     34, 10
    fwd_reflect fp32  37, 10     32, 10     34, 10     36, 13
                bf16  31, 10     26, 10     28, 10     29, 11
    dgrad       fp32  37, 15     36, 15     37, 14     38, 14
                bf16  26, 13     25, 13     27, 14     28, 14
  No case failed on the kernel as it is: all 1069 cases of A and B, the production path bit-identical to the direct call in every one.
  Sensitivity: a kernel made wrong on purpose is not run on the shared GPU machines, so ten faults were applied to the torch restatement
  of the kernel's arithmetic (hgemm_cases.emulate) and the gates of both sections evaluated on its result, on the 485 cases of the table
  that differ in section, instantiation, data kind or pipeline edge (tests/test_hgemm_cases.py; cases the gate fails of those the fault
  applies to):
    fault                                     A signed      B wlow        B xlow
    (l,h) product dropped                     100 of 105    70 of 70      0 of 75     (fp32 tensors; x in {-1, 0, 1} has no low piece ...
    (h,l) product dropped                     100 of 105    0 of 70       75 of 75     ... and neither have weights in {-1, 0, 1})
    two taps swapped for one pixel            108 of 125    60 of 61      70 of 71    (not caught where both taps fall into the padding)
    four channels of one pixel zero, 1 stage  188 of 205    134 of 135    144 of 145  (likewise)
    last live stage read through row T        205 of 205    135 of 135    145 of 145
    iswS[ml] from the next row                0 of 105      70 of 70      0 of 75     (rows of one scale in A and 'xlow': 'wlow' is there for it)
    dead stage runs the first stage again     153 of 153    109 of 109    121 of 121  (cases with an odd stage count)
    slice boundary moved, a stage doubled     37 of 37      29 of 29      29 of 29    (split cases)
    slice boundary moved, a stage lost        37 of 37      29 of 29      29 of 29
    bias added in every slice                 37 of 37      --            29 of 29
  A dropped piece product needs the data kind whose low pieces it carries ('wlow' for (l,h), 'xlow' for (h,l)) and the row-scale fault
  needs the scaled rows of 'wlow'; every other fault fails all three kinds.  In section A a dropped low-piece product fails too: the bound, 5e-5 of the sum of magnitudes at 144 terms, is under the 2^-12 of a term
  that a low piece carries once the term count is small.
  Wall time of the file: 1118 tests in 3.9 s, the slowest 0.9 s (the first launch of a process)."""
import ctypes

import pytest
import torch

import hgemm_cases as T
from gpu_direct import VP, GUARD, ptr, guarded, where, bits, coverage_gate

pytestmark = pytest.mark.gpu

NAMES = list(T.BY_NAME)
SEEN = {}      # case name -> (section, instantiation) of the cases that ran in this process


@pytest.fixture
def force():
    """sets the library's "hgemm_tile" / "hgemm_ks" options (cached launch plans hold workspace sizes that depend on them: dropped on
    every change) and restores the heuristic afterwards"""
    from pcgan_amd.hip import lib as L, ops

    def set_(tile, ks):
        L.set_option('hgemm_tile', tile)
        L.set_option('hgemm_ks', ks)
        ops.clear_plans()
    try:
        yield set_
    finally:
        L.set_option('hgemm_tile', 0)
        L.set_option('hgemm_ks', 0)
        ops.clear_plans()


class _Call(object):
    """one packed weight tensor and the buffers of a direct call under the options as they stand, guards included"""

    def __init__(self, dev, c, w):
        from pcgan_amd.hip import lib as L, ops
        self.lib, self.L, self.c, self.dev = L.load(), L, c, dev
        self.d = ops.make_desc(*c.geom, dtype=L.BF16 if c.half else L.F32)
        self.pass_ = L.PASS_FWD if c.pass_ == 'fwd' else L.PASS_BWD_DATA
        ops._sentinel()      # (registers the non-finite counter with the library, once)
        ref = ctypes.byref(self.d)
        self.M = T.shapes(c)[2]
        assert T.supported(c.geom, c.pass_), 'no shape of the packed implicit GEMM'
        assert bool(self.lib.pcgan_conv2d_hgemm_supported(ref, self.pass_)) == (not c.half), 'the fp32 entry points take fp32 descriptors only'
        self.nb = int(self.lib.pcgan_conv2d_packed_bytes(ref, self.pass_))
        self.wsb = int(self.lib.pcgan_conv2d_workspace_bytes(ref, self.pass_))
        image = 4 * sum(self.M * p.Kp for p in T.hgemm_plan(c).phases)
        assert self.nb >= image and self.wsb >= self.nb
        self.pk, self.ws, self.rm = guarded(dev, self.nb), guarded(dev, self.wsb), guarded(dev, 4 * self.M)
        self.rowmax = self.rm[:4 * self.M].view(torch.float32)
        self.st = VP(torch.cuda.current_stream().cuda_stream)
        assert w.dtype == torch.float32 and w.is_contiguous()
        if c.half:
            L.check(self.lib.pcgan_conv2d_pack_weights(ref, self.pass_, ptr(w), ptr(self.pk), self.st), 'conv2d_pack_weights')
        else:
            L.check(self.lib.pcgan_conv2d_hgemm_pack(ref, self.pass_, ptr(w), ptr(self.rowmax), ptr(self.pk), self.st), 'conv2d_hgemm_pack')

    def run(self, src, b=None, maxima=None, act=0, slope=0.0, want=None):
        """the call into a NaN-filled view between two guards; returns the view (as float64 on the CPU too) after checking the guards,
        the counter and the launch record"""
        from pcgan_amd.hip import ops
        c, lib, L = self.c, self.lib, self.L
        sshape, shape, M = T.shapes(c)
        dt = torch.bfloat16 if c.half else torch.float32
        nbytes = (2 if c.half else 4) * shape[0] * shape[1] * shape[2] * shape[3]
        big = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=self.dev)
        y = big[GUARD:GUARD + nbytes].view(dt).view(shape)
        y.fill_(float('nan'))
        assert src.dtype == dt and src.is_contiguous() and tuple(src.shape) == sshape
        ref = ctypes.byref(self.d)
        seq0 = ops.igemm_last_launch()['seq']
        if not c.half:
            if maxima is None:
                slots = int(lib.pcgan_absmax_slots(src.numel()))
                maxima = torch.full((slots,), float('nan'), device=self.dev)
                L.check(lib.pcgan_absmax(ptr(src), src.numel(), 0, ptr(maxima), slots, self.st), 'absmax')
            assert maxima.dtype == torch.float32 and maxima.is_contiguous()
            if c.pass_ == 'fwd':
                L.check(lib.pcgan_conv2d_fwd_packed_hsplit(ref, ptr(src), ptr(maxima), maxima.numel(), ptr(self.pk), ptr(self.rowmax), ptr(b),
                                                           ptr(y), act, slope, ptr(self.ws), self.wsb, self.st), 'conv2d_fwd_packed_hsplit')
            else:
                assert act == 0
                L.check(lib.pcgan_conv2d_bwd_data_packed_hsplit(ref, ptr(src), ptr(maxima), maxima.numel(), ptr(self.pk), ptr(self.rowmax),
                                                                ptr(b), ptr(y), ptr(self.ws), self.wsb, self.st), 'conv2d_bwd_data_packed_hsplit')
        elif c.pass_ == 'fwd':
            L.check(lib.pcgan_conv2d_fwd_packed(ref, ptr(src), ptr(self.pk), ptr(b), ptr(y), act, slope, ptr(self.ws), self.wsb, self.st),
                    'conv2d_fwd_packed')
        else:
            assert act == 0
            L.check(lib.pcgan_conv2d_bwd_data_packed(ref, ptr(src), ptr(self.pk), ptr(b), ptr(y), ptr(self.ws), self.wsb, self.st),
                    'conv2d_bwd_data_packed')
        torch.cuda.synchronize()
        rec = ops.igemm_last_launch()
        assert bool((big[:GUARD] == 0xFF).all()) and bool((big[GUARD + nbytes:] == 0xFF).all()), 'the call wrote outside its output'
        assert bool((self.pk[self.nb:] == 0xFF).all()), 'the pack wrote behind the %d bytes it asked for' % self.nb
        assert bool((self.ws[self.wsb:] == 0xFF).all()), 'the call wrote behind the %d bytes of workspace it asked for' % self.wsb
        assert bool((self.rm[4 * self.M:] == 0xFF).all()), 'the pack wrote behind the %d row maxima' % self.M
        yc = y.double().cpu()
        assert bool(torch.isfinite(yc).all()), 'elements nobody wrote, or not finite: %d' % int((~torch.isfinite(yc)).sum())
        assert ops.nonfinite_count(reset=False) == 0, 'the non-finite counter moved'
        want = c.want if want is None else want
        got = (rec['form'], rec['mode'], rec['bm'], rec['bp'], rec['ks'], rec['nphase'])
        assert got == tuple(want), 'launched %r, the case names %r' % (got, want)
        assert rec['seq'] == seq0 + 1, 'exactly one implicit-GEMM launch per call: %d -> %d' % (seq0, rec['seq'])
        return y, yc


def _dev(dev, c, d):
    dt = torch.bfloat16 if c.half else torch.float32
    src = d.src.to(dev).to(dt).contiguous()
    assert bool((src.double().cpu() == d.src.double()).all()), 'the operand is no number of the storage type'
    return src, d.w.to(dev).contiguous(), (d.b.to(dev).contiguous() if d.b is not None else None)


def _through_ops(c, src, w, b):
    """the same case on the production path with a fresh pack cache: (output, the routes counted)"""
    from pcgan_amd.hip import ops
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    r0 = dict(ops.ROUTE_STATS)
    if c.pass_ == 'fwd':
        y = ops.conv2d_fwd(src, w, b, st, pad, pm, c.act, T.slope_of(c), pack_cache={})
    else:
        y = ops.conv2d_bwd_data(src, w, (H, W), st, pad, pm, bias=b, pack_cache={})
    torch.cuda.synchronize()
    return y, {k: v - r0.get(k, 0) for k, v in ops.ROUTE_STATS.items() if v != r0.get(k, 0)}


@pytest.mark.parametrize('name', NAMES)
def test_case(dev, force, name):
    from pcgan_amd.hip import ops
    c = T.BY_NAME[name]
    d = T.data(c)
    pl = T.hgemm_plan(c)
    assert T.record(pl) == c.want
    E, bound, want = T.bounds(c)
    if c.kind == 'signed':
        worst, allowed = T.condition(c)
        assert worst < allowed, 'the largest bound %.4f would not catch one lost term' % worst
    else:
        assert T.quanta(c) < 2.0 ** 24
        want = T.exact_expected(c)
    src, w, b = _dev(dev, c, d)
    force(c.tile, c.ks)
    y, yc = _Call(dev, c, w).run(src, b, None, c.act, T.slope_of(c))
    SEEN[name] = (c.sect, T.inst(c))
    err = (yc - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if c.kind == 'signed' else 0.0
    rel = float((yc - want).norm() / want.norm())
    print('HGEMM %s %s: %s %dx%d %s ks %d; max |err| / bound %.4f; relative L2 %.3e; elements != reference %d' % (
        (c.sect, name) + T.inst(c) + (pl.ks, ratio, rel, int((yc != want).sum()))))
    if c.kind == 'signed':
        assert bool((err <= bound).all()), '%d element(s) outside the bound, worst %.3g x the bound at %r' % (
            int((err > bound).sum()), ratio, where(err / bound.clamp_min(1e-300)))
        if pl.need_zero:
            un = d.A == 0
            assert bool(un.any()) and bool((yc[un] == 0).all()) and not bool(torch.signbit(yc[un]).any()), 'a pixel no phase writes is not +0'
    else:
        assert bool((yc == want).all()), '%d element(s) not exact, the first worst at %r: %r, reference %r' % (
            int((yc != want).sum()), where(err), float(yc[where(err)]), float(want[where(err)]))
    seq0 = ops.igemm_last_launch()['seq']
    y2, routes = _through_ops(c, src, w, b)
    assert routes == {(c.pass_, 'packed' if c.half else 'hgemm'): 1}, routes
    rec = ops.igemm_last_launch()
    assert rec['seq'] == seq0 + 1 and (rec['form'], rec['mode'], rec['bm'], rec['bp'], rec['ks'], rec['nphase']) == c.want, rec
    assert torch.equal(bits(y2), bits(y)), 'the production path differs from the direct call in %d element(s)' % int((bits(y2) != bits(y)).sum())


@pytest.mark.parametrize('i', range(len(T.NEED_ZERO_REFUSED)))
def test_bias_with_uncovered_phases_is_refused(dev, force, i):
    """a data gradient with pixels that no phase writes (1x1 stride 2; 3x3 stride 4) would miss the bias there: the call says so"""
    c = T.NEED_ZERO_REFUSED[i]
    d = T.data(c)
    assert d.b is not None and T.hgemm_plan(c).need_zero
    src, w, b = _dev(dev, c, d)
    force(c.tile, c.ks)
    call = _Call(dev, c, w)
    with pytest.raises(RuntimeError, match='bias with uncovered phases'):
        call.run(src, b)


# ---- C. scales and ranges (fp32 tensors) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pass_,n', [('fwd', n) for n in T.MAXPOS_N] + [('dgrad', n) for n in (1, 5, 1025, 4107)])
def test_maximum_in_every_slot(dev, force, pass_, n):
    """sx comes from thread_max_of_partials (256 threads) over a maxima array of the caller's making: the true maximum (2^15 - 1; every
    other magnitude and every other slot is 16) in the first slot, the last, the last lane of the first 4-in-flight round and the last
    float4, with the array 0, 4, 8 and 12 bytes off a 16-byte boundary (the misaligned scalar loop).  A missed slot scales the pinned
    element past fp16: the result is not the exact one and the non-finite counter moves.  (The data gradient shares the code: four
    lengths.)"""
    c = T.MAXPOS[pass_]
    d = T.data(c)
    want = T.exact_expected(c)
    top = 2.0 ** 15 - 1
    assert float(d.src.abs().max()) == top and float(d.src.abs().flatten().topk(2).values[1]) <= 16.0 and T.quanta(c) < 2.0 ** 24
    src, w, b = _dev(dev, c, d)
    force(c.tile, c.ks)
    call = _Call(dev, c, w)
    base = torch.empty(n + 4, dtype=torch.float32, device=dev)
    assert base.data_ptr() % 16 == 0
    for off in range(4):
        for slot in T.maxima_slots(n):
            base.fill_(16.0)
            m = base[off:off + n]
            m[slot] = top
            assert m.data_ptr() % 16 == 4 * off and m.numel() == n
            y, yc = call.run(src, b, m, c.act, T.slope_of(c))
            assert bool((yc == want).all()), 'n %d, slot %d, %d bytes off: %d element(s) wrong' % (n, slot, 4 * off, int((yc != want).sum()))


@pytest.mark.parametrize('pass_', ['fwd', 'dgrad'])
def test_all_zero_input(dev, force, pass_):
    """pow2_scale(0) = 1: an all-zero input gives act(bias) exactly in every element"""
    c = T.ZERO[pass_]
    d = T.data(c)
    assert d.b is not None
    src, w, b = _dev(dev, c, d)
    src = torch.zeros_like(src)
    force(c.tile, c.ks)
    call = _Call(dev, c, w)
    zeros = torch.zeros(3, dtype=torch.float32, device=dev)
    for act in ((0, 1, 2) if pass_ == 'fwd' else (0,)):
        y, yc = call.run(src, b, zeros, act, T.SLOPE)
        want = T.R.activation(d.b, act, T.SLOPE).view(1, -1, 1, 1).expand(T.shapes(c)[1]).double()
        assert bool((yc == want).all()), 'act %d: %d element(s) differ from act(bias)' % (act, int((yc != want).sum()))


@pytest.mark.parametrize('pass_', ['fwd', 'dgrad'])
def test_one_all_zero_weight_row(dev, force, pass_):
    """an all-zero row of the pass's weight matrix (row maximum 0, scale 1) on signed data: that channel equals its bias exactly, the
    others stay inside the section A bound (exact data: the next test)"""
    c = T.ZERO[pass_]
    d = T.data(c)
    w0 = d.w.clone()
    row = 37
    if pass_ == 'fwd':
        w0[row] = 0.0
    else:
        w0[:, row] = 0.0
    ref, A = T.reference(c, d.src, w0, d.b)
    E, bound, want = T.bounds(c, A, ref)
    src, _, b = _dev(dev, c, d)
    force(c.tile, c.ks)
    call = _Call(dev, c, w0.to(dev).contiguous())
    y, yc = call.run(src, b)
    assert float(call.rowmax[row]) == 0.0
    assert bool((yc[:, row] == float(d.b[row])).all())
    assert bool(((yc - want).abs() <= bound).all())


@pytest.mark.parametrize('pass_,tile', sorted(T.ZERO_ROW))
def test_one_all_zero_weight_row_exact(dev, force, pass_, tile):
    """the same on exact data ('xlow' with a bias) on a 64 x 128 and a 128 x 64 tile: the zeroed row equals its bias and EVERY other
    element equals the float64 reference recomputed with that row zeroed"""
    c = T.ZERO_ROW[(pass_, tile)]
    d = T.data(c)
    assert d.b is not None and c.act == 0
    w0 = d.w.clone()
    row = 37
    if pass_ == 'fwd':
        w0[row] = 0.0
    else:
        w0[:, row] = 0.0
    ref, A = T.reference(c, d.src, w0, d.b)
    assert float(A.max()) < 2.0 ** 24 and bool((ref.float().double() == ref).all())
    assert bool((ref[:, row] == d.b[row].double()).all()) and bool((ref != d.ref).any())
    src, _, b = _dev(dev, c, d)
    force(c.tile, c.ks)
    call = _Call(dev, c, w0.to(dev).contiguous())
    y, yc = call.run(src, b)
    assert float(call.rowmax[row]) == 0.0 and float(call.rowmax.min()) == 0.0 and int((call.rowmax == 0).sum()) == 1
    assert bool((yc[:, row] == float(d.b[row])).all())
    assert bool((yc == ref).all()), '%d element(s) not exact' % int((yc != ref).sum())


@pytest.mark.parametrize('kind', T.RANGE_KINDS)
@pytest.mark.parametrize('pass_,tile', sorted(T.RANGE))
def test_operand_ranges(dev, force, monkeypatch, pass_, tile, kind):
    """randn operands over twelve decades inside one tensor, times 1e12 / 1e8, and times 1e-30 / 1e-6, on a 64 x 128 and a 128 x 64 tile:
    per produced channel, relative L2 against float64 < 2 x the fp32 route's own error on the same inputs + 5e-7"""
    from pcgan_amd.hip import ops
    c = T.RANGE[(pass_, tile)]
    N, C, H, W, K, Rr, S, st, pad, pm = c.geom
    src, w, ref = T.range_data(c, kind)
    assert bool(torch.isfinite(src).all()) and float(ref.abs().max()) > 1e-37      # (the true values are fp32 numbers)
    sd, wd = src.to(dev).contiguous(), w.to(dev).contiguous()
    force(c.tile, c.ks)
    y, yc = _Call(dev, c, wd).run(sd)
    e16 = T.per_row_rel(yc, ref)
    monkeypatch.setattr(ops, 'HSPLIT', False)
    monkeypatch.setattr(ops, 'BF16X6', False)      # the fp32 MFMA kernels on the same data
    key = (pass_, 'packed')
    n0 = ops.ROUTE_STATS.get(key, 0)
    if pass_ == 'fwd':
        y32 = ops.conv2d_fwd(sd, wd, None, st, pad, pm, pack_cache={})
    else:
        y32 = ops.conv2d_bwd_data(sd, wd, (H, W), st, pad, pm, pack_cache={})
    rec = ops.igemm_last_launch()
    assert ops.ROUTE_STATS.get(key, 0) == n0 + 1 and rec['form'] == 'igemm2_cg16', 'the comparison did not run on the fp32 route: %r' % (rec,)
    e32 = T.per_row_rel(y32.double().cpu(), ref)
    print('HGEMM C range %s %d %s: relative L2 per channel %.3e .. %.3e (fp32 route %.3e .. %.3e); zeros written %d of %d' % (
        pass_, tile, kind, float(e16.min()), float(e16.max()), float(e32.min()), float(e32.max()), int((yc == 0).sum()), yc.numel()))
    worst = int((e16 - 2 * e32).argmax())
    assert bool((e16 < 2 * e32 + 5e-7).all()), 'channel %d: %.3e against %.3e on the fp32 route' % (worst, float(e16[worst]), float(e32[worst]))
    assert bool((yc != 0).any()), 'the output is all zeros'
    assert ops.nonfinite_count(reset=False) == 0


# ---- D. the pack ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(T.PACK) + 2))
def test_pack_bytes(dev, i):
    """pcgan_conv2d_hgemm_pack against the restatement, bit for bit: the packed K order of pcgan_conv2d_pack_weights, every aligned group
    of four floats replaced by [4 high | 4 low] fp16 pieces of the row scaled by pow2_scale(rowmax); the row maxima; nothing behind the
    image.  Integer and 'wlow' weights, and one randn tensor per pass (cases past the table)"""
    from pcgan_amd.hip import lib as L, ops
    if i < len(T.PACK):
        c = T.PACK[i]
        w = T.data(c).w
    else:
        c = [p for p in T.PACK if p.geom[4 if p.pass_ == 'fwd' else 1] == 136][::2][i - len(T.PACK)]
        w = torch.randn(c.geom[4], c.geom[1], c.geom[5], c.geom[6], generator=torch.Generator().manual_seed(77 + i)) * 0.05
    lib = L.load()
    d = ops.make_desc(*c.geom)
    ref = ctypes.byref(d)
    pass_ = L.PASS_FWD if c.pass_ == 'fwd' else L.PASS_BWD_DATA
    M = T.shapes(c)[2]
    assert lib.pcgan_conv2d_hgemm_supported(ref, pass_) == 1
    nb = int(lib.pcgan_conv2d_packed_bytes(ref, pass_))
    raw, rowmax = T.packed_presplit(c, w)
    assert raw.numel() <= nb
    pk, rm = guarded(dev, nb), guarded(dev, 4 * M)
    L.check(lib.pcgan_conv2d_hgemm_pack(ref, pass_, ptr(w.to(dev).contiguous()), ptr(rm), ptr(pk), VP(torch.cuda.current_stream().cuda_stream)),
            'conv2d_hgemm_pack')
    torch.cuda.synchronize()
    got = pk.cpu()
    bad = got[:raw.numel()] != raw
    assert not bool(bad.any()), '%d byte(s) differ, the first at %d' % (int(bad.sum()), int(torch.nonzero(bad)[0]))
    assert bool((got[raw.numel():] == 0xFF).all()), 'bytes behind the %d of the image were written' % raw.numel()
    assert torch.equal(rm[:4 * M].view(torch.float32).cpu(), rowmax) and bool((rm[4 * M:] == 0xFF).all())
    if c.pass_ == 'dgrad':
        assert len({p.nR * p.nS for p in T.hgemm_plan(c).phases}) == 3, 'phases of unequal taps'


def test_zz_every_instantiation_ran():
    """from the cases that ran in this process: all 24 instantiations in section A and in section B, when the whole file ran.  A
    selection (-k, one worker of several) is held to its own cases only; a process in which no case ran has nothing to check and says so"""
    if not coverage_gate(SEEN, NAMES, T.INSTANTIATIONS, 'AB', T.BY_NAME, T.inst, 'COVERAGE %-11s %3d x %3d %s: A %2d case(s), B %2d'):
        print('COVERAGE not gated: %d of %d cases ran in this process; the 24-instantiation gate applies when the whole file runs in one process' % (
            len(SEEN), len(NAMES)))
