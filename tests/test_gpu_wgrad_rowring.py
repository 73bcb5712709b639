"""GPU: the row-ring weight gradient of the residual convolutions (csrc/wgrad_rowring.hip: rowring_wgrad_kernel / rowring_wgrad_bf16_kernel,
scaled back and transposed by wgd_reduce_kernel of csrc/wgrad_direct.hip; library option "wgrad_rowring", default on) through
pcgan_conv2d_bwd_weight_rowring, against float64 autograd of the oracle's convolution over ALL output channels.

Two metrics, both against float64, with the fp32 route of the product on the same inputs as the yardstick (a split route may
be at most twice as far from float64 as the fp32 kernels, plus 5e-7):
  * relative L2:   e < 3e-6  and  e <= 2 e32 + 5e-7
  * per element:   max|dw - ref| <= 2 max|dw32 - ref| + 5e-7 max|ref|  and  <= 1e-4 max|ref| (the weight-gradient tolerance of test_gpu_ops.py)
A relative L2 norm alone hides a 0.1 % error in a handful of elements (one tap, one border column, one wave's rows: ~1e-6 of the norm).

A. operand ranges: what drives the power-of-two operand scaling (pow2_scale, csrc/common.h: exponent clamped to +-100) and the scale-back
   by (1 / sx) * (1 / sdy) in the reduce -- magnitudes over twelve decades in one tensor, x near 1e-30 (sx at the +100 clamp), true values near 1e21.
B. multi-strip walks: rowring_plan gives a workgroup `per` consecutive 16-pixel strips; shapes chosen from the device's CU count so that a
   workgroup starts mid-row, crosses from one image into the next inside its run (the strip prologue rebuilds ring slots the previous
   strip's last stage has just read) and the last split is short (the s_end clamp).  The plan is recomputed here and pinned to the
   library's workspace size, so the cases cannot silently stop being multi-strip.

Measured on an MI355X (256 CUs), every case inside every clause:
  A (24 cases; one slot per plane and ops.amax_of give the same bits): e 1.04e-7 .. 1.38e-7 against e32 7.4e-8 .. 3.5e-7; per element
    1.42e-7 .. 2.38e-7 of max|ref| against 7.1e-8 .. 9.0e-7; `tiny` and `huge` sit where `relu_normal` does (1.28e-7 / 1.28e-7 / 1.27e-7 at
    (3, 32, 128, 5, 16)).  Closest to the 2 x clause: (1, 32, 128, 3, 16) wide_range, (e, e32) = (1.066e-7, 7.398e-8), per element
    (1.483e-7, 7.086e-8): inside by the 5e-7 term only.  Accumulate <= 7.9e-7.
  B, fp32: per2_one_strip_tail N = 7, 35 strips, per 2, 18 splits; per3_ragged_tail N = 13, 65 strips, per 3, 22 splits (last: 2 strips);
    c512 N = 7, 21 strips, per 2, 11 splits.  (e, e32) from (1.39e-7, 2.81e-7) to (1.93e-7, 3.40e-7); per element (1.76e-7, 4.38e-7) to
    (3.02e-7, 5.29e-7); accumulate <= 2.3e-7.
  B, bf16 (12 cases): e 8.1e-8 .. 1.22e-7, per element 1.57e-7 .. 2.90e-7, accumulate <= 1.8e-7."""
import ctypes
import functools

import pytest
import torch

import gpu_direct as D
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

SPLIT_FORMS = ('hgemm_f16x2', 'hgemm_bf16')


def _reference(x, dy, K, C):
    """float64 autograd of the oracle's convolution, all K output channels, in chunks of 8 images"""
    w = torch.zeros(K, C, 3, 3, dtype=torch.float64, requires_grad=True)
    for n0 in range(0, x.shape[0], 8):
        R.conv2d(x[n0:n0 + 8].double(), w, None, 1, 1, 1).backward(dy[n0:n0 + 8].double())
    return w.grad.detach()


def _reference64(x, dy, geom):
    """_reference by the geometry: the reference of gpu_direct.range_case"""
    return _reference(x, dy, geom[4], geom[1])


@functools.lru_cache(maxsize=None)
def _walk_case(N, C, K, H, W, half):
    """position-dependent data (a shifted or mirrored column cannot cancel): x[n, c, y, x] = randn + 0.01 (y W + x); dy = 0.05 randn.
    half: both rounded to bf16, the reference is float64 of the SAME rounded inputs"""
    g = torch.Generator().manual_seed(N + C + K + H + W)
    x = torch.randn(N, C, H, W, generator=g) + 0.01 * torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W)
    dy = torch.randn(N, K, H, W, generator=g) * 0.05
    if half:
        x, dy = x.bfloat16(), dy.bfloat16()
    return x, dy, _reference(x, dy, K, C)


def _rowring(dev, x, dy, ref, maxima, seed):
    """the kernel twice: accumulate = 0 into a NaN-filled dw (workspace NaN-filled too: a partial sum nobody wrote would show), then
    accumulate = 1 into a random base scaled to max|ref|.  x / dy: device tensors, fp32 or bf16.  maxima: None (bf16) or (xmax, dmax).
    Returns (dw, accumulated - base) as float64 on the CPU."""
    from pcgan_amd.hip import lib as L, ops
    lib = L.load()
    N, C, H, W = x.shape
    K = dy.shape[1]
    half = x.dtype == torch.bfloat16
    d = ops.make_desc(N, C, H, W, K, 3, 3, 1, 1, 1, ops.BF16 if half else ops.F32)
    assert lib.pcgan_conv2d_wgrad_rowring_supported(ctypes.byref(d))
    nb = int(lib.pcgan_conv2d_wgrad_rowring_workspace_bytes(ctypes.byref(d)))
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    if half:
        args = (None, 0, vp(dy.data_ptr()), None, 0)
    else:
        xmax, dmax = maxima
        args = (vp(xmax.data_ptr()), xmax.numel(), vp(dy.data_ptr()), vp(dmax.data_ptr()), dmax.numel())
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(K, C, 3, 3, generator=g) * float(ref.abs().max())
    out = []
    for acc, dw in ((0, torch.full((K, C, 3, 3), float('nan'), device=dev)), (1, base.to(dev).clone())):
        L.check(lib.pcgan_conv2d_bwd_weight_rowring(ctypes.byref(d), vp(x.data_ptr()), args[0], args[1], args[2], args[3], args[4], vp(dw.data_ptr()), acc,
                                                    vp(ws.data_ptr()), nb, vp(torch.cuda.current_stream().cuda_stream)), 'bwd_weight_rowring')
        out.append(dw)
    torch.cuda.synchronize()
    return out[0].double().cpu(), out[1].double().cpu() - base.double()


def _fp32_route(x, dy, K, C):
    """the project's fp32 route (the fp32-MFMA weight gradient) on the same device tensors"""
    from pcgan_amd.hip import ops
    N, _, H, W = x.shape
    old = (ops.HSPLIT, ops.BF16X6)
    ops.HSPLIT = False
    ops.BF16X6 = False
    ops.clear_plans()
    try:
        route = ops._plan(ops._L.PASS_BWD_WEIGHT, N, C, H, W, K, 3, 3, 1, 1, 1, ops.F32).route
        before = ops.igemm_last_launch()
        dw32 = ops.conv2d_bwd_weight(x, dy, (K, C, 3, 3), 1, 1, 1)
        torch.cuda.synchronize()
        after = ops.igemm_last_launch()
    finally:
        ops.HSPLIT, ops.BF16X6 = old
        ops.clear_plans()
    assert route == 'generic', route
    assert after['seq'] == before['seq'] or after['form'] not in SPLIT_FORMS, 'the comparison kernel was a split kernel: %r' % (after,)
    return dw32.double().cpu()


def _check_fp32(what, dw, acc, dw32, ref):
    (e, m), (e32, m32), (ea, _) = D.errors(dw, ref), D.errors(dw32, ref), D.errors(acc, ref)
    print('%s: relative L2 (e, e32) = (%.3e, %.3e); max|err| / max|ref| (row ring, fp32 route) = (%.3e, %.3e); accumulate %.3e' % (what, e, e32, m, m32, ea))
    assert torch.isfinite(dw).all(), what
    assert e < 3e-6 and e <= 2 * e32 + 5e-7, '%s: relative L2 %.3e (fp32 route %.3e)' % (what, e, e32)
    assert m <= 2 * m32 + 5e-7 and m <= 1e-4, '%s: max |error| %.3e of the largest magnitude (fp32 route %.3e)' % (what, m, m32)
    assert ea < 1e-5, '%s: accumulate: relative L2 %.3e' % (what, ea)


# ---- A. operand ranges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('maxima', ['per_plane', 'amax_of'])
@pytest.mark.parametrize('kind', ['relu_normal', 'wide_range', 'tiny', 'huge'])
@pytest.mark.parametrize('N,C,K,H,W', [(3, 32, 128, 5, 16), (1, 32, 128, 3, 16), (2, 64, 256, 6, 32)])
def test_row_ring_operand_ranges(dev, N, C, K, H, W, kind, maxima):
    """fp32 tensors whose magnitudes drive the operand scaling, its exponent clamp and the scale-back of the reduce; the operand maxima
    both ways the product hands them over: one slot per plane (as the instance-norm kernels do) and the tensor of ops.amax_of."""
    from pcgan_amd.hip import ops
    x, dy, ref = D.range_case(kind, (N, C, H, W, K, 3, 3, 1, 1, 1), _reference64)
    # the reference itself is a fair fp32 target: its largest 99 % (by magnitude) lie inside fp32's normal range
    mags = ref.abs().flatten().sort().values
    assert float(mags[mags.numel() // 100]) >= 2.0 ** -126 and float(mags[-1]) < 2.0 ** 127
    xd, dyd = x.to(dev), dy.to(dev)
    if maxima == 'per_plane':
        mx = (xd.abs().amax(dim=(2, 3)).reshape(-1).contiguous(), dyd.abs().amax(dim=(2, 3)).reshape(-1).contiguous())
        assert mx[0].numel() == N * C and mx[1].numel() == N * K
    else:
        mx = (ops.amax_of(xd), ops.amax_of(dyd))
    dw, acc = _rowring(dev, xd, dyd, ref, mx, N + C + K)
    _check_fp32('%s %s %s' % ((N, C, K, H, W), kind, maxima), dw, acc, _fp32_route(xd, dyd, K, C), ref)


# ---- B. multi-strip walks -----------------------------------------------------------------------------------------------------------------
def _ring_plan(cus, N, C, K, W):
    """rowring_plan (csrc/wgrad_rowring.hip): strips of 16 pixels, `per` consecutive strips per workgroup, `splits` partial sums"""
    strips = N * (W // 16)
    want = (2 * cus) // ((K // 128) * (C // 32))
    want = 1 if want < 1 else min(want, strips)
    per = -(-strips // want)
    return strips, per, -(-strips // per)


WALKS = {     # name: (C, K, W, wanted plan)
    'per2_one_strip_tail': (256, 256, 80, lambda strips, per: per == 2 and strips % per == 1),      # 256 CUs: N = 7, 35 strips, 18 splits
    'per3_ragged_tail': (256, 256, 80, lambda strips, per: per == 3 and strips % per != 0),         # 256 CUs: N = 13, 65 strips, 22 splits
    'c512': (512, 256, 48, lambda strips, per: per >= 2 and strips % per != 0),                     # 256 CUs: N = 7, 21 strips, 11 splits
}


def _walk(dev, name, H, half):
    """the smallest batch whose plan on THIS device is the walk `name`; the plan pinned to the library's workspace size"""
    from pcgan_amd.hip import lib as L, ops
    lib = L.load()
    C, K, W, wanted = WALKS[name]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for N in range(1, 129):
        strips, per, splits = _ring_plan(cus, N, C, K, W)
        if wanted(strips, per):
            break
    else:
        pytest.fail('no batch <= 128 gives the walk %s at %d CUs' % (name, cus))
    d = ops.make_desc(N, C, H, W, K, 3, 3, 1, 1, 1, ops.BF16 if half else ops.F32)
    nb = int(lib.pcgan_conv2d_wgrad_rowring_workspace_bytes(ctypes.byref(d)))
    assert splits == (nb - 256) // (9 * K * C * 4), 'the plan changed under this test: %d splits expected, workspace %d bytes' % (splits, nb)
    wq = W // 16
    crossing = [s for s in range(splits) if (s * per) // wq != (min((s + 1) * per, strips) - 1) // wq]
    assert per > 1 and strips % per != 0 and crossing, (cus, N, strips, per, splits)
    print('%s H=%d %s: %d CUs, N = %d, %d strips, per = %d, splits = %d (last split %d strip(s)), %d splits cross images' % (
        name, H, 'bf16' if half else 'fp32', cus, N, strips, per, splits, strips - (splits - 1) * per, len(crossing)))
    return N, C, K, W


@pytest.mark.parametrize('H', [3, 5])
@pytest.mark.parametrize('walk', sorted(WALKS))
def test_row_ring_multi_strip_walk(dev, walk, H):
    """fp32 tensors: workgroups that walk several strips -- starting mid-row, crossing into the next image, a short last split"""
    from pcgan_amd.hip import ops
    N, C, K, W = _walk(dev, walk, H, False)
    x, dy, ref = _walk_case(N, C, K, H, W, False)
    xd, dyd = x.to(dev), dy.to(dev)
    dw, acc = _rowring(dev, xd, dyd, ref, (ops.amax_of(xd), ops.amax_of(dyd)), N + H)
    _check_fp32('%s H=%d' % (walk, H), dw, acc, _fp32_route(xd, dyd, K, C), ref)


@pytest.mark.parametrize('H', [3, 4, 5, 8])
@pytest.mark.parametrize('walk', sorted(WALKS))
def test_row_ring_multi_strip_walk_bf16(dev, walk, H):
    """bf16 tensors: the same walks; H = 4 and 8 leave the four-way unrolled stage loop without tail stages, 3 and 5 with three.  Against
    float64 of the SAME bf16 inputs: bf16 x bf16 products are exact in fp32 and only the order of accumulation differs (1e-6 relative
    L2, as tests/test_gpu_bf16x6.py derives for this kernel); per element the weight-gradient tolerance 1e-4 of the largest magnitude."""
    N, C, K, W = _walk(dev, walk, H, True)
    x, dy, ref = _walk_case(N, C, K, H, W, True)
    dw, acc = _rowring(dev, x.to(dev), dy.to(dev), ref, None, N + H)
    (e, m), (ea, _) = D.errors(dw, ref), D.errors(acc, ref)
    print('%s H=%d bf16: relative L2 %.3e; max|err| / max|ref| %.3e; accumulate %.3e' % (walk, H, e, m, ea))
    assert torch.isfinite(dw).all()
    assert e < 1e-6, e
    assert m <= 1e-4, m
    assert ea < 1e-5, ea
