"""The arithmetic and the small helpers that the conv case tables share (tests/conv_f32_cases.py, hgemm_cases.py, halo_cases.py,
thin_cases.py, hsplit_wgrad_cases.py, bsplit_cases.py): what csrc/common.h and csrc/bsplit.h hold once on the device side -- pow2_scale, split2h, split3,
the walk of thread_max_of_partials -- restated once in torch, so that the emulations can be held to float64 on the CPU; the float64
reference of a forward / data-gradient / weight-gradient call; and the scaling of the operand-range data.  A plain module, CPU only, no GPU and no library
load; it imports no case module (they import it).  The bound derivations, the measured tables and the sensitivity studies stay in the
docstrings of the case modules: nothing here is specific to one kernel."""
import math

import torch

from oracle import ops_ref as R

U = 2.0 ** -24
SLOPE = 0.2                     # LeakyReLU of the signed cases
SLOPE_EXACT = 0.25              # ... of the exact cases: a power of two keeps integers exact


def cdiv(a, b):
    return -(-a // b)


def out_size(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _bf16(t):
    return t.bfloat16().float()


def half_ulp_bf16(v):
    """half the spacing of bf16 numbers (8 significant bits) at magnitude v"""
    e = torch.frexp(v.abs().clamp_min(2.0 ** -120))[1]
    return torch.pow(2.0, (e - 9).double())


def slope_of(kind):
    return SLOPE if kind == 'signed' else SLOPE_EXACT


# ---- the device functions, restated ----------------------------------------------------------------------------------------------------------
def pow2_scale(amax):
    """csrc/common.h pow2_scale: the power of two that puts amax into [2^13, 2^14); 1 for 0; exponent clamped to +-100"""
    if not amax > 0.0:
        return 1.0
    e = 14 - math.frexp(amax)[1]
    return 2.0 ** max(-100, min(100, e))


def split2h(x, sums=False, may_overflow=False):
    """csrc/common.h split2h: fp32 tensor -> (h, l) fp16 pieces as fp32 tensors; the split must not overflow fp16.
    sums: the window of the halo data gradient (csrc/halo_conv.hip), whose sum entries reach up to 4 (2^14 - 1): below 2^16 the high piece
    saturates at 65504 and the low piece takes the rest.  may_overflow: an emulated fault that mis-scales its operand on purpose -- the
    finiteness of h is not asserted"""
    xs = torch.where(x.abs() < 65536.0, x.clamp(-65504.0, 65504.0), x) if sums else x
    h = xs.half()
    l = (x - h.float()).half()
    assert may_overflow or bool(torch.isfinite(h).all()), 'a scaled operand overflows fp16'
    return h.float(), l.float()


def split3(x):
    """csrc/bsplit.h split3: fp32 tensor -> [h, m, l] bf16 pieces as fp32 tensors"""
    h = x.bfloat16().float()
    r1 = x - h
    m = r1.bfloat16().float()
    return [h, m, (r1 - m).bfloat16().float()]


def maxima_slots(n, nt):
    """where the true maximum is put in a maxima array of n slots that thread_max_of_partials (csrc/common.h) walks with nt threads: first,
    last, and from 4 nt slots on the last lane of the float4 at index 4 nt - 1 (the end of the first 4-in-flight round of nt threads; the
    float4 remainder when n / 4 is under 4 nt + 1) and the last element the float4 loops read; from 16 nt slots on also in the second and
    the third of the four loads in flight, which the first and the last slot of a round do not reach"""
    pos = [0, n - 1]
    if n >= 4 * nt:
        pos += [q for q in (4 * (4 * nt - 1) + 3, 4 * (n // 4) - 1) if q < n]
    if n >= 16 * nt:      # the 4-in-flight loop runs: one slot in its second and one in its third load (p4[i + nt], p4[i + 2 nt])
        pos += [4 * nt + 1, 4 * (2 * nt + 77) + 2]
    return sorted(set(pos))


# ---- float64 reference, error measures -------------------------------------------------------------------------------------------------------
def _fwd64(src, w, b, geom):
    return R.conv2d(src, w, b, geom[7], geom[8], geom[9])


def _dgrad64(dy, w, b, geom):
    N, C, H, W = geom[:4]
    xz = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    R.conv2d(xz, w, None, geom[7], geom[8], geom[9]).backward(dy)
    g = xz.grad.detach()
    return g if b is None else g + b.view(1, -1, 1, 1)


def reference(pass_, geom, src, w, b):
    """(float64 result before the activation, the same call on absolute values) of the pass ('fwd' | 'dgrad') of the convolution
    geom = (N, C, H, W, K, R, S, stride, pad, pad_mode) on the given operands"""
    f = _fwd64 if pass_ == 'fwd' else _dgrad64
    s64, w64, b64 = src.double(), w.double(), (b.double() if b is not None else None)
    return f(s64, w64, b64, geom), f(s64.abs(), w64.abs(), b64.abs() if b is not None else None, geom)


def wgrad64(x, dy, geom):
    """float64 weight gradient [K][C][R][S] of the convolution geom on (x, dy): autograd of oracle.ops_ref.conv2d"""
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    w = torch.zeros(K, C, Rr, S, dtype=torch.float64, requires_grad=True)
    R.conv2d(x.double(), w, None, st, pad, pm).backward(dy.double())
    return w.grad.detach()


def quanta(d):
    """exact kinds: the largest A of the Data record d in units of its quantum (1, or 2^j of the row where d.rowexp holds row exponents);
    must stay under 2^24"""
    if d.rowexp is None:
        return float(d.A.max())
    return float((d.A / torch.pow(2.0, d.rowexp.double()).view(1, -1, 1, 1)).max())


def per_row_rel(out, ref):
    """relative L2 error of every produced channel"""
    rows = ref.shape[1]
    dd = (out - ref).transpose(0, 1).reshape(rows, -1).norm(dim=1)
    return dd / ref.transpose(0, 1).reshape(rows, -1).norm(dim=1)


# ---- operand ranges --------------------------------------------------------------------------------------------------------------------------
def range_scale(kind, g, src, w, src_decades, w_decades, tiny, huge):
    """randn operands (src, w) under the range kinds of tests/test_gpu_bf16x6.py.  'wide_range': magnitudes over `span` decades inside one
    tensor, each element times 10^(span rand + offset) with (span, offset) = src_decades | w_decades, the source drawn first; 'tiny' /
    'huge': the pair of factors (source, weight).  The numbers differ per kernel on purpose: every caller passes its own"""
    if kind == 'wide_range':
        src = src * torch.pow(10.0, torch.rand(src.shape, generator=g) * src_decades[0] + src_decades[1])
        w = w * torch.pow(10.0, torch.rand(w.shape, generator=g) * w_decades[0] + w_decades[1])
    elif kind == 'tiny':
        src, w = src * tiny[0], w * tiny[1]
    else:
        assert kind == 'huge'
        src, w = src * huge[0], w * huge[1]
    return src, w
