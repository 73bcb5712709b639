"""Tensor-level wrappers over the Inception-v3 entry points of the C-ABI (include/pcgan_hip.h, csrc/inception.hip): validate, allocate
through torch's caching allocator and launch on torch's current stream.  Forward only, fp32 tensors; no arithmetic happens here."""
import ctypes

import torch

from . import lib as _L
from .lib import IconvDesc, F32
from .ops import _p, _stream

_vp = ctypes.c_void_p


def _f32(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError('pcgan_amd: tensor on %s -- the HIP path needs GPU tensors (no CPU fallback)' % t.device)
        if t.dtype != torch.float32:
            raise RuntimeError('pcgan_amd: the Inception kernels take float32 tensors, got %s' % t.dtype)
        if not t.is_contiguous():
            raise RuntimeError('pcgan_amd: tensor must be contiguous')


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def iconv_desc(x_shape, K, R, S, stride, pad_h, pad_w, k_off=0, K_total=None):
    N, C, H, W = x_shape
    P, Q = out_size(H, R, stride, pad_h), out_size(W, S, stride, pad_w)
    return IconvDesc(N, C, H, W, K, R, S, stride, pad_h, pad_w, P, Q, k_off, K if K_total is None else K_total, F32)


def iconv_supported(d):
    return _L.load().pcgan_iconv_supported(ctypes.byref(d)) == 1


def iconv_pack(w, bn=None, eps=1e-3, pool_expand=False):
    """packed weights (uint8 device tensor) of a convolution with weight w[K][C][R][S] and an optional eval BatchNorm folded in:
    bn = (gamma, beta, running_mean, running_var).  pool_expand: w is 1x1 and becomes the 3x3 pad-1 weight with taps w / 9 (avg_pool2d
    3/1/1 with count_include_pad=True, then the 1x1 conv).  The packed layout depends on K, C, R, S only: any batch / image size uses it."""
    K, C, R, S = w.shape
    if pool_expand:
        if (R, S) != (1, 1):
            raise ValueError('pool_expand takes a 1x1 weight, got %dx%d' % (R, S))
        R = S = 3
    bn = tuple(bn) if bn is not None else (None,) * 4
    _f32(w, *bn)
    pad = 1 if pool_expand else 0
    d = iconv_desc((1, C, R, S), K, R, S, 1, pad, pad)     # the layout needs K, C, R, S only: any valid geometry of that weight
    h = _L.load()
    nbytes = h.pcgan_iconv_packed_bytes(ctypes.byref(d))
    if nbytes == 0:
        raise RuntimeError('pcgan_hip iconv_packed_bytes: %s' % h.pcgan_last_error().decode())
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _L.check(h.pcgan_iconv_pack(ctypes.byref(d), int(pool_expand), _p(w), *[_p(t) for t in bn], float(eps), _p(packed), _stream()),
             'iconv_pack')
    return packed


def iconv_fwd(x, packed, K, R, S, stride, pad, relu=True, out=None, k_off=0):
    """y[:, k_off:k_off+K] = relu(conv(x, W') + b') with the packed W', b' of iconv_pack; `out` (N, K_total, P, Q) or a new (N, K, P, Q)"""
    _f32(x)
    N, C, H, W = x.shape
    P, Q = out_size(H, R, stride, pad[0]), out_size(W, S, stride, pad[1])
    if out is None:
        out = torch.empty((N, K, P, Q), dtype=torch.float32, device=x.device)
    _f32(out)
    if tuple(out.shape) != (N, out.shape[1], P, Q):
        raise RuntimeError('iconv_fwd: output of shape %s for a (%d, *, %d, %d) result' % (tuple(out.shape), N, P, Q))
    d = iconv_desc(x.shape, K, R, S, stride, pad[0], pad[1], k_off, out.shape[1])
    _L.check(_L.load().pcgan_iconv_fwd(ctypes.byref(d), _p(x), _p(packed), _p(out), int(relu), _stream()), 'iconv_fwd')
    return out


def maxpool_slice(x, k=3, stride=2, out=None, k_off=0):
    """max_pool2d(x, k, stride) (no padding, floor mode) into channels [k_off, k_off + C) of `out` (or a new tensor)"""
    _f32(x)
    N, C, H, W = x.shape
    P, Q = out_size(H, k, stride, 0), out_size(W, k, stride, 0)
    if out is None:
        out = torch.empty((N, C, P, Q), dtype=torch.float32, device=x.device)
    _f32(out)
    if out.shape[0] != N or tuple(out.shape[2:]) != (P, Q):
        raise RuntimeError('maxpool_slice: output of shape %s for a (%d, *, %d, %d) result' % (tuple(out.shape), N, P, Q))
    _L.check(_L.load().pcgan_maxpool_slice_fwd(_p(x), _p(out), N, C, H, W, k, stride, P, Q, k_off, out.shape[1], F32, _stream()),
             'maxpool_slice_fwd')
    return out


def prep(x, size=None, scale=None, shift=None):
    """bilinear resize to `size` (align_corners=False; None: keep the size) and y[:, c] = y[:, c] * scale[c] + shift[c] in one pass"""
    _f32(x)
    N, C, H, W = x.shape
    OH, OW = size if size is not None else (H, W)
    y = torch.empty((N, C, OH, OW), dtype=torch.float32, device=x.device)
    arr = ctypes.c_float * 3
    sc = arr(*scale) if scale is not None else None
    sh = arr(*shift) if shift is not None else None
    _L.check(_L.load().pcgan_inception_prep(_p(x), _p(y), N, C, H, W, OH, OW, sc, sh, F32, _stream()), 'inception_prep')
    return y


def linear_softmax(x, w, b=None, want_logits=True):
    """(logits, probs) = (x w^T + b, softmax(logits, dim=1)) through pcgan_linear_softmax_fwd: x (N, C), w (K, C) and b (K,) or None in
    nn.Linear's layout.  want_logits=False: logits is None (the kernel stages them in the probability buffer)."""
    _f32(x, w, b)
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1] or (b is not None and tuple(b.shape) != (w.shape[0],)):
        raise RuntimeError('linear_softmax: x %s, w %s, b %s do not form nn.Linear(C -> K) of (N, C) rows'
                           % (tuple(x.shape), tuple(w.shape), None if b is None else tuple(b.shape)))
    if w.device != x.device or (b is not None and b.device != x.device):
        raise RuntimeError('linear_softmax: x, w and b must be on one device')
    N, C = x.shape
    K = w.shape[0]
    probs = torch.empty((N, K), dtype=torch.float32, device=x.device)
    logits = torch.empty_like(probs) if want_logits else None
    _L.check(_L.load().pcgan_linear_softmax_fwd(_p(x), _p(w), _p(b), _p(logits), _p(probs), N, C, K, F32, _stream()),
             'linear_softmax_fwd')
    return logits, probs


def global_avg_pool(x):
    """AdaptiveAvgPool2d(1) through pcgan_global_pool_fwd"""
    _f32(x)
    N, C, H, W = x.shape
    y = torch.empty((N, C, 1, 1), dtype=torch.float32, device=x.device)
    _L.check(_L.load().pcgan_global_pool_fwd(_p(x), _p(y), _vp(0), N * C, H * W, 0, F32, _stream()), 'global_pool_fwd')
    return y
