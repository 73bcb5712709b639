"""torch.autograd.Function wrappers around the HIP kernels.

Each Function saves exactly what its backward needs and is re-entrant (the generator is
applied twice per step with the first output feeding the second pass; the discriminator
sees the same fake image in two different graphs).  Autograd bookkeeping is the only
thing torch does here -- every forward/backward computation is a libpcgan_hip.so kernel.
"""
import contextlib
import os

import torch

from . import ops
from .lib import ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID  # noqa: F401


def _c(t):
    return t if (t is None or t.is_contiguous()) else t.contiguous()


def _fused_grad_target(p):
    """The parameter's slice of a FusedAdam flat gradient buffer, if it has one: the weight-/bias-gradient
    kernels then add into it directly and autograd receives None (no separate `grad += dw` pass, no dw
    allocation).  FusedAdam marks its parameters with `_pcgan_fused_grad`."""
    if p is not None and getattr(p, '_pcgan_fused_grad', False) and p.grad is not None and p.grad.is_contiguous():
        return p.grad
    return None


def _pack_cache(p):
    """Per-parameter dict holding the packed copies of a conv weight, one per packed form in use (see ops._packed_weights, ops._PACK_FORMS)."""
    if p is None or not isinstance(p, torch.nn.Parameter):
        return None
    c = p.__dict__.get('_pcgan_pack')
    if c is None:
        c = p.__dict__['_pcgan_pack'] = {}
    return c


# ---------------------------------------------------------------------------- conv
def _conv_backward(ctx, x, dy, w, wgrad_operands, cfg, dgrad):
    """What the backward passes of _Conv2dFn and _ConvTranspose2dFn share; returns (dx, dw, db).  dgrad() is the Function's own
    data-gradient call; the weight gradient takes wgrad_operands = (x, dy), swapped for the transposed conv, and cfg = (stride, pad,
    pad_mode); the bias gradient is the channel sum of dy for both."""
    if ctx.x_amax is not None and ctx.x_amax[0] == x._version and '_pcgan_amax' not in x.__dict__:
        x._pcgan_amax = ctx.x_amax      # operand maxima its producer left (saved in forward: a saved tensor comes back without them)
    want_x = ctx.needs_input_grad[0]
    want_w = ctx.needs_input_grad[1]
    want_b = ctx.has_bias and ctx.needs_input_grad[2]
    wt = _fused_grad_target(ctx.params[0]) if want_w else None
    bt = _fused_grad_target(ctx.params[1]) if want_b else None

    def param_grads():
        dw = ops.conv2d_bwd_weight(*wgrad_operands, tuple(w.shape), *cfg, accumulate_into=wt) if want_w else None
        db = ops.channel_sum(dy, accumulate_into=bt) if want_b else None
        return (dw if wt is None else None), (db if bt is None else None)

    if ops.SIDE_STREAM and (not want_w or wt is not None) and (not want_b or bt is not None) and (want_w or want_b):
        # both go straight into the optimizer's gradient buffer: nobody in this backward pass reads them.  Forked BEFORE the data
        # gradient is queued, so the two kernels of this layer may run side by side (all accumulations into that buffer are issued
        # in order on the one parameter-gradient stream).
        with ops.fork_side(x, dy):
            param_grads()
        return (dgrad() if want_x else None), None, None
    dx = dgrad() if want_x else None
    return (dx,) + param_grads()


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, pad_mode, act, slope):
        x, w, b = _c(x), _c(w), _c(b)
        ctx.pack = _pack_cache(w)
        y = ops.conv2d_fwd(x, w, b, stride, pad, pad_mode, act, slope, pack_cache=ctx.pack)
        ctx.cfg = (stride, pad, pad_mode, act, slope)
        ctx.has_bias = b is not None
        ctx.params = (w, b)          # the Parameter objects (for their fused gradient buffers)
        ctx.x_amax = x.__dict__.get('_pcgan_amax')     # operand maxima its producer left (fp16 route): a saved tensor comes back without them
        ctx.save_for_backward(x, w, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, pad, pad_mode, act, slope = ctx.cfg
        dy = _c(dy)
        if act != ACT_NONE:
            dy = ops.act_bwd(dy, y, act, slope)
        return _conv_backward(ctx, x, dy, w, (x, dy), (stride, pad, pad_mode), lambda: ops.conv2d_bwd_data(
            dy, w, (x.shape[2], x.shape[3]), stride, pad, pad_mode, pack_cache=ctx.pack)) + (None,) * 5


class _ResBlockFn(torch.autograd.Function):
    """One ResnetBlock (reference models/networks.py:616-652) as ONE autograd node and ONE library call per pass
    (ops.resblock_fwd / resblock_bwd: the launches of the per-op path, bit for bit).  Taken by nn-level code only when the block's
    shape is on the fp16 route and its parameters feed a FusedAdam gradient buffer (or nothing requires gradients)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, pl, in1, in2):
        upd1 = in1.training and in1.running_mean is not None
        upd2 = in2.training and in2.running_mean is not None
        pack1, pack2 = _pack_cache(w1), _pack_cache(w2)
        out, saved = ops.resblock_fwd(pl, x, w1, b1, w2, b2, in1.running_mean if upd1 else None, in1.running_var if upd1 else None,
                                      in2.running_mean if upd2 else None, in2.running_var if upd2 else None, pack1, pack2)
        ctx.pl, ctx.packs, ctx.params = pl, (pack1, pack2), (w1, b1, w2, b2)
        # the block's activations go through save_for_backward (not a ctx attribute): autograd frees them right after a backward that
        # does not retain the graph, and keeps them for one that does -- update_G_and_E back-propagates twice through the generator
        ctx.save_for_backward(x, w1, w2, *saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w1, w2, *saved = ctx.saved_tensors
        p1, pb1, p2, pb2 = ctx.params
        tw1, tb1, tw2, tb2 = (_fused_grad_target(p) for p in (p1, pb1, p2, pb2))
        assert tw1 is not None and tw2 is not None and (pb1 is None or tb1 is not None) and (pb2 is None or tb2 is not None), \
            'pcgan_amd: the composite residual block needs FusedAdam gradient buffers (checked in forward)'
        dx = ops.resblock_bwd(ctx.pl, _c(dout), x, tuple(saved), w1, w2, tw1, tb1, tw2, tb2, ctx.packs[0], ctx.packs[1])
        return dx, None, None, None, None, None, None, None


def resblock_composite_ok(x, conv1, conv2, in1, in2):
    """the launch plan if this ResnetBlock call can take the composite path, else None"""
    if not (ops.COMPOSITE and ops.SIDE_STREAM and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 4 and x.is_contiguous()):
        return None
    if in1.eps != in2.eps or in1.momentum != in2.momentum or in1.momentum is None:
        return None
    for m in (in1, in2):       # plane statistics (train mode, or no running statistics at all)
        if m.affine or not (m.training or not m.track_running_stats):
            return None
    N, C, H, W = x.shape
    for c in (conv1, conv2):
        if tuple(c.weight.shape) != (C, C, 3, 3) or c.stride != (1, 1) or c.padding != (0, 0) or c.weight.dtype != torch.float32:
            return None
    if (conv1.bias is None) != (conv2.bias is None):
        return None
    pl = ops.resblock_plan(N, C, H, W, in1.eps, in1.momentum, ops.F32 if x.dtype == torch.float32 else ops.BF16)
    if not pl.ok:
        return None
    params = [p for p in (conv1.weight, conv1.bias, conv2.weight, conv2.bias) if p is not None]
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        # training: every parameter's gradient goes straight into its optimizer's flat buffer, and x carries a gradient
        if not (x.requires_grad and all(p.requires_grad and _fused_grad_target(p) is not None for p in params)):
            return None
    return pl


def resblock(x, conv1, conv2, in1, in2, pl):
    return _ResBlockFn.apply(x, conv1.weight, conv1.bias, conv2.weight, conv2.bias, pl, in1, in2)


class _ResTrunkFn(torch.autograd.Function):
    """A run of ResnetBlocks (the generator's nine, reference models/networks.py:589-592) as ONE autograd node and ONE library call per
    pass (ops.restrunk_fwd / restrunk_bwd = the launches of the per-block composite calls, bit for bit).  params: (w1, b1, w2, b2) per
    block, flat, so that autograd sees them."""

    @staticmethod
    def forward(ctx, x, pl, norms, *params):
        nb = len(params) // 4
        blocks = []
        for i in range(nb):
            w1, b1, w2, b2 = params[4 * i:4 * i + 4]
            in1, in2 = norms[i]
            u1 = in1.training and in1.running_mean is not None
            u2 = in2.training and in2.running_mean is not None
            blocks.append((w1, b1, w2, b2, in1.running_mean if u1 else None, in1.running_var if u1 else None,
                           in2.running_mean if u2 else None, in2.running_var if u2 else None, _pack_cache(w1), _pack_cache(w2)))
        out, saved = ops.restrunk_fwd(pl, x, blocks)
        ctx.pl, ctx.params = pl, params
        ctx.save_for_backward(x, *saved)      # (as in _ResBlockFn: freed after the last backward that uses them, ~1.2 GB at batch 32)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, *saved = ctx.saved_tensors
        params = ctx.params
        blocks = []
        for i in range(len(params) // 4):
            w1, b1, w2, b2 = params[4 * i:4 * i + 4]
            t = [_fused_grad_target(p) for p in (w1, b1, w2, b2)]
            assert t[0] is not None and t[2] is not None and (b1 is None or t[1] is not None) and (b2 is None or t[3] is not None), \
                'pcgan_amd: the composite residual trunk needs FusedAdam gradient buffers (checked in forward)'
            blocks.append((w1, w2, t[0], t[1], t[2], t[3], _pack_cache(w1), _pack_cache(w2)))
        dx = ops.restrunk_bwd(ctx.pl, _c(dout), x, tuple(saved), blocks)
        return (dx, None, None) + (None,) * len(params)


def restrunk(x, mods):
    """mods: consecutive ResnetBlock modules with the composite layout; the chain through ONE call when every block qualifies (same
    plan), else None (the caller runs them one by one)"""
    if not (ops.TRUNK and len(mods) >= 2):
        return None
    pl = None
    params, norms = [], []
    for m in mods:
        cb = m.conv_block
        p = resblock_composite_ok(x, cb[1], cb[5], cb[2], cb[6])
        if p is None or (pl is not None and p is not pl):
            return None
        pl = p
        params += [cb[1].weight, cb[1].bias, cb[5].weight, cb[5].bias]
        norms.append((cb[2], cb[6]))
    y = _ResTrunkFn.apply(x, pl, norms, *params)
    ent = ops._LAST_TRUNK.pop('amax', None)
    if ent is not None and '_pcgan_amax' not in y.__dict__ and ent[0] == y._version:
        y._pcgan_amax = ent       # the plane maxima of the chain's output (the next convolution's operand scale)
    return y


def conv2d(x, w, b=None, stride=1, pad=0, pad_mode=0, act=ACT_NONE, slope=0.0):
    """nn.Conv2d (optionally preceded by nn.ReflectionPad2d(pad): pad_mode=1) with the
    following pointwise activation fused into the epilogue."""
    return _Conv2dFn.apply(x, w, b, stride, pad, pad_mode, act, slope)


class _ConvTranspose2dFn(torch.autograd.Function):
    """nn.ConvTranspose2d(w[Cin][Cout][R][S]) expressed through the conv entry points of the
    conv (C=Cout -> K=Cin) whose data-gradient it is."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, out_pad):
        x, w, b = _c(x), _c(w), _c(b)
        R, S = w.shape[2], w.shape[3]
        Ho = (x.shape[2] - 1) * stride - 2 * pad + R + out_pad
        Wo = (x.shape[3] - 1) * stride - 2 * pad + S + out_pad
        ctx.pack = _pack_cache(w)
        y = ops.conv2d_bwd_data(x, w, (Ho, Wo), stride, pad, 0, bias=b, pack_cache=ctx.pack)
        ctx.cfg = (stride, pad)
        ctx.has_bias = b is not None
        ctx.params = (w, b)
        ctx.x_amax = x.__dict__.get('_pcgan_amax')     # (see _Conv2dFn)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad = ctx.cfg
        dy = _c(dy)
        # (the weight gradient of the conv this is the data gradient of: operands swapped)
        return _conv_backward(ctx, x, dy, w, (dy, x), (stride, pad, 0), lambda: ops.conv2d_fwd(
            dy, w, None, stride, pad, 0, pack_cache=ctx.pack)) + (None,) * 3


def conv_transpose2d(x, w, b=None, stride=2, pad=1, out_pad=1):
    return _ConvTranspose2dFn.apply(x, w, b, stride, pad, out_pad)


# ---------------------------------------------------------------------------- norms
class _InstanceNormActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, running_mean, running_var, momentum, eps, act, slope, training):
        x, residual = _c(x), _c(residual)
        N, C = x.shape[0], x.shape[1]
        HW = x.numel() // (N * C)
        if training or running_mean is None:
            y, mean, var = ops.instnorm_fwd(x, residual, eps, act, slope)    # var holds the plane M2
            per_plane = True
            if training and running_mean is not None:
                ops.in_running_update(mean, var, running_mean, running_var, N, C, HW, momentum)
        else:
            mean, var, per_plane = running_mean, running_var, False
            y = ops.norm_act_fwd(x, mean, var, None, None, residual, per_plane, eps, act, slope)
        ctx.cfg = (eps, act, slope, per_plane, residual is not None)
        ctx.save_for_backward(x, y if act != ACT_NONE else None, mean, var)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, var = ctx.saved_tensors
        eps, act, slope, per_plane, has_res = ctx.cfg
        if not per_plane:
            raise NotImplementedError('pcgan_amd: backward through eval-mode InstanceNorm is not on the hot path')
        dy = _c(dy)
        dx = dres = None
        if ctx.needs_input_grad[0]:
            dx = ops.instnorm_bwd(dy, x, y, mean, var, eps, act, slope)
        if has_res and ctx.needs_input_grad[1]:
            dres = dy if act == ACT_NONE else ops.act_bwd(dy, y, act, slope)
        return dx, dres, None, None, None, None, None, None, None


def instance_norm_act(x, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, act=ACT_NONE, slope=0.0,
                      residual=None, training=True):
    """act( InstanceNorm2d(affine=False)(x) + residual ), running statistics updated in place."""
    return _InstanceNormActFn.apply(x, residual, running_mean, running_var, momentum, eps, act, slope, training)


class _BatchNormActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, momentum, eps, act, slope, training, batches, tickets=None):
        x, residual = _c(x), _c(residual)
        N, C = x.shape[0], x.shape[1]
        HW = x.numel() // (N * C)
        fused = training and N * HW <= ops.BN_FUSED_MAX and N * HW > 1
        if fused:      # one launch: statistics + running update + batch counter + normalise / activation
            y, mean, var = ops.bn_fwd_fused(x, gamma, beta, residual, running_mean, running_var, batches, momentum, eps, act, slope)
        else:
            if training and tickets is not None and N * HW > 1:
                # statistics + Chan merge + running statistics + batch counter in one launch (last-arriver merge, csrc/norm.hip)
                mean, var = ops.bn_stats_merged(x, running_mean, running_var, batches, tickets[0], momentum)
            elif training:
                mean_nc, m2_nc = ops.plane_stats(x)
                mean, var = ops.bn_merge(mean_nc, m2_nc, N, C, HW, running_mean, running_var, momentum)
                if batches is not None:
                    batches.add_(1)
            else:
                mean, var = running_mean, running_var
            y = ops.norm_act_fwd(x, mean, var, gamma, beta, residual, False, eps, act, slope)
        ctx.cfg = (eps, act, slope, training, residual is not None, fused)
        ctx.tickets = tickets
        ctx.save_for_backward(x, y if act != ACT_NONE else None, mean, var, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, var, gamma = ctx.saved_tensors
        eps, act, slope, training, has_res, fused = ctx.cfg
        if not training:
            raise NotImplementedError('pcgan_amd: backward through eval-mode BatchNorm is not on the hot path')
        dy = _c(dy)
        N, C = x.shape[0], x.shape[1]
        want_res = has_res and ctx.needs_input_grad[3]
        want_dx = ctx.needs_input_grad[0]
        dx = dres = None
        if fused:
            dx, dres, s1, s2 = ops.bn_bwd_fused(dy, x, y, mean, var, gamma, eps, act, slope, want_dx,
                                                want_res and act != ACT_NONE)
        else:
            if ctx.tickets is not None:
                s1, s2 = ops.bn_bwd_stats_reduced(dy, x, y, mean, var, eps, act, slope, ctx.tickets[1])
            else:
                s1n, s2n = ops.norm_bwd_stats(dy, x, y, mean, var, False, eps, act, slope)
                s1, s2 = ops.bn_bwd_reduce(s1n, s2n, N, C)
            if want_dx or (want_res and act != ACT_NONE):
                dx, dres = ops.norm_bwd_apply(dy, x, y, mean, var, gamma, s1, s2, False, eps, act, slope,
                                              want_res and act != ACT_NONE)
        if want_res and dres is None:
            dres = dy
        dgamma = s2 if ctx.needs_input_grad[1] else None
        dbeta = s1 if ctx.needs_input_grad[2] else None
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None, None, None


def batch_norm_act(x, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, act=ACT_NONE, slope=0.0,
                   residual=None, training=True, batches=None, tickets=None):
    """act( BatchNorm2d(affine=True)(x) + residual ) with batch statistics in train mode; `batches` = the module's
    num_batches_tracked counter (incremented on the device, inside the fused kernel when the tensor is small)."""
    return _BatchNormActFn.apply(x, gamma, beta, residual, running_mean, running_var, momentum, eps, act, slope,
                                 training, batches, tickets)


# ---------------------------------------------------------------------------- pointwise
class _ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, slope):
        y = ops.act_fwd(_c(x), act, slope)
        ctx.cfg = (act, slope)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        act, slope = ctx.cfg
        return ops.act_bwd(_c(dy), y, act, slope), None, None


def activation(x, act, slope=0.0):
    return x if act == ACT_NONE else _ActFn.apply(x, act, slope)


class _ConcatZFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, z):
        img = _c(img)
        z2 = _c(z.reshape(z.size(0), z.size(1)))
        ctx.shapes = (img.shape, z.shape)
        return ops.concat_z(img, z2)

    @staticmethod
    def backward(ctx, dy):
        ishape, zshape = ctx.shapes
        C = ishape[1]
        dimg = dz = None
        if ctx.needs_input_grad[0]:
            dimg = dy[:, :C].contiguous()        # strided device copy (memory plumbing)
        if ctx.needs_input_grad[1]:
            dzc = dy[:, C:].contiguous()
            N, nz = dzc.shape[0], dzc.shape[1]
            # per-(n, j) plane sums: reuse the channel-sum kernel on a [1][N*nz][HW] view
            s = ops.channel_sum(dzc.view(1, N * nz, dzc.shape[2], dzc.shape[3]))
            s = s.view(N, nz)
            if zshape[0] == 1:
                s = ops.channel_sum(s.t().contiguous().view(1, nz, N, 1)).view(1, nz)
            dz = s.reshape(zshape)
        return dimg, dz


class _ConcatZFusedFn(torch.autograd.Function):
    """_ConcatZFn with the backward pass as ONE launch (ops.concat_z_bwd) that computes only what is asked for: with a rating that needs a
    gradient beside an image that needs none, the image planes of dy are neither copied nor read.  dimg has the bits of _ConcatZFn's; dz is
    the same fp32 sum in another (fixed) order."""

    @staticmethod
    def forward(ctx, img, z):
        img = _c(img)
        z2 = _c(z.reshape(z.size(0), z.size(1)))
        ctx.shapes = (img.shape, z.shape)
        return ops.concat_z(img, z2)

    @staticmethod
    def backward(ctx, dy):
        ishape, zshape = ctx.shapes
        want_img, want_z = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_img or want_z):
            return None, None
        dimg, dz = ops.concat_z_bwd(_c(dy), ishape[1], zshape[0], want_img, want_z)
        return dimg, (dz.reshape(zshape) if want_z else None)


# PCGAN_CONCATZ_FUSED=0 (read once, when this module is imported) keeps _ConcatZFn even inside fused_concat_bwd() -- the A/B switch of
# scripts/bench_bigan.py, as PCGAN_FANOUT is for fan_out
_CONCATZ_FUSED_ENV = os.environ.get('PCGAN_CONCATZ_FUSED', '1') != '0'
_concatz_fused = False


@contextlib.contextmanager
def fused_concat_bwd(enabled=True):
    """concat_z calls made inside take the one-launch backward pass (_ConcatZFusedFn) where it has been measured to pay (fused_serves: a
    rating that needs a gradient; a shared one only over few, small planes).  Read when concat_z runs, i.e. at forward time: the backward
    pass of a graph built inside may run anywhere."""
    global _concatz_fused
    old, _concatz_fused = _concatz_fused, bool(enabled)
    try:
        yield
    finally:
        _concatz_fused = old


# Where the one-launch backward pass is taken (measured: scripts/bench_bigan.py, profiles/bigan_step.json).
#   * The rating needs no gradient: the chain is then ONE strided copy, there is nothing to fuse, and the two are level to within the
#     spread between runs -- the default function stays.
#   * One rating shared by the batch (z_batch == 1 < N): ONE workgroup of the fused kernel walks all N planes of a rating channel, at
#     1.1 us (32 KiB plane) to 6.4 us (256 KiB) per plane, where the chain's plane sums use N workgroups and the whole chain takes
#     35 us.  Measured at 128 x 128: the fused call wins at N = 10 (fp32, 640 KiB of planes) and N = 16 (bf16, 512 KiB), loses at
#     N = 16 (fp32, 1 MiB) and N = 24 (bf16, 768 KiB) and everywhere above.  It is taken inside the measured winning region only.
FUSED_SHARED_MAX_PLANES = 16
FUSED_SHARED_MAX_BYTES = 640 << 10


def fused_serves(N, plane_bytes, z_batch):
    """whether the one-launch backward pass is taken for the gradient of a rating of batch `z_batch` joined to N planes of plane_bytes"""
    return z_batch == N or (N <= FUSED_SHARED_MAX_PLANES and N * plane_bytes <= FUSED_SHARED_MAX_BYTES)


def concat_z(img, z):
    """torch.cat((img, z broadcast over H,W), 1); z is (B or 1, nz, 1, 1)."""
    if _concatz_fused and _CONCATZ_FUSED_ENV and z.requires_grad:
        if fused_serves(img.size(0), img.size(2) * img.size(3) * img.element_size(), z.size(0)):
            return _ConcatZFusedFn.apply(img, z)
    return _ConcatZFn.apply(img, z)


class _SkipJoinFn(torch.autograd.Function):
    """torch.cat((act_a(a), act_b(b)), 1) as one launch per pass (ops.skip_join_fwd / skip_join_bwd); an input is saved only for a ReLU"""

    @staticmethod
    def forward(ctx, a, b, act_a, act_b):
        a, b = _c(a), _c(b)
        ctx.cfg = (a.shape[1], act_a, act_b)
        ctx.save_for_backward(a if act_a != ACT_NONE else None, b if act_b != ACT_NONE else None)
        return ops.skip_join_fwd(a, b, act_a, act_b)

    @staticmethod
    def backward(ctx, dout):
        a, b = ctx.saved_tensors
        Ca, act_a, act_b = ctx.cfg
        da, db = ops.skip_join_bwd(_c(dout), a, b, Ca, act_a, act_b, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return da, db, None, None


def skip_join(a, b, act_a=ACT_NONE, act_b=ACT_NONE):
    """The U-Net skip connection (reference models/networks.py:729-733): torch.cat((a, b), 1) with the parent block's ReLU optionally
    folded into either half (act_a / act_b: ACT_NONE or ACT_RELU)."""
    return _SkipJoinFn.apply(a, b, act_a, act_b)


class _FanOutFn(torch.autograd.Function):
    """n aliases of x (no copy, no launch); the backward pass sums the gradients that arrived in ONE ops.add_n launch, in output order,
    where autograd would chain binary adds"""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        live = [g for g in grads if g is not None]
        if not live:
            return None, None
        if len(live) == 1:
            return live[0], None
        if any(g.dtype != live[0].dtype for g in live):
            raise RuntimeError('pcgan_amd: fan_out received gradients of mixed dtypes: %s' % sorted(set(str(g.dtype) for g in live)))
        return ops.add_n([_c(g) for g in live]), None


def fan_out(x, n):
    """x for n consumers: a tuple of n aliases whose gradients are summed by one kernel launch ((g0 + g1) + g2 ..., fp32, in output
    order).  Outputs that are never used, or whose gradient is None, are skipped; a single gradient is handed on as it is."""
    if not 1 <= n <= ops._L.ADD_N_MAX:
        raise ValueError('pcgan_amd: fan_out serves 1 .. %d consumers, got %r' % (ops._L.ADD_N_MAX, n))
    return _FanOutFn.apply(x, n)


class _ChannelScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask_nc, scale):
        ctx.scale = scale
        ctx.save_for_backward(mask_nc)
        return ops.channel_scale(_c(x), mask_nc, scale)

    @staticmethod
    def backward(ctx, dy):
        (mask_nc,) = ctx.saved_tensors
        return ops.channel_scale(_c(dy), mask_nc, ctx.scale), None, None


def dropout2d(x, p, training=True, mask=None):
    """nn.Dropout2d: whole (n,c) planes zeroed with probability p, survivors scaled by 1/(1-p).
    `mask` (N*C keep flags) can be injected for parity tests; otherwise it is drawn with
    torch's device RNG (host-side RNG plumbing, cannot match a CPU stream anyway)."""
    if not training or p <= 0.0:
        return x
    N, C = x.shape[0], x.shape[1]
    if mask is None:
        mask = _keep_flags(N * C, p, x.device)
    return _ChannelScaleFn.apply(x, mask.reshape(-1).contiguous(), 1.0 / (1.0 - p))


# Keep flags are independent Bernoulli(1 - p) draws from torch's device generator: drawn 65536 at a time and handed out in
# consecutive slices (a Bayesian step calls Dropout2d 540 times -- 18 sites x 30 encoder passes -- with 100-4000 flags each: one
# bernoulli_ launch per ~2 encoder passes instead of one per call).  Slices are never reused.
_FLAG_POOL = {}
_FLAG_POOL_SIZE = 1 << 16


def _keep_flags(n, p, device):
    if n > _FLAG_POOL_SIZE // 4:
        return torch.empty(n, dtype=torch.float32, device=device).bernoulli_(1.0 - p)
    # A re-seed (torch.manual_seed) must not be followed by leftover flags of the old stream: the pool remembers the generator's
    # seed and its Philox offset right after the refill; a different seed, or an offset that went BACKWARDS (same seed again),
    # means the generator was re-seeded since -> refill, so a seeded MC-dropout run is reproducible from its seed.
    cuda = device.type == 'cuda'
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()] if cuda else torch.default_generator
    seed, offset = gen.initial_seed(), (gen.get_offset() if cuda else 0)
    key = (device, float(p), torch.cuda.current_stream(device).cuda_stream if cuda else 0)
    ent = _FLAG_POOL.get(key)
    if ent is None or ent[1] + n > _FLAG_POOL_SIZE or ent[2] != seed or offset < ent[3]:
        buf = torch.empty(_FLAG_POOL_SIZE, dtype=torch.float32, device=device).bernoulli_(1.0 - p)
        ent = _FLAG_POOL[key] = [buf, 0, seed, gen.get_offset() if cuda else 0]
    o = ent[1]
    ent[1] = o + n
    return ent[0][o:o + n]


def reset_flag_pool():
    """drop every pre-drawn keep flag (call after re-seeding by other means than torch.manual_seed, e.g. set_rng_state)"""
    _FLAG_POOL.clear()


# ---------------------------------------------------------------------------- pooling / resize
class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, stride, pad):
        x = _c(x)
        y, arg = ops.maxpool_fwd(x, k, stride, pad)
        ctx.cfg = (tuple(x.shape[2:]), k, stride, pad)
        ctx.save_for_backward(arg)
        ctx.mark_non_differentiable(arg)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        hw, k, stride, pad = ctx.cfg
        return ops.maxpool_bwd(_c(dy), arg, hw, k, stride, pad), None, None, None


def max_pool2d(x, k, stride, pad=0):
    return _MaxPoolFn.apply(x, k, stride, pad)


class _AvgPoolPyramidFn(torch.autograd.Function):
    """(x0, x1, ...): x0 an alias of x, x_{i+1} = avgpool(x_i), one launch per level.  The backward pass folds the gradients from the
    coarsest level up, g0 + bwd(g1 + bwd(g2 + ...)): one ops.avgpool_bwd launch per level with the level's own gradient riding in as
    `base`, so autograd adds nothing itself for the image gradient."""

    @staticmethod
    def forward(ctx, x, levels, k, stride, pad):
        ctx.set_materialize_grads(False)
        ctx.cfg = (k, stride, pad)
        out, cur = [x.view_as(x)], _c(x)
        for _ in range(levels - 1):
            cur = ops.avgpool_fwd(cur, k, stride, pad)
            out.append(cur)
        ctx.hw = [tuple(t.shape[2:]) for t in out]
        return tuple(out)

    @staticmethod
    def backward(ctx, *grads):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        carry = None
        for i in range(len(grads) - 1, -1, -1):
            g = _c(grads[i])
            carry = g if carry is None else ops.avgpool_bwd(carry, ctx.hw[i], *ctx.cfg, base=g)
        return carry, None, None, None, None


def avg_pool_pyramid(x, levels, k=3, stride=2, pad=1):
    """The image pyramid of the multi-scale discriminator (reference models/networks.py:1897, 1940-1949): (x0, ..., x_{levels-1}) with
    x0 = x (an alias) and x_{i+1} = AvgPool2d(k, stride, pad, count_include_pad=False)(x_i).  Levels whose gradient is None are skipped
    in the backward pass; levels == 1 returns (x,) without a launch."""
    if levels < 1:
        raise ValueError('pcgan_amd: avg_pool_pyramid needs levels >= 1, got %r' % (levels,))
    if levels == 1:
        ops._act(_c(x))      # refuses CPU tensors and foreign dtypes although nothing is launched
        return (x,)
    return _AvgPoolPyramidFn.apply(x, levels, k, stride, pad)


class _GlobalPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, is_max):
        x = _c(x)
        y, arg = ops.global_pool_fwd(x, is_max)
        ctx.cfg = (tuple(x.shape[2:]), is_max)
        ctx.save_for_backward(arg)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        hw, is_max = ctx.cfg
        return ops.global_pool_bwd(_c(dy), arg, hw, is_max), None


def global_pool(x, is_max):
    """nn.AvgPool2d(H) / nn.MaxPool2d(H) over the whole plane."""
    return _GlobalPoolFn.apply(x, bool(is_max))


class _BilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size):
        x = _c(x)
        ctx.hw = tuple(x.shape[2:])
        return ops.bilinear_fwd(x, (size, size))

    @staticmethod
    def backward(ctx, dy):
        return ops.bilinear_bwd(_c(dy), ctx.hw), None


def upsample2d(x, size):
    """util.upsample2d (util/util.py:111-117): identity if size <= 0 or already that size."""
    if size <= 0 or x.size(2) == size:
        return x
    return _BilinearFn.apply(x, int(size))


# ---------------------------------------------------------------------------- storage casts (bf16 path boundary)
class _CastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return ops.cast(_c(x), dtype)

    @staticmethod
    def backward(ctx, dy):
        return ops.cast(_c(dy), ctx.src), None


def cast(x, dtype):
    """x in another activation storage type (torch.float32 / torch.bfloat16), differentiable; identity if it already is"""
    return x if x.dtype == dtype else _CastFn.apply(x, dtype)


# ---------------------------------------------------------------------------- losses
class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, a, b):
        a, b = _c(a), _c(b)
        want = a.requires_grad
        if kind == 'bce':
            loss, grad = ops.bce_loss(a, b, want)
        elif kind == 'l1':
            loss, grad = ops.l1_loss(a, b, want)
        else:
            loss, grad = ops.mse_loss(a, b, want)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, dl):
        (grad,) = ctx.saved_tensors
        if grad is None:
            return None, None, None
        # d loss / d a, scaled by the upstream scalar which stays on the device
        return None, ops.scale(grad, _c(dl).reshape(1)), None


# ---------------------------------------------------------------------------- classifier head (training pass)
def _linear_backward(ctx, dlogits, x, w):
    """(dx, dw, db) of the head for autograd: dw / db go straight into the FusedAdam gradient buffer when both parameters have one
    (autograd then receives None for them, as in _Conv2dFn.backward)"""
    pw, pb = ctx.params
    want_w, want_b = ctx.needs_input_grad[1], pb is not None and ctx.needs_input_grad[2]
    tw = _fused_grad_target(pw) if want_w else None
    tb = _fused_grad_target(pb) if want_b else None
    fused = (want_w or want_b) and (not want_w or tw is not None) and (not want_b or tb is not None)
    dx, dw, db = ops.linear_bwd(dlogits, x, w, ctx.needs_input_grad[0], want_w, want_b, tw if fused else None, tb if fused else None)
    return (dx, None, None) if fused else (dx, dw, db)


class _LinearFn(torch.autograd.Function):
    """logits = x w^T + b (pcgan_linear_softmax_fwd's logits) with pcgan_linear_bwd as its backward"""

    @staticmethod
    def forward(ctx, x, w, b):
        from . import inception as I
        x, w, b = _c(x), _c(w), _c(b)
        ctx.params = (w, b)
        ctx.save_for_backward(x, w)
        return I.linear_softmax(x, w, b)[0]

    @staticmethod
    def backward(ctx, dlogits):
        x, w = ctx.saved_tensors
        return _linear_backward(ctx, _c(dlogits), x, w)


def linear(x, w, b):
    """nn.Linear on (N, C) rows, differentiable"""
    return _LinearFn.apply(x, w, b)


class _LinearCeFn(torch.autograd.Function):
    """nn.Linear + nn.CrossEntropyLoss(weight) as ONE node (pcgan_linear_ce_fwd): the forward launch leaves d loss / d logits behind, the
    backward is pcgan_linear_bwd.  Only `loss` is differentiable; logits, pred and correct are by-products for the caller's accuracy."""

    @staticmethod
    def forward(ctx, x, w, b, labels, class_weight):
        x, w, b = _c(x), _c(w), _c(b)
        want = x.requires_grad or w.requires_grad or (b is not None and b.requires_grad)
        loss, logits, dlogits, pred, correct = ops.linear_ce_fwd(x, w, b, _c(labels), class_weight, want)
        ctx.params = (w, b)
        ctx.save_for_backward(x, w, dlogits)
        ctx.mark_non_differentiable(logits, pred, correct)
        return loss, logits, pred, correct

    @staticmethod
    def backward(ctx, dloss, *unused):
        x, w, dlogits = ctx.saved_tensors
        # d loss / d logits, scaled by the upstream scalar which stays on the device
        dl = ops.scale(dlogits, _c(dloss).reshape(1))
        return _linear_backward(ctx, dl, x, w) + (None, None)


def linear_cross_entropy(x, w, b, labels, class_weight=None):
    """(loss, logits, pred, correct) of CrossEntropyLoss(class_weight)(nn.Linear(x), labels), mean reduction; pred = first arg-max of
    every row, correct = number of rows with pred == label (device tensors)"""
    return _LinearCeFn.apply(x, w, b, labels, class_weight)


# ---------------------------------------------------------------------------- end of the attribute regressor
_UNIT = {}


def unit_gradient(like):
    """THE gradient 1 of a scalar on `like`'s device: one cached 0-dim fp32 tensor per device.  `loss.backward(unit_gradient(loss))` is
    `loss.backward()` whose factor a node can recognise on the host (by address) without reading device memory: _PooledMseFn then hands
    its stored gradient on as it is.  Any other incoming gradient -- the implicit ones of a bare backward() included -- is a device
    value the host does not look at, and goes through pcgan_scale."""
    key = like.device
    if key not in _UNIT:
        _UNIT[key] = torch.ones((), dtype=torch.float32, device=like.device)
    return _UNIT[key]


class _PooledMseFn(torch.autograd.Function):
    """global pooling + nn.MSELoss + the "within delta" count as ONE node (pcgan_pool_mse_fwd): the forward launch leaves d loss / d x
    behind, so backward launches nothing when the incoming factor is unit_gradient() and one pcgan_scale otherwise.  Only `loss` is
    differentiable; pred and hits are by-products for the caller's accuracy."""

    @staticmethod
    def forward(ctx, x, target, delta, is_max):
        x = _c(x)
        loss, pred, hits, dx, _ = ops.pool_mse_fwd(x, _c(target), delta, is_max, 1.0, x.requires_grad)
        ctx.save_for_backward(dx)
        ctx.mark_non_differentiable(pred, hits)
        ctx.set_materialize_grads(False)
        return loss, pred, hits

    @staticmethod
    def backward(ctx, dloss, *unused):
        (dx,) = ctx.saved_tensors
        if dx is None or dloss is None:
            return None, None, None, None
        unit = _UNIT.get(dloss.device)
        if unit is not None and dloss.data_ptr() == unit.data_ptr():
            return dx, None, None, None
        # d loss / d x, scaled by the upstream scalar which stays on the device
        return ops.scale(dx, _c(dloss).to(torch.float32).reshape(1)), None, None, None


def pooled_mse(x, target, delta, is_max):
    """(loss, pred, hits) of nn.MSELoss()(pool(x), target) for x (N, F, H, W), pool = nn.MaxPool2d(H) (is_max) or nn.AvgPool2d(H):
    pred (N, F, 1, 1) fp32, hits = #{|pred - target| < delta} (a 0-dim int32 device tensor)"""
    return _PooledMseFn.apply(x, target, float(delta), bool(is_max))


# ---------------------------------------------------------------------------- online pair selection + BCE (siamese_online.py)
class _OnlinePairBceFn(torch.autograd.Function):
    """pair selection + draw-aware BCE + rating regularizer + predictions as ONE node (pcgan_online_pair_bce): the forward launch leaves
    d loss3[2] / d f1 and / d f2 behind, so backward launches nothing when the incoming factor is unit_gradient() and one pcgan_scale per
    rating otherwise.  Only `total` (= loss3[2]) carries the graph; loss3 and picks are by-products for the caller's log and file."""

    @staticmethod
    def forward(ctx, f1, f2, label, k, descending, draw_thresh, lambda_reg, key):
        f1, f2 = _c(f1), _c(f2)
        want = f1.requires_grad or f2.requires_grad
        loss3, picks, df1, df2 = ops.online_pair_bce(f1, f2, _c(label), k, descending, draw_thresh, lambda_reg, 1.0,
                                                     None if key is None else _c(key), want)
        # loss3[2] as an output of its own over the same storage (no launch, and no view relation for autograd to track)
        total = torch.empty((0,), dtype=torch.float32, device=loss3.device).set_(loss3.untyped_storage(), loss3.storage_offset() + 2, (), ())
        ctx.save_for_backward(df1, df2)
        ctx.mark_non_differentiable(loss3, picks)
        ctx.set_materialize_grads(False)
        return total, loss3, picks

    @staticmethod
    def backward(ctx, dtotal, *unused):
        df1, df2 = ctx.saved_tensors
        none = (None,) * 6
        if df1 is None or dtotal is None:
            return (None, None) + none
        unit = _UNIT.get(dtotal.device)
        if unit is not None and dtotal.data_ptr() == unit.data_ptr():
            return (df1, df2) + none
        factor = _c(dtotal).to(torch.float32).reshape(1)
        return (ops.scale(df1, factor) if ctx.needs_input_grad[0] else None,
                ops.scale(df2, factor) if ctx.needs_input_grad[1] else None) + none


def online_pair_bce(f1, f2, label, k, descending, draw_thresh, lambda_reg=0.0, key=None):
    """(total, loss3, picks) of the online trainer's loss on the ratings f1, f2 (any shape with N elements) and the int64 labels (0: the
    first rates higher): loss3 = (bce over the k kept pairs, regularizer, sum), total = loss3[2] with the graph attached, picks = (sel[k],
    pseudo[k], pred[N]) int32 -- see ops.online_pair_bce"""
    return _OnlinePairBceFn.apply(f1, f2, label, int(k), bool(descending), float(draw_thresh), float(lambda_reg), key)


# ---------------------------------------------------------------------------- projection discriminator head
class _ProjectionHeadFn(torch.autograd.Function):
    """The head of NLayerProjectionDiscriminator (reference models/networks.py:830-838) as ONE node: pcgan_proj_head_fwd leaves the plane
    sums h behind, the backward is pcgan_proj_head_bwd.  The four parameter gradients go straight into the FusedAdam gradient buffer when
    every wanted one has a slice there (autograd then receives None for them, as in _Conv2dFn.backward)."""

    @staticmethod
    def forward(ctx, p, y, psi_w, psi_b, ly_w, ly_b, sigmoid):
        p, y = _c(p), _c(y)
        out, h = ops.proj_head_fwd(p, y, _c(psi_w), _c(psi_b), _c(ly_w), _c(ly_b), sigmoid)
        ctx.cfg = (tuple(p.shape[2:]), bool(sigmoid))
        ctx.params = (psi_w, psi_b, ly_w, ly_b)
        ctx.save_for_backward(h, y, psi_w, psi_b, ly_w, ly_b)
        return out

    @staticmethod
    def backward(ctx, g):
        h, y, psi_w, psi_b, ly_w, ly_b = ctx.saved_tensors
        hw, sigmoid = ctx.cfg
        want = tuple(ctx.needs_input_grad[2:6])
        targets = [_fused_grad_target(q) if w else None for q, w in zip(ctx.params, want)]
        fused = any(want) and all(t is not None for t, w in zip(targets, want) if w)
        res = ops.proj_head_bwd(_c(g), h, y, _c(psi_w), _c(psi_b), _c(ly_w), _c(ly_b), hw, sigmoid, ctx.needs_input_grad[0], want,
                                ctx.needs_input_grad[1], targets if fused else None)
        dp, dy = res[0], res[5]
        if fused:
            return dp, dy, None, None, None, None, None
        return (dp, dy) + tuple(None if t is None else t.view_as(q) for t, q in zip(res[1:5], ctx.params)) + (None,)


def projection_head(p, y, psi_w, psi_b, ly_w, ly_b, sigmoid):
    """out (B, 1, 3, 3) = sum_c h wy + psi(h) of the projection discriminator, h = plane sums of p (B, C, H, W), wy = l_y(y); y is
    (By, nz) fp32 with By in {1, B}; sigmoid folds torch.sigmoid in.  Gradients reach p, y and the four parameters."""
    return _ProjectionHeadFn.apply(p, y, psi_w, psi_b, ly_w, ly_b, sigmoid)


def bce_loss(pred, target_n):
    """nn.BCELoss(mean) of pred[N,...] against a per-sample target (float tensor [N])."""
    return _LossFn.apply('bce', pred, target_n)


def l1_loss(a, b):
    return _LossFn.apply('l1', a, b)


def mse_loss(a, b):
    return _LossFn.apply('mse', a, b)
