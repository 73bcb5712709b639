"""GPU: the attribute regressor -- the fused pooling + MSE + accuracy + gradient kernel alone against float64, its autograd node, one
training step of the whole regressor (resnet18 / resnet50 / alexnet) against the float64 twin of tests/regression_ref.py, and
regression.py end to end.

Head tolerance, the project's rule through test_gpu_inception._rule as it stands: ||hip - f64|| <= 2 ||torch_fp32_cpu - f64||
+ 1e-30 (the guard for 0 against 0), for pred, the scalar loss and dx.  The kernel sums in float64 and rounds once, so pred and dx are
the fp32 numbers nearest to what float64 arithmetic gives from the kernel's own pred; the maximum is exact.  argmax and hits are exact.
bf16 storage is pinned to the fp32-storage run on the up-cast values bit for bit (dx after .to(torch.bfloat16)), which the rule covers.
"""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import regression_ref as R
from oracle import networks_ref as N
from oracle import weights as W
from test_gpu_inception import _rule
from test_gpu_inception_score import _random_resnet_sd
from test_gpu_nets import _compare, _assert_mostly_close, record_decisions
from util_cmp import assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _held(got, y32, y64, what):
    print('%s: |hip - f64| = %.3e, |torch fp32 - f64| = %.3e' % (what, float((got.detach().double().cpu() - y64.double()).norm()),
                                                              float((y32.double() - y64.double()).norm())))
    _rule(got, y32, y64, what)


# ---- the kernel alone --------------------------------------------------------------------------------------------------------------
# (N, F, HW), planes of up to 64 elements being staged 128 per workgroup: one value; one 7x7 plane; the script's batch (one partly
# filled workgroup); the golden 6x6 / 3x3 maps; an even plane of no multiple of 4 elements over 21 planes; 16 and 48 full workgroups of
# 7x7 / 2x2 planes; 512 8x8 planes (the longest staged plane, even: its LDS rows are padded); a plane longer than the staged path (one
# workgroup per plane, 4099 = 16 * 256 + 3)
SHAPES = [(1, 1, 1), (1, 1, 49), (100, 1, 49), (6, 1, 36), (5, 2, 9), (7, 3, 50), (4, 512, 49), (3, 2048, 4), (512, 1, 64), (2, 1, 4099)]
DELTA = 0.05


def _case(N_, F_, HW, is_max, seed, bf16):
    """x (N, F, H, W) with H W = HW (H = 1 when HW is no square: the kernel sees planes), and targets beside the float64 prediction:
    every third within 0.01 of it (inside DELTA), the others 0.1 .. 0.6 away (outside)"""
    g = torch.Generator().manual_seed(seed)
    side = int(round(HW ** 0.5))
    hw = (side, side) if side * side == HW else (1, HW)
    x = torch.randn(N_, F_, *hw, generator=g)
    if bf16:
        x = x.to(torch.bfloat16).float()
    if is_max:
        # ONE maximum per plane (bf16 values tie easily, and torch sends a tied maximum's gradient wherever it likes): lift it by 1
        flat = x.view(N_, F_, HW)
        top = flat.argmax(2, keepdim=True)
        flat.scatter_(2, top, (flat.gather(2, top) + 1.0).to(torch.bfloat16).float() if bf16 else flat.gather(2, top) + 1.0)
    p64 = x.double().flatten(2).amax(2) if is_max else x.double().flatten(2).mean(2)
    k = torch.arange(N_ * F_).view(N_, F_)
    off = torch.where(k % 3 == 0, 0.01 * torch.rand(N_, F_, generator=g).double(), 0.1 + 0.5 * torch.rand(N_, F_, generator=g).double())
    sign = torch.where(torch.rand(N_, F_, generator=g) < 0.5, -1.0, 1.0).double()
    t = (p64 + sign * off).float()
    return x, t


def _torch_ref(x, t, is_max, gscale, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    flat = x.flatten(2)
    p = flat.max(dim=2).values if is_max else flat.mean(dim=2)
    loss = ((p - t.to(dtype)) ** 2).mean()
    (gscale * loss).backward()
    return dict(pred=p.detach().view(x.shape[0], x.shape[1], 1, 1), loss=loss.detach().reshape(1), dx=x.grad)


def _one_past(t, dev):
    """a contiguous copy of t on the device that starts ONE ELEMENT past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


@pytest.mark.parametrize('is_max', [False, True], ids=['mean', 'max'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_head_kernel_against_float64(dev, shape, is_max):
    from pcgan_amd.hip import ops
    N_, F_, HW = shape
    for bf16 in (False, True):
        x, t = _case(N_, F_, HW, is_max, N_ * 7919 + F_ * 31 + HW + int(is_max), bf16)
        td = t.to(dev)
        for gscale in (1.0, 0.5):
            what = 'N %d F %d HW %d %s %s gscale %g' % (N_, F_, HW, 'max' if is_max else 'mean', 'bf16' if bf16 else 'fp32', gscale)
            r32, r64 = _torch_ref(x, t, is_max, gscale, torch.float32), _torch_ref(x, t, is_max, gscale, torch.float64)
            xd = x.to(dev)
            loss, pred, hits, dx, arg = ops.pool_mse_fwd(xd, td, DELTA, is_max, gscale)
            again = ops.pool_mse_fwd(xd, td, DELTA, is_max, gscale)
            off = ops.pool_mse_fwd(_one_past(xd, dev), td, DELTA, is_max, gscale)
            torch.cuda.synchronize()
            assert pred.dtype == torch.float32 and tuple(pred.shape) == (N_, F_, 1, 1) and dx.dtype == torch.float32
            got = dict(pred=pred, loss=loss.reshape(1), dx=dx)
            for k, v in got.items():
                assert bool(torch.isfinite(v).all()), '%s: %s not finite' % (what, k)
                _held(v, r32[k], r64[k], '%s: %s' % (what, k))
            # hits: the fp32 comparison on the returned pred, exactly
            want_hits = int((torch.abs(pred.cpu() - t.view_as(pred)) < DELTA).sum())
            assert hits.dtype == torch.int32 and int(hits) == want_hits, '%s: hits %d, torch %d' % (what, int(hits), want_hits)
            if N_ * F_ >= 3:
                assert 0 < want_hits < N_ * F_, what + ': the targets put predictions inside and outside delta'
            assert int(ops.pool_mse_fwd(xd, td, 0.0, is_max, gscale, False)[2]) == 0, what + ': delta 0 counts nothing'
            assert int(ops.pool_mse_fwd(xd, td, 1e30, is_max, gscale, False)[2]) == N_ * F_, what + ': a huge delta counts everything'
            # the first maximum, as pcgan_global_pool_fwd
            if is_max:
                assert arg.dtype == torch.int32 and torch.equal(arg, ops.global_pool_fwd(xd, True)[1]), what + ': argmax'
                assert torch.equal(arg.cpu().long().view(N_, F_), x.flatten(2).argmax(2)), what + ': argmax vs torch'
            else:
                assert arg is None
            # run to run, and the element-wise access path
            for name, other in (('two runs', again), ('one element past a 16-byte boundary', off)):
                for a, c in zip((loss, pred, hits, dx) + ((arg,) if is_max else ()), other):
                    assert torch.equal(a, c), '%s: %s differ' % (what, name)
            if bf16:
                # bf16 storage: the same pred / loss / hits / argmax, dx = the fp32-storage gradient rounded to bf16 (nearest even)
                xb = x.to(torch.bfloat16).to(dev)
                assert torch.equal(xb.float(), xd)
                for src in (xb, _one_past(xb, dev)):
                    lb, pb, hb, dxb, ab = ops.pool_mse_fwd(src, td, DELTA, is_max, gscale)
                    torch.cuda.synchronize()
                    assert dxb.dtype == torch.bfloat16 and pb.dtype == torch.float32
                    assert torch.equal(lb, loss) and torch.equal(pb, pred) and torch.equal(hb, hits), what + ': bf16 storage scalars'
                    assert (ab is None and arg is None) or torch.equal(ab, arg)
                    assert torch.equal(dxb.view(torch.int16), dx.to(torch.bfloat16).view(torch.int16)), what + ': bf16 dx bits'


@pytest.mark.parametrize('HW', [49, 64, 4099])
def test_ties_constant_planes_and_exact_targets(dev, HW):
    """argmax is 0 on a constant plane and the first index on two equal maxima (in one lane's walk, and for the long planes in
    different threads and waves); a row whose target IS its prediction has a zero gradient, counts as a hit for every delta > 0 and
    not for delta = 0; |pred - target| == delta is no hit (strict)"""
    from pcgan_amd.hip import ops
    g = torch.Generator().manual_seed(HW)
    x = torch.randn(6, 1, 1, HW, generator=g).clamp(-3, 3)
    x[0] = 0.25                                              # constant
    x[1, 0, 0, 5], x[1, 0, 0, 40] = 7.0, 7.0                 # two equal maxima
    lo, hi = (HW // 3, HW - 2)
    x[2, 0, 0, hi], x[2, 0, 0, lo] = 9.0, 9.0                # ... far apart: other threads / waves on the long path
    x[3, 0, 0, HW - 1] = 8.0                                 # the last element
    x[4, 0, 0, min(HW - 1, 300)], x[4, 0, 0, min(HW - 2, 100)] = 6.0, 6.0
    xd = x.to(dev)
    t = torch.zeros(6, 1)
    for is_max in (True, False):
        loss, pred, hits, dx, arg = ops.pool_mse_fwd(xd, t.to(dev), DELTA, is_max)
        if is_max:
            assert arg.view(-1).tolist()[:5] == [0, 5, lo, HW - 1, min(HW - 2, 100)]
            assert torch.equal(arg, ops.global_pool_fwd(xd, True)[1])
            assert pred.view(-1).tolist()[:5] == [0.25, 7.0, 9.0, 8.0, 6.0]
        # targets equal to the returned predictions on rows 1, 3, 5
        t2 = t.clone()
        for r in (1, 3, 5):
            t2[r, 0] = float(pred[r, 0, 0, 0])
        loss2, pred2, hits2, dx2, _ = ops.pool_mse_fwd(xd, t2.to(dev), 1e-6, is_max)
        torch.cuda.synchronize()
        assert torch.equal(pred2, pred)
        for r in (1, 3, 5):
            assert float(dx2[r].abs().max()) == 0.0, 'row %d: target == pred, the gradient is zero' % r
        assert float(dx2[0].abs().max()) > 0 and int(hits2) == int((torch.abs(pred2.cpu().view(6, 1) - t2) < 1e-6).sum()) >= 3
        assert int(ops.pool_mse_fwd(xd, t2.to(dev), 0.0, is_max, 1.0, False)[2]) == 0
        # one non-zero gradient element per plane for the maximum, HW equal ones for the mean
        nz = (dx2 != 0).flatten(1).sum(1).tolist()
        assert nz == ([1, 0, 1, 0, 1, 0] if is_max else [HW, 0, HW, 0, HW, 0])
    # strictness at the boundary: planes of one value, pred = x exactly
    xs = torch.tensor([1.0, 1.0, 1.0]).view(3, 1, 1, 1).to(dev)
    ts = torch.tensor([0.5, 0.75, 1.5]).to(dev)
    assert int(ops.pool_mse_fwd(xs, ts, 0.5, False, 1.0, False)[2]) == 1      # |1 - 0.5| == delta and |1 - 1.5| == delta: no hits
    assert int(ops.pool_mse_fwd(xs, ts, 0.5, True, 1.0, False)[2]) == 1


def _raw(h, lib, x, t, outs, ws, N_, F_, HW, is_max, delta=DELTA, gscale=1.0):
    """pcgan_pool_mse_fwd itself: outs = (pred, argmax, dx, loss, hits), each a tensor or None"""
    p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None     # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt = lib.BF16 if x.dtype == torch.bfloat16 else lib.F32
    status = h.pcgan_pool_mse_fwd(p(x), p(t), *[p(o) for o in outs], p(ws), ws.numel() * 8, N_, F_, HW, int(is_max), delta, gscale, dt, st)
    assert status == 0, h.pcgan_last_error()


def test_optional_outputs_and_the_ticket(dev):
    """every output may be NULL; calls of different sizes, staged and long, share one workspace in stream order and leave its ticket
    word zero"""
    from pcgan_amd.hip import lib, ops
    h = lib.load()
    ws = torch.zeros(1 + 2 * 100 * 512, dtype=torch.float64, device=dev)
    for (N_, F_, HW), is_max in (((100, 512, 49), True), ((7, 3, 50), False), ((2, 1, 4099), True), ((1, 1, 1), False), ((100, 1, 49), False)):
        x, t = _case(N_, F_, HW, is_max, 5 + N_, False)
        xd, td = x.to(dev), t.to(dev)
        loss, pred, hits, dx, arg = ops.pool_mse_fwd(xd, td, DELTA, is_max)

        def fresh():
            return (torch.full_like(pred, 3.0), torch.full((N_, F_), -7, dtype=torch.int32, device=dev), torch.full_like(dx, 3.0),
                    torch.full_like(loss, 3.0), torch.full_like(hits, -7))
        full = fresh()
        _raw(h, lib, xd, td, full, ws, N_, F_, HW, is_max)
        torch.cuda.synchronize()
        assert int(ws.view(torch.int32)[0]) == 0 and int(ws.view(torch.int32)[1]) == 0, 'the ticket is left zero'
        assert torch.equal(full[0], pred) and torch.equal(full[2], dx) and torch.equal(full[3], loss) and torch.equal(full[4], hits)
        assert torch.equal(full[1], arg) if is_max else bool((full[1] == -7).all()), 'argmax is written for the maximum only'
        # one output at a time (dx of the maximum with the argmax it needs), the others NULL and untouched
        for keep in ((0,), (3,), (4,), (1, 2) if is_max else (2,), (3, 4)):
            outs = fresh()
            _raw(h, lib, xd, td, tuple(o if i in keep else None for i, o in enumerate(outs)), ws, N_, F_, HW, is_max)
            torch.cuda.synchronize()
            for i in keep:
                assert torch.equal(outs[i], full[i]), 'output %d alone, N %d F %d HW %d' % (i, N_, F_, HW)
            assert int(ws.view(torch.int32)[0]) == 0
    # refused before any launch: the gradient of the maximum without argmax; a workspace that is too short
    outs = fresh()
    st = h.pcgan_pool_mse_fwd(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(td.data_ptr()), None, None, ctypes.c_void_p(outs[2].data_ptr()),
                              None, None, ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, N_, F_, HW, 1, DELTA, 1.0, lib.F32, None)
    assert st != 0 and b'argmax' in h.pcgan_last_error()
    st = h.pcgan_pool_mse_fwd(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(td.data_ptr()), None, None, None, None, None,
                              ctypes.c_void_p(ws.data_ptr()), 64, N_, F_, HW, 0, DELTA, 1.0, lib.F32, None)
    assert st != 0 and b'workspace' in h.pcgan_last_error()
    torch.cuda.synchronize()
    assert bool((outs[2] == 3.0).all())


# ---- the autograd node ---------------------------------------------------------------------------------------------------------------
def test_node_gradients_and_upstream_factor(dev):
    """functional.pooled_mse: d loss / d x against float64 on a leaf; an upstream factor scales it through ONE pcgan_scale, the unit
    gradient through none; under the regressor, gradients reach the conv head and the trunk and scale with the factor"""
    from pcgan_amd.hip import functional as HF, ops
    from pcgan_amd.models import networks
    x, t = _case(9, 2, 36, True, 77, False)
    calls = []
    orig = ops.scale

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    ops.scale = counted
    try:
        for is_max in (True, False):
            r32, r64 = _torch_ref(x, t, is_max, 3.0, torch.float32), _torch_ref(x, t, is_max, 3.0, torch.float64)
            xd = x.to(dev).requires_grad_(True)
            loss, pred, hits = HF.pooled_mse(xd, t.to(dev), DELTA, is_max)
            assert loss.requires_grad and not pred.requires_grad and not hits.requires_grad
            del calls[:]
            (3.0 * loss).backward()
            torch.cuda.synchronize()
            assert len(calls) == 1
            _held(xd.grad, r32['dx'], r64['dx'], 'autograd dx, factor 3')
            x1 = x.to(dev).requires_grad_(True)
            loss1 = HF.pooled_mse(x1, t.to(dev), DELTA, is_max)[0]
            del calls[:]
            loss1.backward(HF.unit_gradient(loss1))
            torch.cuda.synchronize()
            assert len(calls) == 0, 'the unit gradient hands the stored gradient on without a launch'
            assert torch.equal(x1.grad, ops.pool_mse_fwd(x.to(dev), t.to(dev), DELTA, is_max)[3])
            x2 = x.to(dev).requires_grad_(True)
            HF.pooled_mse(x2, t.to(dev), DELTA, is_max)[0].backward()           # a bare backward(): a device 1 the host does not read
            torch.cuda.synchronize()
            assert len(calls) == 1 and torch.equal(x2.grad, x1.grad)
            with torch.no_grad():
                l0, p0, h0 = HF.pooled_mse(x.to(dev), t.to(dev), DELTA, is_max)
            assert not l0.requires_grad and torch.equal(l0, loss.detach()) and torch.equal(p0, pred) and torch.equal(h0, hits)
    finally:
        ops.scale = orig
    torch.manual_seed(3)
    net = networks.define_AR('resnet18', init_type='normal', pooling='avg', cnn_dim=[8, 1]).to(dev).train()
    img = W.seeded_tensor((4, 3, 64, 64), 9).to(dev)
    target = torch.tensor([0.1, -0.2, 0.3, 0.0]).to(dev)
    grads = []
    for factor in (None, 3.0):
        net.zero_grad()
        loss = net.regress(img, target, DELTA)[0]
        if factor is None:
            loss.backward(HF.unit_gradient(loss))
        else:
            (factor * loss).backward()
        torch.cuda.synchronize()
        grads.append({k: p.grad.detach().clone() for k, p in net.named_parameters()})
    for k in ('cnn.3.weight', 'cnn.0.weight', 'base.model.layer4.1.conv2.weight', 'base.model.conv1.weight'):
        assert float(grads[0][k].abs().max()) > 0, k + ' receives a gradient'
        assert_close(grads[1][k], 3.0 * grads[0][k], 1e-4, 'factor 3 on d' + k)


# ---- the whole regressor ---------------------------------------------------------------------------------------------------------------
# (trunk, pooling, cnn_dim, image size, weight seed, output tolerance).  Sizes are the golden file's: 64 -> a 2 x 2 last feature map
# (5e-4, as the encoder test: few samples per BatchNorm channel), alexnet at 63 -> 1 x 1.  Resnet trunks take
# test_gpu_inception_score._random_resnet_sd (the norms that end a residual branch are scaled down, so activations stay O(1) through
# 16 blocks), the conv head and alexnet oracle/weights.py.
STEP_CASES = {
    'resnet18': ('resnet18', 'avg', (64, 1), 64, 81, 5e-4),
    'resnet50': ('resnet50', 'avg', (64, 1), 64, 91, 5e-4),
    'alexnet': ('alexnet', 'max', (64, 1), 63, 42, 5e-4),
    'resnet18_no_head': ('resnet18', 'max', (), 64, 81, 5e-4),
}
TARGET6 = torch.tensor([0.30, -0.45, 0.02, 0.75, -0.10, 0.55])


def _twin_and_input(case):
    which, pooling, cnn_dim, size, seed, tol = STEP_CASES[case]
    twin = R.RegressionNetworkRef(R.base_ref(which), pooling, cnn_dim, 1, 0.7)
    sd = W.fill_state_dict(twin.state_dict(), seed)
    if which != 'alexnet':
        sd.update({'base.model.' + k: v for k, v in _random_resnet_sd(twin.base.model, seed).items()})
    twin.load_state_dict(sd, strict=True)
    return twin, W.seeded_tensor((6, 3, size, size), 160 + seed), tol


def _hip_net(case):
    from pcgan_amd.models import networks
    which, pooling, cnn_dim, _, _, _ = STEP_CASES[case]
    base = networks.AlexNetFeature(3, pooling='') if which == 'alexnet' else networks.ResNetFeature(3, which)
    return networks.RegressionNetwork(base, pooling=pooling, cnn_dim=list(cnn_dim), cnn_pad=1, cnn_relu_slope=0.7)


@pytest.mark.parametrize('case', ['resnet18', 'alexnet'])
def test_regressor_forward_backward_against_the_twin(dev, case):
    """RegressionNetwork.forward(x) in train mode through test_gpu_nets._compare: the fp32 (N, 1, 1, 1) prediction, SHARP gradients on
    the HIP run's decisions, the LOOSE band on the twin's own, running statistics and num_batches_tracked"""
    twin, x, tol = _twin_and_input(case)
    _compare(_hip_net(case).train(), twin, [x], 300, dev, out_tol=tol)


@pytest.mark.parametrize('case', list(STEP_CASES))
def test_regressor_training_step_against_the_twin(dev, case):
    """regress() + backward + FusedAdam.step(): loss, pred, hits, SHARP parameter gradients against the float64 twin replaying the HIP
    run's decisions (the fused node's arg-max included); parameters after the step from the HIP run's gradients through the restated
    Adam; running statistics"""
    from pcgan_amd.hip import functional as HF, ops
    from pcgan_amd.hip.optim import FusedAdam
    twin, x, tol = _twin_and_input(case)
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    hip = _hip_net(case)
    hip.load_state_dict(sd, strict=True)
    hip = hip.to(dev).train()
    F_ = hip.feature_dim
    target = TARGET6.view(6, 1).repeat(1, F_).view(6, F_, 1, 1) * torch.linspace(1.0, 0.5, F_).view(1, F_, 1, 1)
    lr = 2e-4
    opt = FusedAdam(hip.parameters(), lr=lr)
    opt.zero_grad()
    orig = ops.pool_mse_fwd
    with record_decisions() as rec:
        def recorded(*a, **k):
            out = orig(*a, **k)
            if out[4] is not None:
                rec.tape.append(out[4].detach().cpu())
            return out
        ops.pool_mse_fwd = recorded
        try:
            loss, pred, hits = hip.regress(x.to(dev), target.to(dev), DELTA)
            loss.backward(HF.unit_gradient(loss))
        finally:
            ops.pool_mse_fwd = orig
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone().cpu() for k, p in hip.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    twin64 = copy.deepcopy(twin).double()
    N.DecisionTape.replay = iter(rec.tape)
    try:
        pred64, loss64, grads64, _ = R.train_step(twin64, x.double(), target.double(), lr)
        assert next(N.DecisionTape.replay, None) is None, 'the twin consumed fewer decisions than the HIP pass recorded'
    finally:
        N.DecisionTape.replay = None
    assert tuple(pred.shape) == (6, F_, 1, 1) and pred.dtype == torch.float32
    assert_close(pred, pred64, tol, 'pred')
    # loss = mean (pred - target)^2, so with |d pred| <= band = tol max|pred64|:  |d loss| <= 2 mean|pred64 - target| band + band^2
    band = tol * float(pred64.abs().max())
    loss_band = 2 * float((pred64 - target.double()).abs().mean()) * band + band * band
    got_loss = float(loss.detach())
    assert abs(got_loss - float(loss64)) <= loss_band, 'loss %.6e vs %.6e, band %.2e' % (got_loss, float(loss64), loss_band)
    assert int(hits) == int(R.within(pred, target, DELTA).sum())
    for k, g in grads.items():
        l2 = float((g.double() - grads64[k]).norm() / (grads64[k].norm() + 1e-300))
        print('%s d%s: relative L2 %.2e' % (case, k, l2))
    wmax = max(float(g.abs().max()) for g in grads64.values())
    for k, g in grads.items():
        if float(grads64[k].abs().max()) < 1e-5 * wmax:
            assert float(g.abs().max()) < 1e-3 * wmax + 1e-6, 'd%s should be ~0' % k       # cancelled by a following norm
            continue
        _assert_mostly_close(g, grads64[k], 'SHARP d%s vs fp64 twin on the HIP decisions' % k, 5e-4)
    for k, p in hip.named_parameters():
        want = R.adam_update(sd[k].double(), grads[k].double(), lr)
        err = float((p.detach().double().cpu() - want).abs().max())
        # one fp32 rounding of the parameter, and the fp32 arithmetic of an lr-sized update
        assert err <= 2.0 ** -23 * max(1.0, float(want.abs().max())) + 1e-5 * lr, 'parameter %s after the step: %.3e' % (k, err)
    hb = dict(hip.named_buffers())
    for k, b in twin64.named_buffers():
        if 'running' in k:
            assert_close(hb[k], b, 1e-4, 'buffer ' + k, atol=1e-6)
        else:
            assert int(hb[k]) == int(b) == 1, k


# ---- regression.py end to end ----------------------------------------------------------------------------------------------------------
N_IMAGES, SEED, BATCH = 12, 11, 4
MEAN_STD = ('40', '25')


def _dataset(root):
    """12 PNGs whose brightness follows their attribute; names <attribute>_<i>.png, two of the attributes with a fraction"""
    from PIL import Image
    rng = np.random.default_rng(21)
    os.makedirs(root)
    names = []
    for i in range(N_IMAGES):
        attr = 5 + 6 * i + (0.5 if i % 5 == 0 else 0)
        img = rng.integers(0, 64, (64, 64, 3)) + int(2 * attr)
        name = ('%g_%02d.png' % (attr, i))
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(root, name))
        names.append(name)
    return sorted(names)


def _script(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'regression.py')] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_script_trains_and_writes_the_embedding(dev, tmp_path):
    import regression as S
    from pcgan_amd.hip import functional as HF, ops
    from pcgan_amd.hip.optim import FusedAdam
    from pcgan_amd.models import networks
    names = _dataset(str(tmp_path / 'img'))
    common = [str(a) for a in ['--dataroot', tmp_path / 'img', '--name', 'reg_x', '--checkpoint_dir', tmp_path / 'checkpoints', '--which_model',
                               'resnet18', '--loadSize', 64, '--fineSize', 64, '--transforms', 'resize_and_crop', '--no_flip', '--seed', SEED,
                               '--embedding_mean', MEAN_STD[0], '--embedding_std', MEAN_STD[1], '--delta', 0.5, '--display_id', -1]]
    train_argv = common + ['--mode', 'train', '--num_epochs', '2', '--batch_size', str(BATCH), '--pretrained_model_path', '', '--num_workers', '0',
                           '--print_freq', '2', '--lr', '0.001', '--save_epoch_freq', '2']
    out = _script(train_argv)
    save_dir = tmp_path / 'checkpoints' / 'reg_x'
    assert 'epoch 01, iter 000002, loss: ' in out and 'dataset size = 12' in out
    for f in ('opt.txt', 'init_net.pth', 'latest_net.pth', '2_net.pth', 'loss.txt'):
        assert os.path.exists(save_dir / f), f
    with open(save_dir / 'loss.txt') as f:
        losses = [float(v) for v in f.read().split()]
    iters = N_IMAGES // BATCH
    assert len(losses) == 2 * iters and all(np.isfinite(losses)), 'loss.txt: one line per iteration'
    # the checkpoint: the reference's keys, loads strictly into define_AR(...) and into the twin
    ck = torch.load(save_dir / 'latest_net.pth', map_location='cpu')
    twin = R.RegressionNetworkRef(R.base_ref('resnet18'), 'avg', (64, 1), 1, 0.7)
    assert list(ck.keys()) == list(twin.state_dict().keys())
    twin.load_state_dict(ck, strict=True)
    net = networks.define_AR('resnet18', pooling='avg', cnn_dim=[64, 1], cnn_pad=1, cnn_relu_slope=0.7)
    net.load_state_dict(ck, strict=True)
    # the same two epochs here: same seed, same loader, the saved initial weights; hits counted ON THE HOST with the reference's formula
    opt = S.get_options(train_argv, save=False)
    S.K.seed_everything(opt.seed)
    replay = S.get_model(opt)
    replay.load_state_dict(torch.load(save_dir / 'init_net.pth', map_location='cpu'), strict=True)
    ops.invalidate_packed_weights()
    replay = replay.to(dev).train()
    loader = S.K.make_loader(opt, train=True)
    optimizer = FusedAdam(replay.parameters(), lr=opt.lr)
    S.K.seed_everything(opt.seed)
    first, accs, my_losses = None, [], []
    for epoch in (1, 2):
        count = 0
        for img0, path0 in loader:
            label = S.labels_of(path0, opt, 1)
            if first is None:
                first = (img0.clone(), label.clone())
            optimizer.zero_grad()
            loss, pred, _ = replay.regress(img0.to(dev), label.to(dev), opt.delta)
            loss.backward(HF.unit_gradient(loss))
            optimizer.step()
            count += int(np.count_nonzero((torch.abs(pred.cpu() - label) < opt.delta).view(-1).numpy()))      # get_accuracy
            my_losses.append(float(loss.detach()))
        accs.append(count / N_IMAGES)
    for epoch, acc in zip((1, 2), accs):
        assert 'epoch %02d: train accuracy %.4f' % (epoch, acc) in out, (accs, out[-600:])
    assert np.allclose(my_losses, losses, rtol=1e-3, atol=1e-6), (my_losses, losses)
    # the first iteration in float64 on the same batch; the whole net stands behind this number, so the fp32 side of the rule is the
    # twin's whole fp32 forward pass
    ref = {}
    for dt in (torch.float32, torch.float64):
        t0 = R.RegressionNetworkRef(R.base_ref('resnet18'), 'avg', (64, 1), 1, 0.7)
        t0.load_state_dict(torch.load(save_dir / 'init_net.pth', map_location='cpu'), strict=True)
        t0 = t0.to(dt).train()
        ref[dt] = R.mse(t0(first[0].to(dt)), first[1].to(dt)).detach().reshape(1)
    _held(torch.tensor([losses[0]]), ref[torch.float32], ref[torch.float64], 'first iteration loss')
    # --mode embedding from that checkpoint: file order, one row per image, the eval-mode forward
    out = _script(common + ['--mode', 'embedding', '--which_epoch', 'latest'])
    assert [l[4:] for l in out.splitlines() if l.startswith('--> ')] == names
    feats, labels = np.load(save_dir / 'features.npy'), np.load(save_dir / 'labels.npy')
    assert feats.shape == (N_IMAGES, 1) and feats.dtype == np.float32 and labels.shape == (N_IMAGES,)
    assert labels.tolist() == [S.get_attr(n) for n in names]
    eopt = S.get_options(common + ['--mode', 'embedding'], save=False)
    data = S.K.make_loader(eopt, train=False).dataset
    assert data.names == names
    net = net.to(dev).eval()
    with torch.no_grad():
        mine = np.concatenate([net.forward(data[i][0][None].to(dev)).cpu().numpy().reshape(1, 1) for i in range(N_IMAGES)], axis=0)
    assert np.array_equal(feats, mine)
    twin = twin.double().eval()
    with torch.no_grad():
        f64 = torch.cat([twin(data[i][0][None].double()).view(1, 1) for i in range(N_IMAGES)])
    assert_close(torch.from_numpy(feats), f64, 1e-4, 'features.npy vs the float64 twin in eval mode')
