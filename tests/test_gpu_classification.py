"""GPU: the training pass of the attribute classifier -- the head kernels alone against float64, one training step of the whole
classifier (resnet18 / 34 / 50) against the float64 twin of tests/classifier_ref.py, classification.py end to end, the checkpoint it
writes driving compute_inception_score.py, and the inference path left bit-identical by a training step.

Head tolerance, the project's rule through test_gpu_inception._rule as it stands: ||hip - f64|| <= 2 ||torch_fp32_cpu - f64||
+ 1e-30 (the guard for 0 against 0), for every output including the scalar loss.  The kernels sum in float64 and round once, so each
element is the fp32 number nearest to the float64 value and no fp32 computation can be closer.  pred and correct are exact.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import classifier_ref as C
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


def _head_case(N_, C_, K, seed, weighted, scale=1.0, tie=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N_, C_, generator=g).abs()                          # pooled ReLU features are >= 0
    w = torch.randn(K, C_, generator=g) * (scale * 2.0 / C_ ** 0.5)
    b = torch.randn(K, generator=g) * 0.5
    y = torch.randint(0, K, (N_,), generator=g)
    wt = (0.25 + 2 * torch.rand(K, generator=g)) if weighted else None
    if tie and K >= 2:
        # two classes with the same weights and a bias that lifts both above every other class: every row ties at its maximum
        i, j = (K - 1, K // 2) if K > 2 else (1, 0)
        w[i] = w[j]
        b[i] = b[j] = float((x @ w.t()).abs().max()) * 2 + 1
    return x, w, b, y, wt


def _torch_head(x, w, b, y, wt, dtype):
    x, w, b = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    logits = F.linear(x, w, b)
    logits.retain_grad()
    loss = F.cross_entropy(logits, y, weight=None if wt is None else wt.to(dtype))
    loss.backward()
    return dict(logits=logits.detach(), loss=loss.detach().reshape(1), dlogits=logits.grad, dx=x.grad, dw=w.grad, db=b.grad)


SHAPES = [(1, 512, 2), (100, 512, 5), (32, 2048, 10), (7, 516, 3), (512, 512, 1000), (512, 2048, 1024), (3, 4, 1)]


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_head_kernels_against_float64(dev, shape, weighted):
    from pcgan_amd.hip import ops
    N_, C_, K = shape
    for kind, scale, tie in (('plain', 1.0, False), ('logits ~80', 30.0, False), ('tied maxima', 1.0, True)):
        x, w, b, y, wt = _head_case(N_, C_, K, N_ * 7919 + C_ * 31 + K + int(weighted), weighted, scale, tie)
        what = 'N %d C %d K %d %s%s' % (N_, C_, K, kind, ' weighted' if weighted else '')
        r32, r64 = _torch_head(x, w, b, y, wt, torch.float32), _torch_head(x, w, b, y, wt, torch.float64)
        if kind == 'logits ~80' and K > 1:
            assert float(r64['logits'].abs().max()) > 40, what
        xd, wd, bd, yd = x.to(dev), w.to(dev), b.to(dev), y.to(dev)
        wtd = None if wt is None else wt.to(dev)
        loss, logits, dlogits, pred, correct = ops.linear_ce_fwd(xd, wd, bd, yd, wtd)
        dx, dw, db = ops.linear_bwd(dlogits, xd, wd)
        again = ops.linear_ce_fwd(xd, wd, bd, yd, wtd)
        again_b = ops.linear_bwd(dlogits, xd, wd)
        torch.cuda.synchronize()
        got = dict(logits=logits, loss=loss.reshape(1), dlogits=dlogits, dx=dx, dw=dw, db=db)
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), '%s: %s not finite' % (what, k)
            _held(v, r32[k], r64[k], '%s: %s' % (what, k))
        # predictions: the FIRST maximum of the logits the call returned; the float64 choice wherever that one is not a near-tie
        lg = logits.cpu().numpy()
        assert pred.dtype == torch.int64 and pred.cpu().tolist() == lg.argmax(axis=1).tolist(), what
        l64 = r64['logits'].numpy()
        top2 = np.sort(l64, axis=1)[:, -2:] if K > 1 else None
        clear = np.ones(N_, dtype=bool) if K == 1 else (top2[:, 1] - top2[:, 0]) > 1e-5 * np.abs(l64).max()
        assert (pred.cpu().numpy()[clear] == l64.argmax(axis=1)[clear]).all(), what
        if tie and K >= 2:
            first = K // 2 if K > 2 else 0
            assert pred.cpu().tolist() == [first] * N_, '%s: the first of two tied maxima wins' % what
        assert correct.dtype == torch.int32 and int(correct) == int((pred.cpu() == y).sum()), what
        # run to run
        for a, c in zip((loss, logits, dlogits, pred, correct, dx, dw, db), again + again_b):
            assert torch.equal(a, c), '%s: two runs differ' % what
        # accumulate: added to what the buffers held, dx overwritten; against the sum formed in float64
        dw0 = torch.randn(K, C_, generator=torch.Generator().manual_seed(5)).to(dev)
        db0 = torch.randn(K, generator=torch.Generator().manual_seed(6)).to(dev)
        dw_acc, db_acc = dw0.clone(), db0.clone()
        dx2, dw2, db2 = ops.linear_bwd(dlogits, xd, wd, dw_into=dw_acc, db_into=db_acc)
        torch.cuda.synchronize()
        assert dw2.data_ptr() == dw_acc.data_ptr() and db2.data_ptr() == db_acc.data_ptr() and torch.equal(dx2, dx)
        want_w = (dw0.double().cpu() + r64['dw']), (dw0.cpu() + r32['dw'])
        want_b = (db0.double().cpu() + r64['db']), (db0.cpu() + r32['db'])
        _held(dw_acc, want_w[1], want_w[0], what + ': dw accumulated')
        _held(db_acc, want_b[1], want_b[0], what + ': db accumulated')
        # parts of the backward pass alone
        only_dx = ops.linear_bwd(dlogits, xd, wd, True, False, False)
        only_w = ops.linear_bwd(dlogits, xd, wd, False, True, True)
        torch.cuda.synchronize()
        assert torch.equal(only_dx[0], dx) and only_dx[1] is None and only_dx[2] is None
        assert only_w[0] is None and torch.equal(only_w[1], dw) and torch.equal(only_w[2], db)


def test_head_through_autograd_and_an_unaligned_row_buffer(dev):
    """functional.linear_cross_entropy / linear as autograd nodes: gradients reach x, w and b; an upstream factor scales them on the
    device; a 4-byte aligned x takes the element-wise access path with the same values"""
    from pcgan_amd.hip import functional as HF
    x, w, b, y, wt = _head_case(9, 512, 5, 77, True)
    r64 = _torch_head(x, w, b, y, wt, torch.float64)
    r32 = _torch_head(x, w, b, y, wt, torch.float32)
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    loss, logits, pred, correct = HF.linear_cross_entropy(xd, wd, bd, y.to(dev), wt.to(dev))
    assert loss.requires_grad and not logits.requires_grad and not pred.requires_grad
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    for k, t in (('dx', xd), ('dw', wd), ('db', bd)):
        _held(t.grad, 3.0 * r32[k], 3.0 * r64[k], 'autograd ' + k)
    buf = torch.empty(9 * 512 + 1, device=dev)
    xs = buf[1:].view(9, 512)
    xs.copy_(xd.detach())
    loss2, logits2, _, _ = HF.linear_cross_entropy(xs, wd.detach(), bd.detach(), y.to(dev), wt.to(dev))
    assert torch.equal(loss2, loss.detach()) and torch.equal(logits2, logits)
    # logits alone, differentiable
    xd2, wd2, bd2 = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    out = HF.linear(xd2, wd2, bd2)
    dy = torch.randn(9, 5, generator=torch.Generator().manual_seed(3))
    out.backward(dy.to(dev))
    x6, w6, b6 = (t.double().requires_grad_(True) for t in (x, w, b))
    F.linear(x6, w6, b6).backward(dy.double())
    x3, w3, b3 = (t.clone().requires_grad_(True) for t in (x, w, b))
    F.linear(x3, w3, b3).backward(dy)
    for k, got, a32, a64 in (('dx', xd2.grad, x3.grad, x6.grad), ('dw', wd2.grad, w3.grad, w6.grad), ('db', bd2.grad, b3.grad, b6.grad)):
        _held(got, a32, a64, 'linear ' + k)


def test_backward_element_wise_access_path(dev):
    """pcgan_linear_bwd with 4-byte aligned x, w and gradient buffers (views one float into their storage): the element-wise loads and
    stores, the accumulating read-modify-write included, give the values of the 16-byte path bit for bit"""
    from pcgan_amd.hip import ops
    x, w, b, y, wt = _head_case(9, 516, 5, 78, True)
    r32, r64 = _torch_head(x, w, b, y, wt, torch.float32), _torch_head(x, w, b, y, wt, torch.float64)

    def off(t):
        buf = torch.empty(t.numel() + 1, device=dev)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    xd, wd = x.to(dev), w.to(dev)
    dl = ops.linear_ce_fwd(xd, wd, b.to(dev), y.to(dev), wt.to(dev))[2]
    dx, dw, db = ops.linear_bwd(dl, xd, wd)
    dxo, dwo, dbo = ops.linear_bwd(dl, off(xd), off(wd))
    dw0 = torch.randn(5, 516, generator=torch.Generator().manual_seed(8)).to(dev)
    db0 = torch.randn(5, generator=torch.Generator().manual_seed(9)).to(dev)
    acc_w, acc_b, acc_wo, acc_bo = dw0.clone(), db0.clone(), off(dw0), off(db0)
    ops.linear_bwd(dl, xd, wd, dw_into=acc_w, db_into=acc_b)
    ops.linear_bwd(dl, xd, wd, dw_into=acc_wo, db_into=acc_bo)
    torch.cuda.synchronize()
    assert torch.equal(dxo, dx) and torch.equal(dwo, dw) and torch.equal(dbo, db)
    assert torch.equal(acc_wo, acc_w) and torch.equal(acc_bo, acc_b)
    _held(dxo, r32['dx'], r64['dx'], 'element-wise dx')
    _held(dwo, r32['dw'], r64['dw'], 'element-wise dw')
    _held(acc_wo, dw0.cpu() + r32['dw'], dw0.double().cpu() + r64['dw'], 'element-wise dw accumulated')


def test_rows_with_a_label_outside_the_classes_are_ignored(dev):
    """the header's contract for labels the host did not check: the kernel never indexes with them; such a row has weight 0 -- no loss
    term, no share of the denominator, a zero gradient row, never counted correct -- exactly torch's ignore_index rows"""
    from pcgan_amd.hip import ops
    x, w, b, y, wt = _head_case(12, 512, 5, 79, True)
    y[3], y[7] = -1, 5
    keep = torch.tensor([i for i in range(12) if i not in (3, 7)])
    yi = y.clone()
    yi[3] = yi[7] = -100
    r32, r64 = {}, {}
    for dt, r in ((torch.float32, r32), (torch.float64, r64)):
        lg = F.linear(x.to(dt), w.to(dt), b.to(dt)).requires_grad_(True)
        loss = F.cross_entropy(lg, yi, weight=wt.to(dt), ignore_index=-100)
        loss.backward()
        r.update(loss=loss.detach().reshape(1), dlogits=lg.grad)
    loss, logits, dlogits, pred, correct = ops.linear_ce_fwd(x.to(dev), w.to(dev), b.to(dev), y.to(dev), wt.to(dev))
    torch.cuda.synchronize()
    _held(loss.reshape(1), r32['loss'], r64['loss'], 'loss with ignored rows')
    _held(dlogits, r32['dlogits'], r64['dlogits'], 'dlogits with ignored rows')
    assert float(dlogits[3].abs().max()) == 0 and float(dlogits[7].abs().max()) == 0
    assert int(correct) == int((pred.cpu()[keep] == y[keep]).sum())
    bad = torch.full((4,), 9, dtype=torch.int64)
    loss = ops.linear_ce_fwd(x[:4].to(dev), w.to(dev), b.to(dev), bad.to(dev), None)[0]
    assert bool(torch.isnan(loss)), 'all rows ignored: 0 / 0, as torch'


def test_both_heads_at_changing_sizes_on_the_one_workspace(dev):
    """ops hands linear_ce_fwd and pool_mse_fwd the same ticketed workspace: calls of changing N, of both heads, in stream order, each
    held to float64 as the tests of its own kernel hold it; every call leaves the ticket word zero.  The last classifier call was asked
    for at (N, C, K) = (4, 6, 2), which the kernel's contract refuses (C a multiple of 4, include/pcgan_hip.h): that refusal is asserted,
    before any launch, and the call is made at (4, 4, 2) -- the ticket sees N, which is what changes"""
    from pcgan_amd.hip import ops
    import test_gpu_regression as TR
    calls = []
    for i, shape in enumerate(((5, 8, 3), (3, 8, 3), (5, 8, 3), (3, 2, 50), (4, 4, 2))):
        if i == 4:
            x, w, b, y, wt = _head_case(4, 6, 2, 94, True)
            with pytest.raises(RuntimeError, match='multiple of 4'):
                ops.linear_ce_fwd(x.to(dev), w.to(dev), b.to(dev), y.to(dev), wt.to(dev))
        if i == 3:
            x, t = TR._case(*shape, False, 41, False)
            calls.append((shape, (x, t), ops.pool_mse_fwd(x.to(dev), t.to(dev), TR.DELTA, False)))
        else:
            x, w, b, y, wt = _head_case(*shape, 90 + i, True)
            calls.append((shape, (x, w, b, y, wt), ops.linear_ce_fwd(x.to(dev), w.to(dev), b.to(dev), y.to(dev), wt.to(dev))))
    torch.cuda.synchronize()
    for i, (shape, args, out) in enumerate(calls):
        what = 'call %d %s' % (i, shape)
        if i == 3:
            x, t = args
            r32, r64 = TR._torch_ref(x, t, False, 1.0, torch.float32), TR._torch_ref(x, t, False, 1.0, torch.float64)
            loss, pred, hits, dx, arg = out
            for k, v in dict(pred=pred, loss=loss.reshape(1), dx=dx).items():
                TR._held(v, r32[k], r64[k], '%s: %s' % (what, k))
            assert arg is None and int(hits) == int((torch.abs(pred.cpu() - t.view_as(pred)) < TR.DELTA).sum()), what
        else:
            x, w, b, y, wt = args
            r32, r64 = _torch_head(x, w, b, y, wt, torch.float32), _torch_head(x, w, b, y, wt, torch.float64)
            loss, logits, dlogits, pred, correct = out
            for k, v in dict(logits=logits, loss=loss.reshape(1), dlogits=dlogits).items():
                _held(v, r32[k], r64[k], '%s: %s' % (what, k))
            assert pred.cpu().tolist() == logits.cpu().numpy().argmax(axis=1).tolist(), what
            assert int(correct) == int((pred.cpu() == y).sum()), what
    ws = ops._head_workspace('finish', calls[0][2][0].device, 8, True)
    assert ws.numel() >= 1 + 2 * 6, 'the pool the calls above used, not a new one'
    assert ws.view(torch.int32)[:2].tolist() == [0, 0], 'the ticket is left zero'


# ---- the whole classifier, one training step -------------------------------------------------------------------------------------------
# (trunk, image size, weight seed, output tolerance): 64 -> a 2 x 2 last feature map (5e-4, as the encoder test), 96 -> 3 x 3, 128 -> 4 x 4.
# Weights: test_gpu_inception_score._random_resnet_sd (the norms that end a residual branch are scaled down, so activations stay O(1)
# through 16 blocks).  The seeds were chosen on the CPU, from the twin's OWN fp32-vs-float64 error on its own decisions (logits relative
# to their maximum / worst parameter gradient in relative L2): resnet18 seed 81: 9.6e-7 / 3.0e-6; resnet34 seeds 91 .. 96: 7.5e-6 (91) ..
# 8.0e-3, seed 82: 7.6e-3; resnet50 at 128 x 128, seeds 83, 91 .. 96: 1.6e-2 (91) .. 3.1e-2 -- for resnet50 stock fp32 PyTorch itself uses
# half of the LOOSE band (3e-2) at best, so the seed with the most room is taken and the SHARP check is the one that counts there.
CASES = {'resnet18': (64, 81, 5e-4), 'resnet34': (96, 91, 1e-4), 'resnet50': (128, 91, 1e-4)}
LABELS = torch.tensor([0, 4, 2, 2, 1, 3])
CLASS_WEIGHT = torch.tensor([1.0, 0.5, 2.0, 1.0, 0.25])


def _twin_and_input(which):
    size, seed, tol = CASES[which]
    twin = C.ResNetClassifierRef(which, 5)
    twin.load_state_dict(_random_resnet_sd(twin, seed))
    return twin, W.seeded_tensor((6, 3, size, size), 160 + seed), tol


@pytest.mark.parametrize('which', ['resnet18', 'resnet34', 'resnet50'])
def test_classifier_forward_backward_against_the_twin(dev, which):
    """networks.ResNet.forward(x) in train mode through test_gpu_nets._compare: logits, SHARP gradients on the HIP run's decisions,
    the LOOSE band on the twin's own, running statistics and num_batches_tracked"""
    from pcgan_amd.models import networks
    twin, x, tol = _twin_and_input(which)
    hip = networks.ResNet(3, 5, which).train()
    _compare(hip, twin, [x], 300, dev, out_tol=tol)


@pytest.mark.parametrize('which', ['resnet18', 'resnet34', 'resnet50'])
def test_classifier_training_step_against_the_twin(dev, which):
    """classify() + backward + FusedAdam.step(): loss, logits, pred, correct, SHARP parameter gradients against the float64 twin replaying
    the HIP run's decisions; parameters after the step from the HIP run's gradients through the restated Adam"""
    import copy
    from pcgan_amd.hip.optim import FusedAdam
    from pcgan_amd.models import networks
    twin, x, tol = _twin_and_input(which)
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    hip = networks.ResNet(3, 5, which)
    hip.load_state_dict(sd, strict=True)
    hip = hip.to(dev).train()
    lr = 2e-4
    opt = FusedAdam(hip.parameters(), lr=lr)
    opt.zero_grad()
    with record_decisions() as rec:
        loss, logits, pred, correct = hip.classify(x.to(dev), LABELS.to(dev), CLASS_WEIGHT.to(dev))
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone().cpu() for k, p in hip.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    twin64 = copy.deepcopy(twin).double()
    N.DecisionTape.replay = iter(rec.tape)
    try:
        logits64, loss64, grads64, _ = C.train_step(twin64, x.double(), LABELS, CLASS_WEIGHT, lr)
        assert next(N.DecisionTape.replay, None) is None, 'the twin consumed fewer decisions than the HIP pass recorded'
    finally:
        N.DecisionTape.replay = None
    assert_close(logits, logits64, tol, 'logits')
    assert_close(loss.reshape(1), loss64.reshape(1), tol, 'loss')
    top2 = logits64.sort(dim=1).values[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 10 * tol * logits64.abs().max()
    assert bool((pred.cpu()[clear] == C.predictions(logits64)[clear]).all())
    assert pred.cpu().tolist() == C.predictions(logits).tolist() and int(correct) == int((pred.cpu() == LABELS).sum())
    for k, g in grads.items():
        l2 = float((g.double() - grads64[k]).norm() / (grads64[k].norm() + 1e-300))
        print('%s d%s: relative L2 %.2e' % (which, k, l2))
    for k, g in grads.items():
        _assert_mostly_close(g, grads64[k], 'SHARP d%s vs fp64 twin on the HIP decisions' % k, 5e-4)
    for k, p in hip.named_parameters():
        want = C.adam_update(sd[k].double(), grads[k].double(), lr)
        err = float((p.detach().double().cpu() - want).abs().max())
        # one fp32 rounding of the parameter, and the fp32 arithmetic of an lr-sized update
        assert err <= 2.0 ** -23 * max(1.0, float(want.abs().max())) + 1e-5 * lr, 'parameter %s after the step: %.3e' % (k, err)
    hb = dict(hip.named_buffers())
    for k, b in twin64.named_buffers():
        if 'running' in k:
            assert_close(hb[k], b, 1e-4, 'buffer ' + k, atol=1e-6)
        else:
            assert int(hb[k]) == int(b) == 1, k


def test_training_leaves_the_inference_path_alone(dev):
    """eval-mode forward under no_grad is torch.equal before and after one training step that was rolled back (weights reloaded)"""
    from pcgan_amd.hip import ops
    from pcgan_amd.hip.optim import FusedAdam
    from pcgan_amd.models import networks
    twin, x, _ = _twin_and_input('resnet18')
    sd = {k: v.clone() for k, v in twin.state_dict().items()}
    net = networks.ResNet(3, 5, 'resnet18')
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    xd = x.to(dev)
    with torch.no_grad():
        before = [t.clone() for t in net(xd, probs=True)]
        before_logits = net(xd).clone()
    assert torch.equal(before[0], before_logits)
    net.train()
    opt = FusedAdam(net.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = net.classify(xd, LABELS.to(dev), CLASS_WEIGHT.to(dev))[0]
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    with torch.no_grad():
        moved = net.eval()(xd)
    assert not torch.equal(moved, before_logits), 'the step did not change the net'
    net.load_state_dict(sd, strict=True)
    ops.invalidate_packed_weights()
    net.eval()
    with torch.no_grad():
        after = net(xd, probs=True)
        after_logits = net(xd)
    torch.cuda.synchronize()
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1]) and torch.equal(after_logits, before_logits)
    # with gradients enabled, eval-mode logits come with a graph and are the same numbers
    net.zero_grad()
    graph_logits = net(xd)
    assert graph_logits.requires_grad and torch.equal(graph_logits.detach(), before_logits)


# ---- classification.py end to end ------------------------------------------------------------------------------------------------------
BINS = '[1, 21, 41]'
N_IMAGES, SEED = 24, 11


def _dataset(root):
    """24 PNGs whose mean colour follows their class; names <attribute>_<i>.png with attributes in every bin of BINS"""
    from PIL import Image
    rng = np.random.default_rng(21)
    os.makedirs(root)
    for i in range(N_IMAGES):
        cls = i % 3
        attr = (5, 30, 70)[cls] + (i // 3)
        img = rng.integers(0, 96, (40, 40, 3)).astype(np.int64)
        img[..., cls] += 140
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(root, '%d_%02d.png' % (attr, i)))


def _script(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'classification.py')] + argv, cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_script_trains_tests_and_feeds_the_inception_score(dev, tmp_path):
    import classification as S
    _dataset(str(tmp_path / 'img'))
    common = [str(a) for a in ['--dataroot', tmp_path / 'img', '--name', 'class_x', '--checkpoint_dir', tmp_path / 'checkpoints',
                               '--num_classes', 3, '--attr_bins', BINS, '--loadSize', 36, '--fineSize', 32, '--transforms',
                               'resize_and_crop', '--seed', SEED]]
    train_argv = common + ['--mode', 'train', '--num_epochs', '2', '--batch_size', '8', '--pretrained_model_path', '', '--num_workers', '0',
                           '--weight', '1', '2', '0.5', '--print_freq', '2', '--lr', '0.001']
    out = _script(train_argv)
    save_dir = tmp_path / 'checkpoints' / 'class_x'
    assert 'epoch 01, iter 000002, loss: ' in out and 'dataset size = 24' in out and os.path.exists(save_dir / 'opt.txt')
    with open(save_dir / 'loss.txt') as f:
        losses = [float(v) for v in f.read().split()]
    assert len(losses) == 2 * 3, 'loss.txt: one line per iteration'
    # the checkpoint: the reference's keys, loads strictly into the twin
    ck = torch.load(save_dir / 'latest_net.pth', map_location='cpu')
    twin = C.ResNetClassifierRef('resnet18', 3)
    assert list(ck.keys()) == list(twin.state_dict().keys())
    twin.load_state_dict(ck, strict=True)
    # the first iteration in float64 on the same batch: same seed, same loader, the saved initial weights
    opt = S.get_options(train_argv, save=False)
    S.seed_everything(opt.seed)
    loader = S.make_loader(opt, train=True)
    img0, names = next(iter(loader))
    labels = torch.tensor(S.labels_of(names, opt))
    first = {}
    for dt in (torch.float32, torch.float64):
        t0 = C.ResNetClassifierRef('resnet18', 3)
        t0.load_state_dict(torch.load(save_dir / 'init_net.pth', map_location='cpu'), strict=True)
        t0 = t0.to(dt).train()
        first[dt] = C.cross_entropy(t0(img0.to(dt)), labels, torch.tensor(opt.weight)).detach().reshape(1)
    # the whole net stands behind this number, so the fp32 side of the rule is the twin's whole fp32 forward pass
    _held(torch.tensor([losses[0]]), first[torch.float32], first[torch.float64], 'first iteration loss')
    assert losses[-1] < losses[0], 'the loss after two epochs over 24 images is not below the first: %r' % (losses,)
    # --mode test from that checkpoint
    res = tmp_path / 'acc.txt'
    out = _script(common + ['--mode', 'test', '--which_epoch', 'latest', '--result_path', str(res)])
    lines = [l for l in out.splitlines() if l.startswith('--> image #')]
    assert len(lines) == N_IMAGES
    topt = S.get_options(common + ['--mode', 'test'], save=False)
    random.seed(SEED)
    data = S.make_loader(topt, train=False).dataset
    twin = twin.double().eval()
    aside = hits = 0
    for i in range(N_IMAGES):
        img, name = data[i]
        with torch.no_grad():
            l64 = twin(img.double()[None])[0]
        target = S.labels_of([name], topt)[0]
        got = lines[i].split()
        assert lines[i] == '--> image #%d: target %d   pred %s' % (i + 1, target, got[-1])
        hits += int(int(got[-1]) == target)
        top2 = l64.sort().values[-2:]
        if float(top2[1] - top2[0]) < 1e-3 * float(l64.abs().max()):
            aside += 1
        else:
            assert int(got[-1]) == int(l64.argmax()), 'image %d: pred %s, float64 twin %d' % (i + 1, got[-1], int(l64.argmax()))
    assert aside == 0, 'the float64 twin alone sets %d image(s) aside as near-ties: choose another seed' % aside
    assert 'accuracy: %.4f' % (100. * hits / N_IMAGES) in out
    assert open(res).read() == '%f\n' % (100. * hits / N_IMAGES)
    # the link this exists for: the checkpoint drives the Inception Score script
    is_path = tmp_path / 'is.txt'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'compute_inception_score.py')] + [str(a) for a in [
        '--dataroot', tmp_path / 'img', '--num_classes', 3, '--which_model_IS', 'resnet18', '--pretrained_model_path_IS',
        save_dir / 'latest_net.pth', '--loadSize', 36, '--fineSize', 32, '--batchSize_IS', 8, '--splits', 2, '--result_path', is_path,
        '--seed', 3, '--checkpoints_dir', tmp_path / 'ck']], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    mu, sd = (float(v) for v in open(is_path).read().split())
    assert 1.0 <= mu <= 3.0 + 1e-6 and sd >= 0, (mu, sd)
