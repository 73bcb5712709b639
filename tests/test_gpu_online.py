"""GPU: the one-launch online pair selection + draw-aware BCE (csrc/online_pair.hip) against the float64 restatement of
tests/online_ref.py and against what the reference's classes computed (tests/golden/online_select.npz), its autograd node, and
siamese_online.py end to end.

Bounds.  Against the restatement: picks (sel, pseudo, pred) are EQUAL; each loss and each gradient element is within 2^-23 |ref| -- one
rounding of a float64 result to fp32 (2^-24) with room for the device's float64 exp / log1p, whose error is far below that.  Against
the golden file: the restatement's own bounds of tests/test_online_ref.py (16 * 2^-24 * mean|term| for the loss, 4 * 2^-24 / k for a
gradient element) plus that 2^-23.  Before pred is compared the test asserts on the CPU side that no probability lies within 1e-6 of
0.5 or of 0.5 +- draw_thresh, so a boundary case cannot hide as a tolerance.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import online_ref as R
from test_online_ref import CASES, GOLD, U24, golden_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U23 = 2.0 ** -23
THRESH = 0.16


def _inputs(N, seed, spread=4.0):
    g = torch.Generator().manual_seed(seed)
    f2 = torch.randn(N, generator=g) * 2.0
    f1 = f2 + (torch.rand(N, generator=g) * 2.0 - 1.0) * spread
    label = torch.randint(0, 3, (N,), generator=g)
    return f1, f2, label


def _run(dev, f1, f2, label, k, descending, lam, gscale=1.0, key=None, want_grad=True):
    from pcgan_amd.hip import ops
    out = ops.online_pair_bce(f1.to(dev), f2.to(dev), label.to(dev), k, descending, THRESH, lam, gscale,
                              None if key is None else key.to(dev), want_grad)
    torch.cuda.synchronize()
    return out


def _check(out, ref, what, lam, pred=True):
    loss, picks, df1, df2 = out
    k = ref['sel'].size
    got = picks.cpu().numpy()
    assert picks.dtype == torch.int32 and got.size == 2 * k + ref['pred'].size
    assert np.array_equal(got[:k], ref['sel']), what + ': sel'
    assert np.array_equal(got[k:2 * k], ref['pseudo']), what + ': pseudo'
    if pred:
        assert ref['min_p_margin'] >= 1e-6, what + ': a probability sits on a decision boundary, choose other inputs'
        assert np.array_equal(got[2 * k:], ref['pred']), what + ': pred'
    l = loss.cpu().numpy().astype(np.float64)
    for i in range(3):
        assert abs(l[i] - ref['loss'][i]) <= U23 * abs(ref['loss'][i]), '%s: loss[%d] %r vs %r' % (what, i, l[i], ref['loss'][i])
    for name, d, want in (('df1', df1, ref['df1']), ('df2', df2, ref['df2'])):
        d = d.cpu().numpy().astype(np.float64).reshape(-1)
        worst = np.max(np.abs(d - want) - U23 * np.abs(want))
        assert worst <= 0, '%s: %s exceeds 2^-23 |ref| by %.3e' % (what, name, worst)
        if lam == 0:
            outside = np.ones(d.size, dtype=bool)
            outside[ref['sel']] = False
            assert not d[outside].any(), what + ': a gradient outside sel'


@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 100, 256, 257, 512, 513, 1023, 1024, 1025, 2048, 2049, 3072, 3073, 4096])
def test_node_against_the_restatement(dev, N):
    f1, f2, label = _inputs(N, 31 * N + 7)
    for k in sorted({1, N // 4 or 1, N}):
        for descending in (False, True):
            for lam in (0.0, 0.3):
                what = 'N %d k %d %s lambda %g' % (N, k, 'easy' if descending else 'hard', lam)
                ref = R.online_pair_bce(f1.numpy(), f2.numpy(), label.numpy(), k, descending, THRESH, lam)
                _check(_run(dev, f1.view(N, 1, 1, 1), f2.view(N, 1, 1, 1), label, k, descending, lam), ref, what, lam)


@pytest.mark.parametrize('hard', [True, False], ids=['hard', 'easy'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%d' % c)
def test_autograd_node_against_the_reference(dev, case, hard):
    """every recorded case through functional.online_pair_bce with backward"""
    from pcgan_amd.hip import functional as HF
    gold = np.load(GOLD)
    N, max_kept = case
    g = golden_case(gold, N, max_kept, hard)
    k = min(N, max_kept)
    f1 = torch.from_numpy(g['f1']).view(N, 1, 1, 1).to(dev).requires_grad_(True)
    f2 = torch.from_numpy(g['f2']).view(N, 1, 1, 1).to(dev).requires_grad_(True)
    label = torch.from_numpy(g['label'].astype(np.int64)).to(dev)
    total, loss3, picks = HF.online_pair_bce(f1, f2, label, k, not hard, THRESH, 0.0)
    assert total.requires_grad and not loss3.requires_grad and not picks.requires_grad
    total.backward()
    torch.cuda.synchronize()
    got = picks.cpu().numpy()
    assert np.array_equal(got[:k], g['sel'].astype(np.int32)) and np.array_equal(got[k:2 * k], g['pseudo'].astype(np.int32))
    ref = R.online_pair_bce(g['f1'], g['f2'], g['label'], k, not hard, THRESH, 0.0)
    want = float(g['loss'])
    value = float(total.detach())
    assert value == float(loss3[2]) == float(loss3[0]) and float(loss3[1]) == 0.0
    assert abs(value - want) <= 16 * U24 * ref['mean_abs_term'] + U23 * abs(want)
    for d, w in ((f1.grad, g['df1']), (f2.grad, g['df2'])):
        assert tuple(d.shape) == (N, 1, 1, 1)
        err = np.abs(d.cpu().numpy().reshape(-1).astype(np.float64) - w)
        assert np.all(err <= 4 * U24 / k + U23 * np.abs(w))


@pytest.mark.parametrize('N', [64, 300, 1025, 3000])       # the sorting network on 64, 512, 2048 and 4096 entries
def test_ties_and_overlap(dev, N):
    half = N // 2
    d = 1.0 + (torch.arange(half) % 7).float() * 0.375
    s = torch.cat([d, -d, torch.full((N - 2 * half,), 0.625)])
    f2 = torch.zeros(N)
    label = torch.arange(N) % 3
    for f1 in (s, torch.full((N,), 2.0)):                             # +-d pairs; all ratings equal
        for descending in (False, True):
            for k in (1, N // 3, N // 2 + 3, N):                      # 2 k > N: sel and pseudo overlap
                ref = R.online_pair_bce(f1.numpy(), f2.numpy(), label.numpy(), k, descending, THRESH, 0.0)
                assert ref['min_key_gap'] == 0.0
                if 2 * k > N:
                    assert np.intersect1d(ref['sel'], ref['pseudo']).size == 2 * k - N
                _check(_run(dev, f1, f2, label, k, descending, 0.0), ref, 'ties N %d k %d desc %d' % (N, k, descending), 0.0)
    up = _run(dev, torch.full((N,), 2.0), f2, label, N, False, 0.0)[1].cpu().numpy()
    assert np.array_equal(up[:N], np.arange(N)) and np.array_equal(up[N:2 * N], np.arange(N))
    down = _run(dev, torch.full((N,), 2.0), f2, label, N, True, 0.0)[1].cpu().numpy()
    assert np.array_equal(down[:N], np.arange(N)[::-1])
    # an explicit key with -inf, inf, -0 / +0 and one NaN: the order only
    f1, _, _ = _inputs(N, 5)
    key = torch.randn(N, generator=torch.Generator().manual_seed(N)).round()          # many equal keys
    key[3], key[N - 2], key[10], key[20], key[21], key[40] = float('inf'), float('inf'), float('-inf'), 0.0, -0.0, float('nan')
    for descending in (False, True):
        ref = R.online_pair_bce(f1.numpy(), f2.numpy(), label.numpy(), N, descending, THRESH, 0.0, key=key.numpy())
        got = _run(dev, f1, f2, label, N, descending, 0.0, key=key)[1].cpu().numpy()
        assert np.array_equal(got[:N], ref['sel']) and np.array_equal(got[N:2 * N], ref['pseudo'])
        assert got[:N][-1 if not descending else 0] == 40, 'the NaN key comes after +inf'


@pytest.mark.parametrize('N', [100, 1025])
def test_uniform_labels_and_far_ratings(dev, N):
    f1, f2, _ = _inputs(N, 11 + N)
    for value in (0, 1, 2):
        label = torch.full((N,), value, dtype=torch.int64)
        for lam in (0.0, 0.3):
            ref = R.online_pair_bce(f1.numpy(), f2.numpy(), label.numpy(), N // 2, False, THRESH, lam)
            _check(_run(dev, f1, f2, label, N // 2, False, lam), ref, 'labels all %d' % value, lam)
    # |s| = 80: logsigmoid must not overflow; the loss is finite and the restatement's, the gradients hold no inf / NaN
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    f1, f2 = 40.0 * sign, -40.0 * sign
    label = torch.arange(N) % 3
    ref = R.online_pair_bce(f1.numpy(), f2.numpy(), label.numpy(), N, True, THRESH, 0.0)
    loss, picks, df1, df2 = _run(dev, f1, f2, label, N, True, 0.0)
    assert np.isfinite(ref['loss']).all() and ref['loss'][0] > 10
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(df1).all()) and bool(torch.isfinite(df2).all())
    _check((loss, picks, df1, df2), ref, '|s| = 80', 0.0)


def test_determinism_null_outputs_and_the_upstream_factor(dev):
    from pcgan_amd.hip import functional as HF, lib, ops
    N, k = 1025, 300
    f1, f2, label = _inputs(N, 77)
    a = _run(dev, f1, f2, label, k, False, 0.3)
    b = _run(dev, f1, f2, label, k, False, 0.3)
    for x, y in zip(a, b):
        assert torch.equal(x, y), 'two calls give the same bits'
    # want_grad=False: no gradient buffers; the C entry with only picks wanted leaves poisoned buffers alone
    c = _run(dev, f1, f2, label, k, False, 0.3, want_grad=False)
    assert c[2] is None and c[3] is None and torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])
    d1, d2, d3 = (torch.full((N,), 7.0, device=dev) for _ in range(3))
    loss = torch.full((3,), 7.0, device=dev)
    picks = torch.full((2 * k + N,), -7, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    x1, x2, lb = f1.to(dev), f2.to(dev), label.to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = lib.load()
    assert h.pcgan_online_pair_bce(p(x1), p(x2), p(lb), None, None, None, None, p(picks), N, k, 0, THRESH, 0.3, 1.0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(picks, a[1]) and bool((d1 == 7.0).all()) and bool((d2 == 7.0).all()) and bool((loss == 7.0).all())
    assert h.pcgan_online_pair_bce(p(x1), p(x2), p(lb), None, p(loss), p(d1), None, None, N, k, 0, THRESH, 0.3, 1.0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, a[0]) and torch.equal(d1, a[2]) and bool((d2 == 7.0).all()) and bool((d3 == 7.0).all())
    # gscale in the launch, and an upstream factor through the node: gscale * df within one rounding
    s = _run(dev, f1, f2, label, k, False, 0.3, gscale=3.0)
    ref = R.online_pair_bce(f1.numpy(), f2.numpy(), label.numpy(), k, False, THRESH, 0.3, gscale=3.0)
    _check(s, ref, 'gscale 3', 0.3)
    calls = []
    orig = ops.scale

    def counted(*args, **kw):
        calls.append(1)
        return orig(*args, **kw)
    ops.scale = counted
    try:
        y1, y2 = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        total = HF.online_pair_bce(y1, y2, lb, k, False, THRESH, 0.3)[0]
        (3.0 * total).backward()
        torch.cuda.synchronize()
        assert len(calls) == 2, 'one pcgan_scale per rating'
        for got, base in ((y1.grad, a[2]), (y2.grad, a[3])):
            want = 3.0 * base.double()
            assert bool(((got.double() - want).abs() <= U24 * want.abs()).all())
        del calls[:]
        z1, z2 = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        total = HF.online_pair_bce(z1, z2, lb, k, False, THRESH, 0.3)[0]
        total.backward(HF.unit_gradient(total))
        torch.cuda.synchronize()
        assert len(calls) == 0, 'the unit gradient hands the stored gradients on without a launch'
        assert torch.equal(z1.grad, a[2]) and torch.equal(z2.grad, a[3])
        with torch.no_grad():
            t0, l0, p0 = HF.online_pair_bce(x1, x2, lb, k, False, THRESH, 0.3)
        assert not t0.requires_grad and torch.equal(l0, a[0]) and torch.equal(p0, a[1]) and float(t0) == float(a[0][2])
    finally:
        ops.scale = orig


# ---- siamese_online.py end to end ------------------------------------------------------------------------------------------------------
def _train(tmp_path, name, selector):
    """two iterations of the script in this process, ops.online_pair_bce and the batch fetch wrapped: per iteration the ratings, labels
    and dataset indices the node saw, and what it returned"""
    import siamese_online as SO
    from pcgan_amd.hip import ops
    argv = ['--mode', 'train', '--dataroot', 'synthetic', '--fineSize', '32', '--loadSize', '32', '--transforms', 'none', '--batch_size', '8',
            '--max_kept', '3', '--max_dataset_size', '16', '--pretrained_model_path', '', '--pair_selector_type', selector,
            '--use_pseudo_label', '--save_latest_freq', '1', '--checkpoint_dir', str(tmp_path), '--name', name]
    seen, fetched = [], []
    orig_op, orig_fetch = ops.online_pair_bce, SO.fetch_batch

    def op(f1, f2, label, *a, **k):
        out = orig_op(f1, f2, label, *a, **k)
        seen.append((f1.detach().cpu().numpy().reshape(-1), f2.detach().cpu().numpy().reshape(-1), label.cpu().numpy(), a, out[1].cpu().numpy()))
        return out

    def fetch(*a, **k):
        out = orig_fetch(*a, **k)
        fetched.append(out[4].numpy().copy())
        return out
    ops.online_pair_bce, SO.fetch_batch = op, fetch
    try:
        log = SO.main(argv)
    finally:
        ops.online_pair_bce, SO.fetch_batch = orig_op, orig_fetch
    return SO, log, seen, fetched


def test_script_end_to_end(dev, tmp_path):
    SO, log, seen, fetched = _train(tmp_path, 'hard', 'hard')
    save_dir = tmp_path / 'hard'
    lines = open(save_dir / 'online.txt').read().splitlines(True)
    assert len(lines) == 2 * (3 + 3) and len(seen) == 2 and len(fetched) == 2
    for f in ('loss.txt', 'latest_net.pth', 'opt.txt'):
        assert os.path.exists(save_dir / f), f
    want, diff = [], 0
    for (f1, f2, label, args, picks), index in zip(seen, fetched):
        assert args[:2] == (3, False) and f1.size == 8
        ref = R.online_pair_bce(f1, f2, label, 3, False, 0.16, 0.0)
        assert ref['min_p_margin'] >= 1e-6
        assert np.array_equal(picks, R.picks_of(ref))
        for j in ref['sel']:
            i = int(index[j])
            assert int(label[j]) == SO.OnlinePairDataset.synthetic_label(i)
            want.append('syn_%05d_A.png syn_%05d_B.png %d\n' % (i, i, label[j]))
            diff += int(label[j]) != 1
        for j in ref['pseudo']:
            want.append('syn_%05d_A.png syn_%05d_B.png %d\n' % (int(index[j]), int(index[j]), ref['pred'][j]))
            diff += int(ref['pred'][j]) != 1
    assert lines == want
    assert sorted(np.concatenate(fetched).tolist()) == list(range(16))
    assert (log.cnt_online, log.cnt_online_diff) == (6, diff)
    # --mode embedding on that checkpoint
    SO.main(['--mode', 'embedding', '--dataroot', 'synthetic', '--fineSize', '32', '--loadSize', '32', '--transforms', 'none',
             '--max_dataset_size', '5', '--checkpoint_dir', str(tmp_path), '--name', 'hard'])
    feats, labels = np.load(save_dir / 'features_latest.npy'), np.load(save_dir / 'labels_latest.npy')
    assert feats.shape == (5, 1) and labels.shape == (5,) and np.isfinite(feats).all()
    # easy on the same data (same seed: the same batches) keeps the complementary end of the order: what hard, on the ratings of that
    # iteration, would have kept is easy's pseudo list reversed, and the other way round
    _, _, seen_easy, fetched_easy = _train(tmp_path, 'easy', 'easy')
    assert np.array_equal(fetched_easy[0], fetched[0]) and np.array_equal(fetched_easy[1], fetched[1])
    for f1, f2, label, args, picks in seen_easy:
        assert args[:2] == (3, True)
        assert np.array_equal(picks, R.picks_of(R.online_pair_bce(f1, f2, label, 3, True, 0.16, 0.0)))
        hard = R.online_pair_bce(f1, f2, label, 3, False, 0.16, 0.0)
        assert np.array_equal(picks[:3], hard['pseudo'][::-1]) and np.array_equal(picks[3:6], hard['sel'][::-1])
        assert not set(picks[:3]) & set(picks[3:6])
    assert len(open(tmp_path / 'easy' / 'online.txt').read().splitlines()) == 12
