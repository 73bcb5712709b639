#!/usr/bin/env python
"""Attribute-regressor throughput on the HIP path: resnet18 at 224 x 224, batch 100, cnn_dim [64, 1], average pooling (regression.py's
geometry with classification.py's trunk), fp32, synthetic GPU-resident batches.  One JSON line, also written to
profiles/regression_bench.json:
  train      ms per training step (zero_grad, regress, backward, FusedAdam.step) over a timed loop closed by HIP events, images/s, the
             forward pass alone (regress under no_grad, train-mode BatchNorm) and the host's issue time per step (wall time of the loop
             body with the device left to run behind: no synchronisation);
  head       the end of the net alone at (N, F, HW) = (100, 1, 49) and (100, 512, 49), fp32: us per call of pcgan_pool_mse_fwd (ONE
             launch: pred, loss, hits, dx) against the chain it replaces -- pcgan_global_pool_fwd, pcgan_cast, pcgan_mse_loss,
             pcgan_global_pool_bwd -- both as raw C entry points on preallocated buffers, back to back between two HIP events.  The two
             are ALTERNATED in windows inside this one process (fused, chain, fused, chain, ...) and the median window of each is
             reported with the fastest and slowest, so that a drift of the machine hits both alike.  The chain computes no hit count:
             in the reference that is torch arithmetic on the host after pred.cpu().  With fp32 maps functional.cast is the identity,
             so `chain3_us` is the chain without the cast launch, what the Python layers would issue.
Seeded random weights (speed does not depend on them).

    python scripts/bench_regression.py [--iters 20] [--batch 100] [--size 224]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def head_times(torch, dev, N, F, HW, is_max, windows, calls):
    from bench_inception_score import _time
    from pcgan_amd.hip import lib as L
    h = L.load()
    side = int(round(HW ** 0.5))
    x = torch.randn(N, F, side, side).to(dev)
    target = torch.randn(N * F).to(dev)
    pred, dpred, dx = torch.empty(N * F, device=dev), torch.empty(N * F, device=dev), torch.empty_like(x)
    pred2 = torch.empty_like(pred)
    arg = torch.empty(N * F, dtype=torch.int32, device=dev)
    loss = torch.empty((), device=dev)
    hits = torch.empty((), dtype=torch.int32, device=dev)
    nb = h.pcgan_pool_mse_workspace_bytes(N * F)
    ws = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    lb = max(int(h.pcgan_loss_workspace_bytes(N * F)), 256)
    lws = torch.empty(lb, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused():
        return h.pcgan_pool_mse_fwd(p(x), p(target), p(pred), p(arg), p(dx), p(loss), p(hits), p(ws), nb, N, F, HW, is_max, 0.05, 1.0, L.F32, st)

    def chain(with_cast):
        def run():
            status = h.pcgan_global_pool_fwd(p(x), p(pred), p(arg), N * F, HW, is_max, L.F32, st)
            src = pred
            if with_cast:
                status |= h.pcgan_cast(p(pred), L.F32, p(pred2), L.F32, N * F, st)
                src = pred2
            status |= h.pcgan_mse_loss(p(src), p(target), p(loss), p(dpred), N * F, 1.0, p(lws), lb, L.F32, st)
            return status | h.pcgan_global_pool_bwd(p(dpred), p(arg), p(dx), N * F, HW, is_max, L.F32, st)
        return run
    variants = {'fused_us': fused, 'chain_us': chain(True), 'chain3_us': chain(False)}
    for k, fn in variants.items():
        assert fn() == 0, '%s: %s' % (k, h.pcgan_last_error())
        _time(fn, 50, warmup=20)
    samples = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            samples[k].append(_time(fn, calls, warmup=5) * 1000.0)
    out = {'N': N, 'F': F, 'HW': HW, 'pooling': 'max' if is_max else 'avg', 'windows': windows, 'calls_per_window': calls}
    for k, v in samples.items():
        out[k] = round(statistics.median(v), 2)
        out[k.replace('_us', '_min_max_us')] = [round(min(v), 2), round(max(v), 2)]
    out['chain_over_fused'] = round(out['chain_us'] / out['fused_us'], 2)
    out['chain3_over_fused'] = round(out['chain3_us'] / out['fused_us'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--which_model', type=str, default='resnet18')
    ap.add_argument('--windows', type=int, default=9)
    args = ap.parse_args()
    import torch
    from bench_inception_score import _time
    from pcgan_amd.hip import functional as HF
    from pcgan_amd.hip.optim import FusedAdam
    from pcgan_amd.models import networks
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = networks.define_AR(args.which_model, init_type='normal', pooling='avg', cnn_dim=[64, 1], cnn_relu_slope=0.7).to(dev).train()
    opt = FusedAdam(net.parameters(), lr=2e-4)
    x = torch.randn(args.batch, 3, args.size, args.size).to(dev)
    y = torch.randn(args.batch, 1, 1, 1).to(dev)
    res = {'metric': 'regression_train_images_per_s', 'model': args.which_model, 'batch': args.batch, 'size': args.size, 'dtype': 'fp32',
           'cnn_dim': [64, 1], 'pooling': 'avg'}

    def step():
        opt.zero_grad()
        loss = net.regress(x, y, 0.05)[0]
        loss.backward(HF.unit_gradient(loss))
        opt.step()
    ms = _time(step, args.iters, warmup=5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        step()
    host_ms = (time.perf_counter() - t0) * 1000.0 / args.iters
    torch.cuda.synchronize()
    with torch.no_grad():
        fwd = _time(lambda: net.regress(x, y, 0.05)[0], args.iters)
    res['train'] = {'ms_per_step': round(ms, 3), 'images_per_s': round(args.batch * 1000.0 / ms, 1), 'forward_ms': round(fwd, 3),
                    'host_issue_ms_per_step': round(host_ms, 3), 'step_over_forward': round(ms / fwd, 2)}
    res['head'] = [head_times(torch, dev, args.batch, 1, 49, 0, args.windows, 400),
                   head_times(torch, dev, args.batch, 512, 49, 0, args.windows, 400)]
    res['value'] = res['train']['images_per_s']
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'regression_bench.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
