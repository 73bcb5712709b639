#!/usr/bin/env python
"""Attribute-classifier throughput on the HIP path: resnet18 at 224 x 224, batch 100 (the reference's defaults), fp32, synthetic
GPU-resident batches, 10 classes.  One JSON line, also written to profiles/classification_bench.json:
  train      ms per training step (zero_grad, classify, backward, FusedAdam.step) over a timed loop closed by HIP events, images/s,
             and the host's issue time per step (wall time of the loop body with the device left to run behind: no synchronisation);
  head       pcgan_linear_ce_fwd and pcgan_linear_bwd alone at N = 100, C = 512, K = 10: us per launch of the raw C entry points on
             preallocated outputs (`*_kernel_us`: the launch interval of a back-to-back chain; the kernels' own durations come from
             `rocprofv3 --kernel-trace --stats -- python scripts/bench_classification.py`), and of the tensor wrappers, which also
             allocate the outputs (`*_wrapper_us`);
  test       --mode test's forward (eval mode, classify under no_grad) at batch 100 and batch 1: images/s.
Seeded random weights (speed does not depend on them).

    python scripts/bench_classification.py [--iters 20] [--batch 100] [--size 224]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--which_model', type=str, default='resnet18')
    args = ap.parse_args()
    import torch
    from bench_inception_score import _time
    from pcgan_amd.hip import ops
    from pcgan_amd.hip.optim import FusedAdam
    from pcgan_amd.models import networks
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    K = 10
    net = networks.ResNet(3, K, args.which_model).to(dev).train()
    opt = FusedAdam(net.parameters(), lr=2e-4)
    x = torch.randn(args.batch, 3, args.size, args.size).to(dev)
    y = torch.randint(0, K, (args.batch,)).to(dev)
    res = {'metric': 'classification_train_images_per_s', 'model': args.which_model, 'batch': args.batch, 'size': args.size, 'dtype': 'fp32'}

    def step():
        opt.zero_grad()
        loss = net.classify(x, y)[0]
        loss.backward()
        opt.step()
    ms = _time(step, args.iters, warmup=5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        step()
    host_ms = (time.perf_counter() - t0) * 1000.0 / args.iters
    torch.cuda.synchronize()
    res['train'] = {'ms_per_step': round(ms, 3), 'images_per_s': round(args.batch * 1000.0 / ms, 1), 'host_issue_ms_per_step': round(host_ms, 3)}

    C = net.model.fc.in_features
    xh = torch.randn(args.batch, C).abs().to(dev)
    w, b = net.model.fc.weight.detach(), net.model.fc.bias.detach()
    # the two kernels alone: the raw C entry points on preallocated outputs, so that neither allocations nor the tensor wrappers are
    # in the loop; back-to-back launches between two HIP events (per-call time = launch interval of a dependent chain on one stream)
    import ctypes
    from pcgan_amd.hip import lib as L
    h = L.load()
    loss, logits, dl, pred, correct = ops.linear_ce_fwd(xh, w, b, y)
    dx, dw, db = ops.linear_bwd(dl, xh, w)
    nbytes = h.pcgan_linear_ce_workspace_bytes(args.batch)
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N_ = args.batch

    def raw_fwd():
        h.pcgan_linear_ce_fwd(p(xh), p(w), p(b), p(y), None, p(logits), p(dl), p(loss), p(pred), p(correct), p(ws), nbytes, N_, C, K,
                              L.F32, st)

    def raw_bwd():
        h.pcgan_linear_bwd(p(dl), p(xh), p(w), p(dx), p(dw), p(db), N_, C, K, 0, L.F32, st)
    res['head'] = {'N': args.batch, 'C': C, 'K': K,
                   'linear_ce_fwd_kernel_us': round(_time(raw_fwd, args.iters * 100, warmup=20) * 1000, 2),
                   'linear_bwd_kernel_us': round(_time(raw_bwd, args.iters * 100, warmup=20) * 1000, 2),
                   'linear_ce_fwd_wrapper_us': round(_time(lambda: ops.linear_ce_fwd(xh, w, b, y), args.iters * 50) * 1000, 2),
                   'linear_bwd_wrapper_us': round(_time(lambda: ops.linear_bwd(dl, xh, w), args.iters * 50) * 1000, 2)}

    net.eval()
    res['test'] = {}
    with torch.no_grad():
        fwd = _time(lambda: net.classify(x, y)[2], args.iters)
        res['test']['batch%d' % args.batch] = {'ms_per_batch': round(fwd, 3), 'images_per_s': round(args.batch * 1000.0 / fwd, 1)}
        x1, y1 = x[:1].contiguous(), y[:1].contiguous()
        one = _time(lambda: net.classify(x1, y1)[2].cpu(), args.iters * 5)
        res['test']['batch1'] = {'ms_per_batch': round(one, 3), 'images_per_s': round(1000.0 / one, 1)}
    res['train']['step_over_forward'] = round(ms / fwd, 2)
    res['value'] = res['train']['images_per_s']
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'classification_bench.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
