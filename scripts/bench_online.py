#!/usr/bin/env python
"""The online trainer's end of the network on one MI355X: the one-launch node (ops.online_pair_bce: order, selection, draw-aware BCE,
gradient, predictions) against the two chains it replaces, and the training loop of siamese_online.py with the host's read-back after or
before backward().  One JSON line, also written to profiles/online_head.json:
  head   per N in (100, 256, 1024, 4096) and k in (N, N / 4), fp32 ratings:
           node      ops.online_pair_bce (allocations of its four outputs included), forward AND gradient: it is one launch
           device    (a) the same chain as torch ops that stay on the device: sub, mul, argsort, two slices, index, two logsigmoid, mean,
                     sigmoid and the compares of get_prediction, and autograd's backward()
           host      (b) the reference's round trip (siamese_online.py:230-265, 331-342, 385-394): three .cpu() copies, numpy argsort,
                     LongTensor -> device, the indexed loss, the prediction's .cpu(), backward()
         `*_us`: HIP events around `calls` back-to-back calls, the median of `windows` windows alternated between the three (fastest and
         slowest beside it); `*_waited_us`: wall clock of ONE call followed by torch.cuda.synchronize(), the median of the same number of
         calls -- what a host that needs the result pays.  For the host chain only the waited figure means anything.
  loop   ms per iteration (wall clock over the loop, the device drained at the end) of siamese_online.py's functions at batch 100,
         224 x 224, resnet18, one synthetic batch resident on the GPU: fetch -> forward_loss -> backward_step -> picks.cpu() -> OnlineLog
         (the script's order) against forward_loss -> picks.cpu() -> OnlineLog -> backward_step (the reference's order: the host stalls
         before backward() can be queued).

    python scripts/bench_online.py [--iters 20] [--windows 9]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

THRESH = 0.16


def head_times(torch, dev, N, k, windows, calls):
    import torch.nn.functional as F
    from bench_inception_score import _time
    from pcgan_amd.hip import ops
    g = torch.Generator().manual_seed(N + k)
    f1 = (torch.randn(N, 1, 1, 1, generator=g) * 2).to(dev).requires_grad_(True)
    f2 = (torch.randn(N, 1, 1, 1, generator=g) * 2).to(dev).requires_grad_(True)
    label = torch.randint(0, 3, (N,), generator=g).to(dev)
    lut = torch.tensor([1.0, 0.5, 0.0], device=dev)

    def node():
        return ops.online_pair_bce(f1.detach(), f2.detach(), label, k, False, THRESH, 0.0)

    def prediction(score):
        prob = torch.sigmoid(score)
        idx1 = torch.abs(0.5 - prob) < THRESH
        return (prob > 0.5) & ~idx1, idx1, (prob <= 0.5) & ~idx1

    def device():
        f1.grad = f2.grad = None
        score = (f1 - f2).view(N)
        order = torch.argsort(score.detach() * score.detach())
        sel, pseudo = order[:k], order[-k:]
        sc, t = score[sel], lut[label][sel]
        loss = -(t * F.logsigmoid(sc) + (1 - t) * F.logsigmoid(-sc)).mean()
        idx0, idx1, idx2 = prediction(score.detach())
        pred = idx0 * 0 + idx1 * 1 + idx2 * 2
        loss.backward()
        return loss, sel, pseudo, pred

    def host():
        f1.grad = f2.grad = None
        score = f1 - f2
        score.detach().cpu().numpy()                                                       # :232 (its argmax is always 0)
        dist2 = (f1.detach() - f2.detach()).pow(2).cpu().numpy().reshape(N)                # :244-246
        order = dist2.argsort()
        sel, pseudo = torch.LongTensor(order[:k]).to(dev), order[-k:]
        sc, t = score.view(N, -1)[sel], lut[label].view(N, -1)[sel]
        loss = -(t * F.logsigmoid(sc) + (1 - t) * F.logsigmoid(-sc)).mean()
        sel.cpu().numpy()                                                                  # :342
        idx0, idx1, idx2 = prediction(score.detach())
        pred = (idx0 * 0 + idx1 * 1 + idx2 * 2).cpu().numpy()                              # :392
        loss.backward()
        return loss, pseudo, pred

    variants = {'node': node, 'device': device, 'host': host}
    for fn in variants.values():
        _time(fn, 20, warmup=10)
    samples = {k_: [] for k_ in variants}
    waited = {k_: [] for k_ in variants}
    for _ in range(windows):
        for name, fn in variants.items():
            samples[name].append(_time(fn, calls, warmup=3) * 1000.0)
    for name, fn in variants.items():
        for _ in range(windows * 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            waited[name].append((time.perf_counter() - t0) * 1e6)
    out = {'N': N, 'k': k, 'windows': windows, 'calls_per_window': calls}
    for name in variants:
        out[name + '_us'] = round(statistics.median(samples[name]), 2)
        out[name + '_min_max_us'] = [round(min(samples[name]), 2), round(max(samples[name]), 2)]
        out[name + '_waited_us'] = round(statistics.median(waited[name]), 2)
    out['device_over_node'] = round(out['device_us'] / out['node_us'], 2)
    out['host_waited_over_node_waited'] = round(out['host_waited_us'] / out['node_waited_us'], 2)
    return out


def loop_times(torch, dev, iters):
    import siamese as S
    import siamese_online as SO
    tmp = tempfile.mkdtemp(prefix='pcgan_online_bench_')
    opt = SO.get_options(['--dataroot', 'synthetic', '--pair_selector_type', 'hard', '--max_kept', '25', '--use_pseudo_label',
                          '--checkpoint_dir', tmp, '--name', 'bench'], save=False)
    os.makedirs(os.path.join(tmp, 'bench'))
    torch.manual_seed(0)
    net = S.build_net(opt, dev)
    optimizer = SO.build_optimizer(opt, net)
    data = SO.OnlinePairDataset(opt, 'synthetic', '')
    batch = torch.utils.data.default_collate([data[i] for i in range(opt.batch_size)])
    img0, img1, label, label_host, index = SO.fetch_batch(batch, None, dev)
    log = SO.OnlineLog(opt, data.text)

    def script_order():
        optimizer.zero_grad()
        total, _, picks = SO.forward_loss(opt, net, img0, img1, label)
        SO.backward_step(total, optimizer)
        log.record(picks.cpu(), label_host, index)

    def reference_order():
        optimizer.zero_grad()
        total, _, picks = SO.forward_loss(opt, net, img0, img1, label)
        log.record(picks.cpu(), label_host, index)
        SO.backward_step(total, optimizer)

    out = {'batch': opt.batch_size, 'size': opt.fineSize, 'model': opt.which_model, 'max_kept': opt.max_kept, 'iters': iters}
    for name, fn in (('picks_after_step_ms', script_order), ('picks_before_backward_ms', reference_order)):
        rounds = []
        for _ in range(3):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            rounds.append((time.perf_counter() - t0) * 1000.0 / iters)
        out[name] = round(statistics.median(rounds), 3)
        out[name.replace('_ms', '_min_max_ms')] = [round(min(rounds), 3), round(max(rounds), 3)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--no_loop', action='store_true')
    args = ap.parse_args()
    import torch
    dev = torch.device('cuda:0')
    res = {'metric': 'online_pair_head_us', 'dtype': 'fp32', 'draw_thresh': THRESH}
    res['head'] = [head_times(torch, dev, N, k, args.windows, args.calls) for N in (100, 256, 1024, 4096) for k in (N, N // 4)]
    if not args.no_loop:
        res['loop'] = loop_times(torch, dev, args.iters)
    res['value'] = res['head'][0]['node_us']
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'online_head.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
