#!/usr/bin/env python
"""Inception Score throughput on the HIP path.  Three numbers, one JSON line:
  head       pcgan_linear_softmax_fwd alone at N = 32 / 100, C = 2048, K = 1000 (torchvision inception_v3's fc): us per call over a
             timed loop of back-to-back calls, and the W bytes per batch over that time;
  inception  the IS classifier path per batch of 100 GPU-resident normalised 128 x 128 images: resize to 299, Inception-v3 blocks 0-3,
             head, probabilities copied to the host (what pcgan_amd/util/inception_score.predictions runs per batch; image decoding
             and the PIL transform are not included); images/s, and the head's share of the batch time;
  resnet18   the same for networks.ResNet resnet18 (5 classes) at 224 x 224, batch 32 (eval_emb.py's --batchSize_IS) and 100.
Seeded random weights (speed does not depend on them).

    python scripts/bench_inception_score.py [--iters 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def _time(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    import torch
    from bench_inception import random_weights
    from pcgan_amd.hip import inception as I
    from pcgan_amd.models import networks
    from pcgan_amd.models.inception import InceptionV3Classifier
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    res = {'metric': 'inception_score_images_per_s', 'head': {}, 'inception': {}, 'resnet18': {}}

    w = (torch.randn(1000, 2048, generator=g) * 0.05).to(dev)
    b = torch.randn(1000, generator=g).to(dev)
    for n in (32, 100):
        x = torch.randn(n, 2048, generator=g).abs().to(dev)
        ms = _time(lambda: I.linear_softmax(x, w, b), args.iters * 50)
        res['head']['N%d' % n] = {'us': round(ms * 1000, 2), 'w_GB_per_s': round(w.numel() * 4 / (ms * 1e6), 1)}

    sd = random_weights(1)
    sd['fc.weight'], sd['fc.bias'] = w.cpu(), b.cpu()
    net = InceptionV3Classifier(weights=sd)
    x = (torch.rand(100, 3, 128, 128, generator=g) * 2 - 1).to(dev)
    ms = _time(lambda: net(x, probs=True)[1].cpu(), args.iters)
    res['inception'] = {'batch': 100, 'size': 128, 'ms_per_batch': round(ms, 3), 'images_per_s': round(100 * 1000.0 / ms, 1),
                        'head_share': round(res['head']['N100']['us'] / 1000.0 / ms, 5)}

    rn = networks.ResNet(3, 5, 'resnet18').to(dev).eval()
    for bs in (32, 100):
        x = torch.randn(bs, 3, 224, 224, generator=g).to(dev)
        ms = _time(lambda: rn(I.prep(x, (224, 224)), probs=True)[1].cpu(), args.iters)
        res['resnet18']['batch%d' % bs] = {'ms_per_batch': round(ms, 3), 'images_per_s': round(bs * 1000.0 / ms, 1)}
    res['value'] = res['inception']['images_per_s']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
