#!/usr/bin/env python
"""Throughput of the Inception-v3 feature network on the HIP path (pcgan_amd/models/inception.py): images/s for batches of GPU-resident
[0, 1] images at 128 x 128 (the generator's size, so the resize to 299 is included), all four blocks, and the time per block.
Weights are seeded random in torchvision's layout (speed does not depend on them).  Prints one JSON line.

    python scripts/bench_inception.py [--batches 50 100 200] [--iters 10] [--size 128]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/bench_inception.py --iters 3     # per-kernel table
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GFLOP_PER_IMAGE = 2 * 5.71      # 5.71 GMAC at 299 x 299 (tests/test_inception_ref.py)


def random_weights(seed=0):
    import torch
    from pcgan_amd.models import inception as M
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in M.expected_shapes().items():
        if k.endswith('conv.weight'):
            fan_in = shape[1] * shape[2] * shape[3]
            sd[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif k.endswith('running_var') or k.endswith('bn.weight'):
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        else:
            sd[k] = 0.2 * torch.rand(shape, generator=g) - 0.1
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[50, 100, 200])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--size', type=int, default=128)
    args = ap.parse_args()
    import torch
    from pcgan_amd.models.inception import InceptionV3
    dev = torch.device('cuda:0')
    net = InceptionV3([0, 1, 2, 3], weights=random_weights())
    res = {'metric': 'inception_images_per_s', 'size': args.size, 'gflop_per_image': GFLOP_PER_IMAGE, 'batches': {}}
    for bs in args.batches:
        x = torch.rand(bs, 3, args.size, args.size, generator=torch.Generator().manual_seed(bs)).to(dev)
        for _ in range(args.warmup):
            net(x)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.iters):
            net(x)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.iters
        # per block: events around prepare and each block of one more forward
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        with torch.no_grad():
            ev[0].record()
            h = net.prepare(x)
            ev[1].record()
            for i in range(4):
                h = net._block(i, h)
                ev[i + 2].record()
        torch.cuda.synchronize()
        parts = [ev[i].elapsed_time(ev[i + 1]) for i in range(5)]
        res['batches'][str(bs)] = {
            'ms_per_batch': round(ms, 3), 'images_per_s': round(bs * 1000.0 / ms, 1),
            'tflops': round(bs * GFLOP_PER_IMAGE / ms, 2),
            'ms_prep': round(parts[0], 3), 'ms_block': [round(p, 3) for p in parts[1:]]}
    res['value'] = res['batches'].get('100', next(iter(res['batches'].values())))['images_per_s']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
