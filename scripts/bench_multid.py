"""The multi-scale discriminator's image pyramid (hip/functional.py: avg_pool_pyramid -- pcgan_avgpool_fwd / pcgan_avgpool_bwd) against the
same chain as torch operations on the device, and what the second discriminator costs a wsgan_cycle step.

  1. pyramid of 2 and of 3 levels, forward + backward with every level's gradient live, float32 and bfloat16, at [16, 3, 256, 256] (BASELINE
     config 5 per GPU) and [32, 3, 128, 128]: device time between events and wall time of one call that is waited for.  The comparison is
     F.avg_pool2d(3, 2, 1, count_include_pad=False) per level, its autograd and autograd's adds.  The two sides alternate inside one process,
     every shape is warmed first, and the spread over the repeats is reported beside the median.  Bytes per second come from the shapes: every
     level is read once and its pooled copy written once on the way down; on the way up each level's gradient is read once, the pooled
     level's gradient once, and the sum written once.  `device_ms` is the time between events around calls issued as fast as the host can
     (at these sizes that is the host's launch rate on both sides); `device_ms_queued` brackets the same calls queued behind a spin kernel, so
     the kernels run back to back as they do in a step whose host runs ahead.
  2. pcgan_avgpool_bwd with `base` against pcgan_avgpool_bwd followed by pcgan_add, and the forward kernel beside torch's, at the first level
     of the same shapes.
  3. the wsgan_cycle step at config 5's shape (256 x 256, batch 16, resnet_9blocks, --n_layers_D 3) with --which_model_netD n_layers and with
     n_layers_multi --num_Ds 2, rounds interleaved.  The second discriminator costs time by design: information, not a gate.

    python scripts/bench_multid.py [--out profiles/multi_d.json] [--repeats 7] [--iters 200] [--no-step]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

SHAPES = [(16, 3, 256, 256), (32, 3, 128, 128)]
DTYPES = [('fp32', torch.float32), ('bf16', torch.bfloat16)]


def level_shapes(shape, levels):
    out = [tuple(shape)]
    for _ in range(levels - 1):
        n, c, h, w = out[-1]
        out.append((n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    return out


def pyramid_bytes(shape, levels, esize):
    """algorithmic traffic of forward + backward with all gradients live (see the module docstring)"""
    numel = [n * c * h * w for n, c, h, w in level_shapes(shape, levels)]
    fwd = sum(numel[i] + numel[i + 1] for i in range(levels - 1))
    bwd = sum(numel[i + 1] + 2 * numel[i] for i in range(levels - 1))
    return (fwd + bwd) * esize


def stats(ms):
    s = sorted(ms)
    return {'median': s[len(s) // 2], 'min': s[0], 'max': s[-1], 'spread': (s[-1] - s[0]) / s[len(s) // 2]}


def device_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


_SPIN = {}


def queued_ms(fn, iters=100, behind_ms=40.0):
    """device time per call with the host out of the way: the calls are queued behind a spin kernel of about `behind_ms` (calibrated once),
    so the events bracket kernels that run back to back, as they do inside a training step whose host runs ahead of the device"""
    if 'cycles_per_ms' not in _SPIN:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000000)
        s.record()
        torch.cuda._sleep(10000000)
        e.record()
        torch.cuda.synchronize()
        _SPIN['cycles_per_ms'] = 10000000 / s.elapsed_time(e)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(int(behind_ms * _SPIN['cycles_per_ms']))
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def wall_ms(fn, n=20):
    t = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return sorted(t)[n // 2]


def alternate(sides, repeats, iters):
    """{name: {'device_ms': stats, 'wall_ms_one_call': median}} of callables timed in turn, `repeats` rounds"""
    for fn in sides.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms, qd = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            ms[k].append(device_ms(fn, iters))
        for k, fn in sides.items():
            qd[k].append(queued_ms(fn))
    return {k: {'device_ms': stats(ms[k]), 'device_ms_queued': stats(qd[k]), 'wall_ms_one_call': wall_ms(fn)} for k, fn in sides.items()}


def time_pyramids(dev, repeats, iters):
    from pcgan_amd.hip import functional as HF
    rows = []
    for shape in SHAPES:
        for name, dtype in DTYPES:
            for levels in (2, 3):
                x = torch.randn(shape, device=dev).to(dtype).requires_grad_(True)
                gs = [torch.randn(s, device=dev).to(dtype) for s in level_shapes(shape, levels)]

                def hip():
                    x.grad = None
                    torch.autograd.backward(list(HF.avg_pool_pyramid(x, levels)), gs)

                def chain():
                    x.grad = None
                    out = [x.view_as(x)]
                    for _ in range(levels - 1):
                        out.append(F.avg_pool2d(out[-1], 3, stride=2, padding=1, count_include_pad=False))
                    torch.autograd.backward(out, gs)
                r = alternate({'hip': hip, 'torch': chain}, repeats, iters)
                nbytes = pyramid_bytes(shape, levels, x.element_size())
                row = {'shape': list(shape), 'dtype': name, 'levels': levels, 'bytes': nbytes, 'hip': r['hip'], 'torch': r['torch'],
                       'hip_GB_s': nbytes / r['hip']['device_ms']['median'] / 1e6, 'torch_GB_s': nbytes / r['torch']['device_ms']['median'] / 1e6,
                       'hip_over_torch_device': r['hip']['device_ms']['median'] / r['torch']['device_ms']['median'],
                       'hip_over_torch_queued': r['hip']['device_ms_queued']['median'] / r['torch']['device_ms_queued']['median'],
                       'hip_queued_GB_s': nbytes / r['hip']['device_ms_queued']['median'] / 1e6}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def time_base(dev, repeats, iters):
    from pcgan_amd.hip import ops
    rows = []
    for shape in SHAPES:
        for name, dtype in DTYPES:
            big, small = level_shapes(shape, 2)
            dy, g = torch.randn(small, device=dev).to(dtype), torch.randn(big, device=dev).to(dtype)
            hw = big[2:]
            r = alternate({'bwd_with_base': lambda: ops.avgpool_bwd(dy, hw, 3, 2, 1, base=g),
                           'bwd_then_add': lambda: ops.add(ops.avgpool_bwd(dy, hw, 3, 2, 1), g),
                           'fwd': lambda: ops.avgpool_fwd(g, 3, 2, 1),
                           'fwd_torch': lambda: F.avg_pool2d(g, 3, stride=2, padding=1, count_include_pad=False)}, repeats, iters)
            row = dict(r, shape=list(shape), dtype=name)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def time_steps(rounds, steps):
    from pcgan_amd.options.train_options import TrainOptions
    from pcgan_amd.models import create_model, networks
    tmp = tempfile.mkdtemp(prefix='bench_multid_')
    torch.manual_seed(0)
    e = networks.define_E('resnet18', 3, 'normal', 'avg', [32, 1], 1, 0.7)
    torch.save(e.base.model.state_dict(), tmp + '/base.pth')
    torch.save(networks.define_IP('alexnet', 3).state_dict(), tmp + '/IP.pth')
    common = ['x', '--dataroot', 'synthetic', '--checkpoints_dir', tmp, '--gpu_ids', '0', '--model', 'wsgan_cycle', '--which_model_netG',
              'resnet_9blocks', '--n_layers_D', '3', '--fineSize', '256', '--loadSize', '256', '--display_id', '-1', '--batchSize', '16',
              '--attr_bins', '[10,30,50]', '--pretrained_model_path_E', tmp + '/base.pth', '--pretrained_model_path_IP', tmp + '/IP.pth']
    variants = {'n_layers': ['--which_model_netD', 'n_layers', '--name', 'd1'],
                'n_layers_multi_num_Ds_2': ['--which_model_netD', 'n_layers_multi', '--num_Ds', '2', '--name', 'd2']}
    models = {}
    for k, extra in variants.items():
        old, sys.argv = sys.argv, common + extra
        so, sys.stdout = sys.stdout, open(os.devnull, 'w')
        try:
            opt = TrainOptions().parse()
            m = create_model(opt)
            m.setup(opt)
        finally:
            sys.stdout.close()
            sys.argv, sys.stdout = old, so
        models[k] = m
    g = torch.Generator().manual_seed(1)
    batch = {'A': (torch.rand(16, 3, 256, 256, generator=g) * 2 - 1).pin_memory(), 'B_attr': torch.rand(16, 1, 1, 1, generator=g) * 100,
             'A_paths': [''] * 16, 'B_paths': [''] * 16}
    for m in models.values():
        for _ in range(3):
            m.set_input(batch)
            m.optimize_parameters()
    torch.cuda.synchronize()
    ms = {k: [] for k in models}
    for _ in range(rounds):
        for k, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                m.set_input(batch)
                m.optimize_parameters()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    res = {k: {'wall_ms_per_step': stats(v)} for k, v in ms.items()}
    res['shape'] = 'wsgan_cycle 256x256 batch 16, resnet_9blocks, n_layers_D 3, fp32, %d rounds of %d steps' % (rounds, steps)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_d.json'))
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_multid.py measures on the GPU'
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'iters_per_repeat': args.iters}
    res['pyramid'] = time_pyramids(dev, args.repeats, args.iters)
    res['backward_base'] = time_base(dev, args.repeats, args.iters)
    if not args.no_step:
        res['cycle_step'] = time_steps(3, 5)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote ' + args.out)


if __name__ == '__main__':
    main()
