#!/usr/bin/env python
"""wsgan_disc on the HIP path: the image-pool exchange alone and the training step without and with a pool.  One JSON line, also
written to profiles/disc_step.json:
  pool    at [10, 3, 128, 128] fp32 (fake_B of the step below) against a full pool of 50 images, under a half-exchange plan (every
          other image is exchanged with a slot, the rest pass): pcgan_pool_exchange -- ONE launch -- beside the reference's own
          per-image loop (util/image_pool.py:16-31: unsqueeze, clone of the slot, list assignment, one cat at the end) run as torch ops
          on the same device under the same plan.  Two clocks each: HIP events around a back-to-back chain of calls on one stream,
          windows of >= 0.5 s (what the device is busy for when the host keeps up), and the host's wall clock around single calls
          that are waited for (what a caller who needs the result sees), with the host time to issue a call.  The calls rotate over
          copies of the batch and of the pool that add up to >= 512 MiB, twice the 256 MiB Infinity Cache, so both work from memory.
          The exchange is given through ops.pool_exchange (allocates the returned batch, as the torch loop does) and through the raw C
          entry point on a preallocated batch; bytes moved are (2 * pass + 3 * exchange) images;
  step    ms per optimize_parameters() of wsgan_disc at the model's own defaults -- batch 10, 128x128, --which_model_netG unet (7
          downsamplings, ngf 64), n_layers_D 4 (ndf 64), 5 classes, resnet18 classifier and AlexNet at 224 -- with --pool_size 0 and
          with full pools of 50: ONE model whose pools are swapped between alternating windows of steps, and the host time to issue a
          step.  Label triples are drawn as in training.
Seeded random weights (speed does not depend on them).

    python scripts/bench_disc.py [--steps 10] [--no-step]
"""
import argparse
import ctypes
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_unet import HBM_PEAK, _issue_and_total, _window  # noqa: E402

POOL, BATCH, CLASSES = 50, 10, 5


def _waited(fn, n):
    """(host ms to issue, ms until done) of ONE call that is waited for, mean of n"""
    import torch
    issue = total = 0.0
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        issue, total = issue + (t1 - t0), total + (t2 - t0)
    return issue * 1000 / n, total * 1000 / n


def bench_pool(res):
    import torch
    from pcgan_amd.hip import lib as L, ops
    dev = torch.device('cuda:0')
    h = L.load()
    vp = ctypes.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    shape = (3, 128, 128)
    n = 3 * 128 * 128
    rng = random.Random(7)
    plan = [L.pool_swap(rng.randrange(POOL)) if i % 2 == 0 else L.POOL_PASS for i in range(BATCH)]
    c_plan = (ctypes.c_int * BATCH)(*plan)
    n_swap = sum(1 for p in plan if p >= 0)
    moved = (2 * (BATCH - n_swap) + 3 * n_swap) * n * 4
    n_pools, n_x = 32, 128                # 32 * 9.8 MB + 128 * 2 * 1.97 MB > 512 MiB
    xs = [torch.randn((BATCH,) + shape, device=dev) for _ in range(n_x)]
    ys = [torch.empty((BATCH,) + shape, device=dev) for _ in range(n_x)]
    pools = [torch.randn((POOL,) + shape, device=dev) for _ in range(n_pools)]
    lists = [[p[i:i + 1].clone() for i in range(POOL)] for p in pools]       # the reference keeps a list of [1, C, H, W] tensors
    turn = [0]

    def hip_ops():
        i = turn[0]
        turn[0] += 1
        return ops.pool_exchange(pools[i % n_pools], xs[i % n_x], plan)

    def hip_raw():
        i = turn[0]
        turn[0] += 1
        assert h.pcgan_pool_exchange(vp(pools[i % n_pools].data_ptr()), POOL, vp(xs[i % n_x].data_ptr()), vp(ys[i % n_x].data_ptr()), c_plan,
                                     BATCH, n, L.F32, st) == 0, h.pcgan_last_error()

    def torch_loop():
        i = turn[0]
        turn[0] += 1
        images, ret = lists[i % n_pools], []
        for image, op in zip(xs[i % n_x], plan):
            image = torch.unsqueeze(image.data, 0)
            if op >= 0:
                tmp = images[op >> 1].clone()
                images[op >> 1] = image
                ret.append(tmp)
            else:
                ret.append(image)
        return torch.cat(ret, 0)

    # the two must agree before they are timed
    turn[0] = 0
    a = hip_ops()
    turn[0] = 0
    b = torch_loop()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'the exchange and the torch loop must return the same bits'
    before = L.pool_exchange_launches()
    hip_raw()
    assert L.pool_exchange_launches() - before == 1
    out = {'shape': [BATCH] + list(shape), 'pool_size': POOL, 'dtype': 'fp32', 'plan': plan, 'bytes_moved': moved,
           'launches_per_query': 1, 'rotating_copies': [n_pools, n_x]}
    for key, fn in (('exchange_raw', hip_raw), ('exchange_ops', hip_ops), ('torch_loop', torch_loop)):
        ev_ms, iters = _window(fn, 20)
        issue_ms, wall_ms = _waited(fn, 200)
        out[key] = {'event_us': round(ev_ms * 1000, 2), 'wall_us': round(wall_ms * 1000, 2), 'host_issue_us': round(issue_ms * 1000, 2),
                    'calls_per_window': iters}
    out['exchange_raw']['GBps'] = round(moved / out['exchange_raw']['event_us'] / 1e3, 1)
    out['exchange_raw']['share_of_hbm_peak'] = round(moved / (out['exchange_raw']['event_us'] / 1e6) / HBM_PEAK, 4)
    out['wall_speedup_vs_torch_loop'] = round(out['torch_loop']['wall_us'] / out['exchange_ops']['wall_us'], 3)
    out['event_speedup_vs_torch_loop'] = round(out['torch_loop']['event_us'] / out['exchange_ops']['event_us'], 3)
    res['pool'] = out
    del xs, ys, pools, lists
    torch.cuda.empty_cache()


def _build(tmp):
    import torch
    from pcgan_amd.models import create_model, networks
    from pcgan_amd.options.train_options import TrainOptions
    torch.manual_seed(0)
    ac_path, ip_path = os.path.join(tmp, 'AC.pth'), os.path.join(tmp, 'IP.pth')
    stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
    old = sys.argv
    try:
        torch.save(networks.define_AC('resnet18', 3, 'normal', CLASSES).state_dict(), ac_path)
        torch.save(networks.define_IP('alexnet', 3).state_dict(), ip_path)
        # the model's own defaults (batch 10, 128 x 128, n_layers_D 4, 224 x 224 side networks, embedding_nc 5); `unet` is the name
        # define_G takes for the reference's default `unet_128`
        sys.argv = ['bench_disc.py', '--dataroot', 'synthetic', '--model', 'wsgan_disc', '--name', 'bench', '--checkpoints_dir', tmp,
                    '--gpu_ids', '0', '--which_model_netG', 'unet', '--num_classes', str(CLASSES), '--attr_bins', '[0, 20, 30, 40, 50]',
                    '--pretrained_model_path_AC', ac_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1', '--dtype', 'fp32']
        opt = TrainOptions().parse()
        assert (opt.batchSize, opt.fineSize, opt.n_layers_D, opt.pool_size, opt.embedding_nc) == (BATCH, 128, 4, 0, CLASSES)
        model = create_model(opt)
        model.setup(opt)
    finally:
        sys.stdout.close()
        sys.argv, sys.stdout = old, stdout
    return model


def bench_step(res, steps):
    import torch
    from pcgan_amd.hip import lib as L
    from pcgan_amd.util.image_pool import ImagePool
    model = _build(tempfile.mkdtemp(prefix='pcgan_disc_bench_'))
    g = torch.Generator().manual_seed(1234)
    batch = {}
    for c in range(CLASSES):
        batch[c] = torch.rand(BATCH, 3, 128, 128, generator=g) * 2 - 1
        batch['path_%d' % c] = [''] * BATCH
    random.seed(99)
    pools = {'pool_size_0': model.fake_B_pool, 'pool_size_50': [ImagePool(POOL) for _ in range(CLASSES)]}
    for pool in pools['pool_size_50']:         # full pools: every query draws and exchanges
        for _ in range(POOL // BATCH):
            pool.query(torch.rand(BATCH, 3, 128, 128, device=model.device) * 2 - 1)
        assert pool.num_imgs == POOL

    def step():
        model.set_input(batch)
        model.optimize_parameters()
    times = {k: [] for k in pools}
    launches = {}
    try:
        for key in times:
            model.fake_B_pool = pools[key]
            _issue_and_total(step, 3)
        for _ in range(3):
            for key in times:
                model.fake_B_pool = pools[key]
                before = L.pool_exchange_launches()
                times[key].append(_issue_and_total(step, steps))
                launches[key] = (L.pool_exchange_launches() - before) / float(steps)
    finally:
        model.fake_B_pool = pools['pool_size_0']
    res['step'] = {'batch': BATCH, 'size': 128, 'dtype': 'fp32', 'netG': 'unet', 'n_layers_D': 4, 'classes': CLASSES, 'netAC': 'resnet18',
                   'steps_per_window': steps}
    for key, v in times.items():
        best = min(v, key=lambda t: t[1])
        res['step'][key] = {'ms_per_step': round(best[1], 3), 'host_issue_ms': round(best[0], 3), 'pool_launches_per_step': launches[key],
                            'windows_ms': [round(t[1], 3) for t in v], 'issue_windows_ms': [round(t[0], 3) for t in v]}
    losses = model.get_current_losses()
    assert all(v == v and abs(v) != float('inf') for v in losses.values()), losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-step', action='store_true', help='skip the training-step comparison')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_disc.py measures on the GPU; there is no other path'
    res = {'metric': 'disc_step_ms', 'hbm_peak_Bps': HBM_PEAK}
    bench_pool(res)
    if not args.no_step:
        bench_step(res, args.steps)
        res['value'] = res['step']['pool_size_0']['ms_per_step']
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'disc_step.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
