#!/usr/bin/env python
"""wsgan_cont on the HIP path: the n-ary gradient sum alone and the training step with the fan-out on and off.  One JSON line, also
written to profiles/cont_step.json:
  add_n   at [32, 3, 128, 128] fp32 (the shape of fake_B's gradient in the step below): pcgan_add_n over k = 2 and k = 5 sources in one
          launch beside the same sum as a chain of k - 1 pcgan_add calls (what autograd's binary accumulation amounts to, with the
          library's own add kernel).  us per sum of the raw C entry points on preallocated buffers: the interval of a back-to-back
          chain on one stream between two HIP events, windows of >= 0.5 s.  The calls rotate over copies of their buffers that add up to
          >= 512 MiB, twice the 256 MiB Infinity Cache, so these are MEMORY figures; bytes moved are (k + 1) n 4 for the one launch
          and 3 (k - 1) n 4 for the chain, given with their share of the 8.0 TB/s HBM peak;
  step    ms per optimize_parameters() of wsgan_cont at batch 32, 128x128, resnet_9blocks (ngf = ndf = 64, n_layers_D 3, regressor and
          AlexNet at 224, the model's default loss weights: fake_B has three readers, the shared 224x224 image two, rec_A two) with
          the fan-out on and off -- ONE model, alternating windows of steps -- and the host time to issue a step.
Seeded random weights (speed does not depend on them).

    python scripts/bench_cont.py [--steps 10] [--no-step]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_unet import HBM_PEAK, _issue_and_total, _window  # noqa: E402


def bench_add_n(res):
    import torch
    from pcgan_amd.hip import lib as L
    dev = torch.device('cuda:0')
    h = L.load()
    vp = ctypes.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    shape = (32, 3, 128, 128)
    n = 32 * 3 * 128 * 128
    for k in (2, 5):
        one_bytes, chain_bytes = (k + 1) * n * 4, 3 * (k - 1) * n * 4
        copies = min(256, max(2, -(-(512 << 20) // one_bytes)))
        src = [[torch.randn(shape, device=dev) for _ in range(k)] for _ in range(copies)]
        out = [torch.empty(shape, device=dev) for _ in range(copies)]
        tmp = [torch.empty(shape, device=dev) for _ in range(copies)]
        tables = [(vp * k)(*[t.data_ptr() for t in s]) for s in src]
        turn = [0, 0]

        def one():
            i = turn[0] % copies
            turn[0] += 1
            assert h.pcgan_add_n(tables[i], k, vp(out[i].data_ptr()), n, L.F32, st) == 0, h.pcgan_last_error()

        def chain():
            i = turn[1] % copies
            turn[1] += 1
            s, a, b = src[i], out[i], tmp[i]
            if (k - 1) % 2 == 0:        # ping-pong between two buffers so that the last add lands in out[i]
                a, b = b, a
            h.pcgan_add(vp(s[0].data_ptr()), vp(s[1].data_ptr()), vp(a.data_ptr()), n, L.F32, st)
            for j in range(2, k):
                h.pcgan_add(vp(a.data_ptr()), vp(s[j].data_ptr()), vp(b.data_ptr()), n, L.F32, st)
                a, b = b, a
        one()
        want = out[(turn[0] - 1) % copies].clone()
        turn[1] = turn[0] - 1
        chain()
        assert torch.equal(want, out[(turn[1] - 1) % copies]), 'the chain and the one launch must give the same bits'
        o_ms, o_it = _window(one, copies)
        c_ms, c_it = _window(chain, copies)
        res['add_n']['k%d' % k] = {
            'one_launch_us': round(o_ms * 1000, 2), 'chained_add_us': round(c_ms * 1000, 2), 'speedup': round(c_ms / o_ms, 3),
            'one_launch_bytes': one_bytes, 'chained_add_bytes': chain_bytes,
            'one_launch_GBps': round(one_bytes / o_ms / 1e6, 1), 'chained_add_GBps': round(chain_bytes / c_ms / 1e6, 1),
            'one_launch_share_of_hbm_peak': round(one_bytes / (o_ms / 1000) / HBM_PEAK, 3),
            'rotating_copies': copies, 'calls_per_window': [o_it, c_it]}
        del src, out, tmp, tables
        torch.cuda.empty_cache()


def _build(tmp):
    import torch
    from pcgan_amd.models import create_model, networks
    from pcgan_amd.options.train_options import TrainOptions
    torch.manual_seed(0)
    e_path, ip_path = os.path.join(tmp, 'E.pth'), os.path.join(tmp, 'IP.pth')
    stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
    old = sys.argv
    try:
        torch.save(networks.define_AR('resnet18', 3, 'normal', 'avg', [64, 1], 1, 0.7).state_dict(), e_path)
        torch.save(networks.define_IP('alexnet', 3).state_dict(), ip_path)
        sys.argv = ['bench_cont.py', '--dataroot', 'synthetic', '--model', 'wsgan_cont', '--name', 'bench', '--checkpoints_dir', tmp,
                    '--gpu_ids', '0', '--which_model_netG', 'resnet_9blocks', '--which_model_netD', 'n_layers', '--n_layers_D', '3', '--ngf',
                    '64', '--ndf', '64', '--fineSize', '128', '--loadSize', '128', '--fineSize_E', '224', '--fineSize_IP', '224',
                    '--batchSize', '32', '--pretrained_model_path_E', e_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1',
                    '--dtype', 'fp32']
        opt = TrainOptions().parse()
        model = create_model(opt)
        model.setup(opt)
    finally:
        sys.stdout.close()
        sys.argv, sys.stdout = old, stdout
    return model


def bench_step(res, steps):
    import torch
    from pcgan_amd.models import wsgan_shared as M
    model = _build(tempfile.mkdtemp(prefix='pcgan_cont_bench_'))
    g = torch.Generator().manual_seed(1234)
    batch = {'A': torch.rand(32, 3, 128, 128, generator=g) * 2 - 1, 'B': torch.rand(32, 3, 128, 128, generator=g) * 2 - 1,
             'A_attr': torch.rand(32, 1, 1, 1, generator=g) * 60.0, 'B_attr': torch.rand(32, 1, 1, 1, generator=g) * 60.0,
             'label': torch.randint(0, 3, (32,), generator=g), 'A_paths': [''] * 32, 'B_paths': [''] * 32}

    def step():
        model.set_input(batch)
        model.optimize_parameters()
    default = M._FANOUT
    times = {'fan_out_on': [], 'fan_out_off': []}
    try:
        for key in times:
            M._FANOUT = key == 'fan_out_on'
            _issue_and_total(step, 3)
        for _ in range(3):
            for key in times:
                M._FANOUT = key == 'fan_out_on'
                times[key].append(_issue_and_total(step, steps))
    finally:
        M._FANOUT = default
    res['step'] = {'batch': 32, 'size': 128, 'dtype': 'fp32', 'netG': 'resnet_9blocks', 'steps_per_window': steps, 'default_fan_out': bool(default)}
    for key, v in times.items():
        best = min(v, key=lambda t: t[1])
        res['step'][key] = {'ms_per_step': round(best[1], 3), 'host_issue_ms': round(best[0], 3),
                            'windows_ms': [round(t[1], 3) for t in v], 'issue_windows_ms': [round(t[0], 3) for t in v]}
    losses = model.get_current_losses()
    assert all(v == v and abs(v) != float('inf') for v in losses.values()), losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-step', action='store_true', help='skip the training-step comparison')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_cont.py measures on the GPU; there is no other path'
    res = {'metric': 'cont_step_ms', 'hbm_peak_Bps': HBM_PEAK, 'add_n': {}}
    bench_add_n(res)
    if not args.no_step:
        bench_step(res, args.steps)
        res['value'] = res['step']['fan_out_on' if res['step']['default_fan_out'] else 'fan_out_off']['ms_per_step']
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'cont_step.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
