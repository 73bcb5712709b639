#!/usr/bin/env python
"""U-Net generator on the HIP path: the skip-join kernel alone, the generator alone, and the training step beside resnet_9blocks.
One JSON line, also written to profiles/unet.json:
  join       pcgan_skip_join_fwd (ReLU on the skip half, as the blocks call it) and pcgan_skip_join_bwd at B = 32 with 64 + 64 channels
             at 64x64 and 512 + 512 channels at 2x2, fp32 and bf16: us per call of the raw C entry points on preallocated buffers (the
             interval of a back-to-back chain on one stream between two HIP events, windows of >= 0.5 s) and the bytes the call must
             move (forward: a, b read, out written; backward: dout and a read, da, db written) over that time, as bytes/s and as a
             share of the 8.0 TB/s HBM peak.  The calls rotate over copies of their buffers that add up to >= 512 MiB, twice the
             256 MiB Infinity Cache, so the large shape's figures are MEMORY figures; the small shape (0.5 MiB per call) is one
             launch's latency, not bandwidth;
  generator  forward + backward of the generator alone (train mode, fp32, batch 32, 128x128, ngf 64): `unet` with 7 downsamplings
             beside `resnet_9blocks`, device time per call and the host time to issue it;
  step       ms per optimize_parameters() of wsgan_emb at bench.py's geometry (batch 32, 128x128, ngf = ndf = 64, encoder and AlexNet at
             224) with --which_model_netG unet --n_layers_G 7 and with resnet_9blocks, alternating windows of steps in one process, and
             the host time to issue a step (host clock from the first call to the return of the last, no synchronise inside): a step
             whose issue time is its whole time is bound by the host.
Seeded random weights (speed does not depend on them).

    python scripts/bench_unet.py [--steps 10] [--no-step]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

HBM_PEAK = 8.0e12      # bytes/s, MI355X specification
WINDOW_S = 0.5


def _window(fn, warmup):
    """ms per call over a window of at least WINDOW_S: a short calibration run sizes the timed one"""
    from bench_inception_score import _time
    t = _time(fn, 50, warmup=warmup)
    iters = max(200, int(1.2 * WINDOW_S * 1000 / max(t, 1e-4)))
    return _time(fn, iters, warmup=10), iters


def bench_join(res):
    import torch
    from pcgan_amd.hip import lib as L
    dev = torch.device('cuda:0')
    h = L.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    B = 32
    for ca, cb, side in ((64, 64, 64), (512, 512, 2)):
        HW = side * side
        for name, dt, code in (('fp32', torch.float32, L.F32), ('bf16', torch.bfloat16, L.BF16)):
            es = 2 if dt == torch.bfloat16 else 4
            n_out = B * (ca + cb) * HW
            fwd_bytes = 2 * n_out * es                            # a + b read, out written
            bwd_bytes = (2 * n_out + B * ca * HW) * es            # dout read, da + db written, a read for its mask
            copies = max(2, -(-(512 << 20) // fwd_bytes))
            copies = min(copies, 256)
            a = [torch.randn(B, ca, side, side, device=dev).to(dt) for _ in range(copies)]
            b = [torch.randn(B, cb, side, side, device=dev).to(dt) for _ in range(copies)]
            out = [torch.empty(B, ca + cb, side, side, device=dev, dtype=dt) for _ in range(copies)]
            da, db = [torch.empty_like(t) for t in a], [torch.empty_like(t) for t in b]
            turn = [0, 0]

            def fwd():
                i = turn[0] % copies
                turn[0] += 1
                h.pcgan_skip_join_fwd(vp(a[i]), vp(b[i]), vp(out[i]), B, ca, cb, HW, L.ACT_RELU, L.ACT_NONE, code, st)

            def bwd():
                i = turn[1] % copies
                turn[1] += 1
                h.pcgan_skip_join_bwd(vp(out[i]), vp(a[i]), None, vp(da[i]), vp(db[i]), B, ca, cb, HW, L.ACT_RELU, L.ACT_NONE, code, st)
            f_ms, f_it = _window(fwd, copies)
            b_ms, b_it = _window(bwd, copies)
            res['join']['%d+%d_%dx%d_%s' % (ca, cb, side, side, name)] = {
                'fwd_us': round(f_ms * 1000, 2), 'bwd_us': round(b_ms * 1000, 2), 'fwd_bytes': fwd_bytes, 'bwd_bytes': bwd_bytes,
                'fwd_GBps': round(fwd_bytes / f_ms / 1e6, 1), 'bwd_GBps': round(bwd_bytes / b_ms / 1e6, 1),
                'fwd_share_of_hbm_peak': round(fwd_bytes / (f_ms / 1000) / HBM_PEAK, 3),
                'bwd_share_of_hbm_peak': round(bwd_bytes / (b_ms / 1000) / HBM_PEAK, 3),
                'rotating_copies': copies, 'calls_per_window': [f_it, b_it]}
            del a, b, out, da, db
            torch.cuda.empty_cache()


def _issue_and_total(fn, n):
    """(host ms to issue one call, ms per call in all): host clock around n calls, before and after the synchronise"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) * 1000 / n, (t2 - t0) * 1000 / n


def bench_generator(res):
    import torch
    from pcgan_amd.hip import ops
    from pcgan_amd.models import networks
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    x = (torch.rand(32, 3, 128, 128, device=dev) * 2 - 1).requires_grad_(True)
    z = torch.randn(32, 1, 1, 1, device=dev)
    dy = torch.randn(32, 3, 128, 128, device=dev)
    for which, kw in (('unet', {'n_layers_G': 7}), ('resnet_9blocks', {})):
        stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
        try:
            net = networks.define_G(3, 3, 1, 64, which, norm='instance', init_type='normal', gpu_ids=[0], **kw)
        finally:
            sys.stdout.close()
            sys.stdout = stdout

        def fn():
            x.grad = None
            net.zero_grad(set_to_none=True)
            net(x, z).backward(dy)
            ops.join_side_stream()
        for _ in range(3):
            fn()
        best = None
        for _ in range(3):
            issue, total = _issue_and_total(fn, 20)
            best = (issue, total) if best is None or total < best[1] else best
        res['generator'][which] = {'params': sum(p.numel() for p in net.parameters()), 'fwd_bwd_ms': round(best[1], 3),
                                   'host_issue_ms': round(best[0], 3)}
        del net
        torch.cuda.empty_cache()


def _build(which_g, extra, tmp):
    """wsgan_emb at bench.py's geometry (bench.build_model's options) with --which_model_netG `which_g`"""
    import torch
    from pcgan_amd.models import create_model, networks
    from pcgan_amd.options.train_options import TrainOptions
    torch.manual_seed(0)
    e_path, ip_path = os.path.join(tmp, 'E.pth'), os.path.join(tmp, 'IP.pth')
    stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
    old = sys.argv
    try:
        torch.save(networks.define_E('resnet18', 3, 'normal', 'avg', [32, 1], 1, 0.7).state_dict(), e_path)
        torch.save(networks.define_IP('alexnet', 3).state_dict(), ip_path)
        sys.argv = ['bench_unet.py', '--dataroot', 'synthetic', '--model', 'wsgan_emb', '--name', 'bench', '--checkpoints_dir', tmp,
                    '--gpu_ids', '0', '--which_model_netG', which_g, '--which_model_netD', 'n_layers', '--n_layers_D', '3', '--ngf', '64',
                    '--ndf', '64', '--fineSize', '128', '--loadSize', '128', '--fineSize_E', '224', '--fineSize_IP', '224', '--batchSize',
                    '32', '--pretrained_model_path_E', e_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1', '--dtype',
                    'fp32'] + list(extra)
        opt = TrainOptions().parse()
        model = create_model(opt)
        model.setup(opt)
    finally:
        sys.stdout.close()
        sys.argv, sys.stdout = old, stdout
    return model


def bench_step(res, steps):
    import bench
    from pcgan_amd.models import networks
    models = {}
    for key, which, extra, cls in (('unet', 'unet', ['--n_layers_G', '7'], networks.UnetGenerator),
                                   ('resnet_9blocks', 'resnet_9blocks', [], networks.ResnetGenerator)):
        models[key] = _build(which, extra, tempfile.mkdtemp(prefix='pcgan_unet_bench_'))
        assert type(models[key].netG) is cls, 'asked for %s, built %s' % (which, type(models[key].netG).__name__)
    batch = bench.synthetic_batch(32, 128, 0)

    def stepper(m):
        def f():
            m.set_input(batch)
            m.optimize_parameters()
        return f
    times = {k: [] for k in models}
    for k, m in models.items():
        _issue_and_total(stepper(m), 3)
    for _ in range(3):
        for k, m in models.items():
            times[k].append(_issue_and_total(stepper(m), steps))
    res['step'] = {'batch': 32, 'size': 128, 'dtype': 'fp32', 'steps_per_window': steps}
    for k, v in times.items():
        best = min(v, key=lambda t: t[1])
        res['step'][k] = {'ms_per_step': round(best[1], 3), 'host_issue_ms': round(best[0], 3),
                          'windows_ms': [round(t[1], 3) for t in v], 'issue_windows_ms': [round(t[0], 3) for t in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-step', action='store_true', help='skip the training-step comparison')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_unet.py measures on the GPU; there is no other path'
    res = {'metric': 'unet_step_ms', 'hbm_peak_Bps': HBM_PEAK, 'join': {}, 'generator': {}}
    bench_join(res)
    bench_generator(res)
    if not args.no_step:
        bench_step(res, args.steps)
        res['value'] = res['step']['unet']['ms_per_step']
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'unet.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
