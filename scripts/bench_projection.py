#!/usr/bin/env python
"""Projection discriminator head on the HIP path: the two kernels alone, the same formula in stock torch eager ops, and the training step.
One JSON line, also written to profiles/projection_head.json:
  head       pcgan_proj_head_fwd and pcgan_proj_head_bwd at B = 32, C = 512 with 7x7, 15x15 and 31x31 maps, fp32 and bf16: us per call of
             the raw C entry points on preallocated outputs (the interval of a back-to-back chain on one stream between two HIP events;
             each call is two launches), and the effective bandwidth of the pass over p / dp.  `*_us` / `*_GBps`: one p and one dp,
             called again and again -- 3 to 63 MB that stay in the 256 MiB Infinity Cache, so these are CACHE-RESIDENT figures.
             `*_rot_us` / `*_rot_GBps`: the calls rotate over copies of p / dp that add up to 512 MiB, twice the cache: memory figures;
  eager      forward + backward of the same formula composed of stock torch-ROCm eager ops (sum, 1x1 convolutions, multiply, sum, add,
             sigmoid and autograd's backward through them) at the same shapes, fp32, beside the two fused kernels, alternating in one
             process (`gate`: fused forward + backward must not be slower than eager at (32, 512, 15, 15));
  step       ms per optimize_parameters() of wsgan_emb at bench.py's geometry (batch 32, 128x128, ngf = ndf = 64, resnet_9blocks) with
             --which_model_netD n_layers and n_layers_proj, alternating blocks of steps.
Seeded random weights (speed does not depend on them).

    python scripts/bench_projection.py [--iters 2000] [--steps 10] [--no-step]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=2000, help='calls per timed window (windows of 20 ms and more)')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-step', action='store_true', help='skip the training-step comparison')
    args = ap.parse_args()
    import torch
    import torch.nn.functional as TF
    from bench_inception_score import _time
    from pcgan_amd.hip import lib as L
    from pcgan_amd.hip import ops
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    h = L.load()
    B, C, nz = 32, 512, 1
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {'metric': 'projection_head_fwd_bwd_us', 'B': B, 'C': C, 'nz': nz, 'sigmoid': True, 'head': {}, 'eager': {}}
    y = torch.randn(B, nz, device=dev)
    psi_w, psi_b = torch.randn(1, C, 1, 1, device=dev) * 0.02, torch.zeros(1, device=dev)
    ly_w, ly_b = torch.randn(C, nz, 1, 1, device=dev) * 0.02, torch.zeros(C, device=dev)
    g32 = torch.randn(B, 1, 3, 3, device=dev)
    nbytes = h.pcgan_proj_head_bwd_workspace_bytes(B, nz)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    for side in (7, 15, 31):
        HW = side * side
        p32 = TF.leaky_relu(torch.randn(B, C, side, side, device=dev), 0.2)
        for name, dt, code in (('fp32', torch.float32, L.F32), ('bf16', torch.bfloat16, L.BF16)):
            p, g = p32.to(dt), g32.to(dt)
            out, hh = ops.proj_head_fwd(p, y, psi_w, psi_b, ly_w, ly_b, True)
            dp, dpw, dpb, dlw, dlb, dy = ops.proj_head_bwd(g, hh, y, psi_w, psi_b, ly_w, ly_b, (side, side), True)

            def raw_fwd():
                h.pcgan_proj_head_fwd(vp(p), vp(y), vp(psi_w), vp(psi_b), vp(ly_w), vp(ly_b), vp(out), vp(hh), B, C, HW, nz, B, 1, code, st)

            def raw_bwd():
                h.pcgan_proj_head_bwd(vp(g), vp(hh), vp(y), vp(psi_w), vp(psi_b), vp(ly_w), vp(ly_b), vp(dp), vp(dpw), vp(dpb), vp(dlw),
                                      vp(dlb), vp(dy), vp(ws), nbytes, B, C, HW, nz, B, 1, 0, code, st)
            f_us = _time(raw_fwd, args.iters, warmup=20) * 1000
            b_us = _time(raw_bwd, args.iters, warmup=20) * 1000
            nb = p.numel() * p.element_size()
            # the same calls over rotating copies of p / dp, 512 MiB in all: nothing a call touches is left in the cache by the last one
            copies = -(-(512 << 20) // nb)
            ps, dps = [p.clone() for _ in range(copies)], [torch.empty_like(dp) for _ in range(copies)]
            turn = [0, 0]

            def rot_fwd():
                q = ps[turn[0] % copies]
                turn[0] += 1
                h.pcgan_proj_head_fwd(vp(q), vp(y), vp(psi_w), vp(psi_b), vp(ly_w), vp(ly_b), vp(out), vp(hh), B, C, HW, nz, B, 1, code, st)

            def rot_bwd():
                q = dps[turn[1] % copies]
                turn[1] += 1
                h.pcgan_proj_head_bwd(vp(g), vp(hh), vp(y), vp(psi_w), vp(psi_b), vp(ly_w), vp(ly_b), vp(q), vp(dpw), vp(dpb), vp(dlw),
                                      vp(dlb), vp(dy), vp(ws), nbytes, B, C, HW, nz, B, 1, 0, code, st)
            fr_us = _time(rot_fwd, args.iters, warmup=copies) * 1000
            br_us = _time(rot_bwd, args.iters, warmup=copies) * 1000
            del ps, dps
            res['head']['%dx%d_%s' % (side, side, name)] = {'fwd_us': round(f_us, 2), 'bwd_us': round(b_us, 2),
                                                            'fwd_GBps': round(nb / f_us / 1e3, 1), 'bwd_GBps': round(nb / b_us / 1e3, 1),
                                                            'fwd_rot_us': round(fr_us, 2), 'bwd_rot_us': round(br_us, 2),
                                                            'fwd_rot_GBps': round(nb / fr_us / 1e3, 1), 'bwd_rot_GBps': round(nb / br_us / 1e3, 1)}
            if name != 'fp32':
                continue
            # the same formula in stock eager ops, forward + backward, against the two fused calls; alternated, best of three windows
            pe = p32.clone().requires_grad_(True)
            leaves = [t.clone().requires_grad_(True) for t in (y.view(B, nz, 1, 1), psi_w, psi_b, ly_w, ly_b)]

            def eager():
                ye, pw, pb, lw, lb = leaves
                for t in [pe] + leaves:
                    t.grad = None
                hsum = torch.sum(pe, dim=(2, 3), keepdim=True)
                o = torch.sigmoid(torch.sum(hsum * TF.conv2d(ye, lw, lb), dim=1, keepdim=True) + TF.conv2d(hsum, pw, pb, padding=1))
                o.backward(g32)

            def fused():
                raw_fwd()
                raw_bwd()
            te, tf = [], []
            for _ in range(3):
                te.append(_time(eager, args.iters, warmup=10) * 1000)
                tf.append(_time(fused, args.iters, warmup=10) * 1000)
            res['eager']['%dx%d_fp32' % (side, side)] = {'eager_fwd_bwd_us': round(min(te), 2), 'fused_fwd_bwd_us': round(min(tf), 2),
                                                         'eager_windows_us': [round(v, 2) for v in te],
                                                         'fused_windows_us': [round(v, 2) for v in tf]}
    gate = res['eager']['15x15_fp32']
    res['gate'] = {'shape': [B, C, 15, 15], 'eager_us': gate['eager_fwd_bwd_us'], 'fused_us': gate['fused_fwd_bwd_us'],
                   'pass': gate['fused_fwd_bwd_us'] <= gate['eager_fwd_bwd_us']}
    res['value'] = gate['fused_fwd_bwd_us']

    if not args.no_step:
        import bench
        from pcgan_amd.models import networks
        models = {}
        for which, cls in (('n_layers', networks.NLayerDiscriminator), ('n_layers_proj', networks.NLayerProjectionDiscriminator)):
            models[which] = _build(which, tempfile.mkdtemp(prefix='pcgan_proj_bench_'))
            assert type(models[which].netD) is cls, 'asked for %s, built %s' % (which, type(models[which].netD).__name__)
        batch = bench.synthetic_batch(32, 128, 0)
        times = {k: [] for k in models}

        def stepper(m):
            def f():
                m.set_input(batch)
                m.optimize_parameters()
            return f
        for k, m in models.items():
            _time(stepper(m), 3, warmup=2)
        for _ in range(3):
            for k, m in models.items():
                times[k].append(_time(stepper(m), args.steps, warmup=1))
        res['step'] = {'batch': 32, 'size': 128, 'dtype': 'fp32',
                       'n_layers_ms': round(min(times['n_layers']), 3), 'n_layers_proj_ms': round(min(times['n_layers_proj']), 3),
                       'n_layers_windows_ms': [round(v, 3) for v in times['n_layers']],
                       'n_layers_proj_windows_ms': [round(v, 3) for v in times['n_layers_proj']]}
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'projection_head.json'), 'w') as f:
        f.write(line + '\n')


def _build(which, tmp):
    """wsgan_emb at bench.py's geometry (bench.build_model's options) with --which_model_netD `which`"""
    import torch
    from pcgan_amd.models import create_model, networks
    from pcgan_amd.options.train_options import TrainOptions
    torch.manual_seed(0)
    # seeded-random stand-ins for the pretrained Elo encoder / AlexNet, as bench.py builds them
    e_path, ip_path = os.path.join(tmp, 'E.pth'), os.path.join(tmp, 'IP.pth')
    torch.save(networks.define_E('resnet18', 3, 'normal', 'avg', [32, 1], 1, 0.7).state_dict(), e_path)
    torch.save(networks.define_IP('alexnet', 3).state_dict(), ip_path)
    argv = ['bench_projection.py', '--dataroot', 'synthetic', '--model', 'wsgan_emb', '--name', 'bench', '--checkpoints_dir', tmp,
            '--gpu_ids', '0', '--which_model_netG', 'resnet_9blocks', '--which_model_netD', which, '--n_layers_D', '3', '--ngf', '64',
            '--ndf', '64', '--fineSize', '128', '--loadSize', '128', '--fineSize_E', '224', '--fineSize_IP', '224', '--batchSize', '32',
            '--pretrained_model_path_E', e_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1', '--dtype', 'fp32']
    old, sys.argv = sys.argv, argv
    stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
    try:
        opt = TrainOptions().parse()
        model = create_model(opt)
        model.setup(opt)
    finally:
        sys.stdout.close()
        sys.argv, sys.stdout = old, stdout
    return model


if __name__ == '__main__':
    main()
