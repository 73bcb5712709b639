#!/usr/bin/env python
"""wsgan_bigan on the HIP path: the one-launch backward pass of the rating join beside the chain it replaces, and the training step with
the switch on and off.  One JSON line, also written to profiles/bigan_step.json:
  concat_bwd   per case -- dy [10, 3 + 1, 128, 128] and [32, 3 + 1, 256, 256], fp32 and bf16, a rating per sample (z_batch N) and one
               shared rating (z_batch 1), wanting dz only, dimg only, or both -- ops.concat_z_bwd (csrc/concat_bwd.hip) beside the chain of
               hip.functional._ConcatZFn.backward: the strided `.contiguous()` copies, ops.channel_sum, and for a shared rating the
               transposed copy and the second channel_sum.  Both through their Python entry points, allocations included, as a step pays
               for them.  Two figures each, in us per call:
                 device   the interval between a HIP event recorded in front of the call and one behind it, median over the calls of a
                          window issued back to back.  Where the host cannot issue the launches as fast as the device retires them the
                          device idles inside that interval: the figure is then the host's, and `host_bound` says so;
                 waited   host clock around one call and the synchronise that follows it, median.
               The calls rotate over copies of dy that add up to > 512 MiB, twice the 256 MiB Infinity Cache.  Windows of fused and chain
               alternate, REPEATS of each; `spread` is (slowest - fastest) / fastest over a side's windows, the run-to-run spread this
               script itself saw, and `fused_not_slower` holds when the fused median is at most the chain's times 1 + the larger spread.
               Bytes the fused call must move and their share of the 8.0 TB/s HBM peak are given beside the device figure;
  shared_rating_sweep   the same comparison, dz only, for one shared rating at [N, 3 + 1, 128, 128] with N = 10 .. 48: ONE workgroup of the
               fused kernel walks all N planes of a rating channel, so it stops paying at some size.  `routed_to_fused` says what
               hip.functional.concat_z does with the case inside fused_concat_bwd() (fused_serves), and
               `fused_not_slower_wherever_routed` whether the fused call held its own in every case that is routed to it;
  step         ms per optimize_parameters() of wsgan_bigan at the model's defaults (batch 10, 128 x 128, n_layers_D 4, ngf = ndf = 64,
               encoder and AlexNet at 224) with --which_model_netG unet, PCGAN_CONCATZ_FUSED 1 and 0 -- ONE model, alternating windows of
               steps -- with the host time to issue a step; a step whose issue time is most of its total is reported as host-bound.
Seeded random weights (speed does not depend on them).

    python scripts/bench_bigan.py [--steps 10] [--no-step] [--window 0.3]
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

from bench_unet import HBM_PEAK, _issue_and_total  # noqa: E402

REPEATS = 3
ROTATE_BYTES = (512 << 20) + 1


def chain_backward(dy, C, z_batch, want_img, want_z):
    """hip.functional._ConcatZFn.backward, statement for statement"""
    from pcgan_amd.hip import ops
    dimg = dz = None
    if want_img:
        dimg = dy[:, :C].contiguous()
    if want_z:
        dzc = dy[:, C:].contiguous()
        N, nz = dzc.shape[0], dzc.shape[1]
        s = ops.channel_sum(dzc.view(1, N * nz, dzc.shape[2], dzc.shape[3]))
        s = s.view(N, nz)
        if z_batch == 1:
            s = ops.channel_sum(s.t().contiguous().view(1, nz, N, 1)).view(1, nz)
        dz = s
    return dimg, dz


def _device_window(fn, seconds):
    """median us between the events around one call, over a window of back-to-back calls sized to `seconds`"""
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 50
    iters = max(100, min(10000, int(seconds / max(per, 1e-6))))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1000.0, iters


def _waited(fn, n=100):
    import torch
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def _issue_us(fn, n=200):
    """host us to issue one call (no synchronise inside the loop)"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t = (time.perf_counter() - t0) * 1e6 / n
    torch.cuda.synchronize()
    return t


def _measure_case(dys, C, zb, want_img, want_z, seconds):
    """one case of the comparison on the rotating copies `dys`"""
    import torch
    from pcgan_amd.hip import functional as HF
    from pcgan_amd.hip import ops
    copies = len(dys)
    N, Ct, H, W = dys[0].shape
    plane = H * W * dys[0].element_size()
    turn = [0]

    def fused():
        turn[0] += 1
        return ops.concat_z_bwd(dys[turn[0] % copies], C, zb, want_img, want_z)

    def chain():
        turn[0] += 1
        return chain_backward(dys[turn[0] % copies], C, zb, want_img, want_z)
    # same results first: dimg bit-equal, dz to the fp32 rounding of two summation orders
    a, b = fused(), chain_backward(dys[turn[0] % copies], C, zb, want_img, want_z)
    if want_img:
        assert torch.equal(a[0], b[0])
    if want_z:
        mass = dys[turn[0] % copies][:, C:].double().abs().sum()
        assert float((a[1].double() - b[1].double()).abs().max()) <= 64 * 2.0 ** -24 * float(mass)
    win = {'fused': [], 'chain': []}
    for _ in range(REPEATS):
        for key, fn in (('fused', fused), ('chain', chain)):
            win[key].append(_device_window(fn, seconds)[0])
    med = {k: statistics.median(v) for k, v in win.items()}
    spread = {k: (max(v) - min(v)) / min(v) for k, v in win.items()}
    waited = {'fused': _waited(fused), 'chain': _waited(chain)}
    issue = {'fused': _issue_us(fused), 'chain': _issue_us(chain)}
    moved = (N * (Ct - C) * plane if want_z else 0) + (2 * N * C * plane if want_img else 0)
    tol = 1.0 + max(spread.values())
    return {'fused_device_us': round(med['fused'], 2), 'chain_device_us': round(med['chain'], 2),
            'fused_waited_us': round(waited['fused'], 2), 'chain_waited_us': round(waited['chain'], 2),
            'fused_issue_us': round(issue['fused'], 2), 'chain_issue_us': round(issue['chain'], 2),
            'fused_windows_us': [round(v, 2) for v in win['fused']], 'chain_windows_us': [round(v, 2) for v in win['chain']],
            'spread': {k: round(v, 3) for k, v in spread.items()},
            'speedup_device': round(med['chain'] / med['fused'], 3), 'speedup_waited': round(waited['chain'] / waited['fused'], 3),
            'fused_not_slower': bool(med['fused'] <= med['chain'] * tol and waited['fused'] <= waited['chain'] * tol),
            # what HF.concat_z does with this case inside fused_concat_bwd() (hip/functional.py: fused_serves): the chain stays where the
            # rating needs no gradient and where one workgroup would walk too many planes of a shared rating
            'routed_to_fused': bool(want_z and HF.fused_serves(N, H * W * dys[0].element_size(), zb)),
            'host_bound': {k: bool(issue[k] >= 0.8 * med[k]) for k in med},
            'fused_bytes': moved, 'fused_GBps': round(moved / med['fused'] / 1e3, 1),
            'fused_share_of_hbm_peak': round(moved / (med['fused'] * 1e-6) / HBM_PEAK, 4), 'rotating_copies': copies}


def _copies(N, Ct, side, dt, dev):
    import torch
    one = N * Ct * side * side * (4 if dt == torch.float32 else 2)
    return [torch.randn(N, Ct, side, side, device=dev).to(dt) for _ in range(-(-ROTATE_BYTES // one))]


def bench_concat_bwd(res, seconds):
    import torch
    dev = torch.device('cuda:0')
    C, nz = 3, 1
    types = (('fp32', torch.float32), ('bf16', torch.bfloat16))
    for N, side in ((10, 128), (32, 256)):
        for dname, dt in types:
            dys = _copies(N, C + nz, side, dt, dev)
            for zb in (N, 1):
                for mode, want_img, want_z in (('dz', False, True), ('dimg', True, False), ('both', True, True)):
                    if mode == 'dimg' and zb == 1:
                        continue        # the rating's batch plays no part in the copy
                    key = 'N%d_%dx%d_%s_zbatch%s_%s' % (N, side, side, dname, 'N' if zb == N else '1', mode)
                    res['concat_bwd'][key] = _measure_case(dys, C, zb, want_img, want_z, seconds)
            del dys
            torch.cuda.empty_cache()
    # where a shared rating stops paying: ONE workgroup walks all N planes of a rating channel, the chain's plane sums use N
    for dname, dt in types:
        for N in (10, 16, 24, 32, 48):
            dys = _copies(N, C + nz, 128, dt, dev)
            res['shared_rating_sweep']['N%d_128x128_%s_dz' % (N, dname)] = _measure_case(dys, C, 1, False, True, seconds)
            del dys
            torch.cuda.empty_cache()
    cases = list(res['concat_bwd'].values()) + list(res['shared_rating_sweep'].values())
    res['fused_not_slower_everywhere'] = all(v['fused_not_slower'] for v in cases)
    res['fused_not_slower_wherever_routed'] = all(v['fused_not_slower'] for v in cases if v['routed_to_fused'])


def _build(tmp):
    import torch
    from pcgan_amd.models import create_model, networks
    from pcgan_amd.options.train_options import TrainOptions
    torch.manual_seed(0)
    e_path, ip_path = os.path.join(tmp, 'E.pth'), os.path.join(tmp, 'IP.pth')
    stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
    old = sys.argv
    try:
        torch.save(networks.ResNetFeature(3, 'resnet18').model.state_dict(), e_path)
        torch.save(networks.define_IP('alexnet', 3).state_dict(), ip_path)
        sys.argv = ['bench_bigan.py', '--dataroot', 'synthetic', '--model', 'wsgan_bigan', '--name', 'bench', '--checkpoints_dir', tmp,
                    '--gpu_ids', '0', '--which_model_netG', 'unet', '--pretrained_model_path_E', e_path, '--pretrained_model_path_IP', ip_path,
                    '--display_id', '-1', '--dtype', 'fp32']
        opt = TrainOptions().parse()
        model = create_model(opt)
        model.setup(opt)
    finally:
        sys.stdout.close()
        sys.argv, sys.stdout = old, stdout
    return model, opt


def bench_step(res, steps):
    import torch
    from pcgan_amd.hip import functional as HF
    model, opt = _build(tempfile.mkdtemp(prefix='pcgan_bigan_bench_'))
    B, S = opt.batchSize, opt.fineSize
    g = torch.Generator().manual_seed(1234)
    batch = {'A': torch.rand(B, 3, S, S, generator=g) * 2 - 1, 'B_attr': torch.rand(B, 1, 1, 1, generator=g) * 60.0,
             'A_paths': [''] * B, 'B_paths': [''] * B}

    def step():
        model.set_input(batch)
        model.optimize_parameters()
    default = HF._CONCATZ_FUSED_ENV
    times = {'fused_on': [], 'fused_off': []}
    try:
        for key in times:
            HF._CONCATZ_FUSED_ENV = key == 'fused_on'
            _issue_and_total(step, 3)
        for _ in range(REPEATS):
            for key in times:
                HF._CONCATZ_FUSED_ENV = key == 'fused_on'
                times[key].append(_issue_and_total(step, steps))
    finally:
        HF._CONCATZ_FUSED_ENV = default
    res['step'] = {'batch': B, 'size': S, 'dtype': 'fp32', 'netG': 'unet', 'n_layers_D': opt.n_layers_D, 'ngf': opt.ngf, 'ndf': opt.ndf,
                   'fineSize_E': opt.fineSize_E, 'fineSize_IP': opt.fineSize_IP, 'steps_per_window': steps, 'default_fused': bool(default)}
    for key, v in times.items():
        best = min(v, key=lambda t: t[1])
        totals = [t[1] for t in v]
        res['step'][key] = {'ms_per_step': round(best[1], 3), 'host_issue_ms': round(best[0], 3),
                            'windows_ms': [round(t, 3) for t in totals], 'issue_windows_ms': [round(t[0], 3) for t in v],
                            'spread': round((max(totals) - min(totals)) / min(totals), 3), 'host_bound': bool(best[0] >= 0.8 * best[1])}
    losses = model.get_current_losses()
    assert all(v == v and abs(v) != float('inf') for v in losses.values()), losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--window', type=float, default=0.3, help='seconds per timed window of the kernel comparison')
    ap.add_argument('--no-step', action='store_true', help='skip the training-step comparison')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_bigan.py measures on the GPU; there is no other path'
    res = {'metric': 'bigan_step_ms', 'hbm_peak_Bps': HBM_PEAK, 'concat_bwd': {}, 'shared_rating_sweep': {}}
    bench_concat_bwd(res, args.window)
    if not args.no_step:
        bench_step(res, args.steps)
        res['value'] = res['step']['fused_on' if res['step']['default_fused'] else 'fused_off']['ms_per_step']
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'bigan_step.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
