#!/usr/bin/env python
"""The two device steps of `siamese.py --mode attention` (csrc/gradcam.hip) beside the chains of torch operations they replace, on the
same GPU.  One JSON line, also written to profiles/attention.json:
  map       ops.gradcam_map for the four map types at the activation shapes of one image per pass -- 64 x 56 x 56 (the default
            --gcam_layer, base.model.layer1.0.conv1), 512 x 7 x 7 (resnet18 layer4) and 2048 x 7 x 7 (resnet50 layer4) -- in fp32 and bf16,
            beside util/gradcam.py: generate of the reference written with plain torch operations on the device (the channel sum instead of
            its grouped conv3d, which is the same sum: tests/test_gradcam_host.py);
  overlay   ops.heatmap_overlay at 1 x 3 x 224 x 224 with a one- and a three-channel map beside feature2image / tensor2image / the blend
            (siamese.py:401-410, 965-978 of the reference) as torch operations on the device (the reference runs them in numpy on the host,
            after a copy that is not counted here).
Two figures each, in us per call, both through the Python entry points, allocations included:
  device    the interval between a HIP event recorded in front of the call and one behind it, median over a window of calls issued back
            to back.  These calls are far shorter than the host takes to issue one, so the device idles inside that interval and the
            figure is an upper bound set by the host (`host_bound`);
  waited    host clock around one call and the synchronise that follows it, median: what the script pays, since it waits for every image.
Windows of kernel and chain alternate, REPEATS of each; `spread` is (slowest - fastest) / fastest over a side's windows.  The calls
rotate over 8 copies of the inputs (6.4 - 12.8 MB at the largest shape): the tensors of the real call were written by the pass just
before it, so they are cache-warm there too.

    python scripts/bench_attention.py [--window 0.1]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_window(fn, seconds):
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
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1000.0


def waited_us(fn, n=100):
    """median host us around one call and the synchronise that follows it"""
    import torch
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def issue_us(fn, n=200):
    """host us to issue one call (no synchronise inside the loop)"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t = (time.perf_counter() - t0) * 1e6 / n
    torch.cuda.synchronize()
    return t


REPEATS = 3
COPIES = 8
MAP_SHAPES = ((1, 64, 56, 56), (1, 512, 7, 7), (1, 2048, 7, 7))
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


def chain_map(A, g, kind):
    """util/gradcam.py: generate of the reference in torch operations (fp32 accumulation is torch's own business)"""
    import torch
    import torch.nn.functional as F
    if kind == 'raw':
        return torch.abs(torch.sum(A, dim=1))[:, None]
    if kind == 'pw':
        return F.relu(torch.sum(g * A, dim=1))[:, None]
    w = F.avg_pool2d(F.relu(g), tuple(g.shape[2:]))
    x = g * A if kind == 'pw_cw' else A
    return F.relu(torch.sum(w * x, dim=1, keepdim=True))


def chain_overlay(m, img, mean, std, alpha):
    """feature2image, tensor2image and the blend, per image 0 as the reference has it"""
    att = m.expand(1, 3, m.shape[2], m.shape[3])
    lo, hi = att.min(), att.max()
    heat = (att - lo) / (hi - lo) * 255
    pix = (img * std + mean) * 255
    return heat * (1 - alpha) + pix * alpha


def _compare(kernel, chain, seconds):
    win = {'kernel': [], 'chain': []}
    for _ in range(REPEATS):
        for key, fn in (('kernel', kernel), ('chain', chain)):
            win[key].append(device_window(fn, seconds))
    med = {k: statistics.median(v) for k, v in win.items()}
    spread = {k: (max(v) - min(v)) / min(v) for k, v in win.items()}
    waited = {'kernel': waited_us(kernel), 'chain': waited_us(chain)}
    issue = {'kernel': issue_us(kernel), 'chain': issue_us(chain)}
    tol = 1.0 + max(spread.values())
    return {'kernel_device_us': round(med['kernel'], 2), 'chain_device_us': round(med['chain'], 2),
            'kernel_waited_us': round(waited['kernel'], 2), 'chain_waited_us': round(waited['chain'], 2),
            'kernel_issue_us': round(issue['kernel'], 2), 'chain_issue_us': round(issue['chain'], 2),
            'kernel_windows_us': [round(v, 2) for v in win['kernel']], 'chain_windows_us': [round(v, 2) for v in win['chain']],
            'spread': {k: round(v, 3) for k, v in spread.items()},
            'speedup_device': round(med['chain'] / med['kernel'], 3), 'speedup_waited': round(waited['chain'] / waited['kernel'], 3),
            'kernel_not_slower': bool(med['kernel'] <= med['chain'] * tol and waited['kernel'] <= waited['chain'] * tol),
            'host_bound': {k: bool(issue[k] >= 0.8 * med[k]) for k in med}}


def bench_map(res, seconds):
    import torch
    from pcgan_amd.hip import ops
    dev = torch.device('cuda:0')
    for shape in MAP_SHAPES:
        for dname, dt in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
            As = [torch.randn(shape, device=dev).to(dt) for _ in range(COPIES)]
            gs = [torch.randn(shape, device=dev).to(dt) for _ in range(COPIES)]
            for kind in ('raw', 'pw', 'cw_pos', 'pw_cw'):
                turn = [0]

                def kernel():
                    turn[0] += 1
                    return ops.gradcam_map(As[turn[0] % COPIES], gs[turn[0] % COPIES], kind)

                def chain():
                    turn[0] += 1
                    return chain_map(As[turn[0] % COPIES], gs[turn[0] % COPIES], kind)
                a, b = kernel().double(), chain_map(As[turn[0] % COPIES], gs[turn[0] % COPIES], kind).double()
                scale = float(b.abs().max()) + 1e-30
                # same results first (bf16: torch rounds its intermediate tensors to bf16, the kernel keeps fp32)
                assert float((a - b).abs().max()) <= (1e-4 if dt == torch.float32 else 5e-2) * scale, (shape, dname, kind)
                case = _compare(kernel, chain, seconds)
                case['bytes'] = (1 if kind == 'raw' else 2) * As[0].numel() * As[0].element_size() + 4 * shape[2] * shape[3]
                res['map']['%dx%dx%d_%s_%s' % (shape[1], shape[2], shape[3], dname, kind)] = case


def bench_overlay(res, seconds):
    import torch
    from pcgan_amd.hip import ops
    dev = torch.device('cuda:0')
    mean_t, std_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    for Cm in (1, 3):
        ms = [torch.randn(1, Cm, 224, 224, device=dev) for _ in range(COPIES)]
        imgs = [torch.randn(1, 3, 224, 224, device=dev) for _ in range(COPIES)]
        turn = [0]

        def kernel():
            turn[0] += 1
            return ops.heatmap_overlay(ms[turn[0] % COPIES], imgs[turn[0] % COPIES], MEAN, STD, 0.01)

        def chain():
            turn[0] += 1
            return chain_overlay(ms[turn[0] % COPIES], imgs[turn[0] % COPIES], mean_t, std_t, 0.01)
        a, b = kernel()[0], chain_overlay(ms[turn[0] % COPIES], imgs[turn[0] % COPIES], mean_t, std_t, 0.01)
        assert float((a - b).abs().max()) <= 1e-3, Cm
        case = _compare(kernel, chain, seconds)
        case['bytes'] = 4 * 224 * 224 * (Cm + (1 if Cm == 1 else 3) + 3 + 3)      # the map twice (reduce, then blend), the image, the output
        res['overlay']['1x%dx224x224_fp32' % Cm] = case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.1, help='seconds per timed window')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_attention.py measures on the GPU; there is no other path'
    res = {'metric': 'attention_call_us', 'map': {}, 'overlay': {}}
    bench_map(res, args.window)
    bench_overlay(res, args.window)
    cases = list(res['map'].values()) + list(res['overlay'].values())
    res['kernel_not_slower_everywhere'] = all(v['kernel_not_slower'] for v in cases)
    res['slower_cases'] = sorted(k for part in ('map', 'overlay') for k, v in res[part].items() if not v['kernel_not_slower'])
    res['value'] = res['map']['64x56x56_fp32_raw']['kernel_waited_us']
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'attention.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
