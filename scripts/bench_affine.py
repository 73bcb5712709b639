"""Affine modes of the loader on the GPU at the reference's Elo-trainer geometry (siamese.py: 200x200 sources -> 240x240 bicubic ->
RandomAffine(5 deg, 0.95-1.05, BICUBIC, fill 127) -> 224x224 crop -> flip), one reference batch of pairs = 200 images:

  1. the two kernels alone (pcgan_image_resize_u8 + pcgan_image_affine, inputs resident), bytes moved against the HBM rate;
  2. GpuAffineTransform per batch including the upload of the decoded bytes;
  3. the PIL path (base_dataset.get_transform) per image on ONE core;
  4. siamese.py --mode train steps per second at --batch_size 100 with and without --gpu_transform, --num_workers 4 and 16, on PNG
     files written to a temporary folder first (fresh child process per run, a fixed number of iterations, the first ones not timed).

    python scripts/bench_affine.py [--out profiles/affine_elo.json] [--iters 12] [--skip 4] [--no-train]
"""
import argparse
import ctypes
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

N, SRC, LOAD, FINE = 200, 200, 240, 224
HBM_GBS = 8000.0       # MI355X peak HBM3E rate


class O(object):
    loadSize, fineSize, transforms, isTrain, no_flip = LOAD, FINE, 'resize_affine_crop', True, False
    affineDegrees, affineScale = 5.0, [0.95, 1.05]


def smooth_images(n, seed):
    """photo-like 200x200 RGB images (smooth gradients + blobs + mild noise): PNG decode cost like a face crop, not like noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:SRC, 0:SRC].astype(np.float32) / SRC
    out = []
    for _ in range(n):
        c = rng.uniform(0, 1, (3, 4))
        img = np.stack([c[k, 0] + c[k, 1] * xx + c[k, 2] * yy + c[k, 3] * np.sin(6.28 * (xx * c[k, 0] + yy * c[k, 1])) for k in range(3)], -1)
        for _b in range(4):
            cx, cy, r = rng.uniform(0.2, 0.8, 3)
            img += 0.4 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (0.02 + 0.05 * r))[..., None] * rng.uniform(-1, 1, 3)
        img = img / max(float(img.max()), 1e-3) * 220 + rng.normal(0, 3, img.shape)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def time_kernels(dev, arrs, draws):
    from pcgan_amd.data.gpu_transform import GpuAffineTransform
    from pcgan_amd.hip import lib as L
    tf = GpuAffineTransform(O, dev)
    imgs = [torch.from_numpy(a) for a in arrs]
    for _ in range(3):
        tf(imgs, draws)
    torch.cuda.synchronize()
    g, r = tf.geometry(SRC, SRC, 3), tf.resize_geometry(SRC, SRC)
    src = torch.stack(imgs).to(dev)
    resized = torch.empty(N, LOAD, LOAD, 3, dtype=torch.uint8, device=dev)
    a = torch.tensor([[int(v) for v in d[:3]] + [i] for i, d in enumerate(draws)], dtype=torch.int32, device=dev)
    m = draws[:, 3:].contiguous().to(dev)
    out = torch.empty(N, 3, FINE, FINE, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    h = L.load()

    def resize():
        L.check(h.pcgan_image_resize_u8(ctypes.byref(r.desc), src.data_ptr(), r.kh.data_ptr(), r.bh.data_ptr(), r.kv.data_ptr(),
                                        r.bv.data_ptr(), resized.data_ptr(), N, r.band, r.rows, st), 'image_resize_u8')

    def warp():
        L.check(h.pcgan_image_affine(ctypes.byref(g.desc), resized.data_ptr(), m.data_ptr(), a.data_ptr(), out.data_ptr(), N, st),
                'image_affine')

    res = {}
    for name, fn, nbytes in (('resize_u8', resize, N * (SRC * SRC * 3 + LOAD * LOAD * 3)),
                             ('affine', warp, N * (LOAD * LOAD * 3 + 3 * FINE * FINE * 4))):
        for _ in range(5):
            fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(50):
            fn()
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / 50
        res[name] = {'ms': ms, 'bytes': nbytes, 'GB_s': nbytes / ms / 1e6, 'of_hbm_peak': nbytes / ms / 1e6 / HBM_GBS}
    t0 = time.perf_counter()
    for _ in range(20):
        tf(imgs, draws)
    torch.cuda.synchronize()
    res['host_call_ms'] = (time.perf_counter() - t0) / 20 * 1e3
    return res


def time_pil(arrs):
    from pcgan_amd.data.base_dataset import get_transform
    torch.set_num_threads(1)
    tf = get_transform(O)
    res = {}
    for mode in ('resize_and_crop', 'resize_affine_crop'):
        O.transforms = mode
        pimgs = [Image.fromarray(a) for a in arrs[:50]]
        tf(pimgs[0])
        t0 = time.perf_counter()
        for im in pimgs:
            tf(im)
        res[mode + '_ms_per_image'] = (time.perf_counter() - t0) / len(pimgs) * 1e3
    O.transforms = 'resize_affine_crop'
    return res


CHILD = r'''
import sys, time, json
sys.path.insert(0, %(root)r)
import siamese
stamps = []
inner = siamese.iteration_loss
def timed(*a):
    import torch
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    return inner(*a)
siamese.iteration_loss = timed
opt = siamese.build_parser().parse_args(%(argv)r)
siamese.train(opt)
import torch
torch.cuda.synchronize()
stamps.append(time.perf_counter())
print('STAMPS ' + json.dumps(stamps))
'''


def time_train(folder, n_pairs, workers, gpu, skip, timeout):
    argv = ['--dataroot', folder, '--datafile', os.path.join(folder, 'pairs.txt'), '--checkpoint_dir', os.path.join(folder, 'ck'),
            '--name', 'b', '--batch_size', '100', '--num_epochs', '1', '--num_workers', str(workers), '--pretrained_model_path', '',
            '--transforms', 'resize_affine_crop', '--max_dataset_size', str(n_pairs), '--print_freq', '1000', '--save_latest_freq', '100000']
    if gpu:
        argv.append('--gpu_transform')
    p = subprocess.run([sys.executable, '-c', CHILD % {'root': ROOT, 'argv': argv}], capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError('siamese.py run failed (%d):\n%s' % (p.returncode, p.stderr[-3000:]))
    stamps = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('STAMPS ')][-1][7:])
    t = stamps[skip:]
    return {'workers': workers, 'gpu_transform': gpu, 'timed_steps': len(t) - 1, 'steps_per_s': (len(t) - 1) / (t[-1] - t[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--skip', type=int, default=4)
    ap.add_argument('--no-train', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    arrs = smooth_images(N, 0)
    rng = random.Random(0)
    from pcgan_amd.data.base_dataset import draw_affine
    draws = torch.tensor([[rng.randint(0, LOAD - FINE), rng.randint(0, LOAD - FINE), rng.randint(0, 1)] + draw_affine(LOAD, LOAD, 5.0, (0.95, 1.05))
                          for _ in range(N)], dtype=torch.float64)
    res = {'device': torch.cuda.get_device_name(0), 'geometry': '%d images %dx%d -> %d -> affine -> %d' % (N, SRC, SRC, LOAD, FINE)}
    res['kernels'] = time_kernels(dev, arrs, draws)
    print(json.dumps(res, indent=1), flush=True)
    res['pil_one_core'] = time_pil(arrs)
    print(json.dumps(res['pil_one_core']), flush=True)
    if not args.no_train:
        folder = tempfile.mkdtemp(prefix='elo_bench_')
        for i, a in enumerate(arrs):
            Image.fromarray(a).save(os.path.join(folder, '%d_img.png' % i))
        n_pairs = 100 * (args.iters + args.skip)
        r = random.Random(1)
        with open(os.path.join(folder, 'pairs.txt'), 'w') as f:
            for _ in range(n_pairs):
                f.write('%d_img.png %d_img.png %d\n' % (r.randrange(N), r.randrange(N), r.randrange(3)))
        res['siamese_train'] = []
        try:
            for workers in (4, 16):
                for gpu in (False, True):
                    row = time_train(folder, n_pairs, workers, gpu, args.skip, timeout=600)
                    print(json.dumps(row), flush=True)
                    res['siamese_train'].append(row)
        finally:
            shutil.rmtree(folder, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
