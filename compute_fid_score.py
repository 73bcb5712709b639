#!/usr/bin/env python
"""Frechet Inception Distance between two image sets (reference compute_fid_score.py).

    python compute_fid_score.py gen_dir real_dir --features inception --inception_weights inception_v3_google.pth [--dims 2048]
    python compute_fid_score.py gen.txt real.txt --dataroot rootA rootB --features inception --inception_weights ...
    python compute_fid_score.py stats_a.npz stats_b.npz            # precomputed 'mu' + 'sigma', or raw 'act'
    python compute_fid_score.py gen_dir real_dir --features alexnet --pretrained_model_path_IP alexnet.pth

Each path is a directory of *.jpg / *.png, a .txt list of file names under the matching --dataroot (both as in the
reference), or an .npz of statistics.  The metric is pcgan_amd/util/fid.py, held to the reference's own function by
tests/test_fid.py.

`--features inception` is the reference's feature extractor: torchvision's Inception-v3 blocks (models/inception.py) on the
HIP path (pcgan_amd/models/inception.py), features of the block `--dims` selects (64, 192, 768 or 2048 = pool3, the default),
spatially averaged when not 1 x 1.  The reference downloads the weights (models/inception.py:60); nothing is downloaded here,
so `--inception_weights` must name a torchvision inception_v3 state_dict (inception_v3_google-*.pth) and the script refuses
to run without one -- FID from random weights is not FID.  pytorch-fid's FIDInception weights (1008 classes) are a different
network and are refused.  `--features alexnet` = the AlexNet identity network of the training step (conv5 features,
spatially averaged, 256 dims): numbers from it are Frechet-AlexNet distances, not FID.
"""
import argparse
import os
import pathlib

import numpy as np


def list_images(path, dataroot):
    if path.endswith('.txt'):
        with open(path, 'r') as f:
            return [os.path.join(dataroot, line.rstrip('\n')) for line in f.readlines()]
    p = pathlib.Path(path)
    return sorted(str(x) for x in list(p.glob('*.jpg')) + list(p.glob('*.png')))


def load_images(files):
    """(n, 3, H, W) float32 in [0, 1] (compute_fid_score.py:208-220)"""
    from PIL import Image
    imgs = np.array([np.asarray(Image.open(fn).convert('RGB'), dtype=np.float32) for fn in files])
    return imgs.transpose((0, 3, 1, 2)) / 255.0


def alexnet_features(weights, device):
    import torch
    from pcgan_amd.models import networks
    net = networks.define_IP('alexnet', 3, [device.index])
    if weights:
        getattr(net, 'module', net).load_pretrained(weights)
    else:
        print('WARNING: --pretrained_model_path_IP not given: random AlexNet features')
    net.eval()
    from pcgan_amd.util.script import MEAN, STD
    from pcgan_amd.util.util import upsample2d
    norm = networks.Normalize(MEAN, STD)
    return lambda batch: net(norm(upsample2d(batch.to(device) * 2 - 1, 224)))


def inception_features(weights, device, dims):
    """the reference's InceptionV3([BLOCK_INDEX_BY_DIM[dims]]) on the HIP path; batch -> (b, dims, h, w) features"""
    from pcgan_amd.models.inception import InceptionV3
    net = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]], weights=weights, gpu_ids=[device.index])
    return lambda batch: net(batch.float())[0]


def statistics_of(path, dataroot, model, batch_size):
    from pcgan_amd.util.fid import activation_statistics, get_activations
    if path.endswith('.npz'):
        z = np.load(path)
        return (z['mu'], z['sigma']) if 'mu' in z else activation_statistics(z['act'])
    if model is None:
        raise RuntimeError('image paths need a feature extractor: pass --features inception --inception_weights PATH (or alexnet)')
    import torch
    files = list_images(path, dataroot)
    if not files:
        raise RuntimeError('Invalid path: %s' % path)
    return activation_statistics(get_activations(torch.from_numpy(load_images(files)), model, batch_size))


def main():
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('path', type=str, nargs=2, help='generated / real images: directory, .txt list or .npz statistics')
    ap.add_argument('--dataroot', type=str, nargs=2, default=['', ''])
    ap.add_argument('--batch-size', type=int, default=64)
    ap.add_argument('--features', choices=['none', 'alexnet', 'inception'], default='none')
    ap.add_argument('--dims', type=int, default=2048, choices=[64, 192, 768, 2048],
                    help='Inception features: block 0 / 1 / 2 / 3 (pool3) of the reference InceptionV3')
    ap.add_argument('--inception_weights', type=str, default='', help='torchvision inception_v3 state_dict (.pth)')
    ap.add_argument('--pretrained_model_path_IP', type=str, default='')
    ap.add_argument('-c', '--gpu', default='0', type=str)
    ap.add_argument('--result_path', type=str, default='')
    args = ap.parse_args()
    if args.features == 'inception' and not args.inception_weights:
        ap.error('--features inception needs --inception_weights PATH (a torchvision inception_v3 state_dict): '
                 'the weights are not downloaded, and FID is never computed from random weights')
    from pcgan_amd.util.fid import frechet_distance
    model = None
    if args.features == 'alexnet':
        import torch
        model = alexnet_features(args.pretrained_model_path_IP, torch.device('cuda:%d' % int(args.gpu)))
    elif args.features == 'inception':
        import torch
        model = inception_features(args.inception_weights, torch.device('cuda:%d' % int(args.gpu)), args.dims)
    m1, s1 = statistics_of(args.path[0], args.dataroot[0], model, args.batch_size)
    m2, s2 = statistics_of(args.path[1], args.dataroot[1], model, args.batch_size)
    value = frechet_distance(m1, s1, m2, s2)
    what = ('inception %d' % args.dims) if args.features == 'inception' else args.features
    print('Frechet distance (%s features): %.6f' % (what if model else 'precomputed', value))
    if args.result_path:
        with open(args.result_path, 'a') as f:
            f.write('%s %s %.6f\n' % (args.path[0], args.path[1], value))
    return value


if __name__ == '__main__':
    main()
