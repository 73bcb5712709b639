"""CPU: host side of the affine GPU pipeline -- which class the loader picks for each --transforms mode, the refusals, the
loader's collate of the affine draws (matrix included), and siamese.py's new switches with their defaults unchanged."""
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _O(object):
    loadSize, fineSize, isTrain, no_flip, affineDegrees, affineScale = 40, 32, True, False, 5.0, [0.95, 1.05]

    def __init__(self, transforms):
        self.transforms = transforms


def test_factory_picks_the_class_by_mode():
    from pcgan_amd.data.gpu_transform import GpuAffineTransform, GpuTransform, make_gpu_transform
    for mode in ('resize_affine_crop', 'resize_affine_center'):
        assert type(make_gpu_transform(_O(mode), 'cuda:0')) is GpuAffineTransform
        with pytest.raises(NotImplementedError, match='GpuAffineTransform'):
            GpuTransform(_O(mode), 'cuda:0')
    for mode in ('resize_and_crop', 'crop', 'scale_width', 'scale_width_and_crop', 'none'):
        assert type(make_gpu_transform(_O(mode), 'cuda:0')) is GpuTransform
        with pytest.raises(NotImplementedError, match='affine modes'):
            GpuAffineTransform(_O(mode), 'cuda:0')
    with pytest.raises(RuntimeError, match='no fallback'):
        GpuAffineTransform(_O('resize_affine_crop'), 'cpu')


def test_collate_carries_the_matrix():
    from pcgan_amd.data import _collate_keep_raw
    from pcgan_amd.data.base_dataset import decode_raw
    rng = np.random.default_rng(0)
    samples = []
    random.seed(5)
    for k, size in enumerate(((50, 50), (44, 61), (50, 50))):
        raw, draws = decode_raw(Image.fromarray(rng.integers(0, 256, size + (3,), dtype=np.uint8)), _O('resize_affine_crop'))
        samples.append({'A_raw': raw, 'A_aug': draws, 'label': k})
    batch = _collate_keep_raw(samples)
    assert isinstance(batch['A_raw'], list) and [tuple(r.shape) for r in batch['A_raw']] == [(50, 50, 3), (44, 61, 3), (50, 50, 3)]
    assert batch['A_aug'].dtype == torch.float64 and batch['A_aug'].shape == (3, 9)
    assert all(torch.equal(batch['A_aug'][i], s['A_aug']) for i, s in enumerate(samples))


def test_siamese_switches_and_defaults():
    sys.path.insert(0, ROOT)
    import siamese
    opt = siamese.build_parser().parse_args(['--dataroot', 'x'])
    assert opt.gpu_transform is False and opt.transforms == 'resize_and_crop'
    assert opt.affineDegrees == 5 and opt.affineScale == [0.95, 1.05]
    opt = siamese.build_parser().parse_args(['--dataroot', 'x', '--gpu_transform', '--transforms', 'resize_affine_crop',
                                             '--affineDegrees', '10', '--affineScale', '0.9', '1.1'])
    assert opt.gpu_transform and opt.affineDegrees == 10.0 and opt.affineScale == [0.9, 1.1]


def test_siamese_pair_dataset_raw_and_pil_agree(tmp_path):
    """with --gpu_transform the pair data set hands out the decoded bytes and the draws the PIL path consumes; collate keeps the
    bytes a list and slices per rank stay aligned"""
    sys.path.insert(0, ROOT)
    import siamese
    from affine_ref import pipeline
    rng = np.random.default_rng(3)
    for i in range(4):
        Image.fromarray(rng.integers(0, 256, (50, 50, 3), dtype=np.uint8)).save(tmp_path / ('%d.png' % i))
    with open(tmp_path / 'pairs.txt', 'w') as f:
        f.write('0.png 1.png 2\n2.png 3.png 0\n')
    args = ['--dataroot', str(tmp_path), '--datafile', str(tmp_path / 'pairs.txt'), '--loadSize', '40', '--fineSize', '32',
            '--transforms', 'resize_affine_crop']
    pil = siamese.PairDataset(siamese.build_parser().parse_args(args), str(tmp_path), str(tmp_path / 'pairs.txt'))
    raw = siamese.PairDataset(siamese.build_parser().parse_args(args + ['--gpu_transform']), str(tmp_path), str(tmp_path / 'pairs.txt'))
    for i in range(2):
        random.seed(i)
        A, B, lab = pil[i]
        random.seed(i)
        rA, dA, rB, dB, lab2 = raw[i]
        assert int(lab) == int(lab2)
        for want, r, d in ((A, rA, dA), (B, rB, dB)):
            resized = np.asarray(Image.fromarray(r.numpy()).resize((40, 40), Image.BICUBIC))
            x0, y0, flip = (int(v) for v in d[:3])
            assert torch.equal(pipeline(resized, [float(v) for v in d[3:]], x0, y0, 32, flip), want)
    batch = siamese.collate_keep_raw([raw[0], raw[1]])
    assert isinstance(batch[0], list) and batch[1].shape == (2, 9) and batch[4].tolist() == [2, 0]
