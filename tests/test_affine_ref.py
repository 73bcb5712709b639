"""CPU: the float64 restatement of Pillow's bicubic affine warp (tests/affine_ref.py) is byte-equal to
`Image.transform(..., AFFINE, BICUBIC, fillcolor=127)` -- the warp of the loader's affine modes, pinned here -- and
`decode_raw` hands the GPU path exactly the draws and matrix `get_transform` consumes for both affine modes."""
import math
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import affine_ref as A


def _pillow(arr, m):
    H, W = arr.shape[:2]
    return np.asarray(Image.fromarray(arr).transform((W, H), Image.AFFINE, tuple(m), Image.BICUBIC, fillcolor=127))


def _image(h, w, seed, binary=False):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (a > 127).astype(np.uint8) * 255 if binary else a


def _matrix(w, h, angle, scale):
    from pcgan_amd.data.base_dataset import _inverse_affine_matrix
    return _inverse_affine_matrix((w * 0.5 + 0.5, h * 0.5 + 0.5), angle, (0, 0), scale, 0.0)


CASES = [
    # (h, w, angle, scale, binary)
    (40, 40, 3.7, 1.03, False), (40, 40, -4.9, 0.951, False), (60, 60, 0.3, 1.049, True), (33, 33, -2.2, 0.97, False),
    (40, 40, 171.0, 0.55, False), (40, 40, -133.3, 1.9, True), (31, 31, 540.0, 1.0, False), (24, 24, 630.0, 0.77, False),
    (40, 40, 90.0, 1.0, False), (40, 40, 180.0, 1.0, False), (40, 40, -90.0, 1.0, True), (37, 37, 270.0, 1.0, False),
    (23, 40, 12.5, 1.2, False), (40, 17, -27.0, 0.8, True), (9, 9, 45.0, 1.0, False), (9, 14, -3.0, 2.0, False),
    (1, 1, 30.0, 1.0, False), (2, 3, 10.0, 0.6, True), (40, 40, 0.0, 1.0, False),
]


@pytest.mark.parametrize('h,w,angle,scale,binary', CASES)
def test_restatement_matches_pillow(h, w, angle, scale, binary):
    arr = _image(h, w, h * 1000 + w + int(angle), binary)
    m = _matrix(w, h, angle, scale)
    got, want = A.warp(arr, m), _pillow(arr, m)
    assert got.dtype == np.uint8 and np.array_equal(got, want), 'differs in %d bytes' % int((got != want).sum())


def test_reference_range_random_draws_match_pillow():
    rng = random.Random(11)
    for k in range(12):
        h, w = rng.choice([(40, 40), (48, 48), (30, 44)])
        arr = _image(h, w, 500 + k, binary=(k % 4 == 3))
        m = _matrix(w, h, rng.uniform(-5, 5), rng.uniform(0.95, 1.05))
        assert np.array_equal(A.warp(arr, m), _pillow(arr, m))


def test_points_on_the_far_edge_take_the_fill():
    """xi == W / yi == H exactly is outside (Pillow: `xin >= im->xsize`), xi == 0 is inside"""
    arr = _image(12, 16, 3)
    for m in ([1.0, 0.0, 0.5, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0, 1.0, 0.5], [1.0, 0.0, -0.5, 0.0, 1.0, -0.5], [2.0, 0.0, -1.0, 0.0, 2.0, -1.0]):
        got, want = A.warp(arr, m), _pillow(arr, m)
        assert np.array_equal(got, want)
    got = A.warp(arr, [1.0, 0.0, 0.5, 0.0, 1.0, 0.0])
    assert (got[:, -1] == A.FILL).all() and not (got[:, 0] == A.FILL).all()


def test_fill_is_red_127_only():
    """an integer fill colour on an RGB image is packed into R: (127, 0, 0) -- the reference's observable behaviour"""
    arr = _image(10, 10, 4)
    got = _pillow(arr, [1.0, 0.0, 100.0, 0.0, 1.0, 100.0])
    assert (got == np.array([127, 0, 0], dtype=np.uint8)).all()
    assert np.array_equal(A.warp(arr, [1.0, 0.0, 100.0, 0.0, 1.0, 100.0]), got)


def _opt(tmp_path, mode, extra=()):
    from pcgan_amd.options.train_options import TrainOptions
    argv = ['train.py', '--dataroot', str(tmp_path), '--model', 'wsgan_emb', '--gpu_ids', '-1', '--checkpoints_dir', str(tmp_path / 'ck'),
            '--sourcefile_A', str(tmp_path / 'pairs.txt'), '--loadSize', '40', '--fineSize', '32', '--nThreads', '0',
            '--transforms', mode] + list(extra)
    old, sys.argv = sys.argv, argv
    try:
        return TrainOptions().parse()
    finally:
        sys.argv = old


@pytest.mark.parametrize('mode,extra', [('resize_affine_crop', ()), ('resize_affine_center', ()),
                                        ('resize_affine_crop', ('--affineDegrees', '40', '--affineScale', '0.6', '1.5')),
                                        ('resize_affine_center', ('--no_flip',))])
def test_decode_raw_draws_what_get_transform_consumes(tmp_path, mode, extra):
    from pcgan_amd.data.base_dataset import decode_raw, get_transform
    opt = _opt(tmp_path, mode, extra)
    src = Image.fromarray(_image(50, 57, 9))
    tf = get_transform(opt)
    resized = np.asarray(src.resize((40, 40), Image.BICUBIC))
    flips = set()
    for seed in range(8):
        random.seed(seed)
        want = tf(src)
        after_pil = random.random()
        random.seed(seed)
        raw, draws = decode_raw(src, opt)
        after_raw = random.random()
        assert after_pil == after_raw, 'decode_raw consumed a different number of draws'
        assert raw.dtype == torch.uint8 and np.array_equal(raw.numpy(), np.asarray(src))
        assert draws.dtype == torch.float64 and draws.shape == (9,)
        x0, y0, flip = (int(v) for v in draws[:3])
        m = [float(v) for v in draws[3:]]
        # the matrix is the one the PIL path built: angle, then scale, from the same seed
        random.seed(seed)
        angle = random.uniform(-opt.affineDegrees, opt.affineDegrees)
        scale = random.uniform(*opt.affineScale)
        assert m == _matrix(40, 40, angle, scale)
        if mode == 'resize_affine_center':
            assert (x0, y0) == (4, 4)
        assert torch.equal(A.pipeline(resized, m, x0, y0, 32, flip), want)
        flips.add(flip)
    assert flips == ({0} if '--no_flip' in extra else {0, 1})


def test_decode_raw_keeps_the_non_affine_draws():
    """the other modes' draws stay int32 (x0, y0, flip)"""
    from pcgan_amd.data.base_dataset import decode_raw

    class O(object):
        transforms, loadSize, fineSize, isTrain, no_flip = 'resize_and_crop', 40, 32, True, False
    random.seed(1)
    _, aug = decode_raw(Image.fromarray(_image(50, 50, 1)), O)
    assert aug.dtype == torch.int32 and aug.shape == (3,)
    assert math.isfinite(float(aug.sum()))
