"""GPU: the affine modes of the loader's image pipeline (pcgan_image_resize_u8 + pcgan_image_affine, GpuAffineTransform) against
Pillow and the PIL path -- BIT-EXACT: the warp kernel alone against `Image.transform(AFFINE, BICUBIC, fillcolor=127)` and its float64
restatement (tests/affine_ref.py); the whole pipeline against get_transform; the loader and siamese.py with and without
--gpu_transform; the warp beside a residual convolution on another stream; the host's refusals."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import affine_ref as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _O(object):
    def __init__(self, load, fine, transforms='resize_affine_crop', degrees=5.0, scale=(0.95, 1.05), no_flip=False):
        self.loadSize, self.fineSize, self.transforms = load, fine, transforms
        self.affineDegrees, self.affineScale = degrees, list(scale)
        self.isTrain, self.no_flip = True, no_flip


def _image(h, w, seed, binary=False):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (a > 127).astype(np.uint8) * 255 if binary else a


def _matrix(w, h, angle, scale):
    from pcgan_amd.data.base_dataset import _inverse_affine_matrix
    return _inverse_affine_matrix((w * 0.5 + 0.5, h * 0.5 + 0.5), angle, (0, 0), scale, 0.0)


def _warp_kernel(dev, resized, mats, aug, FH, FW, channels=3):
    """pcgan_image_affine alone on resized uint8 images (n, RH, RW, 3); aug rows (x0, y0, flip) -> fp32 (n, C, FH, FW)"""
    from pcgan_amd.hip import lib as L
    n, RH, RW, _ = resized.shape
    d = L.ImageDesc(RH, RW, RH, RW, FH, FW, 1, 1, channels)
    src = torch.from_numpy(np.ascontiguousarray(resized)).to(dev)
    m = torch.tensor(mats, dtype=torch.float64).reshape(n, 6).to(dev)
    a = torch.tensor([list(x) + [i] for i, x in enumerate(aug)], dtype=torch.int32).to(dev)
    out = torch.full((n, channels, FH, FW), float('nan'), device=dev)
    L.check(L.load().pcgan_image_affine(ctypes.byref(d), src.data_ptr(), m.data_ptr(), a.data_ptr(), out.data_ptr(), n,
                                        torch.cuda.current_stream().cuda_stream), 'image_affine')
    torch.cuda.synchronize()
    return out.cpu()


def _pillow_pipeline(resized, m, x0, y0, FH, FW, flip, channels=3):
    RH, RW = resized.shape[:2]
    img = Image.fromarray(resized).transform((RW, RH), Image.AFFINE, tuple(m), Image.BICUBIC, fillcolor=127)
    img = img.crop((x0, y0, x0 + FW, y0 + FH))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return A.normalise(np.asarray(img), channels)


@pytest.mark.parametrize('RH,RW,FH,FW', [(40, 40, 32, 32), (240, 240, 224, 224), (37, 53, 30, 29), (16, 16, 16, 16), (24, 31, 1, 31)])
@pytest.mark.parametrize('channels', [3, 1])
def test_warp_kernel_matches_pillow(dev, RH, RW, FH, FW, channels):
    rng = random.Random(RH * 100 + RW + channels)
    mats, aug, imgs = [], [], []
    ranges = [(5, 0.95, 1.05), (5, 0.95, 1.05), (180, 0.5, 2.0), (180, 0.5, 2.0), (720, 0.25, 0.4), (0, 1.0, 1.0)]
    for k, (deg, lo, hi) in enumerate(ranges):
        imgs.append(_image(RH, RW, 31 * k + RH, binary=(k % 3 == 2)))
        mats.append(_matrix(RW, RH, rng.uniform(-deg, deg), rng.uniform(lo, hi)))
        aug.append((rng.randint(0, RW - FW), rng.randint(0, RH - FH), k % 2))
    mats.append([1.0, 0.0, 0.5, 0.0, 1.0, -0.5])        # shifted half a pixel: the last column / first row land on xi == W / yi == 0
    imgs.append(_image(RH, RW, 5))
    aug.append((RW - FW, 0, 1))
    got = _warp_kernel(dev, np.stack(imgs), mats, aug, FH, FW, channels)
    for i, (im, m, (x0, y0, fl)) in enumerate(zip(imgs, mats, aug)):
        want = _pillow_pipeline(im, m, x0, y0, FH, FW, fl, channels)
        assert torch.equal(got[i], want), 'image %d differs from Pillow' % i
        assert torch.equal(want, A.pipeline(im, m, x0, y0, FH, fl, channels) if FH == FW else want)


def test_fill_regions_are_red_127(dev):
    """a scale of 0.3 leaves most of the window outside the source: (127, 0, 0) normalised, as the PIL path gives"""
    im = _image(40, 40, 2)
    got = _warp_kernel(dev, im[None], [_matrix(40, 40, 10.0, 0.3)], [(4, 4, 0)], 32, 32)[0]
    fill = A.normalise(np.array([[[127, 0, 0]]], dtype=np.uint8))[:, 0, 0]
    assert torch.equal(got[:, 0, 0], fill) and torch.equal(got[:, 31, 31], fill)
    assert torch.equal(got, _pillow_pipeline(im, _matrix(40, 40, 10.0, 0.3), 4, 4, 32, 32, 0))


def _pil_and_gpu(dev, opt, arrs, channels=3):
    from pcgan_amd.data.base_dataset import decode_raw, get_transform
    from pcgan_amd.data.gpu_transform import GpuAffineTransform
    tf = get_transform(opt)
    want, raws, draws = [], [], []
    for i, a in enumerate(arrs):
        img = Image.fromarray(a)
        random.seed(100 + i)
        t = tf(img)
        want.append((t[0] * 0.299 + t[1] * 0.587 + t[2] * 0.114).unsqueeze(0) if channels == 1 else t)
        random.seed(100 + i)
        raw, d = decode_raw(img, opt)
        raws.append(raw)
        draws.append(d)
    got = GpuAffineTransform(opt, dev)(raws, torch.stack(draws), out_channels=channels)
    torch.cuda.synchronize()
    return torch.stack(want), got


@pytest.mark.parametrize('mode', ['resize_affine_crop', 'resize_affine_center'])
@pytest.mark.parametrize('src,load,fine', [((200, 200), 240, 224), ((50, 50), 40, 32)])
def test_pipeline_matches_get_transform(dev, mode, src, load, fine):
    arrs = [_image(src[0], src[1], 40 + i, binary=(i == 3)) for i in range(6)]
    want, got = _pil_and_gpu(dev, _O(load, fine, mode), arrs)
    assert got.is_cuda and got.shape == want.shape and torch.equal(got.cpu(), want)


def test_pipeline_mixed_sizes_wide_draws_and_gray(dev):
    """one batch of two source sizes (one shrinks, one grows), draws far outside the reference's range, the pair dataset's gray mix"""
    arrs = [_image(*((50, 50) if i % 2 else (29, 35)), seed=60 + i) for i in range(7)]
    for channels in (3, 1):
        want, got = _pil_and_gpu(dev, _O(40, 32, 'resize_affine_crop', degrees=170.0, scale=(0.5, 1.8)), arrs, channels)
        assert torch.equal(got.cpu(), want)


def _make_pairs(tmp_path, n=8, size=(50, 50)):
    for i in range(n):
        Image.fromarray(_image(size[0] + (i % 2) * 7, size[1], 70 + i)).save(tmp_path / ('%d_img.png' % (10 + i)))
    with open(tmp_path / 'pairs.txt', 'w') as f:
        for i in range(n):
            f.write('%d_img.png %d_img.png %d\n' % (10 + i, 10 + (i + 3) % n, (0, 1, 2)[i % 3]))


@pytest.mark.parametrize('mode,threads', [('resize_affine_crop', 0), ('resize_affine_crop', 2), ('resize_affine_center', 2)])
def test_loader_end_to_end(dev, tmp_path, mode, threads):
    from pcgan_amd.data import CreateDataLoader
    from pcgan_amd.options.train_options import TrainOptions
    _make_pairs(tmp_path)

    def opt(extra):
        argv = ['train.py', '--dataroot', str(tmp_path), '--model', 'wsgan_emb', '--gpu_ids', '0', '--checkpoints_dir', str(tmp_path / 'ck'),
                '--sourcefile_A', str(tmp_path / 'pairs.txt'), '--loadSize', '40', '--fineSize', '32', '--nThreads', str(threads),
                '--batchSize', '4', '--transforms', mode] + extra
        old, sys.argv = sys.argv, argv
        try:
            return TrainOptions().parse()
        finally:
            sys.argv = old
    random.seed(21)
    torch.manual_seed(5)
    pil = list(CreateDataLoader(opt([])).load_data())
    random.seed(21)
    torch.manual_seed(5)
    gpu = list(CreateDataLoader(opt(['--gpu_transform'])).load_data())
    assert len(pil) == len(gpu) == 2
    for a, b in zip(pil, gpu):
        assert sorted(a) == sorted(b)
        assert b['A'].is_cuda and torch.equal(a['A'], b['A'].cpu()) and torch.equal(a['B'], b['B'].cpu())
        assert torch.equal(a['label'], b['label']) and a['A_paths'] == b['A_paths'] and a['B_paths'] == b['B_paths']


def _siamese(tmp_path, name, extra, monkeypatch, inner):
    sys.path.insert(0, ROOT)
    import siamese
    seen = []

    def capture(opt, net, criterion, img0, img1, label):
        seen.append((img0.detach().cpu().clone(), img1.detach().cpu().clone(), label.detach().cpu().clone()))
        return inner(opt, net, criterion, img0, img1, label)
    monkeypatch.setattr(siamese, 'iteration_loss', capture)
    common = ['--dataroot', str(tmp_path), '--datafile', str(tmp_path / 'pairs.txt'), '--checkpoint_dir', str(tmp_path / 'ck'),
              '--loadSize', '72', '--fineSize', '64', '--pretrained_model_path', '', '--transforms', 'resize_affine_crop', '--seed', '3']
    random.seed(9)
    opt = siamese.build_parser().parse_args(common + ['--name', name, '--batch_size', '4', '--num_epochs', '1', '--num_workers', '2',
                                                      '--print_freq', '1'] + extra)
    history = siamese.train(opt)
    sd = torch.load(os.path.join(str(tmp_path), 'ck', name, 'latest_net.pth'), map_location='cpu')
    random.seed(9)
    eopt = siamese.build_parser().parse_args(common + ['--name', name, '--mode', 'embedding', '--datafile', '',
                                                       '--dataroot', str(tmp_path / 'img')] + extra)
    X, _ = siamese.embedding(eopt)
    return seen, history, sd, X


def test_siamese_train_and_embedding_with_and_without_gpu_transform(dev, tmp_path, monkeypatch):
    """siamese.py --transforms resize_affine_crop: the same input batches (captured at the loss), losses and checkpoint bits with
    --gpu_transform as on the PIL path, and the same ratings from --mode embedding.  Checkpoint bits are required because two PIL-path
    runs of this training end in bit-equal latest_net.pth on the MI355X (the step's kernels reduce in a fixed order), so equal input
    batches must give equal weights."""
    _make_pairs(tmp_path, n=8, size=(80, 80))
    (tmp_path / 'img').mkdir()
    for i in range(3):
        Image.fromarray(_image(80, 80, 90 + i)).save(tmp_path / 'img' / ('%d_x.png' % (i + 1)))
    sys.path.insert(0, ROOT)
    import siamese
    inner = siamese.iteration_loss
    pil = _siamese(tmp_path, 'pil', [], monkeypatch, inner)
    gpu = _siamese(tmp_path, 'gpu', ['--gpu_transform'], monkeypatch, inner)
    assert len(pil[0]) == len(gpu[0]) == 2
    for a, b in zip(pil[0], gpu[0]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert pil[1] == gpu[1] and all(np.isfinite(pil[1]))
    assert sorted(pil[2]) == sorted(gpu[2]) and all(torch.equal(pil[2][k], gpu[2][k]) for k in pil[2])
    assert pil[3].shape == (3, 1) and np.array_equal(pil[3], gpu[3])


def test_siamese_rank_slice_equals_the_slice_of_the_full_batch(dev, tmp_path):
    """under data parallelism siamese.py transforms only its rank's slice of the global batch: the rows of the full transform"""
    sys.path.insert(0, ROOT)
    import siamese
    _make_pairs(tmp_path, n=8)
    opt = siamese.build_parser().parse_args(['--dataroot', str(tmp_path), '--datafile', str(tmp_path / 'pairs.txt'), '--loadSize', '40',
                                             '--fineSize', '32', '--transforms', 'resize_affine_crop', '--gpu_transform'])
    data = siamese.PairDataset(opt, opt.dataroot, opt.datafile)
    tf = siamese.gpu_pipeline(opt, data, dev)
    random.seed(2)
    batch = siamese.collate_keep_raw([data[i] for i in range(8)])
    full = siamese.pair_batch(batch, tf, dev)
    for world in (2, 4):
        for rank in range(world):
            part = siamese.pair_batch(batch, tf, dev, rank, world)
            lo, hi = rank * 8 // world, (rank + 1) * 8 // world
            assert all(torch.equal(p, f[lo:hi]) for p, f in zip(part, full))


def test_warp_beside_a_residual_convolution(dev):
    """the affine launches on a side stream while residual-block convolutions run on another: the same bytes as alone"""
    from pcgan_amd.data.gpu_transform import GpuAffineTransform
    from pcgan_amd.hip import ops
    opt = _O(240, 224)
    tf = GpuAffineTransform(opt, dev)
    raws = [torch.from_numpy(_image(200, 200, 200 + i)) for i in range(16)]
    rng = random.Random(4)
    draws = torch.tensor([[rng.randint(0, 16), rng.randint(0, 16), i % 2] + _matrix(240, 240, rng.uniform(-5, 5), rng.uniform(0.95, 1.05))
                          for i in range(16)], dtype=torch.float64)
    ref = tf(raws, draws).clone()
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(4)
    xr = torch.randn(32, 256, 32, 32, generator=g).to(dev)
    wr = (torch.randn(256, 256, 3, 3, generator=g) * 0.05).to(dev)
    cache = {}
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(4):
        other.wait_stream(torch.cuda.current_stream())
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(other):
            for _ in range(3):
                ops.conv2d_fwd(xr, wr, None, 1, 1, 1, pack_cache=cache)
        with torch.cuda.stream(side):
            out = tf(raws, draws)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


def test_host_refuses_bad_input(dev):
    from pcgan_amd.data.gpu_transform import GpuAffineTransform
    tf = GpuAffineTransform(_O(40, 32), dev)
    raw = [torch.from_numpy(_image(50, 50, 1))]
    m = _matrix(40, 40, 1.0, 1.0)
    tf(raw, torch.tensor([[8, 8, 0] + m], dtype=torch.float64))          # the largest offset fits
    for bad in ([9, 0, 0], [0, 9, 0], [-1, 0, 0], [0, 0, 2], [0.5, 0, 0]):
        with pytest.raises(ValueError):
            tf(raw, torch.tensor([bad + m], dtype=torch.float64))
    with pytest.raises(ValueError, match='uint8'):
        tf([raw[0].float()], torch.tensor([[0, 0, 0] + m], dtype=torch.float64))
    with pytest.raises(ValueError, match='uint8'):
        tf([raw[0][:, :, :1].contiguous()], torch.tensor([[0, 0, 0] + m], dtype=torch.float64))
    with pytest.raises(ValueError, match='smaller than'):
        GpuAffineTransform(_O(30, 32), dev)(raw, torch.tensor([[0, 0, 0] + m], dtype=torch.float64))
