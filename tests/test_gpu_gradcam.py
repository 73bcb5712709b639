"""pcgan_gradcam_map and pcgan_heatmap_overlay (csrc/gradcam.hip) against the float64 restatements of tests/gradcam_ref.py, the capture of
util/gradcam.py against the float64 twin of the encoder replaying the HIP pass's decisions, and `siamese.py --mode attention` end to end.

The bound on the map.  Inputs are taken as stored (bf16 values are widened exactly), the unit is built with contraction off, so every
operation is one fp32 rounding and |map - exact| <= d * 2^-24 * sum_c |term| per pixel (relu and abs are 1-Lipschitz: the bound on the
channel sum passes through them), d = the longest chain of roundings an element passes through in the kernel as written
(chain_length below mirrors the launch geometry):
    a unit is V consecutive pixels, V = 4 (fp32) / 8 (bf16) in the 16-byte form and 1 in the element form; units = HW / V;
    LP = min(64, next power of two >= units) lanes share a tile, the S = 1024 / LP slices of the workgroup split the channels
      ceil(C / S)   additions of a slice's channels in ascending c (the first is 0 + x, exact)
    + log2(S)       the halving tree over the slices in LDS
    + 1             pw, cw_pos: the product g * A or w * A;  + 2 for pw_cw: (w * g) * A
    + log2(V) + ceil(units / 64) + 6 + 1     cw_pos, pw_cw: the relative error of w[n][c], a sum of non-negative terms -- the relu'd elements
                    of a unit in a balanced tree, the units a lane owns in index order (the first addition exact), the wave64 butterfly and
                    the division by HW.
The exact additions cover the second-order terms of (1 + 2^-24)^d - 1.  The largest d here is 142 (2048 x 7 x 7, pw_cw, element
form: 128 + 4 + 2 + 0 + 1 + 6 + 1); the default layer 64 x 56 x 56 in fp32 has 4 + 4 + 2 + 2 + 13 + 6 + 1 = 32.

The bound on the overlay.  heat = (((m - lo) / (hi - lo)) * 255) * (1 - alpha) passes m - lo, hi - lo, the division, * 255, 1 - alpha
and the product: 6 roundings on a value <= 255; pix * alpha passes img * std, + mean, * 255 and * alpha: 4 roundings, the first of them
relative to |img * std| <= |img * std + mean| + |mean| (|mean| * 255 < 126); the final addition is one more on each.  In all at most
7 * 255 + 5 * |pix| + 126 <= 8 * (255 + |pix|) units of 2^-24: the issue's count of one rounding per operation holds for the kernel as
written.  lo and hi are selections and carry no rounding."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import gradcam_ref as R
from oracle import networks_ref as N
from oracle import weights as W
from test_gpu_nets import _assert_mostly_close, record_decisions
from util_cmp import assert_close

pytestmark = pytest.mark.gpu

MAP_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 17, 8, 8), (1, 64, 9, 9), (2, 512, 7, 7), (1, 2048, 7, 7), (1, 64, 56, 56)]
OVERLAY_SHAPES = [(1, 3, 1, 1), (2, 3, 5, 7), (1, 3, 64, 66), (2, 3, 224, 224)]
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
PAD = 64                    # canary elements on either side of an output (256 bytes of fp32)
U = 2.0 ** -24
THREADS = 1024
DTYPES = [torch.float32, torch.bfloat16]


def _ids(s):
    return 'x'.join(str(v) for v in s)


def _wide(HW, esize, *ptrs):
    return (HW * esize) % 16 == 0 and all(p % 16 == 0 for p in ptrs)


def chain_length(kind, C, HW, esize, wide):
    V = 16 // esize if wide else 1
    units = HW // V
    LP = 1
    while LP < 64 and LP < units:
        LP *= 2
    S = THREADS // LP
    d = -(-C // S) + int(math.log2(S))
    d += {'raw': 0, 'pw': 1, 'cw_pos': 1, 'pw_cw': 2}[kind]
    if kind in ('cw_pos', 'pw_cw'):
        d += int(math.log2(V)) + -(-units // 64) + 6 + 1
    return d


class Guarded(object):
    """an fp32 output buffer with PAD canary elements on either side, the whole of it filled with the canary"""

    def __init__(self, shape, dev, canary):
        numel = int(np.prod(shape))
        self.buf = torch.full((numel + 2 * PAD,), canary, dtype=torch.float32, device=dev)
        self.before = self.buf.clone()
        self.body = self.buf[PAD:PAD + numel].view(shape)

    def pads_intact(self):
        n = self.buf.numel()
        return torch.equal(self.buf[:PAD], self.before[:PAD]) and torch.equal(self.buf[n - PAD:], self.before[n - PAD:])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _map_call(act, grad, kind):
    """one pcgan_gradcam_map call into a guarded buffer; returns (map, took the 16-byte form)"""
    from pcgan_amd.hip import lib, ops
    Nb, C, H, Wd = act.shape
    out = Guarded((Nb, 1, H, Wd), act.device, -7.0)
    dt = lib.F32 if act.dtype == torch.float32 else lib.BF16
    pg = grad.data_ptr() if grad is not None else None
    lib.check(lib.load().pcgan_gradcam_map(act.data_ptr(), pg, out.body.data_ptr(), Nb, C, H, Wd, lib.GCAM_TYPES[kind], dt, ops._stream()),
              'gradcam_map')
    torch.cuda.synchronize()
    assert out.pads_intact(), 'a canary beside the map changed'
    used = [act.data_ptr(), out.body.data_ptr()] + ([pg] if (grad is not None and kind != 'raw') else [])
    return out.body, _wide(H * Wd, act.element_size(), *used)


def _check_map(act, grad, kind, label):
    Nb, C, H, Wd = act.shape
    exact, mass = R.gradcam_map(act, grad, kind)
    got, wide = _map_call(act, grad, kind)
    d = chain_length(kind, C, H * Wd, act.element_size(), wide)
    err, bound = np.abs(got.cpu().double().numpy() - exact), d * U * mass
    print('%s %s: d = %d (%s form), worst error / bound %.3f' % (label, kind, d, '16-byte' if wide else 'element',
                                                               float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), '%s %s: map off by at most %r, bound %r' % (label, kind, err.max(), bound.max())
    again, _ = _map_call(act, grad, kind)
    assert torch.equal(_bits(again), _bits(got)), '%s %s: two calls, different bits' % (label, kind)
    return got


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', MAP_SHAPES, ids=_ids)
def test_map_against_float64(shape, dtype, dev):
    act = W.seeded_normal(shape, 700 + sum(shape)).to(dtype).to(dev)
    grad = W.seeded_normal(shape, 900 + sum(shape)).to(dtype).to(dev)
    label = 'shape %r %s' % (shape, 'fp32' if dtype == torch.float32 else 'bf16')
    maps = {kind: _check_map(act, grad, kind, label) for kind in R.MAP_TYPES}
    # raw reads no gradient: a NULL gradient gives the same bits
    assert torch.equal(_bits(_map_call(act, None, 'raw')[0]), _bits(maps['raw'])), label
    if shape[1] > 1 and shape[2] * shape[3] > 1:
        assert float(maps['pw'].max()) > 0 and float(maps['cw_pos'].max()) > 0 and float(maps['pw_cw'].max()) > 0


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 64, 56, 56)], ids=_ids)
def test_map_signs(shape, dtype, dev):
    """an all-negative gradient leaves no positive weight: the weighted maps are exactly zero; a negative channel sum gives its absolute
    value under raw"""
    act = W.seeded_normal(shape, 41).to(dtype).to(dev)
    grad = (-W.seeded_normal(shape, 42).abs() - 0.5).to(dtype).to(dev)
    for kind in ('cw_pos', 'pw_cw'):
        got, _ = _map_call(act, grad, kind)
        assert bool((got == 0).all()), kind
    neg = -act.abs() - 0.25
    got = _check_map(neg, None, 'raw', 'negative sums %r' % (shape,))
    assert bool((got > 0).all())
    assert torch.equal(_bits(got), _bits(_map_call(-neg, None, 'raw')[0]))


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_weighted_map_at_the_channel_limit(dtype, dev):
    """C = 4096, the most the weighted types admit, in the 16-byte form: the largest dynamic LDS of any launch (bf16: 32 KiB of partial sums
    + 16 KiB of plane means)"""
    shape = (1, 4096, 4, 4)
    act, grad = W.seeded_normal(shape, 71).to(dtype).to(dev), W.seeded_normal(shape, 72).to(dtype).to(dev)
    for kind in ('cw_pos', 'pw_cw'):
        _check_map(act, grad, kind, 'channel limit %s' % dtype)
    assert _map_call(act, grad, 'cw_pos')[1]


def test_map_view_at_an_odd_storage_offset(dev):
    """act one element into its storage, HW % 4 == 0: the base pointer is not 16-byte aligned, so the element form must be taken"""
    shape = (2, 5, 8, 8)
    n = int(np.prod(shape))
    store = torch.zeros(n + 1, device=dev)
    store[1:] = W.seeded_normal((n,), 93).to(dev)
    act = store[1:].view(shape)
    grad = W.seeded_normal(shape, 94).to(dev)
    assert act.is_contiguous() and act.data_ptr() % 16 != 0
    for kind in R.MAP_TYPES:
        _check_map(act, grad, kind, 'offset view')
    assert not _map_call(act, grad, 'pw')[1]


# --------------------------------------------------------------------------------------------------------------------------- overlay
def _overlay_call(hmap, img, alpha):
    from pcgan_amd.hip import lib, ops
    import ctypes
    Nb, Cm, H, Wd = hmap.shape
    out, lohi = Guarded((Nb, 3, H, Wd), img.device, -7.0), Guarded((Nb, 2), img.device, -9.0)
    dt = lib.F32 if img.dtype == torch.float32 else lib.BF16
    f3 = ctypes.c_float * 3
    lib.check(lib.load().pcgan_heatmap_overlay(hmap.data_ptr(), img.data_ptr(), f3(*MEAN), f3(*STD), alpha, out.body.data_ptr(),
                                               lohi.body.data_ptr(), Nb, Cm, H, Wd, dt, ops._stream()), 'heatmap_overlay')
    torch.cuda.synchronize()
    assert out.pads_intact() and lohi.pads_intact(), 'a canary beside an output changed'
    return out.body, lohi.body


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('Cm', [1, 3])
@pytest.mark.parametrize('shape', OVERLAY_SHAPES, ids=_ids)
def test_overlay_against_float64(shape, Cm, dtype, dev):
    Nb, _, H, Wd = shape
    alpha = 0.3
    hmap = W.seeded_normal((Nb, Cm, H, Wd), 50 + H).to(dev)
    img = W.seeded_tensor(shape, 60 + H, -2.0, 2.0).to(dtype).to(dev)
    got, lohi = _overlay_call(hmap, img, alpha)
    exact, lohi_r, pix = R.overlay(hmap, img, MEAN, STD, alpha)
    assert np.array_equal(lohi.cpu().double().numpy(), lohi_r), 'lohi %r vs %r' % (lohi.cpu(), lohi_r)
    err, bound = np.abs(got.cpu().double().numpy() - exact), 8 * U * (255.0 + np.abs(pix))
    print('overlay %r Cm=%d: worst error / bound %.3f' % (shape, Cm, float((err / bound).max())))
    assert (err <= bound).all(), 'overlay off by at most %r' % err.max()
    # the reference's alpha, and two calls
    got2, _ = _overlay_call(hmap, img, 0.01)
    exact2, _, pix2 = R.overlay(hmap, img, MEAN, STD, 0.01)
    assert (np.abs(got2.cpu().double().numpy() - exact2) <= 8 * U * (255.0 + np.abs(pix2))).all()
    assert torch.equal(_bits(_overlay_call(hmap, img, 0.01)[0]), _bits(got2))
    # a constant map: the heat term is 0, what is left is exactly ((img * std + mean) * 255) * alpha in separate fp32 operations
    flat = torch.full((Nb, Cm, H, Wd), 3.5, device=dev)
    got, lohi = _overlay_call(flat, img, alpha)
    x = img.cpu().float()
    want = ((x * torch.tensor(STD).view(1, 3, 1, 1) + torch.tensor(MEAN).view(1, 3, 1, 1)) * 255.0) * torch.tensor(alpha, dtype=torch.float32)
    assert bool((lohi == 3.5).all()) and torch.equal(got.cpu(), want)
    if H * Wd == 1 and Cm == 1:       # a one-pixel map is constant whatever it holds
        assert torch.equal(_overlay_call(hmap, img, alpha)[0].cpu(), want)


def test_overlay_wrapper(dev):
    from pcgan_amd.hip import ops
    hmap = W.seeded_normal((2, 1, 16, 16), 5).to(dev)
    img = W.seeded_tensor((2, 3, 16, 16), 6).to(dev)
    out, lohi = ops.heatmap_overlay(hmap, img, MEAN, STD, 0.01)
    assert torch.equal(_bits(out), _bits(_overlay_call(hmap, img, 0.01)[0])) and lohi.shape == (2, 2)
    plain, _ = ops.heatmap_overlay(hmap, img, MEAN, STD, 1.0)          # alpha = 1: the de-normalised image alone
    want = (img.cpu() * torch.tensor(STD).view(1, 3, 1, 1) + torch.tensor(MEAN).view(1, 3, 1, 1)) * 255.0
    assert torch.equal(plain.cpu(), want)
    A, g = W.seeded_normal((2, 5, 4, 4), 7).to(dev), W.seeded_normal((2, 5, 4, 4), 8).to(dev)
    for kind in R.MAP_TYPES:
        assert torch.equal(_bits(ops.gradcam_map(A, g, kind)), _bits(_map_call(A, g, kind)[0]))
    assert torch.equal(_bits(ops.gradcam_map(A, None, 'raw')), _bits(_map_call(A, g, 'raw')[0]))
    with pytest.raises(RuntimeError, match='needs the gradient'):
        ops.gradcam_map(A, None, 'pw')


# --------------------------------------------------------------------------------------------------------------------------- capture
@pytest.fixture(scope='module')
def encoder_pair(dev):
    """a resnet18 SiameseFeature on the HIP modules and its float64 twin with the same weights, one 64 x 64 image"""
    from pcgan_amd.models import networks
    twin = N.SiameseFeatureRef(N.ResNetFeatureRef('resnet18'), 'avg', (8, 1), 1, 0.7, False)
    twin.load_state_dict(W.fill_state_dict(twin.state_dict(), 33))
    hip = networks.SiameseFeature(networks.ResNetFeature(3, 'resnet18', dropout=0.), pooling='avg', cnn_dim=[8, 1], cnn_pad=1,
                                  cnn_relu_slope=0.7, drop_layer=networks.get_dropout_layer(dropout=0.))
    hip.load_state_dict({k: v.clone() for k, v in twin.state_dict().items()})
    return hip.to(dev), twin.double(), W.seeded_tensor((1, 3, 64, 64), 133)


def _twin_capture(twin, resolved, x, tape):
    """(A, g) of the float64 twin on the HIP pass's decisions"""
    box = []

    def hook(mod, args, out):
        leaf = out.detach().requires_grad_(True)
        box.append(leaf)
        return leaf
    handle = dict(twin.named_modules())[resolved].register_forward_hook(hook)
    N.DecisionTape.replay = iter(tape)
    try:
        rating = twin(x.double())
        assert next(N.DecisionTape.replay, None) is None, 'the twin consumed fewer decisions than the HIP pass recorded'
    finally:
        N.DecisionTape.replay = None
        handle.remove()
    (g,) = torch.autograd.grad(rating.sum(), box[-1])
    return box[-1].detach(), g


@pytest.mark.parametrize('layer,resolved,shape', [('base.model.layer1.0.conv1', 'base.model.layer1.0.conv1', (1, 64, 16, 16)),
                                                 ('base.model.layer4', 'base.model.layer4.1', (1, 512, 2, 2)),
                                                 ('cnn.0', 'cnn.0', (1, 8, 2, 2))])
def test_capture_against_the_float64_twin(layer, resolved, shape, encoder_pair, dev):
    from pcgan_amd.util.gradcam import GradCAM
    hip, twin, x = encoder_pair
    gcam = GradCAM(hip, layer)
    assert gcam.resolved == resolved
    with record_decisions() as rec:
        A, g = gcam.capture(x.to(dev))
    torch.cuda.synchronize()
    assert tuple(A.shape) == shape == tuple(g.shape) and A.dtype == g.dtype == torch.float32
    assert all(p.grad is None for p in hip.parameters()), 'the capture left a parameter gradient behind'
    assert all(p.requires_grad for p in hip.parameters()) and not A.requires_grad
    A_r, g_r = _twin_capture(copy.deepcopy(twin), resolved, x, rec.tape)
    print('%s: A rel. max error %.3e, g rel. L2 error %.3e' % (layer, float((A.cpu().double() - A_r).abs().max() / A_r.abs().max()),
                                                             float((g.cpu().double() - g_r).norm() / g_r.norm())))
    assert float(g_r.abs().max()) > 0
    assert_close(A, A_r, 1e-4, 'A at %s vs fp64 twin on the HIP decisions' % layer)
    # util_cmp.assert_close has no relative-L2 form: the project's gradient criterion (5e-4 relative L2, NaN fails) lives in test_gpu_nets
    _assert_mostly_close(g, g_r, 'd rating / dA at %s vs fp64 twin on the HIP decisions' % layer, 5e-4)
    # the map of the pair is the kernel's map of exactly these two tensors
    from pcgan_amd.hip import ops
    assert torch.equal(_bits(gcam.map(x.to(dev), 'pw_cw')), _bits(ops.gradcam_map(A, g, 'pw_cw')))


def test_input_gradient_against_the_float64_twin(encoder_pair, dev):
    from pcgan_amd.util.gradcam import GradCAM
    hip, twin, x = encoder_pair
    with record_decisions() as rec:
        g = GradCAM(hip, 'cnn').input_gradient(x.to(dev))
    N.DecisionTape.replay = iter(rec.tape)
    try:
        g_r = R.input_gradient(copy.deepcopy(twin), x.double())
    finally:
        N.DecisionTape.replay = None
    assert tuple(g.shape) == (1, 3, 64, 64) and all(p.grad is None for p in hip.parameters())
    _assert_mostly_close(g, g_r, 'd rating / d image vs fp64 twin on the HIP decisions', 5e-4)


# ---------------------------------------------------------------------------------------------------------------------------- script
def _script_options(tmp_path, *extra):
    import siamese
    return siamese.build_parser().parse_args(
        ['--dataroot', 'synthetic', '--mode', 'attention', '--name', 'elo', '--checkpoint_dir', str(tmp_path), '--fineSize', '64',
         '--cnn_dim', '8', '1', '--batch_size', '1', '--max_dataset_size', '2', '--pretrained_model_path', '',
         '--gcam_dir', str(tmp_path / 'attn')] + list(extra))


def _fresh_checkpoint(tmp_path, dev):
    import siamese
    torch.manual_seed(5)
    net = siamese.build_net(_script_options(tmp_path), dev)
    os.makedirs(str(tmp_path / 'elo'), exist_ok=True)
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, str(tmp_path / 'elo' / 'latest_net.pth'))


def test_attention_script(tmp_path, dev):
    import siamese
    from PIL import Image
    from pcgan_amd.hip import functional as HF, ops
    from pcgan_amd.util.gradcam import GradCAM
    _fresh_checkpoint(tmp_path, dev)
    opt = _script_options(tmp_path, '--gcam_save', '--gcam_type', 'cw_pos')
    results = siamese.attention(opt)
    assert len(results) == 2 and all(len(r) == 4 for r in results)
    net = siamese.build_net(opt, dev)                    # (attention() set continue_train: the checkpoint is loaded again)
    gcam = GradCAM(net, opt.gcam_layer)
    data = siamese.PairDataset(opt, opt.dataroot, opt.datafile)
    for i in range(2):
        imgs = data[i][:2]
        for k, tag in enumerate('AB'):
            img = imgs[k][None].to(dev)
            A, g = gcam.capture(img)
            m = ops.gradcam_map(A, g, 'cw_pos')
            assert tuple(m.shape) == (1, 1, 16, 16) and torch.equal(_bits(results[i][k]), _bits(m.cpu())), 'pair %d image %s' % (i, tag)
            over, lohi = ops.heatmap_overlay(HF.upsample2d(m, 64).contiguous(), img, MEAN, STD, 0.01)
            assert torch.equal(results[i][2 + k], lohi.cpu())
            want = np.clip(np.rint(over[0].cpu().numpy()), 0, 255).astype(np.uint8).transpose(1, 2, 0)
            a = np.array(Image.open(str(tmp_path / 'attn' / ('iter%d_%s_a.png' % (i, tag)))))
            x = np.array(Image.open(str(tmp_path / 'attn' / ('iter%d_%s_x.png' % (i, tag)))))
            assert a.shape == x.shape == (64, 64, 3) and a.dtype == np.uint8 and a.size == 3 * 64 * 64
            assert np.array_equal(a, want)
            plain = (imgs[k] * torch.tensor(STD).view(3, 1, 1) + torch.tensor(MEAN).view(3, 1, 1)) * 255.0
            assert np.array_equal(x, np.clip(np.rint(plain.numpy()), 0, 255).astype(np.uint8).transpose(1, 2, 0))
    assert sorted(os.listdir(str(tmp_path / 'attn'))) == sorted('iter%d_%s_%s.png' % (i, t, s) for i in range(2) for t in 'AB' for s in 'xa')


def test_attention_script_input_type(tmp_path, dev):
    import siamese
    _fresh_checkpoint(tmp_path, dev)
    results = siamese.attention(_script_options(tmp_path, '--gcam_type', 'input'))
    assert len(results) == 2 and not os.path.exists(str(tmp_path / 'attn'))
    for mA, mB, lhA, lhB in results:
        for m, lh in ((mA, lhA), (mB, lhB)):
            assert tuple(m.shape) == (1, 3, 64, 64) and float(m.abs().max()) > 0
            assert float(lh[0, 0]) == float(m.min()) and float(lh[0, 1]) == float(m.max())
