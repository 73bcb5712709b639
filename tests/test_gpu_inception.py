"""GPU: the Inception-v3 feature network on the HIP path (csrc/inception.hip, pcgan_amd/models/inception.py) against the CPU oracle
(tests/inception_ref.py).  fp32 results are judged against float64 by the SURVEY 8c rule: ||y - y64|| <= 2 ||y32 - y64|| + tiny, y32 =
torch fp32 on the CPU.  Slice writes leave the rest of the output bit-unchanged; the slice max pool is exact."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.678


def _rule(got, y32, y64, what, tiny=1e-30):
    got, y32, y64 = got.detach().double().cpu(), y32.double(), y64.double()
    e, e32 = float((got - y64).norm()), float((y32 - y64).norm())
    assert e <= 2 * e32 + tiny, '%s: ||y - y64|| = %.3e > 2 ||y32 - y64|| = %.3e' % (what, e, 2 * e32)


# (N, C, H, W, K, (R, S), stride, pad): the nine geometry classes of the feature path, the C = 3 stem, ragged K (80, 48, 448, 320),
# ragged and non-square pixel counts, batch 1 and 7
GEOMETRIES = [
    (7, 192, 35, 35, 80, (1, 1), 1, (0, 0)),
    (1, 288, 35, 35, 48, (1, 1), 1, (0, 0)),
    (7, 1280, 8, 8, 448, (1, 1), 1, (0, 0)),
    (1, 128, 17, 13, 128, (1, 7), 1, (0, 3)),
    (7, 160, 17, 17, 192, (7, 1), 1, (3, 0)),
    (1, 64, 35, 35, 96, (3, 3), 1, (1, 1)),
    (7, 288, 35, 35, 384, (3, 3), 2, (0, 0)),
    (1, 192, 17, 17, 320, (3, 3), 2, (0, 0)),
    (7, 32, 37, 33, 32, (3, 3), 1, (0, 0)),
    (7, 3, 75, 75, 32, (3, 3), 2, (0, 0)),
    (1, 384, 8, 8, 384, (1, 3), 1, (0, 1)),
    (7, 384, 8, 8, 384, (3, 1), 1, (1, 0)),
    (7, 48, 35, 35, 64, (5, 5), 1, (2, 2)),
]


def _ids(g):
    return 'N%d_C%d_%dx%d_K%d_%dx%d_s%d_p%d%d' % (g[0], g[1], g[2], g[3], g[4], g[5][0], g[5][1], g[6], g[7][0], g[7][1])


@pytest.mark.parametrize('geo', GEOMETRIES, ids=[_ids(g) for g in GEOMETRIES])
def test_conv_per_geometry_class(dev, geo):
    from pcgan_amd.hip import inception as I
    N, C, H, W, K, (r, s), stride, pad = geo
    g = torch.Generator().manual_seed(sum(geo[:5]))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, r, s, generator=g) / (C * r * s) ** 0.5
    packed = I.iconv_pack(w.to(dev))
    got = I.iconv_fwd(x.to(dev), packed, K, r, s, stride, pad, relu=False)
    torch.cuda.synchronize()
    y64 = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    y32 = F.conv2d(x, w, stride=stride, padding=pad)
    assert got.shape == y64.shape
    _rule(got, y32, y64, 'conv %s' % (geo,))


def test_conv_writes_its_channel_slice_only(dev):
    """a conv into [k_off, k_off + K) of a sentinel-filled output: the slice equals the standalone result bit for bit, every other
    element is bit-unchanged (ragged K and pixel count)"""
    from pcgan_amd.hip import inception as I
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 40, 17, 17, generator=g).to(dev)
    w = (torch.randn(80, 40, 7, 1, generator=g) * 0.1).to(dev)
    packed = I.iconv_pack(w)
    alone = I.iconv_fwd(x, packed, 80, 7, 1, 1, (3, 0))
    for k_off, k_total in ((0, 80 + 17), (23, 23 + 80), (5, 200)):
        out = torch.full((3, k_total, 17, 17), SENTINEL, device=dev)
        I.iconv_fwd(x, packed, 80, 7, 1, 1, (3, 0), out=out, k_off=k_off)
        torch.cuda.synchronize()
        assert torch.equal(out[:, k_off:k_off + 80], alone)
        rest = torch.cat([out[:, :k_off].flatten(), out[:, k_off + 80:].flatten()])
        assert bool((rest == SENTINEL).all()), 'iconv wrote outside its slice (k_off %d, K_total %d)' % (k_off, k_total)


def test_maxpool_slice_is_exact_and_stays_in_its_slice(dev):
    from pcgan_amd.hip import inception as I
    g = torch.Generator().manual_seed(4)
    x = torch.randn(5, 36, 35, 33, generator=g).to(dev)
    out = torch.full((5, 100, 17, 16), SENTINEL, device=dev)
    I.maxpool_slice(x, 3, 2, out=out, k_off=50)
    alone = I.maxpool_slice(x, 3, 2)
    torch.cuda.synchronize()
    want = F.max_pool2d(x.cpu(), 3, 2)
    assert torch.equal(out[:, 50:86].cpu(), want) and torch.equal(alone.cpu(), want)
    assert bool((out[:, :50] == SENTINEL).all()) and bool((out[:, 86:] == SENTINEL).all())


def _bn(K, g):
    return (0.6 + 0.8 * torch.rand(K, generator=g), 0.4 * torch.rand(K, generator=g) - 0.2,
            0.4 * torch.rand(K, generator=g) - 0.2, 0.5 + torch.rand(K, generator=g))


def _bn_ref(y, bn):
    gamma, beta, mean, var = (t.to(y.dtype) for t in bn)
    return F.relu(F.batch_norm(y, mean, var, gamma, beta, False, 0.0, 1e-3))


@pytest.mark.parametrize('pool', [False, True], ids=['conv', 'pool_branch'])
def test_folded_batchnorm_relu(dev, pool):
    """BasicConv2d = conv -> eval BatchNorm(eps 1e-3) -> ReLU with non-trivial gamma, beta, mean, var, folded by pcgan_iconv_pack; the
    pool branch: avg_pool2d(3, 1, 1) -> 1x1 BasicConv2d as the expanded 3x3 conv"""
    from pcgan_amd.hip import inception as I
    g = torch.Generator().manual_seed(5 + pool)
    N, C, H, K = 4, 96, 17, 112
    x = torch.randn(N, C, H, H, generator=g).relu()
    if pool:
        w = torch.randn(K, C, 1, 1, generator=g) / C ** 0.5
    else:
        w = torch.randn(K, C, 3, 3, generator=g) / (9 * C) ** 0.5
    bn = _bn(K, g)
    packed = I.iconv_pack(w.to(dev), tuple(t.to(dev) for t in bn), eps=1e-3, pool_expand=pool)
    got = I.iconv_fwd(x.to(dev), packed, K, 3, 3, 1, (1, 1), relu=True)
    torch.cuda.synchronize()

    def ref(dt):
        xx, ww = x.to(dt), w.to(dt)
        y = F.conv2d(F.avg_pool2d(xx, 3, 1, 1), ww) if pool else F.conv2d(xx, ww, padding=1)
        return _bn_ref(y, bn)
    _rule(got, ref(torch.float32), ref(torch.float64), 'BasicConv2d (pool %s)' % pool)


@pytest.mark.parametrize('hw', [(32, 32), (128, 128), (224, 224), (299, 299), (300, 300), (512, 512), (97, 160)])
def test_input_prep_matches_interpolate_and_normalize(dev, hw):
    from pcgan_amd.models.inception import InceptionV3
    g = torch.Generator().manual_seed(hw[0] * 1000 + hw[1])
    x = torch.rand(2, 3, hw[0], hw[1], generator=g)
    net = InceptionV3([3])
    got = net.prepare(x.to(dev))
    torch.cuda.synchronize()
    want = R.prepare_input(x)
    assert got.shape == (2, 3, 299, 299)
    err = float((got.cpu() - want).abs().max())
    assert err <= 1e-6, 'prep %s: max |diff| %.3e' % (hw, err)
    # normalisation alone (resize off): the affine of the reference, bit for bit
    net = InceptionV3([3], resize_input=False)
    assert torch.equal(net.prepare(x.to(dev)).cpu(), R.prepare_input(x, resize_input=False))


@pytest.fixture(scope='module')
def oracle():
    sd = R.random_state_dict(11)
    return sd, R.make_ref(sd, dtype=torch.float32), R.make_ref(sd, dtype=torch.float64)


def test_whole_network_blocks_against_the_float64_oracle(dev, oracle):
    from pcgan_amd.models.inception import InceptionV3
    sd, ref32, ref64 = oracle
    x = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(12))
    net = InceptionV3([0, 1, 2, 3], weights=sd)
    got = net(x.to(dev))
    torch.cuda.synchronize()
    y32 = R.forward_ref(ref32, x, (0, 1, 2, 3))
    y64 = R.forward_ref(ref64, x.double(), (0, 1, 2, 3))
    assert [tuple(t.shape) for t in got] == [(4, 64, 73, 73), (4, 192, 35, 35), (4, 768, 17, 17), (4, 2048, 1, 1)]
    for i in range(4):
        _rule(got[i], y32[i], y64[i], 'block %d' % i)
    # a single-block model computes the same block bits
    only = InceptionV3([2], weights=sd)(x.to(dev))
    torch.cuda.synchronize()
    assert len(only) == 1 and torch.equal(only[0], got[2])


def test_model_refusals_on_the_device(dev, oracle):
    from pcgan_amd.models.inception import InceptionV3
    net = InceptionV3([3], weights=oracle[0])
    with pytest.raises(RuntimeError, match='float32'):
        net(torch.rand(1, 3, 32, 32, device=dev).to(torch.bfloat16))
    with pytest.raises(RuntimeError, match='forward-only'):
        net(torch.rand(1, 3, 32, 32, device=dev).requires_grad_())


def test_forward_is_bit_identical_beside_training_kernels(dev, oracle):
    """one forward while the training step's convolutions (residual-block forward, data and weight gradients) run on another
    stream: the features are bit-identical to the same forward alone"""
    from pcgan_amd.hip import ops
    from pcgan_amd.models.inception import InceptionV3
    net = InceptionV3([0, 1, 2, 3], weights=oracle[0])
    x = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(13)).to(dev)
    g = torch.Generator().manual_seed(14)
    xr = torch.randn(32, 256, 32, 32, generator=g).to(dev)
    wr = (torch.randn(256, 256, 3, 3, generator=g) * 0.05).to(dev)
    we = (torch.randn(128, 128, 3, 3, generator=g) * 0.05).to(dev)
    de = torch.randn(32, 128, 28, 28, generator=g).to(dev)
    cr, ce = {}, {}

    def company():
        for _ in range(4):
            ops.conv2d_fwd(xr, wr, None, 1, 1, 1, pack_cache=cr)
            ops.conv2d_bwd_data(de, we, (28, 28), 1, 1, 0, pack_cache=ce)
            ops.conv2d_bwd_weight(xr, xr, (256, 256, 3, 3), 1, 1, 1)
    company()
    alone = [t.clone() for t in net(x)]
    torch.cuda.synchronize()
    other = torch.cuda.Stream()
    for _ in range(3):
        other.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(other):
            company()
        got = net(x)
        torch.cuda.synchronize()
        for a, b in zip(alone, got):
            assert torch.equal(a, b), 'Inception features changed beside the training kernels'


def _write_sets(root, n=80):
    from PIL import Image
    rng = np.random.default_rng(21)
    for name, lo in (('a', 0), ('b', 80)):
        os.makedirs(root / name)
        for i in range(n):
            Image.fromarray(rng.integers(lo, lo + 176, (32, 32, 3), dtype=np.uint8)).save(root / name / ('%03d.png' % i))


def _run_script(args):
    cmd = [sys.executable, os.path.join(ROOT, 'compute_fid_score.py')] + [str(a) for a in args]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return float(re.search(r': ([-0-9.e]+)\s*$', p.stdout.strip()).group(1))


def test_compute_fid_score_inception_end_to_end(dev, tmp_path, oracle):
    """compute_fid_score.py --features inception on two PNG directories (80 images of 32 x 32 each) with a torchvision-layout .pth
    written here: a set against itself ~ 0, against the other positive, .npz statistics reproduce the value; at --dims 64 the features
    meet the block rule against the oracle's and the FID matches the oracle's to 1e-4 relative.  At 2048 dims and 80 images the
    covariance is singular: only same ~ 0 and different > 0 are checked."""
    sys.path.insert(0, ROOT)
    import compute_fid_score as S
    from pcgan_amd.util.fid import activation_statistics, frechet_distance, get_activations
    sd, ref32, ref64 = oracle
    torch.save(sd, tmp_path / 'inception_v3.pth')
    _write_sets(tmp_path)
    a, b = tmp_path / 'a', tmp_path / 'b'
    common = ['--features', 'inception', '--inception_weights', tmp_path / 'inception_v3.pth', '--batch-size', '20']
    for dims in (64, 2048):
        same = _run_script([a, a, '--dims', dims] + common)
        diff = _run_script([a, b, '--dims', dims] + common)
        assert abs(same) < 1e-3 * abs(diff) and diff > 0, (dims, same, diff)
        if dims != 64:
            continue
        imgs = {k: torch.from_numpy(S.load_images(S.list_images(str(p), ''))) for k, p in (('a', a), ('b', b))}
        model = S.inception_features(str(tmp_path / 'inception_v3.pth'), dev, 64)
        feats = {k: get_activations(v, model, 20) for k, v in imgs.items()}
        for k, v in imgs.items():
            f32 = torch.cat([R.forward_ref(ref32, v[i:i + 20], (0,))[0].mean(dim=(2, 3)) for i in range(0, 80, 20)])
            f64 = torch.cat([R.forward_ref(ref64, v[i:i + 20].double(), (0,))[0].mean(dim=(2, 3)) for i in range(0, 80, 20)])
            _rule(torch.from_numpy(feats[k]), f32, f64, 'dims 64 features of set %s' % k)
            if k == 'a':
                oracle_a = f64.numpy()
            else:
                oracle_b = f64.numpy()
        ours = frechet_distance(*activation_statistics(feats['a']), *activation_statistics(feats['b']))
        want = frechet_distance(*activation_statistics(oracle_a), *activation_statistics(oracle_b))
        assert abs(ours - want) <= 1e-4 * abs(want), (ours, want)
        assert abs(diff - ours) <= 1e-6 + 1e-5 * abs(ours), (diff, ours)     # the script's value (printed to 6 decimals)
        # the .npz statistics path reproduces the value
        for k in ('a', 'b'):
            mu, sigma = activation_statistics(feats[k])
            np.savez(tmp_path / ('%s.npz' % k), mu=mu, sigma=sigma)
        from_npz = _run_script([tmp_path / 'a.npz', tmp_path / 'b.npz'])
        assert abs(from_npz - ours) <= 1e-6 + 1e-5 * abs(ours), (from_npz, ours)
