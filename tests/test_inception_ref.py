"""CPU: the Inception-v3 oracle (tests/inception_ref.py) against torchvision's published architecture figures, the HIP model's
architecture table against the oracle, the pool-branch identity the kernels rely on, and every refusal that must happen before any
device use (the weights loader, compute_fid_score.py without weights, the C-ABI's argument checks)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import inception_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parameter_count_matches_torchvision_inception_v3():
    net = R.Inception3Ref()
    sd = net.state_dict()
    assert sum(p.numel() for p in net.parameters()) == 27161264      # torchvision's published count for inception_v3
    assert len(sd) == 580
    feat = sum(p.numel() for k, p in net.named_parameters() if not k.startswith(('AuxLogits.', 'fc.')))
    assert feat == 21785568


def test_block_output_shapes_at_299():
    net = R.make_ref(seed=0)
    out = R.forward_ref(net, torch.rand(1, 3, 299, 299), output_blocks=(0, 1, 2, 3), resize_input=False)
    assert [tuple(o.shape[1:]) for o in out] == [(64, 73, 73), (192, 35, 35), (768, 17, 17), (2048, 1, 1)]


def test_model_architecture_table_matches_the_oracle():
    """pcgan_amd.models.inception's conv table: the same keys and shapes as the oracle's feature path, 94 convolutions in the
    issue's geometry classes"""
    from pcgan_amd.models import inception as M
    sd = R.Inception3Ref().state_dict()
    want = {k: tuple(v.shape) for k, v in sd.items()
            if not k.startswith(('AuxLogits.', 'fc.')) and not k.endswith('num_batches_tracked')}
    assert M.expected_shapes() == want
    convs = M.feature_convs()
    assert len(convs) == 94
    classes = {}
    for name, _, _, ks, stride, pad in convs:
        classes[(ks, stride, pad)] = classes.get((ks, stride, pad), 0) + 1
    assert classes == {((1, 1), 1, (0, 0)): 40, ((1, 7), 1, (0, 3)): 13, ((7, 1), 1, (3, 0)): 13, ((3, 3), 1, (1, 1)): 10,
                       ((3, 3), 2, (0, 0)): 5, ((3, 3), 1, (0, 0)): 2, ((1, 3), 1, (0, 1)): 4, ((3, 1), 1, (1, 0)): 4,
                       ((5, 5), 1, (2, 2)): 3}
    # 5.71 GMAC per image at 299 x 299 (the two stem pools included in the sizes)
    macs, h = 0, {}
    x = torch.zeros(1, 3, 299, 299)
    net = R.Inception3Ref().eval()

    def hook(m, i, o):
        h[m] = o.shape

    hooks = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        R.forward_ref(net, x, output_blocks=(3,), resize_input=False, normalize_input=False)
    for m, shape in h.items():
        macs += shape[1] * shape[2] * shape[3] * m.in_channels * m.kernel_size[0] * m.kernel_size[1]
    for hk in hooks:
        hk.remove()
    assert abs(macs / 1e9 - 5.71) < 0.01


def test_pool_branch_is_a_3x3_conv_with_taps_over_nine():
    """avg_pool2d(3, 1, 1, count_include_pad=True) then a 1x1 conv == the 3x3 pad-1 conv with every tap w / 9 (float64): what
    pcgan_iconv_pack's pool_expand writes"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 24, 11, 9, generator=g, dtype=torch.float64)
    w = torch.randn(16, 24, 1, 1, generator=g, dtype=torch.float64)
    a = F.conv2d(F.avg_pool2d(x, 3, 1, 1), w)
    b = F.conv2d(x, w.expand(16, 24, 3, 3) / 9.0, padding=1)
    assert torch.allclose(a, b, rtol=0, atol=1e-13)


def _sd():
    return R.random_state_dict(1)


@pytest.mark.parametrize('case', ['missing', 'shape', 'fid1008', 'unknown'])
def test_loader_refusals_before_any_device_use(case, tmp_path):
    from pcgan_amd.models.inception import InceptionV3
    sd = _sd()
    if case == 'missing':
        del sd['Mixed_6c.branch7x7dbl_3.bn.running_var']
        err, msg = KeyError, 'missing'
    elif case == 'shape':
        sd['Mixed_7b.branch3x3_2a.conv.weight'] = torch.zeros(384, 384, 3, 1)
        err, msg = ValueError, 'shape'
    elif case == 'fid1008':
        sd['fc.weight'] = torch.zeros(1008, 2048)
        sd['fc.bias'] = torch.zeros(1008)
        err, msg = ValueError, 'pytorch-fid'
    else:
        sd['Mixed_5b.branch9x9.conv.weight'] = torch.zeros(1)
        err, msg = KeyError, 'unexpected'
    with pytest.raises(err, match=msg):
        InceptionV3([3], weights=sd, gpu_ids=[0])
    path = tmp_path / 'w.pth'
    torch.save(sd, path)
    with pytest.raises(err, match=msg):
        InceptionV3([3], weights=str(path), gpu_ids=[0])


def test_model_refuses_grad_inputs_and_runs_nowhere_without_weights():
    from pcgan_amd.models.inception import InceptionV3
    net = InceptionV3([3])
    with pytest.raises(RuntimeError, match='forward-only'):
        net(torch.rand(1, 3, 32, 32, requires_grad=True))
    with pytest.raises(RuntimeError, match='no weights'):
        net(torch.rand(1, 3, 32, 32))
    with pytest.raises(ValueError):
        InceptionV3([3], gpu_ids=[])


def test_fid_script_refuses_inception_without_weights_and_fid_weights(tmp_path):
    base = [sys.executable, os.path.join(ROOT, 'compute_fid_score.py'), str(tmp_path), str(tmp_path)]
    p = subprocess.run(base + ['--features', 'inception'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and '--inception_weights' in p.stderr and 'random weights' in p.stderr
    sd = _sd()
    sd['fc.weight'] = torch.zeros(1008, 2048)
    torch.save(sd, tmp_path / 'fid.pth')
    p = subprocess.run(base + ['--features', 'inception', '--inception_weights', str(tmp_path / 'fid.pth')], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and 'pytorch-fid' in p.stderr
    p = subprocess.run(base + ['--features', 'inception', '--dims', '100', '--inception_weights', 'x'], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and '--dims' in p.stderr


def test_c_abi_refuses_bf16_and_unsupported_geometry():
    """argument checks of the Inception entry points run before any launch (no GPU needed)"""
    from pcgan_amd.hip import lib
    from pcgan_amd.hip.inception import iconv_desc
    h = lib.load()
    d = iconv_desc((2, 288, 35, 35), 384, 3, 3, 2, 0, 0)
    assert h.pcgan_iconv_supported(ctypes.byref(d)) == 1
    assert h.pcgan_iconv_packed_bytes(ctypes.byref(d)) == (384 + 2592 * 384) * 4      # bias + W^T[CRS rounded to 16][K rounded to 64]
    d3 = iconv_desc((1, 3, 299, 299), 32, 3, 3, 2, 0, 0)
    assert h.pcgan_iconv_packed_bytes(ctypes.byref(d3)) == (64 + 32 * 64) * 4
    bad = iconv_desc((2, 288, 35, 35), 384, 3, 3, 2, 0, 0)
    bad.dtype = lib.BF16
    assert h.pcgan_iconv_supported(ctypes.byref(bad)) == 0 and b'bf16' in h.pcgan_last_error()
    assert h.pcgan_iconv_fwd(ctypes.byref(bad), None, None, None, 1, None) != 0 and b'bf16' in h.pcgan_last_error()
    assert h.pcgan_iconv_packed_bytes(ctypes.byref(bad)) == 0
    for args, what in ((((1, 8, 9, 9), 4, 3, 3, 3, 0, 0), b'stride'), (((1, 8, 9, 9), 4, 9, 9, 1, 4, 4), b'kernel'),
                       (((1, 8, 9, 9), 4, 3, 3, 1, 3, 1), b'padding')):
        g = iconv_desc(*args)
        assert h.pcgan_iconv_supported(ctypes.byref(g)) == 0 and what in h.pcgan_last_error(), (args, h.pcgan_last_error())
    g = iconv_desc((1, 8, 9, 9), 4, 1, 7, 1, 0, 3, k_off=6, K_total=8)        # slice [6, 10) of 8 channels
    assert h.pcgan_iconv_supported(ctypes.byref(g)) == 0 and b'slice' in h.pcgan_last_error()
    g = iconv_desc((1, 8, 9, 9), 4, 1, 7, 1, 0, 3)
    g.Q = 8
    assert h.pcgan_iconv_supported(ctypes.byref(g)) == 0 and b'output dims' in h.pcgan_last_error()
    assert h.pcgan_maxpool_slice_fwd(None, None, 1, 4, 9, 9, 3, 2, 4, 4, 0, 4, lib.BF16, None) != 0 and b'fp32' in h.pcgan_last_error()
    assert h.pcgan_maxpool_slice_fwd(None, None, 1, 4, 9, 9, 3, 2, 4, 4, 2, 4, lib.F32, None) != 0
    assert h.pcgan_inception_prep(None, None, 1, 3, 8, 8, 299, 299, None, None, lib.BF16, None) != 0 and b'fp32' in h.pcgan_last_error()
