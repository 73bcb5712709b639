"""CPU side of `siamese.py --mode attention`: the options, the layer-name resolution of util/gradcam.py, the wrappers' refusal of CPU
tensors, the argument validation of the two entry points of csrc/gradcam.hip (before any launch, so without a GPU) and the float64
restatement's two forms of the weighted maps."""
import ctypes

import numpy as np
import pytest
import torch

import gradcam_ref as R
from oracle import weights as W


def test_attention_mode_parses_with_the_reference_defaults():
    import siamese
    opt = siamese.build_parser().parse_args(['--dataroot', 'synthetic', '--mode', 'attention'])
    assert opt.mode == 'attention' and callable(siamese.attention)
    assert opt.gcam_layer == 'base.model.layer1.0.conv1' and opt.gcam_save is False and opt.gcam_type == 'raw'
    assert opt.gcam_alpha == 0.01 and opt.gcam_dir == 'results_attn'
    assert '--gcam_save' in siamese.build_parser().format_help()        # argparse %-formats every help string
    for kind in ('raw', 'pw', 'pw_cw', 'cw_pos', 'input'):
        assert siamese.build_parser().parse_args(['--dataroot', 'x', '--gcam_type', kind, '--gcam_save']).gcam_save is True
    with pytest.raises(SystemExit):
        siamese.build_parser().parse_args(['--dataroot', 'x', '--gcam_type', 'guided'])
    assert siamese.GCAM_MEAN == (0.4914, 0.4822, 0.4465) and siamese.GCAM_STD == (0.2023, 0.1994, 0.2010)


@pytest.fixture(scope='module')
def net():
    from pcgan_amd.models import networks
    return networks.SiameseFeature(networks.ResNetFeature(3, 'resnet18'), pooling='avg', cnn_dim=[8, 1], cnn_pad=1, cnn_relu_slope=0.7)


def test_layer_names_resolve(net):
    from pcgan_amd.util.gradcam import GradCAM, resolve_layer
    mods = dict(net.named_modules())
    assert resolve_layer(net, 'base.model.layer1.0.conv1') == ('base.model.layer1.0.conv1', mods['base.model.layer1.0.conv1'])
    assert resolve_layer(net, 'base.model.maxpool')[1] is mods['base.model.maxpool']
    assert resolve_layer(net, 'base.model.layer2.1')[1] is mods['base.model.layer2.1']
    # a stage resolves to its last block, the head to its last convolution, a downsample to its last child
    assert resolve_layer(net, 'base.model.layer4') == ('base.model.layer4.1', mods['base.model.layer4.1'])
    assert resolve_layer(net, 'cnn') == ('cnn.4', mods['cnn.4']) and isinstance(mods['cnn.4'], torch.nn.Conv2d)
    assert resolve_layer(net, 'base.model.layer2.0.downsample')[0] == 'base.model.layer2.0.downsample.1'
    g = GradCAM(net, 'base.model.layer3')
    assert g.resolved == 'base.model.layer3.1' and g.module is mods['base.model.layer3.1']


@pytest.mark.parametrize('name', ['base.model.bn1', 'base.model.layer1.0.bn2', 'base.model.relu', 'base.model.layer1.0.relu',
                                  'base.model.layer1.0.drop1', 'base', 'base.model', 'cnn.1'])
def test_layers_without_a_tensor_of_their_own_are_refused(net, name):
    from pcgan_amd.util.gradcam import resolve_layer
    with pytest.raises(ValueError) as e:
        resolve_layer(net, name)
    assert name in str(e.value) and 'a convolution, base.model.maxpool, a residual block' in str(e.value)


@pytest.mark.parametrize('name', ['base.model.layer9', 'features.3', ''])
def test_missing_layer_is_quoted(net, name):
    from pcgan_amd.util.gradcam import GradCAM
    with pytest.raises(ValueError) as e:
        GradCAM(net, name)
    assert str(e.value) == 'invalid layers: %s' % name


def test_wrappers_refuse_cpu_tensors():
    from pcgan_amd.hip import ops
    A = torch.zeros(1, 2, 3, 3)
    for kind in R.MAP_TYPES:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            ops.gradcam_map(A, A, kind)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.heatmap_overlay(torch.zeros(1, 1, 3, 3), torch.zeros(1, 3, 3, 3), (0., 0., 0.), (1., 1., 1.), 0.5)
    with pytest.raises(RuntimeError, match='gradcam_map type'):
        ops.gradcam_map(A, A, 'guided')


def test_arguments_are_validated_before_any_launch():
    from pcgan_amd.hip import lib
    h = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    raw, pw = lib.GCAM_TYPES['raw'], lib.GCAM_TYPES['pw']

    def err():
        return h.pcgan_last_error()

    assert h.pcgan_gradcam_map(p, p, p, 1, 0, 2, 2, raw, lib.F32, None) != 0 and b'gradcam_map' in err() and b'C = 0' in err()
    assert h.pcgan_gradcam_map(None, p, p, 1, 2, 2, 2, raw, lib.F32, None) != 0 and b'null pointer (act' in err()
    assert h.pcgan_gradcam_map(p, p, None, 1, 2, 2, 2, raw, lib.F32, None) != 0 and b'null pointer (act or map)' in err()
    for kind in ('pw', 'cw_pos', 'pw_cw'):
        assert h.pcgan_gradcam_map(p, None, p, 1, 2, 2, 2, lib.GCAM_TYPES[kind], lib.F32, None) != 0 and b'null pointer (grad)' in err()
    assert h.pcgan_gradcam_map(p, p, p, 1, 2, 2, 2, 7, lib.F32, None) != 0 and b'unknown map type 7' in err()
    assert h.pcgan_gradcam_map(p, p, p, 1, 2, 2, 2, pw, 5, None) != 0 and b'dtype' in err()
    assert h.pcgan_gradcam_map(p, p, p, 1, 4097, 2, 2, lib.GCAM_TYPES['cw_pos'], lib.F32, None) != 0 and b'4096' in err()
    assert h.pcgan_gradcam_map(p, p, p, 1 << 20, 1 << 10, 2, 2, pw, lib.F32, None) != 0 and b'overflow' in err()
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert h.pcgan_heatmap_overlay(p, p, f3, f3, 0.5, p, p, 1, 2, 2, 2, lib.F32, None) != 0 and b'1 or 3' in err()
    assert h.pcgan_heatmap_overlay(None, p, f3, f3, 0.5, p, p, 1, 1, 2, 2, lib.F32, None) != 0 and b'null pointer' in err()
    assert h.pcgan_heatmap_overlay(p, p, f3, f3, 0.5, p, None, 1, 1, 2, 2, lib.F32, None) != 0 and b'null pointer' in err()
    assert h.pcgan_heatmap_overlay(p, p, None, f3, 0.5, p, p, 1, 1, 2, 2, lib.F32, None) != 0 and b'mean or std' in err()
    assert h.pcgan_heatmap_overlay(p, p, f3, f3, 0.5, p, p, 1, 1, 0, 2, lib.F32, None) != 0 and b'positive' in err()
    assert h.pcgan_heatmap_overlay(p, p, f3, f3, 0.5, p, p, 1, 3, 2, 2, 9, None) != 0 and b'dtype' in err()


@pytest.mark.parametrize('kind', ['cw_pos', 'pw_cw'])
def test_grouped_conv3d_form_is_the_channel_sum(kind):
    A, g = W.seeded_normal((3, 5, 4, 6), 1), W.seeded_normal((3, 5, 4, 6), 2)
    plain, _ = R.gradcam_map(A, g, kind)
    assert plain.shape == (3, 1, 4, 6)
    np.testing.assert_allclose(R.gradcam_map_conv3d(A, g, kind), plain, rtol=1e-13, atol=1e-15)


def test_restatement_rules():
    A = -torch.ones(1, 3, 2, 2)
    assert (R.gradcam_map(A, None, 'raw')[0] == 3.0).all()                                  # abs of a negative channel sum
    assert (R.gradcam_map(A, -A.abs(), 'cw_pos')[0] == 0.0).all()                           # no positive gradient: every weight is 0
    out, lohi, pix = R.overlay(torch.full((1, 1, 2, 2), 4.0), torch.zeros(1, 3, 2, 2), (0.5, 0.5, 0.5), (1., 1., 1.), 0.25)
    assert (lohi == 4.0).all() and np.array_equal(out, pix * 0.25)                           # hi == lo: the heat term is 0
    out, lohi, _ = R.overlay(torch.tensor([0., 1., 2., 4.]).view(1, 1, 2, 2), torch.zeros(1, 3, 2, 2), (0., 0., 0.), (1., 1., 1.), 0.0)
    assert list(lohi[0]) == [0.0, 4.0] and np.array_equal(out[0, 2].ravel(), np.array([0., 63.75, 127.5, 255.]))
