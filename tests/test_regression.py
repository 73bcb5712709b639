"""CPU: the attribute regressor's oracle side and host logic.

* tests/regression_ref.py (twin + restated training step) reproduces tests/golden/regression_step.npz, which was captured from the
  reference's own networks.RegressionNetwork / MSELoss / Adam (scripts/make_regression_golden.py).  The twin runs in float32 like the
  reference; its loss is written out instead of calling MSELoss and its reductions may split differently over threads, so the bounds
  are the project's (tests/test_classification.py): outputs 1e-4 of the largest element, gradients on their own ReLU /
  max-pool decisions 3e-2 relative L2.  Adam is sign-like at step 1, so the restated update is pinned separately and sharply: fed the
  fixture's own gradients it must give the fixture's parameters to one fp32 rounding.
* argument validation of pcgan_pool_mse_fwd happens before any launch, so it runs without a GPU.
* regression.py: every reference option with its default, labels from file names, the seeded initialisation, and what the build
  refuses.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import regression_ref as R
from oracle import weights as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'regression_step.npz')
OUT_TOL, GRAD_L2 = 1e-4, 3e-2
CASES = ['resnet18', 'alexnet']


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _close(got, want, what, tol=OUT_TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, '%s: shape %s vs %s' % (what, got.shape, want.shape)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    assert err <= tol * scale + 1e-12, '%s: %.3e > %.1e * %.3e' % (what, err, tol, scale)


def _rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    return float(np.sqrt(((got - want) ** 2).sum()) / (np.sqrt((want ** 2).sum()) + 1e-300))


def _twin(gold, which):
    cnn_dim = [int(v) for v in gold['cnn_dim']]
    return R.RegressionNetworkRef(R.base_ref(which), str(gold['%s/pooling' % which]), cnn_dim, 1, 0.7)


def _check_gradients(gold, prefix, named, stride):
    """every tensor: l2 norm and abs-sum against the recorded statistics; the head's last layer in full and a strided sample of the rest
    in relative L2"""
    wmax = max(float(gold['%s/stat/%s' % (prefix, k)][2]) for k in named)
    for k, t in named.items():
        a = t.detach().numpy().astype(np.float64)
        stat = gold['%s/stat/%s' % (prefix, k)]
        if stat[2] < 1e-5 * wmax:
            # the bias of a convolution that a BatchNorm follows: its true gradient is 0, both sides hold fp32 noise (test_gpu_nets._compare)
            assert np.sqrt((a * a).sum()) < 1e-3 * wmax, '%s %s should be ~0' % (prefix, k)
            continue
        assert abs(np.abs(a).sum() - stat[1]) <= GRAD_L2 * stat[1], '%s %s: abs-sum' % (prefix, k)
        assert abs(np.sqrt((a * a).sum()) - stat[2]) <= GRAD_L2 * stat[2], '%s %s: l2' % (prefix, k)
        full = '%s/full/%s' % (prefix, k)
        want = gold[full] if full in gold.files else gold['%s/samp/%s' % (prefix, k)]
        got = a if full in gold.files else a.reshape(-1)[::stride]
        if want.size >= 16:        # a sample of a few elements says nothing in relative L2: the statistics above cover those tensors
            assert _rel_l2(got, want) <= GRAD_L2, '%s %s: relative L2 %.3e' % (prefix, k, _rel_l2(got, want))


@pytest.mark.parametrize('which', CASES)
def test_twin_and_restated_step_reproduce_the_reference(gold, which):
    size, seed = (int(v) for v in gold['%s/case' % which])
    target = torch.from_numpy(gold['%s/target' % which])
    net = _twin(gold, which)
    assert list(net.state_dict().keys()) == [str(k) for k in gold['%s/keys' % which]]
    net.load_state_dict(W.fill_state_dict(net.state_dict(), seed), strict=True)
    x = W.seeded_tensor((len(target), 3, size, size), 100 + seed)
    pred, loss, grads, after = R.train_step(net, x, target, lr=float(gold['lr']))
    assert tuple(pred.shape) == (len(target), 1, 1, 1)
    _close(pred, gold['%s/out' % which], 'output')
    _close(loss, gold['%s/loss' % which], 'loss')
    delta = float(gold['delta'])
    want_flags = gold['%s/within' % which]
    assert 0 < int(want_flags.sum()) < len(target), 'the fixture has predictions inside and outside delta'
    assert R.within(pred, target.view_as(pred), delta).tolist() == want_flags.tolist()
    stride = int(gold['stride'])
    _check_gradients(gold, which + '/dparam', grads, stride)
    # the restated Adam against the reference's optimizer.step(), element by element: the fixture's own gradient in, its parameter out
    before = net.state_dict()
    for k in grads:
        for kind in ('full', 'samp'):
            key = '%s/dparam/%s/%s' % (which, kind, k)
            if key not in gold.files:
                continue
            g = torch.from_numpy(gold[key])
            p0 = before[k].detach() if kind == 'full' else before[k].detach().reshape(-1)[::stride]
            want = gold['%s/param_after/%s/%s' % (which, kind, k)]
            got = R.adam_update(p0, g, lr=float(gold['lr'])).numpy()
            assert np.abs(got - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max()), 'Adam step of %s' % k
    assert set(after) == set(grads)
    for k, b in net.named_buffers():
        want = gold['%s/buf/%s' % (which, k)]
        if 'running' in k:
            a = b.double().numpy()
            assert abs(a.sum() - want[0]) <= OUT_TOL * want[1] and abs(np.abs(a).sum() - want[1]) <= OUT_TOL * want[1], k
        else:
            assert int(b) == int(want) == 1, k


@pytest.mark.parametrize('which', CASES)
def test_state_dict_keys_are_the_references(gold, which):
    from pcgan_amd.models import networks
    want = [str(k) for k in gold['%s/keys' % which]]
    cnn_dim = [int(v) for v in gold['cnn_dim']]
    pooling = str(gold['%s/pooling' % which])
    base = networks.AlexNetFeature(3, pooling='') if which == 'alexnet' else networks.ResNetFeature(3, which)
    net = networks.RegressionNetwork(base, pooling=pooling, cnn_dim=cnn_dim, cnn_pad=1, cnn_relu_slope=0.7)
    assert list(net.state_dict().keys()) == want and net.feature_dim == 1
    assert all(k.startswith('base.') or k.startswith('cnn.') for k in want) and want[-1] == 'cnn.3.bias'
    ar = networks.define_AR(which, cnn_dim=cnn_dim)
    assert isinstance(ar, networks.RegressionNetwork) and list(ar.state_dict().keys()) == want and ar.pooling == 'max'
    ar.load_state_dict(_twin(gold, which).state_dict(), strict=True)
    # without a conv head the trunk's channels are the features
    bare = networks.define_AR(which)
    assert bare.cnn is None and bare.feature_dim == (256 if which == 'alexnet' else 512)
    assert all(k.startswith('base.') for k in bare.state_dict())


def test_define_ar_defaults_and_refusals():
    import inspect
    from pcgan_amd.models import networks
    sig = inspect.signature(networks.define_AR)
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
        input_nc=3, init_type='kaiming', pooling='max', cnn_dim=[], cnn_pad=1, cnn_relu_slope=0.2, gpu_ids=[])
    sig = inspect.signature(networks.RegressionNetwork.__init__)
    assert [k for k in sig.parameters][1:] == ['base', 'pooling', 'cnn_dim', 'cnn_pad', 'cnn_relu_slope']
    assert sig.parameters['pooling'].default == 'avg' and sig.parameters['cnn_relu_slope'].default == 0.2
    for which in ('vgg16', 'DTN', 'resnet101'):
        with pytest.raises(NotImplementedError, match=which):
            networks.define_AR(which)
    assert networks.define_AR('resnet50').feature_dim == 2048


def test_load_pretrained_loads_the_trunk_only():
    from pcgan_amd.models import networks
    net = networks.define_AR('resnet18', cnn_dim=[8, 1])
    donor = R.ResNetTrunkRef('resnet18').model
    sd = W.fill_state_dict(donor.state_dict(), 3)
    head = {k: v.detach().clone() for k, v in net.cnn.state_dict().items()}
    net.load_pretrained(dict(sd))
    assert torch.equal(net.base.model.conv1.weight, sd['conv1.weight'])
    assert all(torch.equal(v, head[k]) for k, v in net.cnn.state_dict().items())


# ---- C-ABI argument validation (no launch) -------------------------------------------------------------------------------------------
def test_pool_mse_fwd_refuses_bad_arguments_before_any_launch():
    from pcgan_amd.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(4096)         # a non-null, aligned address that is never dereferenced: every call below fails its checks

    def call(N=8, F=2, HW=49, is_max=0, dtype=lib.F32, x=one, target=one, argmax=None, dx=None, ws=one, ws_bytes=1 << 20):
        return h.pcgan_pool_mse_fwd(x, target, None, argmax, dx, None, None, ws, ws_bytes, N, F, HW, is_max, 0.05, 1.0, dtype, None)
    for bad in (dict(N=0), dict(F=0), dict(HW=0), dict(N=-3), dict(N=1 << 20, F=1 << 10), dict(HW=(1 << 20) + 1)):
        assert call(**bad) != 0 and b'pool_mse_fwd' in h.pcgan_last_error() and b'outside' in h.pcgan_last_error(), bad
    assert call(dtype=7) != 0 and b'dtype' in h.pcgan_last_error()
    assert call(x=None) != 0 and b'null' in h.pcgan_last_error()
    assert call(target=None) != 0 and b'null' in h.pcgan_last_error()
    assert call(is_max=1, dx=one) != 0 and b'argmax' in h.pcgan_last_error()
    assert call(ws=None) != 0 and b'workspace' in h.pcgan_last_error()
    assert call(ws_bytes=(1 + 2 * 16) * 8 - 1) != 0 and b'workspace' in h.pcgan_last_error()
    assert call(ws=ctypes.c_void_p(4100)) != 0 and b'aligned' in h.pcgan_last_error()
    assert h.pcgan_pool_mse_workspace_bytes(100) == (1 + 200) * 8
    assert h.pcgan_pool_mse_workspace_bytes(0) == 0 and h.pcgan_pool_mse_workspace_bytes((1 << 22) + 1) == 0


def test_tensor_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from pcgan_amd.hip import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.pool_mse_fwd(torch.zeros(2, 1, 3, 3), torch.zeros(2), 0.05, False)


# ---- regression.py: host logic ---------------------------------------------------------------------------------------------------------
REFERENCE_DEFAULTS = dict(
    mode='train', name='exp', datafile='', dataroot_val='', datafile_val='', pretrained_model_path='pretrained_models/resnet18-5c106cde.pth',
    checkpoint_dir='checkpoints', save_epoch_freq=10, num_workers=4, init_type='normal', num_classes=10, num_epochs=100, batch_size=100,
    lr=0.0002, which_epoch='latest', which_model='alexnet', n_layers=3, nf=64, pooling='avg', loadSize=240, fineSize=224, gpu_ids='0',
    print_freq=50, display_id=1, display_port=8097, delta=0.05, embedding_mean=0, embedding_std=1, cnn_dim=[64, 1], cnn_pad=1,
    cnn_relu_slope=0.7, transforms='resize_affine_crop', affineScale=[0.95, 1.05], affineDegrees=5, use_color_jitter=False, no_flip=False,
    epoch_count=1)


def test_options_are_the_references(tmp_path, capsys):
    import regression as S
    opt = S.get_options(['--dataroot', 'some/where', '--checkpoint_dir', str(tmp_path)])
    for k, v in REFERENCE_DEFAULTS.items():
        assert getattr(opt, k) == (str(tmp_path) if k == 'checkpoint_dir' else v), k
    assert S.build_parser().get_default('checkpoint_dir') == 'checkpoints'
    assert opt.dataroot == 'some/where' and opt.isTrain and opt.seed is None
    assert set(vars(opt)) - set(REFERENCE_DEFAULTS) == {'dataroot', 'isTrain', 'use_gpu', 'seed', 'test_batch_size', 'embedding_normalize'}
    text = open(tmp_path / 'exp' / 'opt.txt').read()
    assert text.startswith('--------------- Options -----------------') and 'which_model: alexnet' in text
    assert 'embedding_normalize' not in text and 'dataroot: some/where' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        S.get_options([])                                            # --dataroot is required
    opt = S.get_options(['--dataroot', 'd', '--mode', 'embedding', '--cnn_dim', '32', '16', '1', '--display_id', '-1', '--checkpoint_dir',
                         str(tmp_path)])
    assert not opt.isTrain and opt.cnn_dim == [32, 16, 1] and opt.display_id == -1


def test_labels_are_the_normalised_floats_the_names_start_with(tmp_path):
    import regression as S
    opt = S.get_options(['--dataroot', 'd', '--embedding_mean', '33', '--embedding_std', '20', '--checkpoint_dir', str(tmp_path)],
                        save=False)
    names = ['1_0_0_a.jpg\n', '20.5_1.png', '33_x.png', '116_0_2.png\n']
    assert [S.get_attr(n) for n in names] == [1.0, 20.5, 33.0, 116.0]
    label = S.labels_of(names, opt, 1)
    assert label.dtype == torch.float32 and tuple(label.shape) == (4, 1, 1, 1)
    want = (torch.FloatTensor([1.0, 20.5, 33.0, 116.0]) - 33) / 20             # the reference's arithmetic, in fp32
    assert torch.equal(label.view(-1), want) and float(label[2]) == 0.0
    plain = S.get_options(['--dataroot', 'd', '--checkpoint_dir', str(tmp_path)], save=False)
    assert torch.equal(S.labels_of(names, plain, 1).view(-1), torch.FloatTensor([1.0, 20.5, 33.0, 116.0]))
    with pytest.raises(ValueError):
        S.labels_of(['young_0.png'], opt, 1)
    with pytest.raises(RuntimeError):
        S.labels_of(names, opt, 2)                                   # as in the reference the view only fits one feature


@pytest.mark.parametrize('which', CASES)
def test_seeded_initialisation_coincides_with_the_references(gold, which, tmp_path):
    import regression as S
    opt = S.get_options(['--dataroot', 'd', '--which_model', which, '--pretrained_model_path', '', '--pooling',
                         str(gold['%s/pooling' % which]), '--checkpoint_dir', str(tmp_path)], save=False)
    torch.manual_seed(int(gold['init_seed']))
    net = S.get_model(opt)
    assert net.training and net.pooling == str(gold['%s/pooling' % which])
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold['%s/keys' % which]]
    for k, t in sd.items():
        if 'num_batches' in k:
            continue
        want = gold['%s/init/%s' % (which, k)]
        a = t.double().numpy()
        assert abs(a.sum() - want[0]) <= 1e-6 * want[1] + 1e-9 and abs(np.abs(a).sum() - want[1]) <= 1e-6 * want[1] + 1e-9, k
    assert float(sd['cnn.1.bias'].abs().max()) == 0 and abs(float(sd['cnn.1.weight'].mean()) - 1) < 0.02


def test_refusals(tmp_path):
    import regression as S

    def opt(*extra):
        return S.get_options(['--dataroot', 'd', '--checkpoint_dir', str(tmp_path), '--pretrained_model_path', ''] + list(extra), save=False)
    for which in ('vgg16', 'alexnet_lite', 'resnet101'):
        with pytest.raises(NotImplementedError, match=which):
            S.get_model(opt('--which_model', which))
    for mode in ('test', 'visualize'):
        with pytest.raises(NotImplementedError, match=r'Mode \[%s\] is not implemented\.' % mode):
            S.main(['--dataroot', 'd', '--checkpoint_dir', str(tmp_path), '--mode', mode])
    net = S.get_model(opt('--which_model', 'resnet18', '--pooling', ''))
    with pytest.raises(NotImplementedError, match='pooling'):
        net.regress(torch.zeros(1, 3, 8, 8), torch.zeros(1), 0.05)
