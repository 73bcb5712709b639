"""CPU: the attribute classifier's oracle side and host logic.

* tests/classifier_ref.py (twin + restated training step) reproduces tests/golden/classification_step.npz, which was captured from the
  reference's own networks.ResNet / CrossEntropyLoss / Adam (scripts/make_classification_golden.py).  The twin runs in float32 like the
  reference; its loss is written out instead of calling CrossEntropyLoss and its reductions may split differently over threads, so the
  bounds are the project's (tests/test_gpu_nets.py): outputs 1e-4 of the largest element, gradients on their own ReLU /
  max-pool decisions 3e-2 relative L2 (the reference's own fp32-vs-float64 gradient error is 4.9e-6 for the resnet18 case and 2e-2 for
  the resnet50 one).  Adam is sign-like at step 1, so the restated update is pinned separately and sharply: fed the fixture's own
  gradients it must give the fixture's parameters to one fp32 rounding.
* argument validation of pcgan_linear_ce_fwd / pcgan_linear_bwd happens before any launch, so it runs without a GPU.
* classification.py: every reference option with its default, labels from file names, the seeded initialisation, load_pretrained, and
  what the build refuses.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import classifier_ref as C
from oracle import weights as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'classification_step.npz')
OUT_TOL, GRAD_L2 = 1e-4, 3e-2


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


def _check_gradients(gold, prefix, named, stride):
    """every tensor: l2 norm and abs-sum against the recorded statistics; fc in full and a strided sample of the rest in relative L2"""
    for k, t in named.items():
        a = t.detach().numpy().astype(np.float64)
        stat = gold['%s/stat/%s' % (prefix, k)]
        assert abs(np.abs(a).sum() - stat[1]) <= GRAD_L2 * stat[1], '%s %s: abs-sum' % (prefix, k)
        assert abs(np.sqrt((a * a).sum()) - stat[2]) <= GRAD_L2 * stat[2], '%s %s: l2' % (prefix, k)
        full = '%s/full/%s' % (prefix, k)
        want = gold[full] if full in gold.files else gold['%s/samp/%s' % (prefix, k)]
        got = a if full in gold.files else a.reshape(-1)[::stride]
        if want.size >= 16:        # a sample of a few elements says nothing in relative L2: the statistics above cover those tensors
            assert _rel_l2(got, want) <= GRAD_L2, '%s %s: relative L2 %.3e' % (prefix, k, _rel_l2(got, want))


@pytest.mark.parametrize('which', ['resnet18', 'resnet50'])
def test_twin_and_restated_step_reproduce_the_reference(gold, which):
    size, seed = (int(v) for v in gold['%s/case' % which])
    labels = torch.from_numpy(gold['labels']).long()
    weight = torch.from_numpy(gold['class_weight'])
    net = C.ResNetClassifierRef(which, len(weight))
    net.load_state_dict(W.fill_state_dict(net.state_dict(), seed), strict=True)
    x = W.seeded_tensor((len(labels), 3, size, size), 100 + seed)
    logits, loss, grads, after = C.train_step(net, x, labels, weight, lr=float(gold['lr']))
    _close(logits, gold['%s/logits' % which], 'logits')
    _close(loss, gold['%s/loss' % which], 'weighted loss')
    _close(C.cross_entropy(logits, labels), gold['%s/loss_plain' % which], 'plain loss')
    assert C.predictions(logits).tolist() == gold['%s/pred' % which].tolist()
    # the closed-form gradient of the loss equals autograd's
    lg = logits.double().requires_grad_(True)
    C.cross_entropy(lg, labels, weight).backward()
    _close(C.cross_entropy_grad(logits.double(), labels, weight), lg.grad, 'closed-form d loss / d logits', 1e-12)
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
            got = C.adam_update(p0, g, lr=float(gold['lr'])).numpy()
            assert np.abs(got - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max()), 'Adam step of %s' % k
    assert set(after) == set(grads)
    for k, b in net.named_buffers():
        want = gold['%s/buf/%s' % (which, k)]
        if 'running' in k:
            a = b.double().numpy()
            assert abs(a.sum() - want[0]) <= OUT_TOL * want[1] and abs(np.abs(a).sum() - want[1]) <= OUT_TOL * want[1], k
        else:
            assert int(b) == int(want) == 1, k


def test_twin_has_the_reference_keys_and_the_hip_net_shares_them():
    from pcgan_amd.models import networks
    for which in ('resnet18', 'resnet34', 'resnet50'):
        twin = C.ResNetClassifierRef(which, 7)
        net = networks.ResNet(3, 7, which)
        assert list(twin.state_dict().keys()) == list(net.state_dict().keys())
        assert list(net.state_dict())[0] == 'model.conv1.weight' and list(net.state_dict())[-1] == 'model.fc.bias'
        net.load_state_dict(twin.state_dict(), strict=True)


# ---- C-ABI argument validation (no launch) -------------------------------------------------------------------------------------------
def test_linear_ce_fwd_refuses_bad_arguments_before_any_launch():
    from pcgan_amd.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(4096)         # a non-null, aligned address that is never dereferenced: every call below fails its checks
    ok = dict(N=8, C=512, K=5)

    def call(N=8, C=512, K=5, dtype=lib.F32, x=one, w=one, labels=one, ws=one, ws_bytes=1 << 20):
        return h.pcgan_linear_ce_fwd(x, w, None, labels, None, None, None, None, None, None, ws, ws_bytes, N, C, K, dtype, None)
    assert call(dtype=lib.BF16) != 0 and b'fp32' in h.pcgan_last_error()
    for bad in (dict(N=0), dict(N=513), dict(C=0), dict(C=510), dict(C=2052), dict(K=0), dict(K=1025)):
        assert call(**dict(ok, **bad)) != 0 and b'linear_ce_fwd' in h.pcgan_last_error(), bad
    assert call(x=None) != 0 and call(w=None) != 0 and call(labels=None) != 0
    assert b'null' in h.pcgan_last_error()
    assert call(ws=None) != 0 and b'workspace' in h.pcgan_last_error()
    assert call(ws_bytes=8) != 0 and b'workspace' in h.pcgan_last_error()
    assert call(ws=ctypes.c_void_p(4100)) != 0 and b'aligned' in h.pcgan_last_error()
    assert h.pcgan_linear_ce_workspace_bytes(100) == (1 + 200) * 8
    assert h.pcgan_linear_ce_workspace_bytes(0) == 0 and h.pcgan_linear_ce_workspace_bytes(513) == 0


def test_linear_bwd_refuses_bad_arguments_before_any_launch():
    from pcgan_amd.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(4096)

    def call(N=8, C=512, K=5, dtype=lib.F32, dl=one, x=one, w=one, dx=one, dw=one, db=one):
        return h.pcgan_linear_bwd(dl, x, w, dx, dw, db, N, C, K, 0, dtype, None)
    assert call(dtype=lib.BF16) != 0 and b'fp32' in h.pcgan_last_error()
    for bad in (dict(N=0), dict(N=513), dict(C=6), dict(C=4096), dict(K=0), dict(K=2000)):
        assert call(**bad) != 0 and b'linear_bwd' in h.pcgan_last_error(), bad
    assert call(dl=None) != 0 and b'dlogits' in h.pcgan_last_error()
    assert call(dx=None, dw=None, db=None) != 0 and b'nothing to compute' in h.pcgan_last_error()
    assert call(w=None) != 0 and b'dx needs w' in h.pcgan_last_error()
    assert call(x=None) != 0 and b'dw needs x' in h.pcgan_last_error()


def test_tensor_wrappers_refuse_cpu_tensors():
    from pcgan_amd.hip import ops
    x, w, b = torch.zeros(4, 8), torch.zeros(3, 8), torch.zeros(3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.linear_ce_fwd(x, w, b, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.linear_bwd(torch.zeros(4, 3), x, w)


# ---- classification.py: host logic -----------------------------------------------------------------------------------------------------
REFERENCE_DEFAULTS = dict(
    mode='train', name='exp', datafile='', dataroot_val='', datafile_val='', pretrained_model_path='pretrained_models/resnet18-5c106cde.pth',
    checkpoint_dir='checkpoints', save_epoch_freq=10, num_workers=4, init_type='normal', num_classes=10, num_epochs=100, batch_size=100,
    lr=0.0002, which_epoch='latest', which_model='resnet18', n_layers=3, nf=64, pooling='avg', loadSize=240, fineSize=224, gpu_ids='0',
    attr_bins=[], weight=[], dropout=0.5, finetune_fc_only=False, print_freq=50, display_id=1, display_port=8097,
    transforms='resize_affine_crop', affineScale=[0.95, 1.05], affineDegrees=5, use_color_jitter=False, no_flip=False, continue_train=False,
    epoch_count=1, result_path='')


def test_options_are_the_references(tmp_path, capsys):
    import classification as S
    opt = S.get_options(['--dataroot', 'some/where', '--checkpoint_dir', str(tmp_path)])
    for k, v in REFERENCE_DEFAULTS.items():
        assert getattr(opt, k) == (str(tmp_path) if k == 'checkpoint_dir' else v), k
    assert S.build_parser().get_default('checkpoint_dir') == 'checkpoints'
    assert opt.dataroot == 'some/where' and opt.isTrain and opt.attr_bins_with_inf == [float('inf')]
    assert opt.seed is None and opt.test_batch_size == 1                       # the build-only flags
    assert set(vars(opt)) - set(REFERENCE_DEFAULTS) == {'dataroot', 'isTrain', 'use_gpu', 'attr_bins_with_inf', 'seed', 'test_batch_size'}
    text = open(tmp_path / 'exp' / 'opt.txt').read()
    assert text.startswith('--------------- Options -----------------') and 'which_model: resnet18' in text
    assert 'dataroot: some/where' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        S.get_options([])                                            # --dataroot is required
    opt = S.get_options(['--dataroot', 'd', '--mode', 'test', '--attr_bins', '[1, 21, 41]', '--num_classes', '3', '--weight', '1',
                                   '2', '0.5', '--checkpoint_dir', str(tmp_path)])
    assert not opt.isTrain and opt.attr_bins_with_inf == [1, 21, 41, float('inf')] and opt.weight == [1.0, 2.0, 0.5]
    with pytest.raises(AssertionError):
        S.get_options(['--dataroot', 'd', '--num_classes', '3', '--weight', '1', '2', '--checkpoint_dir', str(tmp_path)])


def test_labels_come_from_file_names_through_the_bins(tmp_path):
    import classification as S
    opt = S.get_options(['--dataroot', 'd', '--attr_bins', '[1, 21, 41, 61, 81]', '--num_classes', '5', '--checkpoint_dir',
                                   str(tmp_path)], save=False)
    names = ['1_0_0_a.jpg\n', '20_1.png', '21_x.png', '60.5_x.png', '61_0.png', '99_0.png', '500_1.png\n']
    assert S.labels_of(names, opt) == [0, 0, 1, 2, 3, 4, 4]
    assert S.labels_of(['0_below_the_first_edge.png'], opt) == [4]             # the reference's fall-through to the last bin
    opt.num_classes = 4
    with pytest.raises(ValueError, match='outside the 4 classes'):
        S.labels_of(['99_0.png'], opt)                                         # label 4 of 4 classes: refused on the host
    opt.attr_bins_with_inf = [float('inf')]
    with pytest.raises(ValueError):
        S.labels_of(['3_0.png'], opt)                                          # no bins: get_attr_label gives None


@pytest.mark.parametrize('which', ['resnet18', 'resnet50'])
def test_seeded_initialisation_coincides_with_the_references(gold, which, tmp_path):
    import classification as S
    opt = S.get_options(['--dataroot', 'd', '--which_model', which, '--num_classes', '5', '--pretrained_model_path', '',
                                   '--checkpoint_dir', str(tmp_path)], save=False)
    torch.manual_seed(int(gold['init_seed']))
    net = S.get_model(opt)
    assert net.training
    sd = net.state_dict()
    for k, t in sd.items():
        if 'num_batches' in k:
            continue
        want = gold['%s/init/%s' % (which, k)]
        a = t.double().numpy()
        assert abs(a.sum() - want[0]) <= 1e-6 * want[1] + 1e-9 and abs(np.abs(a).sum() - want[1]) <= 1e-6 * want[1] + 1e-9, k
    # BatchNorm bias 0, weights around 1; the Linear bias keeps nn.Linear's default (uniform within 1 / sqrt(fan_in))
    assert float(sd['model.bn1.bias'].abs().max()) == 0 and abs(float(sd['model.bn1.weight'].mean()) - 1) < 0.02
    bound = 1.0 / sd['model.fc.weight'].shape[1] ** 0.5
    assert 0 < float(sd['model.fc.bias'].abs().max()) <= bound


def test_load_pretrained_drops_fc_and_loads_the_trunk_non_strictly():
    from pcgan_amd.models import networks
    net = networks.ResNet(3, 5, 'resnet18')
    donor = C.ResNetClassifierRef('resnet18', 1000).model            # an ImageNet-style checkpoint: bare keys, 1000 classes
    sd = W.fill_state_dict(donor.state_dict(), 3)
    del sd['layer4.1.bn2.weight']                                    # non-strict: a missing key is tolerated
    before_fc = net.model.fc.weight.detach().clone()
    before_bn = net.model.layer4[1].bn2.weight.detach().clone()
    net.load_pretrained(dict(sd))
    assert torch.equal(net.model.conv1.weight, sd['conv1.weight']) and torch.equal(net.model.layer3[0].downsample[1].running_var,
                                                                                   sd['layer3.0.downsample.1.running_var'])
    assert torch.equal(net.model.fc.weight, before_fc) and tuple(net.model.fc.weight.shape) == (5, 512)
    assert torch.equal(net.model.layer4[1].bn2.weight, before_bn)
    assert 'fc.weight' in sd                                          # the caller's dict is not emptied behind its back


def test_refusals(tmp_path):
    import classification as S
    from pcgan_amd.models import networks

    def opt(*extra):
        return S.get_options(['--dataroot', 'd', '--checkpoint_dir', str(tmp_path), '--pretrained_model_path', ''] + list(extra),
                                       save=False)
    for which in ('resnet101', 'resnet152'):
        with pytest.raises(NotImplementedError, match=which):
            networks.ResNet(3, 5, which)
        with pytest.raises(NotImplementedError, match=which):
            S.get_model(opt('--which_model', which))
    for which in ('alexnet', 'alexnet_lite', 'vgg16'):
        with pytest.raises(NotImplementedError, match=which):
            S.get_model(opt('--which_model', which))
    with pytest.raises(NotImplementedError, match='visualize'):
        S.main(['--dataroot', 'd', '--checkpoint_dir', str(tmp_path), '--mode', 'visualize'])
    with pytest.raises(AttributeError, match='get_finetune_parameters'):
        S.get_model(opt('--finetune_fc_only'))
    with pytest.raises(ValueError, match='not a valid option'):
        S.get_transform(opt('--transforms', 'stretch'))


def test_transform_is_the_references_normalisation(tmp_path):
    """ToTensor then Normalize with the CIFAR statistics on the PIL steps; all seven --transforms modes are accepted"""
    import random
    from PIL import Image
    import classification as S
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (40, 40, 3), dtype=np.uint8))
    for mode in ('resize_and_crop', 'crop', 'scale_width', 'scale_width_and_crop', 'none', 'resize_affine_crop', 'resize_affine_center'):
        o = S.get_options(['--dataroot', 'd', '--checkpoint_dir', str(tmp_path), '--transforms', mode, '--loadSize', '36',
                                     '--fineSize', '32', '--no_flip'], save=False)
        random.seed(1)
        t = S.get_transform(o)(img)
        assert t.dtype == torch.float32 and t.shape[0] == 3 and bool(torch.isfinite(t).all()), mode
    o = S.get_options(['--dataroot', 'd', '--checkpoint_dir', str(tmp_path), '--transforms', 'none', '--no_flip'], save=False)
    t = S.get_transform(o)(img)
    want = (torch.from_numpy(np.asarray(img, dtype=np.float32).transpose(2, 0, 1) / 255.0) - torch.tensor(S.MEAN).view(3, 1, 1)) \
        / torch.tensor(S.STD).view(3, 1, 1)
    assert torch.equal(t, want)
