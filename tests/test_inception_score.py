"""CPU: the Inception Score (pcgan_amd/util/inception_score.py) against closed forms and a literal restatement of the reference's loop
(util/inception_score.py:44-66 with scipy.stats.entropy), the refusals of compute_inception_score.py and of the classifier loaders
before any device use, the script's transform against a numpy restatement, and the C-ABI checks of the classifier head."""
import os
import random

import numpy as np
import pytest
import torch
from scipy.stats import entropy

import inception_ref as R


def _reference_loop(preds, splits):
    N = preds.shape[0]
    split_scores = []
    for k in range(splits):
        part = preds[k * (N // splits): (k + 1) * (N // splits), :]
        py = np.mean(part, axis=0)
        scores = []
        for i in range(part.shape[0]):
            pyx = part[i, :]
            scores.append(entropy(pyx, py))
        split_scores.append(np.exp(np.mean(scores)))
    return np.mean(split_scores), np.std(split_scores)


def test_closed_forms():
    from pcgan_amd.util.inception_score import score
    m, s = score(np.full((24, 8), 0.125), 3)          # uniform rows: nothing to learn from x
    assert m == 1.0 and s == 0.0
    K, splits = 8, 3
    onehot = np.tile(np.eye(K), (2 * splits, 1))      # every class twice per split: p(y) uniform, every KL = log K
    m, s = score(onehot, splits)
    assert abs(m - K) <= 1e-12 * K and s <= 1e-12
    rng = np.random.default_rng(1)
    p = rng.dirichlet(np.ones(10), size=40)
    p[rng.random(p.shape) < 0.3] = 0.0                # exact zeros: 0 log 0 = 0, no NaN
    p /= p.sum(axis=1, keepdims=True)
    m, s = score(p, 4)
    assert np.isfinite(m) and np.isfinite(s) and m >= 1.0


@pytest.mark.parametrize('N,K,splits', [(103, 10, 4), (50, 1000, 1), (37, 5, 10), (64, 7, 3)])
def test_matches_the_reference_loop(N, K, splits):
    from pcgan_amd.util.inception_score import score
    rng = np.random.default_rng(N * K + splits)
    logits = rng.normal(scale=3.0, size=(N, K))
    p = np.exp(logits - logits.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    p[:, 0] = np.where(rng.random(N) < 0.2, 0.0, p[:, 0])      # some exact zeros
    got, want = score(p, splits), _reference_loop(p, splits)
    assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0])
    assert abs(got[1] - want[1]) <= 1e-12 * max(abs(want[0]), 1.0)


def test_batches_are_taken_in_order_with_a_partial_last_one():
    from pcgan_amd.util.inception_score import inception_score, predictions
    g = torch.Generator().manual_seed(2)
    imgs = [torch.rand(3, 4, 4, generator=g) for _ in range(23)]
    proj = torch.randn(48, 6, generator=g, dtype=torch.float64)
    sizes = []

    def predict(batch):
        sizes.append(batch.shape[0])
        return torch.softmax(batch.reshape(batch.shape[0], -1).double() @ proj, dim=1)

    preds = predictions(imgs, predict, 6, 5, verbose=False)
    assert sizes == [5, 5, 5, 5, 3]
    for i, x in enumerate(imgs):
        assert np.array_equal(preds[i], predict(x[None])[0].numpy())
    got = inception_score(imgs, predict, 6, 5, splits=3, verbose=False)
    want = _reference_loop(preds, 3)
    assert abs(got[0] - want[0]) <= 1e-12 * want[0] and abs(got[1] - want[1]) <= 1e-12 * want[0]
    with pytest.raises(AssertionError):
        inception_score(imgs, predict, 6, 23, verbose=False)       # the reference's `assert N > batch_size`


# ---- compute_inception_score.py: refusals before any device use ---------------------------------------------------------------------
def _opt(tmp_path, *flags):
    import compute_inception_score as S
    return S.options(['--dataroot', str(tmp_path), '--checkpoints_dir', str(tmp_path / 'ck')] + [str(f) for f in flags])[1]


@pytest.fixture(scope='module')
def inception_sd():
    return R.random_state_dict(3)


def test_script_refusals(tmp_path, inception_sd):
    import compute_inception_score as S
    with pytest.raises(NotImplementedError, match='vgg16'):
        S.classifier_spec(_opt(tmp_path, '--which_model_IS', 'vgg16', '--num_classes', 5))
    with pytest.raises(NotImplementedError, match='resnet101'):
        S.classifier_spec(_opt(tmp_path, '--which_model_IS', 'resnet101', '--num_classes', 5, '--pretrained_model_path_IS', 'x'))
    with pytest.raises(ValueError, match='--inception_weights.*random weights is not IS'):
        S.classifier_spec(_opt(tmp_path))
    with pytest.raises(ValueError, match='--pretrained_model_path_IS'):
        S.classifier_spec(_opt(tmp_path, '--which_model_IS', 'resnet18', '--num_classes', 5))
    with pytest.raises(ValueError, match='--num_classes'):
        S.classifier_spec(_opt(tmp_path, '--which_model_IS', 'resnet18', '--pretrained_model_path_IS', 'x'))
    torch.save(inception_sd, tmp_path / 'inc.pth')
    with pytest.raises(ValueError, match='--num_classes 5.*1000'):
        S.classifier_spec(_opt(tmp_path, '--inception_weights', tmp_path / 'inc.pth', '--num_classes', 5))
    which, classes, sd = S.classifier_spec(_opt(tmp_path, '--inception_weights', tmp_path / 'inc.pth'))
    assert (which, classes) == ('inception_v3', 1000) and sd['fc.weight'].shape == (1000, 2048)
    with pytest.raises(ValueError, match='not a valid option'):
        S.get_transform(_opt(tmp_path, '--transforms', 'scale_width'))


@pytest.mark.parametrize('case', ['no_fc', 'fid1008'])
def test_inception_classifier_weights_refusals(tmp_path, inception_sd, case):
    import compute_inception_score as S
    from pcgan_amd.models.inception import InceptionV3Classifier, check_state_dict
    sd = dict(inception_sd)
    if case == 'no_fc':
        del sd['fc.weight'], sd['fc.bias']
        err, msg = KeyError, 'fc.weight'
    else:
        sd['fc.weight'], sd['fc.bias'] = torch.zeros(1008, 2048), torch.zeros(1008)
        err, msg = ValueError, 'pytorch-fid'
    with pytest.raises(err, match=msg):
        InceptionV3Classifier(weights=sd, gpu_ids=[0])
    torch.save(sd, tmp_path / 'w.pth')
    with pytest.raises(err, match=msg):
        S.classifier_spec(_opt(tmp_path, '--inception_weights', tmp_path / 'w.pth'))
    if case == 'no_fc':      # the FID feature network keeps taking a feature-only file
        assert len(check_state_dict(sd)) == 94 * 5


def test_resnet_classifier_state_dict_and_refusals(tmp_path):
    import compute_inception_score as S
    from pcgan_amd.models import networks
    for which, dim in (('resnet18', 512), ('resnet34', 512), ('resnet50', 2048)):
        net = networks.ResNet(3, 5, which)
        keys = list(net.state_dict())
        assert keys[0] == 'model.conv1.weight' and keys[-2:] == ['model.fc.weight', 'model.fc.bias']
        assert tuple(net.state_dict()['model.fc.weight'].shape) == (5, dim)
    for which in ('resnet101', 'resnet152', 'vgg16'):
        with pytest.raises(NotImplementedError, match=which):
            networks.ResNet(3, 5, which)
    sd = networks.ResNet(3, 5, 'resnet18').state_dict()
    torch.save(sd, tmp_path / 'ok.pth')
    which, classes, net = S.classifier_spec(_opt(tmp_path, '--which_model_IS', 'resnet18', '--num_classes', 5,
                                                 '--pretrained_model_path_IS', tmp_path / 'ok.pth'))
    assert (which, classes) == ('resnet18', 5) and all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    torch.save({k[len('model.'):]: v for k, v in sd.items()}, tmp_path / 'bare.pth')     # keys without the wrapper's `model.`
    with pytest.raises(RuntimeError, match='Missing key'):
        S.classifier_spec(_opt(tmp_path, '--which_model_IS', 'resnet18', '--num_classes', 5,
                               '--pretrained_model_path_IS', tmp_path / 'bare.pth'))
    with pytest.raises(RuntimeError, match='size mismatch'):
        S.classifier_spec(_opt(tmp_path, '--which_model_IS', 'resnet18', '--num_classes', 7,
                               '--pretrained_model_path_IS', tmp_path / 'ok.pth'))


# ---- the script's transform: ToTensor + CIFAR Normalize after the PIL steps --------------------------------------------------------
@pytest.mark.parametrize('mode', ['resize_and_crop', 'crop', 'resize_affine_crop', 'resize_affine_center'])
def test_transform_is_to_tensor_then_cifar_normalize(tmp_path, mode):
    from PIL import Image
    import compute_inception_score as S
    from pcgan_amd.data.base_dataset import pil_steps
    rng = np.random.default_rng(4)
    img = Image.fromarray(rng.integers(0, 256, (45, 52, 3), dtype=np.uint8))
    opt = _opt(tmp_path, '--transforms', mode, '--loadSize', 48, '--fineSize', 40)
    random.seed(5)
    got = S.get_transform(opt)(img)
    random.seed(5)
    a = np.asarray(pil_steps(opt, img), dtype=np.float32).transpose(2, 0, 1) / np.float32(255)
    want = (a - np.array(S.MEAN, dtype=np.float32)[:, None, None]) / np.array(S.STD, dtype=np.float32)[:, None, None]
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 40, 40)
    assert np.array_equal(got.numpy(), want)


def test_image_list_is_sorted_seeded_and_cut(tmp_path):
    import compute_inception_score as S
    for i in range(9):
        (tmp_path / ('%d.png' % (8 - i))).write_bytes(b'')
    opt = _opt(tmp_path, '--how_many', 5)
    random.seed(6)
    got = S.image_paths(opt)
    random.seed(6)
    want = [os.path.join(str(tmp_path), '%d.png' % i) for i in range(9)]
    random.shuffle(want)
    assert got == want[:5]


def test_c_abi_refuses_bf16_and_empty_shapes():
    from pcgan_amd.hip import lib
    h = lib.load()
    assert h.pcgan_linear_softmax_fwd(None, None, None, None, None, 4, 8, 10, lib.BF16, None) != 0
    assert b'fp32' in h.pcgan_last_error()
    for N, C, K in ((0, 8, 10), (4, 0, 10), (4, 8, 0)):
        assert h.pcgan_linear_softmax_fwd(None, None, None, None, None, N, C, K, lib.F32, None) != 0
        assert b'non-positive' in h.pcgan_last_error()
    assert h.pcgan_linear_softmax_fwd(None, None, None, None, None, 4, 8, 10, lib.F32, None) != 0
    assert b'null' in h.pcgan_last_error()
