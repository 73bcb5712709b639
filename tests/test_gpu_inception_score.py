"""GPU: the classifier head of the Inception Score (pcgan_linear_softmax_fwd) against float64, the two classifiers
(InceptionV3Classifier, networks.ResNet) against float64 restatements with stock torch modules, and compute_inception_score.py end to
end.  Head bounds, per element: |logit - l64| <= (C + 16) u sum|x w| + u |l64| (u = 2^-24, the bias counted in the sum);
|p - p64| <= p64 (2 E_row + 8 u) with E_row the largest logit bound of the row."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import inception_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _check_head(x, w, b, logits, probs, what):
    x64, w64, b64 = x.double().cpu(), w.double().cpu(), b.double().cpu()
    l64 = x64 @ w64.t() + b64
    p64 = torch.softmax(l64, dim=1)
    bound = (x.shape[1] + 16) * U * (x64.abs() @ w64.abs().t() + b64.abs()) + U * l64.abs()
    err = (logits.double().cpu() - l64).abs()
    assert bool((err <= bound).all()), '%s: logit error %.3e over its bound' % (what, float((err - bound).max()))
    pbound = p64 * (2 * bound.max(dim=1, keepdim=True).values + 8 * U)
    perr = (probs.double().cpu() - p64).abs()
    assert bool(torch.isfinite(probs).all()), what
    assert bool((perr <= pbound).all()), '%s: probability error %.3e over its bound' % (what, float((perr - pbound).max()))


@pytest.mark.parametrize('K', [1, 5, 10, 1000, 1001])
@pytest.mark.parametrize('C', [37, 512, 2048])
def test_head_against_float64(dev, C, K):
    from pcgan_amd.hip import inception as I
    for N in (1, 7, 32, 100, 257):
        g = torch.Generator().manual_seed(N * 100000 + C * 10 + K)
        x = torch.randn(N, C, generator=g).abs()                      # pooled ReLU features are >= 0
        w = torch.randn(K, C, generator=g) * (2.0 / C ** 0.5)
        b = torch.randn(K, generator=g) * 0.5
        xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
        logits, probs = I.linear_softmax(xd, wd, bd)
        none, probs2 = I.linear_softmax(xd, wd, bd, want_logits=False)
        torch.cuda.synchronize()
        assert none is None and torch.equal(probs, probs2), 'softmax in place differs (N %d C %d K %d)' % (N, C, K)
        _check_head(x, w, b, logits, probs, 'N %d C %d K %d' % (N, C, K))
    # a 4-byte aligned x with C % 4 == 0: the element-wise load path, same values as the 16-byte path
    if C % 4 == 0:
        buf = torch.empty(7 * C + 1, device=dev)
        xs = buf[1:].view(7, C)
        xs.copy_(xd[:7])
        l2, p2 = I.linear_softmax(xs, wd, bd)
        l1, p1 = I.linear_softmax(xd[:7].contiguous(), wd, bd)
        torch.cuda.synchronize()
        _check_head(x[:7], w, b, l2, p2, 'unaligned x, C %d K %d' % (C, K))
        assert torch.equal(l1, l2) and torch.equal(p1, p2)


def test_head_extreme_and_equal_rows(dev):
    """spreads of 2e4 and 4e4 give exact zeros (no NaN, no inf), a row of equal logits the uniform row, 999 tied maxima 1/999 each"""
    from pcgan_amd.hip import inception as I
    N, C, K = 5, 64, 1000
    w = torch.zeros(K, C)
    w[:, 0] = -1e4
    w[3, 0] = 1e4
    x = torch.zeros(N, C)
    x[:, 0] = torch.tensor([1.0, 0.0, -1.0, 2.0, 0.5])
    b = torch.full((K,), 7.0)
    logits, probs = I.linear_softmax(x.to(dev), w.to(dev), b.to(dev))
    torch.cuda.synchronize()
    _check_head(x, w, b, logits, probs, 'extreme rows')
    p = probs.cpu()
    for r in (0, 3, 4):
        assert p[r, 3] == 1.0 and bool((torch.cat([p[r, :3], p[r, 4:]]) == 0).all())
    assert bool((p[1] == p[1, 0]).all()) and abs(float(p[1, 0]) * K - 1) < 1e-6
    assert p[2, 3] == 0 and bool((torch.cat([p[2, :3], p[2, 4:]]) == p[2, 0]).all()) and abs(float(p[2, 0]) * 999 - 1) < 1e-6


def test_head_is_bit_identical_alone_and_beside_training_kernels(dev):
    from pcgan_amd.hip import inception as I
    from pcgan_amd.hip import ops
    g = torch.Generator().manual_seed(15)
    x = torch.randn(100, 2048, generator=g).abs().to(dev)
    w = (torch.randn(1000, 2048, generator=g) * 0.04).to(dev)
    b = torch.randn(1000, generator=g).to(dev)
    xr = torch.randn(32, 256, 32, 32, generator=g).to(dev)
    wr = (torch.randn(256, 256, 3, 3, generator=g) * 0.05).to(dev)
    cr = {}

    def company():
        for _ in range(4):
            ops.conv2d_fwd(xr, wr, None, 1, 1, 1, pack_cache=cr)
            ops.conv2d_bwd_weight(xr, xr, (256, 256, 3, 3), 1, 1, 1)
    company()
    alone = [t.clone() for t in I.linear_softmax(x, w, b)]
    again = I.linear_softmax(x, w, b)
    torch.cuda.synchronize()
    assert torch.equal(alone[0], again[0]) and torch.equal(alone[1], again[1])
    other = torch.cuda.Stream()
    for _ in range(3):
        other.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(other):
            company()
        got = I.linear_softmax(x, w, b)
        torch.cuda.synchronize()
        assert torch.equal(alone[0], got[0]) and torch.equal(alone[1], got[1]), 'head changed beside the training kernels'


# ---- whole classifiers against float64 -----------------------------------------------------------------------------------------------
class _Basic(nn.Module):
    expansion = 1

    def __init__(self, cin, planes, stride, down):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = down

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        return F.relu(self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x))))) + idt)


class _Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, cin, planes, stride, down):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = down

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = F.relu(self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x))))))
        return F.relu(self.bn3(self.conv3(out)) + idt)


class _ResNetRef(nn.Module):
    """torchvision-style ResNet (the reference's models/resnet.py without dropout) with avgpool + fc"""

    def __init__(self, block, layers, num_classes):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for i, (planes, n, stride) in enumerate(zip((64, 128, 256, 512), layers, (1, 2, 2, 2)), 1):
            blocks = []
            for j in range(n):
                s = stride if j == 0 else 1
                down = None
                if s != 1 or cin != planes * block.expansion:
                    down = nn.Sequential(nn.Conv2d(cin, planes * block.expansion, 1, s, bias=False), nn.BatchNorm2d(planes * block.expansion))
                blocks.append(block(cin, planes, s, down))
                cin = planes * block.expansion
            setattr(self, 'layer%d' % i, nn.Sequential(*blocks))
        self.fc = nn.Linear(cin, num_classes)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(F.adaptive_avg_pool2d(x, 1).flatten(1))


class ResNetClassifierRef(nn.Module):
    """networks.ResNet's layout: the net under `model.`"""
    ARCH = {'resnet18': (_Basic, (2, 2, 2, 2)), 'resnet34': (_Basic, (3, 4, 6, 3)), 'resnet50': (_Bottleneck, (3, 4, 6, 3))}

    def __init__(self, which, num_classes):
        super().__init__()
        block, layers = self.ARCH[which]
        self.model = _ResNetRef(block, layers, num_classes)

    def forward(self, x):
        return self.model(x)


def _random_resnet_sd(ref, seed):
    """He-scaled convolutions, random BatchNorm affine and running statistics, logits of a few units"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    basic = not any(k.endswith('conv3.weight') for k in ref.state_dict())
    for k, v in ref.state_dict().items():
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.zeros_like(v)
        elif v.dim() == 4:
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / v[0].numel()) ** 0.5
        elif k.endswith('fc.weight'):
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / v.shape[1] ** 0.5)
        elif k.endswith('running_var'):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith('.weight') and ('bn' in k or 'downsample.1' in k):
            # the norms that end a residual branch are scaled down: activations stay O(1) through 16 blocks
            last = 'layer' in k and k.endswith(('bn3.weight', 'downsample.1.weight', 'bn2.weight' if basic else 'bn3.weight'))
            sd[k] = (0.2 + 0.2 * torch.rand(v.shape, generator=g)) if last else 0.6 + 0.8 * torch.rand(v.shape, generator=g)
        else:
            sd[k] = 0.4 * torch.rand(v.shape, generator=g) - 0.2
    return sd


def _inception_sd(seed):
    sd = R.random_state_dict(seed)
    g = torch.Generator().manual_seed(seed + 1)
    sd['fc.weight'] = torch.randn(1000, 2048, generator=g) * 0.05      # logits spread over a few units
    sd['fc.bias'] = torch.randn(1000, generator=g) * 0.5
    return sd


def _inception64(sd, x):
    ref = R.make_ref(sd, dtype=torch.float64)
    pooled = R.forward_ref(ref, x.double(), (3,), resize_input=True, normalize_input=False)[0].flatten(1)
    with torch.no_grad():
        return F.linear(pooled, ref.fc.weight, ref.fc.bias)


def _compare(logits, probs, l64, what):
    from pcgan_amd.util.inception_score import score
    p64 = torch.softmax(l64, dim=1)
    el = float((logits.double().cpu() - l64).abs().max())
    ep = float((probs.double().cpu() - p64).abs().max())
    assert el <= 1e-4 * float(l64.abs().max()), '%s: logits off by %.3e' % (what, el)
    assert ep <= 1e-4 * float(p64.max()), '%s: probabilities off by %.3e' % (what, ep)
    ours, want = score(probs.double().cpu().numpy(), 1)[0], score(p64.numpy(), 1)[0]
    assert abs(ours - want) <= 1e-5 * want, '%s: IS %.9f vs float64 %.9f' % (what, ours, want)


def test_inception_classifier_against_float64(dev):
    from pcgan_amd.models.inception import InceptionV3Classifier
    sd = _inception_sd(31)
    x = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(33)) * 2 - 1
    net = InceptionV3Classifier(weights=sd)
    logits, probs = net(x.to(dev), probs=True)
    torch.cuda.synchronize()
    assert net.num_classes == 1000 and tuple(probs.shape) == (4, 1000)
    _compare(logits, probs, _inception64(sd, x), 'inception_v3 128 -> 299')


@pytest.mark.parametrize('which', ['resnet18', 'resnet34', 'resnet50'])
def test_resnet_classifier_against_float64(dev, which):
    from pcgan_amd.models import networks
    ref = ResNetClassifierRef(which, 5)
    sd = _random_resnet_sd(ref, {'resnet18': 41, 'resnet34': 42, 'resnet50': 43}[which])
    ref.load_state_dict(sd)
    ref = ref.double().eval()
    net = networks.ResNet(3, 5, which)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(44))
    logits, probs = net(x.to(dev), probs=True)
    torch.cuda.synchronize()
    with torch.no_grad():
        l64 = ref(x.double())
    _compare(logits, probs, l64, which)
    assert torch.equal(net(x.to(dev)), logits)


# ---- compute_inception_score.py end to end -------------------------------------------------------------------------------------------
def _pngs(root, n, size, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(root, '%03d.png' % i))


def _run_and_restate(argv):
    """runs the script in a child process; returns (its result file's two numbers, the seeded dataset the float64 side gets)"""
    import compute_inception_score as S
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'compute_inception_score.py')] + argv, cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert 'IS: mean ' in p.stdout
    opt = S.options(argv)[1]
    with open(opt.result_path) as f:
        got = [float(v) for v in f.read().split()]
    random.seed(opt.seed)
    ds = S.ImageFolderDataset(S.image_paths(opt), S.get_transform(opt))
    return got, torch.stack([ds[i] for i in range(len(ds))]), opt


def _assert_score(got, p64, splits):
    from pcgan_amd.util.inception_score import score
    mu, sd = score(p64.numpy(), splits)
    assert abs(got[0] - mu) <= 2e-6 + 1e-5 * mu, (got, mu, sd)
    assert abs(got[1] - sd) <= 2e-6 + 1e-5 * mu, (got, mu, sd)


def test_script_inception_v3_end_to_end(dev, tmp_path):
    sd = _inception_sd(51)
    torch.save(sd, tmp_path / 'inception_v3.pth')
    _pngs(str(tmp_path / 'gen'), 12, 40, 52)
    argv = [str(a) for a in ['--dataroot', tmp_path / 'gen', '--which_model_IS', 'inception_v3', '--inception_weights',
                             tmp_path / 'inception_v3.pth', '--loadSize', 48, '--fineSize', 40, '--batchSize_IS', 5, '--splits', 2,
                             '--how_many', 11, '--seed', 7, '--checkpoints_dir', tmp_path / 'ck', '--result_path', tmp_path / 'is.txt']]
    got, imgs, opt = _run_and_restate(argv)
    assert imgs.shape == (11, 3, 40, 40)
    _assert_score(got, torch.softmax(_inception64(sd, imgs), dim=1), 2)


def test_script_resnet18_end_to_end_as_eval_emb_calls_it(dev, tmp_path):
    ref = ResNetClassifierRef('resnet18', 5)
    sd = _random_resnet_sd(ref, 61)
    ref.load_state_dict(sd)
    ref = ref.double().eval()
    os.makedirs(tmp_path / 'checkpoints' / 'class_x')
    ck = tmp_path / 'checkpoints' / 'class_x' / 'latest_net.pth'
    torch.save(sd, ck)
    _pngs(str(tmp_path / 'gen'), 40, 64, 62)
    argv = [str(a) for a in ['--dataroot', tmp_path / 'gen', '--num_classes', 5, '--which_model_IS', 'resnet18',
                             '--pretrained_model_path_IS', ck, '--loadSize', 224, '--fineSize', 224, '--batchSize', 32,
                             '--batchSize_IS', 32, '--splits', 4, '--result_path', tmp_path / 'res_is.txt', '--seed', 3,
                             '--checkpoints_dir', tmp_path / 'ck']]
    got, imgs, opt = _run_and_restate(argv)
    assert imgs.shape == (40, 3, 224, 224)
    with torch.no_grad():
        p64 = torch.softmax(ref(imgs.double()), dim=1)
    _assert_score(got, p64, 4)
