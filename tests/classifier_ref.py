"""Test-side twin of the attribute classifier (networks.ResNet: resnet18 / 34 / 50 with avgpool + fc) and a plain restatement of one
training step of classification.py (weighted cross entropy, Adam).  Stock torch modules in any dtype; every ReLU and the max pooling are
oracle.networks_ref's taped ones, so DecisionTape.replay works on it.  State-dict keys are the reference's: model.conv1.weight ...
model.fc.bias.  Pinned to the reference itself by tests/golden/classification_step.npz (tests/test_classification_golden.py)."""
import torch
import torch.nn as nn

from oracle import networks_ref as N


class BottleneckRef(nn.Module):
    """reference models/resnet.py:76-122 (dropout 0: the drop layers are identities)"""
    expansion = 4

    def __init__(self, cin, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = N.TapedReLU(inplace=False)
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        return self.relu(self.bn3(self.conv3(out)) + idt)


class _BasicRef(N.BasicBlockRef):
    expansion = 1


class ResNetRef(nn.Module):
    """reference models/resnet.py:125-196"""

    def __init__(self, block, layers, num_classes):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = N.TapedReLU(inplace=False)
        self.maxpool = N.TapedMaxPool2d(3, stride=2, padding=1)
        cin = 64
        for li, (planes, n, stride) in enumerate(zip((64, 128, 256, 512), layers, (1, 2, 2, 2)), 1):
            blocks = []
            for b in range(n):
                s = stride if b == 0 else 1
                down = None
                if s != 1 or cin != planes * block.expansion:
                    down = nn.Sequential(nn.Conv2d(cin, planes * block.expansion, 1, stride=s, bias=False),
                                         nn.BatchNorm2d(planes * block.expansion))
                blocks.append(block(cin, planes, s, down))
                cin = planes * block.expansion
            setattr(self, 'layer%d' % li, nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(cin, num_classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(self.avgpool(x).flatten(1))


ARCH = {'resnet18': (_BasicRef, (2, 2, 2, 2)), 'resnet34': (_BasicRef, (3, 4, 6, 3)), 'resnet50': (BottleneckRef, (3, 4, 6, 3))}


class ResNetClassifierRef(nn.Module):
    """reference models/networks.py:1258-1285"""

    def __init__(self, which='resnet18', num_classes=5):
        super().__init__()
        block, layers = ARCH[which]
        self.model = ResNetRef(block, layers, num_classes)

    def forward(self, x):
        return self.model(x)


# ---- the training step, restated ---------------------------------------------------------------------------------------------------
def cross_entropy(logits, labels, weight=None):
    """nn.CrossEntropyLoss(weight)(logits, labels), mean reduction, written out: sum_n w[y_n] (-log_softmax(l_n)[y_n]) / sum_n w[y_n]"""
    z = logits - logits.max(dim=1, keepdim=True).values
    logp = z - z.exp().sum(dim=1, keepdim=True).log()
    w = torch.ones(logits.shape[1], dtype=logits.dtype) if weight is None else weight.to(logits.dtype)
    wy = w[labels]
    return -(wy * logp[torch.arange(logits.shape[0]), labels]).sum() / wy.sum()


def cross_entropy_grad(logits, labels, weight=None):
    """d cross_entropy / d logits in closed form: w[y_n] (softmax(l_n) - onehot(y_n)) / sum_n w[y_n]"""
    p = torch.softmax(logits, dim=1)
    w = torch.ones(logits.shape[1], dtype=logits.dtype) if weight is None else weight.to(logits.dtype)
    wy = w[labels]
    onehot = torch.zeros_like(p)
    onehot[torch.arange(logits.shape[0]), labels] = 1
    return wy[:, None] * (p - onehot) / wy.sum()


def predictions(logits):
    """the reference's get_prediction: numpy's argmax (the first maximum) of every row"""
    return torch.from_numpy(logits.detach().cpu().numpy().argmax(axis=1))


def adam_update(param, grad, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, step=1, exp_avg=None, exp_avg_sq=None):
    """torch.optim.Adam's update of one tensor at step `step` (zero state when none is given); returns the new parameter"""
    m = torch.zeros_like(param) if exp_avg is None else exp_avg
    v = torch.zeros_like(param) if exp_avg_sq is None else exp_avg_sq
    m = betas[0] * m + (1 - betas[0]) * grad
    v = betas[1] * v + (1 - betas[1]) * grad * grad
    mhat = m / (1 - betas[0] ** step)
    vhat = v / (1 - betas[1] ** step)
    return param - lr * mhat / (vhat.sqrt() + eps)


def train_step(net, x, labels, weight=None, lr=2e-4):
    """one iteration of classification.py:374-384 on the twin from a zero Adam state: (logits, loss, {name: gradient},
    {name: parameter after the step}); the net's parameters are left as they were, its running statistics move"""
    net.train()
    net.zero_grad()
    logits = net(x)
    loss = cross_entropy(logits, labels, weight)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    after = {k: adam_update(p.detach(), grads[k], lr) for k, p in net.named_parameters()}
    return logits.detach(), loss.detach(), grads, after
