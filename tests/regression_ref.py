"""Test-side twin of the attribute regressor (networks.RegressionNetwork: alexnet / resnet18 / 34 / 50 trunk, 3x3 conv head, global
pooling) and a plain restatement of one training step of regression.py (nn.MSELoss, Adam).  Stock torch modules in any dtype; every
ReLU / LeakyReLU, the max poolings and the GLOBAL max pooling are oracle.networks_ref's taped ones, so DecisionTape.replay works on it.
State-dict keys are the reference's: base.* and cnn.0 / cnn.1 / cnn.3 ...  Pinned to the reference itself by
tests/golden/regression_step.npz (tests/test_regression.py)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import classifier_ref as C
from classifier_ref import adam_update  # noqa: F401  (the restated Adam update is the classifier's)
from oracle import networks_ref as N


class ResNetTrunkRef(nn.Module):
    """reference models/networks.py:1310-1354: the torchvision-style net without `fc`, keys model.conv1.weight ..."""

    def __init__(self, which='resnet18'):
        super().__init__()
        block, layers = C.ARCH[which]
        model = C.ResNetRef(block, layers, 1)
        del model.fc
        self.model = model
        self.feature_dim = 512 * block.expansion

    def forward(self, x):
        m = self.model
        x = m.maxpool(m.relu(m.bn1(m.conv1(x))))
        return m.layer4(m.layer3(m.layer2(m.layer1(x))))


def base_ref(which):
    return N.AlexNetFeatureRef(3, 'None') if which == 'alexnet' else ResNetTrunkRef(which)


class RegressionNetworkRef(nn.Module):
    """reference models/networks.py:1087-1119"""

    def __init__(self, base, pooling='avg', cnn_dim=(64, 1), cnn_pad=1, cnn_relu_slope=0.2):
        super().__init__()
        self.base, self.pooling = base, pooling
        if cnn_dim:
            blk, prev = [], base.feature_dim
            for nf in cnn_dim[:-1]:
                blk += [nn.Conv2d(prev, nf, 3, padding=cnn_pad), nn.BatchNorm2d(nf), N.TapedLeakyReLU(cnn_relu_slope)]
                prev = nf
            self.cnn = nn.Sequential(*blk, nn.Conv2d(prev, cnn_dim[-1], 3, padding=cnn_pad))
            self.feature_dim = cnn_dim[-1]
        else:
            self.cnn = None
            self.feature_dim = base.feature_dim

    def forward(self, x):
        out = self.base(x)
        if self.cnn is not None:
            out = self.cnn(out)
        if self.pooling == 'avg':
            return F.avg_pool2d(out, out.size(2))
        if self.pooling == 'max':
            return N.global_max_pool(out)
        return out


# ---- the training step, restated ---------------------------------------------------------------------------------------------------
def mse(pred, target):
    """nn.MSELoss()(pred, target), written out"""
    d = pred.reshape(-1) - target.reshape(-1).to(pred.dtype)
    return (d * d).sum() / d.numel()


def within(pred, target, delta):
    """the reference's get_accuracy (regression.py:186-188): one flag per predicted value"""
    return (torch.abs(pred.detach().cpu() - target.cpu()) < delta).view(-1)


def train_step(net, x, target, lr=2e-4):
    """one iteration of regression.py:357-366 on the twin from a zero Adam state: (pred, loss, {name: gradient}, {name: parameter after
    the step}); the net's parameters are left as they were, its running statistics move"""
    net.train()
    net.zero_grad()
    pred = net(x)
    loss = mse(pred, target)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    after = {k: adam_update(p.detach(), grads[k], lr) for k, p in net.named_parameters()}
    return pred.detach(), loss.detach(), grads, after
