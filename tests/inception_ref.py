"""CPU oracle of the Inception-v3 feature network behind the reference's models/inception.py (InceptionV3 over the blocks of
torchvision's inception_v3(pretrained=True)), restated with stock torch ops and torchvision's module and state_dict key names.

torchvision is not a dependency here, so its Inception3 is restated from the published architecture (Szegedy et al. 2016, and
torchvision's published module layout): BasicConv2d = Conv2d(bias=False) + BatchNorm2d(eps=0.001) + ReLU; InceptionA / C / E pool
branches are avg_pool2d(3, 1, 1) with count_include_pad=True, InceptionB / D ones max_pool2d(3, 2).  AuxLogits and fc are kept so that
the parameter count (27,161,264, torchvision's published figure for inception_v3) pins every kernel shape and channel count.
`.double()` gives the float64 twin."""
import torch
import torch.nn as nn
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b5 = self.branch5x5_2(self.branch5x5_1(x))
        b3 = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b5, b3, bp], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3(x)
        bd = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = x
        for i in range(1, 6):
            bd = getattr(self, 'branch7x7dbl_%d' % i)(bd)
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b7, bd, bp], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3_2(self.branch3x3_1(x))
        b7 = x
        for i in range(1, 5):
            b7 = getattr(self, 'branch7x7x3_%d' % i)(b7)
        return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b3 = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(b3), self.branch3x3_2b(b3)], 1)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(bd), self.branch3x3dbl_3b(bd)], 1)
        bp = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b3, bd, bp], 1)


class InceptionAux(nn.Module):
    def __init__(self, cin, num_classes):
        super().__init__()
        self.conv0 = BasicConv2d(cin, 128, kernel_size=1)
        self.conv1 = BasicConv2d(128, 768, kernel_size=5)
        self.fc = nn.Linear(768, num_classes)


class Inception3Ref(nn.Module):
    """torchvision's Inception3 (aux_logits=True, 1000 classes) as far as its parameters and the feature path go"""

    def __init__(self, num_classes=1000):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, pool_features=32)
        self.Mixed_5c = InceptionA(256, pool_features=64)
        self.Mixed_5d = InceptionA(288, pool_features=64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, channels_7x7=128)
        self.Mixed_6c = InceptionC(768, channels_7x7=160)
        self.Mixed_6d = InceptionC(768, channels_7x7=160)
        self.Mixed_6e = InceptionC(768, channels_7x7=192)
        self.AuxLogits = InceptionAux(768, num_classes)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.fc = nn.Linear(2048, num_classes)


def feature_blocks(net):
    """the reference InceptionV3's four blocks (models/inception.py:68-110) as callables"""
    return [
        lambda x: F.max_pool2d(net.Conv2d_2b_3x3(net.Conv2d_2a_3x3(net.Conv2d_1a_3x3(x))), kernel_size=3, stride=2),
        lambda x: F.max_pool2d(net.Conv2d_4a_3x3(net.Conv2d_3b_1x1(x)), kernel_size=3, stride=2),
        lambda x: net.Mixed_6e(net.Mixed_6d(net.Mixed_6c(net.Mixed_6b(net.Mixed_6a(net.Mixed_5d(net.Mixed_5c(net.Mixed_5b(x)))))))),
        lambda x: F.adaptive_avg_pool2d(net.Mixed_7c(net.Mixed_7b(net.Mixed_7a(x))), (1, 1)),
    ]


def prepare_input(x, resize_input=True, normalize_input=True):
    """the reference forward's input steps: F.upsample(size=299, bilinear) -- align_corners=False on current torch -- and
    normalize_input (models/inception.py:137-144)"""
    if resize_input:
        x = F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False)
    if normalize_input:
        x = x.clone()
        for c in range(3):
            x[:, c] = x[:, c] * (STD[c] / 0.5) + (MEAN[c] - 0.5) / 0.5
    return x


@torch.no_grad()
def forward_ref(net, x, output_blocks=(3,), resize_input=True, normalize_input=True):
    """list of the requested block outputs, as the reference InceptionV3.forward"""
    x = prepare_input(x, resize_input, normalize_input)
    out, last = [], max(output_blocks)
    for idx, block in enumerate(feature_blocks(net)):
        x = block(x)
        if idx in output_blocks:
            out.append(x)
        if idx == last:
            break
    return out


def random_state_dict(seed, num_classes=1000):
    """seeded torchvision-layout state_dict with non-trivial BatchNorm statistics: He-scaled conv weights, gamma in [0.6, 1.4],
    beta in [-0.2, 0.2], running mean in [-0.2, 0.2], running var in [0.5, 1.5] (keeps activations O(1) through the 94 layers)"""
    g = torch.Generator().manual_seed(seed)
    net = Inception3Ref(num_classes)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.zeros_like(v)
        elif k.endswith('conv.weight'):
            fan_in = v[0].numel()
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif k.endswith('bn.weight'):
            sd[k] = 0.6 + 0.8 * torch.rand(v.shape, generator=g)
        elif k.endswith('bn.bias') or k.endswith('running_mean'):
            sd[k] = 0.4 * torch.rand(v.shape, generator=g) - 0.2
        elif k.endswith('running_var'):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.01
    return sd


def make_ref(sd=None, seed=0, dtype=torch.float32):
    net = Inception3Ref()
    net.load_state_dict(sd if sd is not None else random_state_dict(seed))
    return net.to(dtype).eval()
