"""Network factories of the PC-GAN hot path on the HIP layer set.

Same plugin surface as the reference's models/networks.py for the part of the zoo that the
wsgan_emb / wsgan_cycle configurations reach:
define_G / define_D / define_E / define_IP / define_AR, get_norm_layer, init_weights, init_net,
get_scheduler, GANLoss, and the module classes with the reference's nn.Sequential index
layout, so state_dict keys are identical (`model.10.conv_block.1.weight`, `model.2.running_mean`,
...).  Architectures outside that scope raise NotImplementedError naming themselves.
"""
import functools

import numpy as np
import torch
import torch.nn as tnn
from torch.nn import init
from torch.optim import lr_scheduler

from ..hip import functional as HF
from ..hip import nn as hnn
from ..hip.nn import IdentityMapping, run_sequential  # noqa: F401  (IdentityMapping is part of the surface)

MAGIC_EPS = 1e-20


# ------------------------------------------------------------------------- helpers
def get_norm_layer(norm_type='instance'):
    """reference models/networks.py:22-34"""
    if norm_type == 'batch':
        return functools.partial(hnn.BatchNorm2d, affine=True)
    if norm_type == 'instance':
        return functools.partial(hnn.InstanceNorm2d, affine=False, track_running_stats=True)
    if norm_type == 'none':
        return IdentityMapping
    raise NotImplementedError('normalization layer [%s] is not found' % norm_type)


def _is_instance_norm(norm_layer):
    f = norm_layer.func if isinstance(norm_layer, functools.partial) else norm_layer
    return f is hnn.InstanceNorm2d or f is tnn.InstanceNorm2d


def get_dropout_layer(dropout=0.):
    """reference models/networks.py:37-42"""
    return functools.partial(hnn.Dropout2d, p=dropout) if dropout > 0 else IdentityMapping


def get_scheduler(optimizer, opt):
    """reference models/networks.py:57-69"""
    if opt.lr_policy == 'lambda':
        def lambda_rule(epoch):
            return 1.0 - max(0, epoch + 1 + opt.epoch_count - opt.niter) / float(opt.niter_decay + 1)
        return lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda_rule)
    if opt.lr_policy == 'step':
        return lr_scheduler.StepLR(optimizer, step_size=opt.lr_decay_iters, gamma=0.1)
    if opt.lr_policy == 'plateau':
        return lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor=0.2, threshold=0.01, patience=5)
    # the reference RETURNS (does not raise) this object; keep the observable behaviour
    return NotImplementedError('learning rate policy [%s] is not implemented', opt.lr_policy)


_WEIGHT_FILLERS = {
    # --init_type -> in-place filler of a Conv / Linear weight (the draws consume torch's global generator exactly as the
    # reference's torch.nn.init calls do, so seeded initialisations coincide)
    'normal': lambda w, gain: init.normal_(w, 0.0, gain),
    'xavier': lambda w, gain: init.xavier_normal_(w, gain=gain),
    'kaiming': lambda w, gain: init.kaiming_normal_(w, a=0, mode='fan_in'),
    'orthogonal': lambda w, gain: init.orthogonal_(w, gain=gain),
}


def init_weights(net, init_type='normal', gain=0.02):
    """Initialisation rule of the reference (models/networks.py:72-93), by module class NAME as there: anything whose
    class name contains 'Conv' or 'Linear' and owns a weight gets the `init_type` filler and a zero bias; anything named
    *BatchNorm2d* gets weight ~ N(1, gain), bias 0; an unknown init_type raises when the first such layer is met."""
    fill = _WEIGHT_FILLERS.get(init_type)

    def visit(module):
        name = type(module).__name__
        if ('Conv' in name or 'Linear' in name) and hasattr(module, 'weight'):
            if fill is None:
                raise NotImplementedError('initialization method [%s] is not implemented' % init_type)
            fill(module.weight.data, gain)
            if getattr(module, 'bias', None) is not None:
                module.bias.data.zero_()
        elif 'BatchNorm2d' in name:
            init.normal_(module.weight.data, 1.0, gain)
            module.bias.data.zero_()

    print('initialize network with %s' % init_type)
    net.apply(visit)
    from ..hip import ops            # .data writes do not bump tensor versions: drop packed-weight copies
    ops.invalidate_packed_weights()


def init_net(net, init_type='normal', gpu_ids=[]):
    """reference models/networks.py:96-102.  One process drives one GPU here: the net moves to
    gpu_ids[0]; data parallelism is the per-rank replica + RCCL gradient all-reduce of
    pcgan_amd.hip.parallel, not nn.DataParallel."""
    if len(gpu_ids) > 0:
        assert torch.cuda.is_available()
        net.to(torch.device('cuda', gpu_ids[0]))
    init_weights(net, init_type)
    return net


# ------------------------------------------------------------------------- factories
def define_G(input_nc, output_nc, nz, ngf, which_model_netG='unet_128', norm='batch', nl='relu',
             dropout=0, init_type='xavier', gpu_ids=[], upsample='bilinear', size=512, embed_size=256, n_layers_G=7):
    """reference models/networks.py:106-143.  `resnet_<n>blocks` for any n (the reference names
    only 6 and 9; BASELINE config 1 needs 2); `unet` (n_layers_G downsamplings, >= 5) and `unet_256` (8)."""
    norm_layer = get_norm_layer(norm_type=norm)
    if which_model_netG.startswith('resnet_') and which_model_netG.endswith('blocks'):
        try:
            n_blocks = int(which_model_netG[len('resnet_'):-len('blocks')])
        except ValueError:
            raise NotImplementedError('Generator model name [%s] is not recognized' % which_model_netG)
        netG = ResnetGenerator(input_nc, output_nc, nz, ngf, norm_layer=norm_layer, dropout=dropout, n_blocks=n_blocks)
    elif which_model_netG == 'unet':
        if n_layers_G < 5:
            raise ValueError('Generator [unet] needs --n_layers_G >= 5 (the four widening blocks and the bottleneck), got %r' % (n_layers_G,))
        netG = UnetGenerator(input_nc, output_nc, nz, n_layers_G, ngf, norm_layer=norm_layer, dropout=dropout)
    elif which_model_netG == 'unet_256':
        netG = UnetGenerator(input_nc, output_nc, nz, 8, ngf, norm_layer=norm_layer, dropout=dropout)
    elif which_model_netG == 'unet_128':
        raise NotImplementedError('Generator [unet_128] is not a name of the MI355X hot path; use --which_model_netG unet --n_layers_G 7, '
                                  'the same network (7 downsamplings: 128 x 128 -> 1 x 1)')
    elif which_model_netG in ('unet_128_input', 'unet_128_all', 'unet_256_input', 'unet_256_all', 'gan_stability', 'mnist_fc',
                              'unet_all'):
        raise NotImplementedError('Generator [%s] is outside the MI355X hot path (SURVEY.md section 8); '
                                  'use resnet_<n>blocks, unet or unet_256' % which_model_netG)
    else:
        raise NotImplementedError('Generator model name [%s] is not recognized' % which_model_netG)
    return init_net(netG, init_type, gpu_ids)


def define_D(input_nc, nz, ndf, which_model_netD, n_layers_D=3, norm='batch', use_sigmoid=False, init_type='normal',
             num_Ds=1, gpu_ids=[], use_projection=True, size=512, embed_size=256, num_classes=1):
    """reference models/networks.py:147-175"""
    norm_layer = get_norm_layer(norm_type=norm)
    if which_model_netD == 'basic':
        netD = NLayerDiscriminator(input_nc, nz, ndf, n_layers=3, norm_layer=norm_layer, use_sigmoid=use_sigmoid)
    elif which_model_netD == 'n_layers':
        netD = NLayerDiscriminator(input_nc, nz, ndf, n_layers_D, norm_layer=norm_layer, use_sigmoid=use_sigmoid)
    elif which_model_netD == 'n_layers_proj':
        netD = NLayerProjectionDiscriminator(input_nc, nz, ndf, n_layers_D, norm_layer=norm_layer, use_sigmoid=use_sigmoid,
                                             proj=use_projection)
    elif which_model_netD == 'n_layers_multi':
        if nz >= 1:
            raise NotImplementedError('Discriminator [n_layers_multi] with a rating (nz = %d) is outside the MI355X hot path (SURVEY.md '
                                      'section 8): the reference\'s multi-scale discriminator is unconditional -- it drops nz and its '
                                      'forward takes the image alone; use it with --model wsgan_cycle, or basic / n_layers here' % nz)
        netD = D_NLayersMulti(input_nc, ndf, n_layers=n_layers_D, norm_layer=norm_layer, use_sigmoid=use_sigmoid, gpu_ids=gpu_ids,
                              num_D=num_Ds)
    elif which_model_netD in ('pixel', 'pyramid', 'gan_stability', 'gan_stability_class', 'mnist_fc'):
        raise NotImplementedError('Discriminator [%s] is outside the MI355X hot path (SURVEY.md section 8); '
                                  'use basic / n_layers' % which_model_netD)
    else:
        raise NotImplementedError('Discriminator model name [%s] is not recognized' % which_model_netD)
    return init_net(netD, init_type, gpu_ids)


def define_IP(which_model_netIP, input_nc, gpu_ids=[]):
    """reference models/networks.py:179-193 (weights are not initialised here: they are loaded)."""
    if which_model_netIP == 'alexnet':
        netIP = AlexNetFeature(input_nc=input_nc, pooling='None')
    elif 'vgg' in which_model_netIP:
        raise NotImplementedError('Identity-preserving net [%s] is outside the MI355X hot path' % which_model_netIP)
    else:
        raise NotImplementedError('Identity-preserving model name [%s] is not recognized' % which_model_netIP)
    if len(gpu_ids) > 0:
        assert torch.cuda.is_available()
        netIP.to(torch.device('cuda', gpu_ids[0]))
    return netIP


def define_E(which_model_netE, input_nc=3, init_type='kaiming', pooling='max', cnn_dim=[], cnn_pad=1,
             cnn_relu_slope=0.2, gpu_ids=[], fine_size_E=224, noisy=False, bnn_dropout=0.):
    """reference models/networks.py:232-253"""
    drop_layer = get_dropout_layer(dropout=bnn_dropout)
    if which_model_netE == 'alexnet':
        base = AlexNetFeature(input_nc=input_nc, pooling='None')
    elif 'resnet' in which_model_netE:
        base = ResNetFeature(input_nc=input_nc, which_model=which_model_netE, dropout=bnn_dropout)
    elif which_model_netE in ('DTN', 'mnist_fc'):
        raise NotImplementedError('Encoder base [%s] is outside the MI355X hot path' % which_model_netE)
    else:
        raise NotImplementedError('Model [%s] is not implemented.' % which_model_netE)
    netE = SiameseFeature(base, pooling=pooling, cnn_dim=cnn_dim, cnn_pad=cnn_pad, cnn_relu_slope=cnn_relu_slope,
                          noisy=noisy, drop_layer=drop_layer)
    return init_net(netE, init_type, gpu_ids)


def define_AC(which_model_netAC, input_nc=3, init_type='normal', num_classes=0, pooling='avg', dropout=0.5, gpu_ids=[]):
    """reference models/networks.py:197-209: the auxiliary classifier of the class-label baseline.  `pooling` and `dropout` reach only
    the reference's AlexNetLite; its ResNet ignores them, and so does this one."""
    if which_model_netAC in ('resnet18', 'resnet34', 'resnet50'):
        netAC = ResNet(input_nc=input_nc, num_classes=num_classes, which_model=which_model_netAC)
    elif which_model_netAC in ('alexnet', 'alexnet_lite') or 'resnet' in which_model_netAC:
        raise NotImplementedError('Auxiliary classifier [%s] is outside the MI355X hot path; use resnet18, resnet34 or resnet50'
                                  % which_model_netAC)
    else:
        raise NotImplementedError('Auxiliary classifier name [%s] is not recognized' % which_model_netAC)
    return init_net(netAC, init_type, gpu_ids)


def define_AR(which_model_netAR, input_nc=3, init_type='kaiming', pooling='max', cnn_dim=[], cnn_pad=1, cnn_relu_slope=0.2,
              gpu_ids=[]):
    """reference models/networks.py:213-228: the auxiliary regressor of the continuous-label baseline"""
    if which_model_netAR == 'alexnet':
        base = AlexNetFeature(input_nc=input_nc, pooling='None')
    elif which_model_netAR in ('resnet18', 'resnet34', 'resnet50'):
        base = ResNetFeature(input_nc=input_nc, which_model=which_model_netAR)
    elif 'resnet' in which_model_netAR:
        raise NotImplementedError('Regressor base [%s] is outside the MI355X hot path; use alexnet, resnet18, resnet34 or resnet50'
                                  % which_model_netAR)
    else:
        raise NotImplementedError('Model [%s] is not implemented.' % which_model_netAR)
    netAR = RegressionNetwork(base, pooling=pooling, cnn_dim=cnn_dim, cnn_pad=cnn_pad, cnn_relu_slope=cnn_relu_slope)
    return init_net(netAR, init_type, gpu_ids)


# ------------------------------------------------------------------------- losses
class GANLoss(tnn.Module):
    """reference models/networks.py:386-420: BCE (or MSE when use_lsgan) against a per-sample
    target (bool, list of 0/1 per sample, or -- extension -- a float device tensor [N])."""

    def __init__(self, use_lsgan=True, tensor=torch.FloatTensor):
        super().__init__()
        self.use_lsgan = use_lsgan
        self.Tensor = tensor
        self._const = {}

    def get_target_vector(self, input, target_label):
        if isinstance(target_label, torch.Tensor):
            return target_label.to(device=input.device, dtype=torch.float32).reshape(-1)
        if not isinstance(target_label, (list, tuple)):
            target_label = [target_label]
        vals = tuple(float(1 if t is True else (0 if t is False else t)) for t in target_label)
        key = (vals, input.device)
        if key not in self._const:   # tiny host->device copies, cached so that the step stays async
            self._const[key] = torch.tensor(np.array(vals, dtype=np.float32), device=input.device)
        return self._const[key]

    def get_target_tensor(self, input, target_label):
        t = self.get_target_vector(input, target_label)
        return t.reshape(-1, 1, 1, 1).expand_as(input)

    def __call__(self, inputs, target_label):
        if not isinstance(inputs, list):
            inputs = [inputs]
        loss = 0.0
        for input in inputs:
            if input.dim() < 4:
                input = input.view(input.size(0), -1, 1, 1)
            t = self.get_target_vector(input, target_label)
            if t.numel() == 1 and input.size(0) != 1:
                t = t.expand(input.size(0)).contiguous()
            if self.use_lsgan:
                loss = loss + HF.mse_loss(input, t.reshape(-1, 1, 1, 1).expand_as(input).contiguous())
            else:
                loss = loss + HF.bce_loss(input, t)
        return loss


class L1Loss(tnn.Module):
    """nn.L1Loss() of the reference model (models/wsgan_emb_model.py:141,149) on the HIP reduction."""

    def forward(self, a, b):
        return HF.l1_loss(a, b.detach())


class MSELoss(tnn.Module):
    """nn.MSELoss() (models/wsgan_emb_model.py:143,148)."""

    def forward(self, a, b):
        return HF.mse_loss(a, b.detach())


# ------------------------------------------------------------------------- generator
class ResnetGenerator(tnn.Module):
    """reference models/networks.py:565-612.  Sequential index layout (9 blocks):
    [0]RefPad3 [1]Conv7 [2]IN [3]ReLU [4]Conv3s2 [5]IN [6]ReLU [7]Conv3s2 [8]IN [9]ReLU
    [10..18]ResnetBlock [19]ConvT [20]IN [21]ReLU [22]ConvT [23]IN [24]ReLU [25]RefPad3 [26]Conv7 [27]Tanh."""

    def __init__(self, input_nc, output_nc, nz=0, ngf=64, norm_layer=hnn.BatchNorm2d, dropout=0, n_blocks=6,
                 padding_type='reflect'):
        assert n_blocks >= 0
        super().__init__()
        if dropout > 0:
            raise NotImplementedError('pcgan_amd: generator nn.Dropout (--dropout > 0) is outside the hot path')
        input_nc = input_nc + nz
        self.input_nc, self.output_nc, self.ngf, self.nz = input_nc, output_nc, ngf, nz
        use_bias = _is_instance_norm(norm_layer)
        model = [tnn.ReflectionPad2d(3), hnn.Conv2d(input_nc, ngf, kernel_size=7, padding=0, bias=use_bias),
                 norm_layer(ngf), tnn.ReLU(True)]
        for i in range(2):
            mult = 2 ** i
            model += [hnn.Conv2d(ngf * mult, ngf * mult * 2, kernel_size=3, stride=2, padding=1, bias=use_bias),
                      norm_layer(ngf * mult * 2), tnn.ReLU(True)]
        for _ in range(n_blocks):
            model += [ResnetBlock(ngf * 4, padding_type=padding_type, norm_layer=norm_layer, dropout=dropout,
                                  use_bias=use_bias)]
        for i in range(2):
            mult = 2 ** (2 - i)
            model += [hnn.ConvTranspose2d(ngf * mult, ngf * mult // 2, kernel_size=3, stride=2, padding=1,
                                          output_padding=1, bias=use_bias),
                      norm_layer(ngf * mult // 2), tnn.ReLU(True)]
        model += [tnn.ReflectionPad2d(3), hnn.Conv2d(ngf, output_nc, kernel_size=7, padding=0), tnn.Tanh()]
        self.model = tnn.Sequential(*model)

    def forward(self, input, z=None):
        x = HF.concat_z(input, z) if z is not None else input
        return run_sequential(self.model, x)


class ResnetBlock(tnn.Module):
    """reference models/networks.py:616-652: x + conv_block(x); the skip add is fused into the
    second InstanceNorm's apply pass."""

    def __init__(self, dim, padding_type, norm_layer, dropout, use_bias):
        super().__init__()
        if padding_type not in ('reflect', 'zero'):
            raise NotImplementedError('padding [%s] is not implemented' % padding_type)
        blk = []
        for half in range(2):
            p = 0
            if padding_type == 'reflect':
                blk += [tnn.ReflectionPad2d(1)]
            else:
                p = 1
            blk += [hnn.Conv2d(dim, dim, kernel_size=3, padding=p, bias=use_bias), norm_layer(dim)]
            if half == 0:
                blk += [tnn.ReLU(True)]
        self.conv_block = tnn.Sequential(*blk)
        # the composite call (hip/functional.py: _ResBlockFn) covers the reference's default block -- reflection padding,
        # InstanceNorm: [RefPad, Conv, IN, ReLU, RefPad, Conv, IN]; any other layout runs layer by layer
        self._composite_layout = (padding_type == 'reflect' and len(blk) == 7 and isinstance(blk[2], hnn.InstanceNorm2d)
                                  and isinstance(blk[6], hnn.InstanceNorm2d))

    def forward(self, x):
        if self._composite_layout:
            cb = self.conv_block
            pl = HF.resblock_composite_ok(x, cb[1], cb[5], cb[2], cb[6])
            if pl is not None:
                return HF.resblock(x, cb[1], cb[5], cb[2], cb[6], pl)
        return run_sequential(self.conv_block, x, residual=x)


class UnetGenerator(tnn.Module):
    """reference models/networks.py:659-677: z broadcast over the image and concatenated, then `num_downs` nested
    UnetSkipConnectionBlocks -- from the inside out: the bottleneck (ngf*8 -> ngf*8), num_downs - 5 more of that width, ngf*4, ngf*2, ngf,
    and the outermost block (output_nc, ngf) reading input_nc + nz channels.  state_dict keys model.model.0.weight,
    model.model.1.model.1.weight, ... as there.  The input side must be a positive multiple of 2**num_downs (a 1 x 1 bottleneck at
    exactly that side)."""

    def __init__(self, input_nc, output_nc, nz=0, num_downs=7, ngf=64, norm_layer=hnn.BatchNorm2d, dropout=0):
        super().__init__()
        if dropout > 0:
            raise NotImplementedError('pcgan_amd: generator nn.Dropout (--dropout > 0) is outside the hot path')
        if num_downs < 5:
            raise ValueError('pcgan_amd: UnetGenerator needs num_downs >= 5, got %r' % (num_downs,))
        self.input_nc, self.output_nc, self.ngf, self.nz, self.num_downs = input_nc + nz, output_nc, ngf, nz, num_downs
        block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, norm_layer=norm_layer, innermost=True)
        for _ in range(num_downs - 5):
            block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, submodule=block, norm_layer=norm_layer, dropout=dropout)
        for mult in (4, 2, 1):
            block = UnetSkipConnectionBlock(ngf * mult, ngf * mult * 2, submodule=block, norm_layer=norm_layer)
        self.model = UnetSkipConnectionBlock(output_nc, ngf, input_nc=input_nc + nz, submodule=block, outermost=True, norm_layer=norm_layer)

    def forward(self, input, z=None):
        side = 1 << self.num_downs
        for s in (input.shape[2], input.shape[3]):
            if s < side or s % side != 0:
                raise ValueError('pcgan_amd: UnetGenerator input side %d is not a positive multiple of %d = 2**num_downs (num_downs = %d)'
                                 % (s, side, self.num_downs))
        return self.model(HF.concat_z(input, z) if z is not None else input)


def _norm_then_act(norm, x, act=hnn.ACT_NONE, slope=0.0):
    """norm(x) with the following activation inside the normalisation pass; norm 'none' (IdentityMapping) leaves the activation alone"""
    if isinstance(norm, (hnn.InstanceNorm2d, hnn.BatchNorm2d)):
        return norm(x, act, slope)
    return HF.activation(norm(x), act, slope)


class UnetSkipConnectionBlock(tnn.Module):
    """reference models/networks.py:683-733.  Sequential layouts (the indices are the state_dict keys):
      outermost  [0]Conv4s2 [1]sub [2]ReLU [3]ConvT4s2 (bias always) [4]Tanh
      middle     [0]LeakyReLU(0.2) [1]Conv4s2 [2]norm [3]sub [4]ReLU [5]ConvT4s2 [6]norm
      innermost  [0]LeakyReLU(0.2) [1]Conv4s2 [2]ReLU [3]ConvT4s2 [4]norm
    A block that is not the outermost returns cat(t, up(down(t))) with t = LeakyReLU(x): the reference's first module rewrites x in
    place, so the skip carries t, not x.  Its parent's ReLU then acts on that whole concatenation.  Here every activation runs inside
    the kernel that produces its operand -- LeakyReLU in the epilogue of the convolution or normalisation above it, ReLU in the
    up-normalisation and, for the skip half, in the join (HF.skip_join) -- so t is written once and read by the down-convolution and
    by the join."""

    def __init__(self, outer_nc, inner_nc, input_nc=None, submodule=None, outermost=False, innermost=False,
                 norm_layer=hnn.BatchNorm2d, dropout=0):
        super().__init__()
        if dropout > 0:
            raise NotImplementedError('pcgan_amd: generator nn.Dropout (--dropout > 0) is outside the hot path')
        if outermost and innermost:
            raise ValueError('pcgan_amd: a UnetSkipConnectionBlock is outermost or innermost, not both')
        if (submodule is None) != bool(innermost):
            raise ValueError('pcgan_amd: exactly the innermost UnetSkipConnectionBlock has no submodule')
        self.outermost, self.innermost = outermost, innermost
        use_bias = _is_instance_norm(norm_layer)
        down = hnn.Conv2d(outer_nc if input_nc is None else input_nc, inner_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
        up_in = inner_nc if innermost else inner_nc * 2
        up = hnn.ConvTranspose2d(up_in, outer_nc, kernel_size=4, stride=2, padding=1, bias=use_bias or outermost)
        # (down before up, as in the reference: a convolution's default initialisation draws from torch's generator; norms draw nothing)
        if outermost:
            seq = [down, submodule, tnn.ReLU(True), up, tnn.Tanh()]
        elif innermost:
            seq = [tnn.LeakyReLU(0.2, True), down, tnn.ReLU(True), up, norm_layer(outer_nc)]
        else:
            seq = [tnn.LeakyReLU(0.2, True), down, norm_layer(inner_nc), submodule, tnn.ReLU(True), up, norm_layer(outer_nc)]
        self.model = tnn.Sequential(*seq)

    def forward(self, x):
        m = self.model
        if self.outermost:
            t = m[0](x, 0, 0, hnn.ACT_LRELU, m[1].model[0].negative_slope)      # the sub-block's LeakyReLU in this epilogue
            return HF.activation(m[3](m[1].joined(t, True)), hnn.ACT_TANH)
        return self.joined(HF.activation(x, hnn.ACT_LRELU, m[0].negative_slope), False)

    def joined(self, t, relu):
        """cat(t, up(down(t))) for t = LeakyReLU(x) already applied by the producer of t; relu: the parent's ReLU folded in (into the
        up-normalisation for the new half, into the join for the skip half)"""
        m = self.model
        act = hnn.ACT_RELU if relu else hnn.ACT_NONE
        if self.innermost:
            u = m[1](t, 0, 0, hnn.ACT_RELU)
            y = _norm_then_act(m[4], m[3](u), act)
        else:
            sub = m[3]
            d = _norm_then_act(m[2], m[1](t), hnn.ACT_LRELU, sub.model[0].negative_slope)
            y = _norm_then_act(m[6], m[5](sub.joined(d, True)), act)
        return HF.skip_join(t, y, act, hnn.ACT_NONE)


# ------------------------------------------------------------------------- discriminator
class NLayerDiscriminator(tnn.Module):
    """reference models/networks.py:737-783: conditional PatchGAN; k4 convs (s2 x n_layers, s1, s1)."""

    def __init__(self, input_nc, nz, ndf=64, n_layers=3, norm_layer=hnn.BatchNorm2d, use_sigmoid=False):
        super().__init__()
        use_bias = _is_instance_norm(norm_layer)
        seq = [hnn.Conv2d(input_nc + nz, ndf, kernel_size=4, stride=2, padding=1), tnn.LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            seq += [hnn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=2, padding=1, bias=use_bias),
                    norm_layer(ndf * mult), tnn.LeakyReLU(0.2, True)]
        prev, mult = mult, min(2 ** n_layers, 8)
        seq += [hnn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=1, padding=1, bias=use_bias),
                norm_layer(ndf * mult), tnn.LeakyReLU(0.2, True)]
        seq += [hnn.Conv2d(ndf * mult, 1, kernel_size=4, stride=1, padding=1)]
        if use_sigmoid:
            seq += [tnn.Sigmoid()]
        self.model = tnn.Sequential(*seq)

    def forward(self, input, z=None):
        x = HF.concat_z(input, z) if z is not None else input
        return run_sequential(self.model, x)


class HeadConv2d(tnn.Conv2d):
    """The parameters of a 1x1 convolution of the projection head -- the reference's key names, shapes, constructor draws and (by its
    class name) init_weights rule -- whose arithmetic lives in the head kernel (HF.projection_head): it is never called as a layer."""

    def forward(self, x):
        raise RuntimeError('pcgan_amd: HeadConv2d only holds parameters; the projection head kernel computes with them')


class NLayerProjectionDiscriminator(tnn.Module):
    """reference models/networks.py:787-838 with proj=True ("cGANs with Projection Discriminator"): phi = NLayerDiscriminator's trunk
    without its last convolution, applied to the image alone; out[B,1,3,3] = sum_c h wy + psi(h) with h the plane SUMS of phi's output,
    wy = l_y(y), psi a 1x1 convolution with padding 1 (so only the centre cell sees h).  state_dict keys phi.*, psi.*, l_y.*."""

    def __init__(self, input_nc, nz, ndf=64, n_layers=3, norm_layer=hnn.BatchNorm2d, use_sigmoid=False, proj=True):
        super().__init__()
        if not proj:
            raise NotImplementedError('NLayerProjectionDiscriminator with use_projection=False (proj=False) is outside the MI355X hot '
                                      'path; use n_layers for the concatenated rating')
        if nz < 1:
            raise NotImplementedError('Discriminator [n_layers_proj] projects a rating (nz >= 1): the unconditional discriminator of '
                                      'wsgan_cycle (nz = %d) cannot be one; use basic / n_layers there' % nz)
        self._proj, self._sigm, self.nz = proj, use_sigmoid, nz
        use_bias = _is_instance_norm(norm_layer)
        seq = [hnn.Conv2d(input_nc, ndf, kernel_size=4, stride=2, padding=1), tnn.LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            seq += [hnn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=2, padding=1, bias=use_bias),
                    norm_layer(ndf * mult), tnn.LeakyReLU(0.2, True)]
        prev, mult = mult, min(2 ** n_layers, 8)
        seq += [hnn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=1, padding=1, bias=use_bias),
                norm_layer(ndf * mult), tnn.LeakyReLU(0.2, True)]
        self.phi = tnn.Sequential(*seq)
        self.psi = HeadConv2d(ndf * mult, 1, kernel_size=1, stride=1, padding=1)
        self.l_y = HeadConv2d(nz, ndf * mult, kernel_size=1, stride=1)

    def forward(self, input, y=None):
        if y is None:
            raise RuntimeError('pcgan_amd: the projection discriminator needs the rating y')
        p = run_sequential(self.phi, input)
        if y.numel() not in (self.nz, p.shape[0] * self.nz):
            raise RuntimeError('pcgan_amd: y of shape %s for batch %d and nz = %d' % (tuple(y.shape), p.shape[0], self.nz))
        return HF.projection_head(p, y.reshape(-1, self.nz), self.psi.weight, self.psi.bias, self.l_y.weight, self.l_y.bias, self._sigm)


class D_NLayersMulti(tnn.Module):
    """reference models/networks.py:1883-1949: the multi-scale PatchGAN.  Unconditional: forward(input) only.  num_D == 1 is one
    Sequential `model` and returns a tensor; num_D > 1 registers `model0`, `model1`, ... on the module itself (the reference's
    ListModule), scale i + 1 judging AvgPool2d(3, stride=2, padding=1, count_include_pad=False) of scale i's image, and returns the
    list of patch maps that GANLoss sums over.  Unlike NLayerDiscriminator EVERY convolution carries a bias, also in front of a batch
    norm, and the widths shrink cumulatively: ndf = int(round(ndf / 2 ** (i + 1))) on the running ndf (64, 32, 8; 16, 8, 2; 8, 4, 1).
    Modules are created in the reference's order, so a seeded construction draws the same initial weights."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=hnn.BatchNorm2d, use_sigmoid=False, gpu_ids=[], num_D=1):
        super().__init__()
        if num_D < 1 or n_layers < 1:
            raise ValueError('pcgan_amd: D_NLayersMulti needs num_D >= 1 and n_layers >= 1, got %r and %r' % (num_D, n_layers))
        self.gpu_ids, self.num_D, self.n_layers = gpu_ids, num_D, n_layers
        if num_D == 1:
            self.model = tnn.Sequential(*self.get_layers(input_nc, ndf, n_layers, norm_layer, use_sigmoid))
            return
        self.add_module('model0', tnn.Sequential(*self.get_layers(input_nc, ndf, n_layers, norm_layer, use_sigmoid)))
        for i in range(num_D - 1):
            ndf = int(round(ndf / (2 ** (i + 1))))
            if ndf < 1:     # (the reference builds convolutions without channels here and dies in its first forward)
                raise ValueError('pcgan_amd: D_NLayersMulti scale %d of %d has no channels left; raise --ndf or lower --num_Ds' % (i + 1, num_D))
            self.add_module('model%d' % (i + 1), tnn.Sequential(*self.get_layers(input_nc, ndf, n_layers, norm_layer, use_sigmoid)))

    @staticmethod
    def get_layers(input_nc, ndf=64, n_layers=3, norm_layer=hnn.BatchNorm2d, use_sigmoid=False):
        seq = [hnn.Conv2d(input_nc, ndf, kernel_size=4, stride=2, padding=1), tnn.LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            seq += [hnn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=2, padding=1), norm_layer(ndf * mult),
                    tnn.LeakyReLU(0.2, True)]
        prev, mult = mult, min(2 ** n_layers, 8)
        seq += [hnn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=1, padding=1), norm_layer(ndf * mult), tnn.LeakyReLU(0.2, True)]
        seq += [hnn.Conv2d(ndf * mult, 1, kernel_size=4, stride=1, padding=1)]
        if use_sigmoid:
            seq += [tnn.Sigmoid()]
        return seq

    def min_side(self):
        """The smallest input side every scale's stack accepts.  A stack halves n_layers times (floor) and then loses one pixel in each
        of its two stride-1 4x4 convolutions, so it needs 3 * 2**n_layers; the pool maps a side s to ceil(s / 2), so each further scale
        asks for 2 * m - 1 in front of it."""
        m = 3 * 2 ** self.n_layers
        for _ in range(self.num_D - 1):
            m = 2 * m - 1
        return m

    def forward(self, input):
        side = min(input.shape[2], input.shape[3])
        if side < self.min_side():
            raise ValueError('pcgan_amd: D_NLayersMulti input %d x %d is too small: with n_layers = %d and num_D = %d the coarsest scale '
                             'needs an input side of at least %d' % (input.shape[2], input.shape[3], self.n_layers, self.num_D, self.min_side()))
        if self.num_D == 1:
            return run_sequential(self.model, input)
        # the image arrives in the model's activation storage type (BaseModel.to_act / the generator's output): the pyramid keeps it,
        # so under --dtype bf16 there is one cast in front of the pyramid and none per scale
        scales = HF.avg_pool_pyramid(input, self.num_D)
        return [run_sequential(getattr(self, 'model%d' % i), x) for i, x in enumerate(scales)]


# ------------------------------------------------------------------------- encoders
class SiameseFeature(tnn.Module):
    """reference models/networks.py:1008-1083: base trunk -> small conv head -> global pooling
    (-> twin `cnn_logvar` head when noisy)."""

    def __init__(self, base=None, pooling='avg', cnn_dim=[], cnn_pad=1, cnn_relu_slope=0.2, noisy=False,
                 drop_layer=None):
        super().__init__()
        self.pooling = pooling
        self.base = base
        self._noisy = noisy
        drop_layer = drop_layer or IdentityMapping

        def head():
            blk, prev = [], base.feature_dim
            for nf in cnn_dim[:-1]:
                blk += [hnn.Conv2d(prev, nf, kernel_size=3, stride=1, padding=cnn_pad, bias=True),
                        hnn.BatchNorm2d(nf), drop_layer(), tnn.LeakyReLU(cnn_relu_slope)]
                prev = nf
            blk += [hnn.Conv2d(prev, cnn_dim[-1], kernel_size=3, stride=1, padding=cnn_pad, bias=True)]
            return tnn.Sequential(*blk)

        if cnn_dim:
            self.cnn = head()
            self.feature_dim = cnn_dim[-1]
        else:
            self.cnn = None
            self.feature_dim = base.feature_dim
        if noisy:
            assert cnn_dim
            self.cnn_logvar = head()

    def _pool(self, t):
        if self.pooling in ('avg', 'max'):
            assert t.size(2) == t.size(3), 'global pooling expects square feature maps'
            return HF.global_pool(t, self.pooling == 'max')
        return t

    def forward(self, x):
        h = self.base.forward(x)
        out = run_sequential(self.cnn, h) if self.cnn is not None else h
        # ratings leave the encoder as fp32 whatever the storage type of its activations (the bf16 path: the rating
        # arithmetic of the step -- normalisation, resampling, bin look-ups, the z_rec loss -- stays fp32)
        out = HF.cast(self._pool(out), torch.float32)
        if self._noisy:
            return out, HF.cast(self._pool(run_sequential(self.cnn_logvar, h)), torch.float32)
        return out

    def load_pretrained(self, state_dict):
        if isinstance(state_dict, str):
            state_dict = torch.load(state_dict, map_location='cpu')
        for key in list(state_dict.keys()):
            if key.startswith('cxn') or key.startswith('fc'):
                state_dict.pop(key)
        self.load_state_dict(state_dict, strict=True)

    def load_base(self, state_dict):
        self.base.load_pretrained(state_dict)


class SiameseNetwork(SiameseFeature):
    """The comparison network the Elo-rating encoder is trained as (reference models/networks.py:872-992): the SAME trunk
    + conv head as SiameseFeature applied to two images, score = rating(x1) - rating(x2).  Its state_dict (`base.*`,
    `cnn.*`) is what wsgan_emb consumes as --pretrained_model_path_E.  Configurations of the reference outside the
    Elo recipe (fully connected comparison head `fc_dim`, `use_cxn`) raise."""

    def __init__(self, base=None, pooling='avg', cnn_dim=[], cnn_pad=1, cnn_relu_slope=0.5, fc_dim=[], fc_relu_slope=0.2,
                 fc_residual=True, dropout=0.5, use_cxn=False, noisy=False, drop_layer=None, rsample=False):
        if fc_dim or use_cxn:
            raise NotImplementedError('pcgan_amd: SiameseNetwork with fc_dim / use_cxn is outside the MI355X hot path')
        super().__init__(base, pooling=pooling, cnn_dim=cnn_dim, cnn_pad=cnn_pad, cnn_relu_slope=cnn_relu_slope,
                         noisy=noisy, drop_layer=drop_layer)
        self._rsample = rsample
        self.fc = self.cxn = None

    def forward_once(self, x):
        out = SiameseFeature.forward(self, x)
        return out if self._noisy else (out, None)

    def forward(self, input1, input2):
        feature1, logvar1 = self.forward_once(input1)
        feature2, logvar2 = self.forward_once(input2)
        if not self._noisy:
            return feature1, feature2, feature1 - feature2
        if self._rsample:
            return feature1, feature2, logvar1, logvar2
        std = torch.sqrt(torch.exp(logvar1) + torch.exp(logvar2))      # sqrt(std1^2 + std2^2)
        return feature1, feature2, feature1 - feature2, std

    def load_pretrained(self, state_dict):
        """only the trunk comes from the pretrained (ImageNet) file: the conv head stays as initialised (:994-997)"""
        self.base.load_pretrained(state_dict)

    def get_finetune_parameters(self):
        return list(self.cnn.parameters()) if self.cnn is not None else []


class RegressionNetwork(tnn.Module):
    """reference models/networks.py:1087-1124: SiameseFeature's trunk -> 3x3 conv head -> global pooling WITHOUT the drop layers (so
    the head's Sequential indices, and with them the state_dict keys cnn.0 / cnn.1 / cnn.3 ..., are its own) and with a load_pretrained
    that loads the trunk only.  state_dict keys base.*, cnn.*.  forward(x) is the fp32 (N, feature_dim, 1, 1) prediction through the
    pooling path of the encoder; regress(x, target, delta) is the training loop's entry (regression.py:359-363): pooling, nn.MSELoss
    and the "within delta" count as one node."""

    def __init__(self, base=None, pooling='avg', cnn_dim=[], cnn_pad=1, cnn_relu_slope=0.2):
        super().__init__()
        self.pooling = pooling
        self.base = base
        if cnn_dim:
            blk, prev = [], base.feature_dim
            for nf in cnn_dim[:-1]:
                blk += [hnn.Conv2d(prev, nf, kernel_size=3, stride=1, padding=cnn_pad, bias=True), hnn.BatchNorm2d(nf),
                        tnn.LeakyReLU(cnn_relu_slope)]
                prev = nf
            blk += [hnn.Conv2d(prev, cnn_dim[-1], kernel_size=3, stride=1, padding=cnn_pad, bias=True)]
            self.cnn = tnn.Sequential(*blk)
            self.feature_dim = cnn_dim[-1]
        else:
            self.cnn = None
            self.feature_dim = base.feature_dim

    def _maps(self, x):
        h = self.base.forward(x)
        return run_sequential(self.cnn, h) if self.cnn is not None else h

    def forward(self, x):
        out = self._maps(x)
        if self.pooling in ('avg', 'max'):
            assert out.size(2) == out.size(3), 'global pooling expects square feature maps'
            out = HF.global_pool(out, self.pooling == 'max')
        return HF.cast(out, torch.float32)

    def regress(self, x, target, delta):
        """(loss, pred, hits) of one batch: nn.MSELoss()(self(x), target), the fp32 (N, feature_dim, 1, 1) prediction and the number of
        its values within `delta` of their target (device tensors: nothing is read back).  Only `loss` carries the graph.  target: N x
        feature_dim fp32 values on x's device."""
        if self.pooling not in ('avg', 'max'):
            raise NotImplementedError('pcgan_amd: RegressionNetwork.regress needs pooling avg or max, got [%s]' % self.pooling)
        out = self._maps(x)
        assert out.size(2) == out.size(3), 'global pooling expects square feature maps'
        if not torch.is_grad_enabled():
            out = out.detach()
        return HF.pooled_mse(out, target, delta, self.pooling == 'max')

    def load_pretrained(self, state_dict):
        """only the trunk comes from the pretrained (ImageNet) file: the conv head stays as initialised (:1121-1124)"""
        self.base.load_pretrained(state_dict)


class BinaryNLLLoss(tnn.Module):
    """Binary cross entropy with draws (reference models/networks.py:473-482): label 0 / 1 / 2 = "first lower" / draw /
    "first higher" -> target 0 / 0.5 / 1; -(t log(p + 1e-20) + (1 - t) log(1 - p + 1e-20)), mean.  (N values: plain
    tensor arithmetic; the LUT follows the probabilities' device instead of the reference's unconditional .cuda().)"""

    def __init__(self):
        super().__init__()
        self.register_buffer('LUT', torch.tensor([0.0, 0.5, 1.0]), persistent=False)

    def forward(self, prob, label):
        lut = self.LUT.to(prob.device)
        target = lut[label].reshape(prob.size(0), 1, 1, 1).expand(prob.size(0), 1, prob.size(2), prob.size(3))
        loss = -(target * torch.log(prob + 1e-20) + (1 - target) * torch.log(1 - prob + 1e-20))
        return loss.mean()


class ResNetFeature(tnn.Module):
    """reference models/networks.py:1310-1359"""

    def __init__(self, input_nc=3, which_model='resnet18', dropout=0.):
        super().__init__()
        from . import resnet
        table = {'resnet18': (resnet.resnet18, 512), 'resnet34': (resnet.resnet34, 512),
                 'resnet50': (resnet.resnet50, 2048)}
        if which_model not in table:
            raise NotImplementedError('pcgan_amd: encoder trunk [%s] is outside the hot path' % which_model)
        ctor, dim = table[which_model]
        model = ctor(False, dropout=dropout)
        del model.fc
        self.model = model
        self.feature_dim = dim

    def forward(self, x):
        return self.model.features(x)

    def load_pretrained(self, state_dict):
        if isinstance(state_dict, str):
            state_dict = torch.load(state_dict, map_location='cpu')
        self.model.load_state_dict(state_dict, strict=False)


class AlexNetFeature(tnn.Module):
    """reference models/networks.py:1218-1255"""

    def __init__(self, input_nc=3, pooling='max'):
        super().__init__()
        self.pooling = pooling
        self.features = tnn.Sequential(
            hnn.Conv2d(input_nc, 64, kernel_size=11, stride=4, padding=2), tnn.ReLU(inplace=True),
            hnn.MaxPool2d(kernel_size=3, stride=2),
            hnn.Conv2d(64, 192, kernel_size=5, padding=2), tnn.ReLU(inplace=True),
            hnn.MaxPool2d(kernel_size=3, stride=2),
            hnn.Conv2d(192, 384, kernel_size=3, padding=1), tnn.ReLU(inplace=True),
            hnn.Conv2d(384, 256, kernel_size=3, padding=1), tnn.ReLU(inplace=True),
            hnn.Conv2d(256, 256, kernel_size=3, padding=1), tnn.ReLU(inplace=True),
            hnn.MaxPool2d(kernel_size=3, stride=2))
        self.feature_dim = 256

    def forward(self, x):
        x = run_sequential(self.features, x)
        if self.pooling in ('avg', 'max'):
            x = HF.global_pool(x, self.pooling == 'max')
        return x

    def load_pretrained(self, state_dict):
        if isinstance(state_dict, str):
            state_dict = torch.load(state_dict, map_location='cpu')
        for key in list(state_dict.keys()):
            if key.startswith('classifier'):
                state_dict.pop(key)
        self.load_state_dict(state_dict, strict=True)


class Normalize(tnn.Module):
    """reference models/networks.py:2421-2439.  With non-empty mean/std the reference's
    `identity_mapping = mean or std` is truthy, so the module is an IDENTITY; only
    that reachable behaviour is reproduced."""

    def __init__(self, mean=[], std=[]):
        super().__init__()
        self.nc = len(mean)
        self.identity_mapping = bool(mean or std)
        if not self.identity_mapping:
            raise NotImplementedError('pcgan_amd: Normalize with empty mean and std crashes in the reference too')

    def forward(self, input):
        return input


class ResNet(tnn.Module):
    """The reference's classifier wrapper (models/networks.py:1258-1285) that classification.py trains and the Inception Score loads
    (compute_inception_score.py:31-36): state_dict keys model.conv1.weight ... model.fc.bias.  forward runs the HIP trunk (eval-mode
    BatchNorm after .eval()), the global average pool and the classifier head kernel (pcgan_linear_softmax_fwd).

    Two paths.  INFERENCE -- gradients off, or no parameter and no input that wants one -- is the forward-only path the Inception Score
    uses, under no_grad.  TRAINING -- train mode, or gradients enabled and a parameter or the input requiring one -- returns logits with
    an autograd graph (the reference's `self.model(x)`, models/networks.py:1284-1285): trunk features() with train-mode BatchNorm
    (running statistics and num_batches_tracked move as in the reference), global average pool, linear head.  `classify(x, labels)` is
    the training loop's entry (classification.py:376-384): the head and CrossEntropyLoss as one node, (loss, logits, pred, correct).
    resnet101 / resnet152 are outside the HIP path."""

    def __init__(self, input_nc=3, num_classes=0, which_model='resnet18', pretrained=False, dropout=0.):
        super().__init__()
        from . import resnet
        table = {'resnet18': resnet.resnet18, 'resnet34': resnet.resnet34, 'resnet50': resnet.resnet50}
        if which_model not in table:
            raise NotImplementedError('pcgan_amd: classifier [%s] is outside the HIP path (resnet18, resnet34, resnet50)' % which_model)
        # as the reference builds it (:1262-1282): the 1000-class net first, then a new fc -- both draw from torch's generator, so a
        # seeded construction + classification.py's weights_init gives the reference's initial weights
        model = table[which_model](pretrained, dropout=dropout)
        model.fc = tnn.Linear(model.fc.in_features, num_classes)
        self.model = model

    def forward(self, x, probs=False):
        """logits (N, num_classes); with probs=True (logits, softmax probabilities), always on the inference path"""
        from ..hip import inception as I
        if not probs and self._wants_graph(x):      # probs=True asks for the scorer's by-product: always the inference path
            fc = self.model.fc
            return HF.linear(self._pooled(x), fc.weight, fc.bias)
        with torch.no_grad():
            pooled = I.global_avg_pool(self.model.features(x)).flatten(1)
            logits, p = I.linear_softmax(pooled, self.model.fc.weight, self.model.fc.bias)
        return (logits, p) if probs else logits

    def _wants_graph(self, x):
        if not torch.is_grad_enabled():
            return False
        return self.training or x.requires_grad or any(p.requires_grad for p in self.parameters())

    def _pooled(self, x):
        """(N, feature_dim) fp32 rows of the trunk's globally averaged features, differentiable"""
        return HF.cast(HF.global_pool(self.model.features(x), False), torch.float32).flatten(1)

    def classify(self, x, labels, class_weight=None):
        """(loss, logits, pred, correct) of one batch: CrossEntropyLoss(weight=class_weight)(self(x), labels) with its default mean
        reduction, the logits, the first arg-max of every row (the reference's get_prediction) and the number of rows it gets right
        (device tensors: nothing is read back).  Only `loss` carries the graph.  labels: (N,) int64 on x's device."""
        fc = self.model.fc
        pooled = self._pooled(x) if torch.is_grad_enabled() else self._pooled(x).detach()
        return HF.linear_cross_entropy(pooled, fc.weight, fc.bias, labels, class_weight)

    def load_pretrained(self, state_dict):
        """reference models/networks.py:1301-1307: the trunk of an (ImageNet) checkpoint of the bare net -- keys conv1.weight ... without
        the `model.` prefix; `fc*` is dropped (another class count), the rest loads non-strictly into self.model"""
        if isinstance(state_dict, str):
            state_dict = torch.load(state_dict, map_location='cpu')
        state_dict = {k: v for k, v in state_dict.items() if not k.startswith('fc')}
        self.model.load_state_dict(state_dict, strict=False)
        from ..hip import ops
        ops.invalidate_packed_weights()
