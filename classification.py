#!/usr/bin/env python
"""Attribute classifier on the HIP path (reference classification.py): `--mode train` writes the checkpoint the Inception Score of
eval_emb.py loads (`--which_model_IS resnet18 --pretrained_model_path_IS checkpoints/class_<dataset>/latest_net.pth`), `--mode test`
measures Acc, the third number of the paper's evaluation (eval_emb.py:108-116).

    python classification.py --mode train --name class_utk --dataroot datasets/UTKFace --datafile train.txt --num_classes 5 \
        --attr_bins '[1, 21, 41, 61, 81]' --pretrained_model_path pretrained_models/resnet18-5c106cde.pth
    python classification.py --mode test --name class_utk --dataroot gen_dir --num_classes 5 --attr_bins '[1, 21, 41, 61, 81]' \
        --which_epoch latest --result_path res_acc.txt

Same option names and defaults as the reference (classification.py:30-67).  The label of an image is the bin of the attribute value its
file name starts with (`get_attr_label(get_attr_value(name), attr_bins + [inf])`).  The net is networks.ResNet (resnet18 / 34 / 50);
one training iteration is the HIP trunk with train-mode BatchNorm, the global average pool, the head + weighted cross entropy as one
kernel (pcgan_linear_ce_fwd), their backward passes and one fused Adam launch.  The loss is read on the host where the reference
prints it (--print_freq) and once per epoch for loss.txt; predictions and the hit count stay on the device until the epoch ends.

Build-only flags: --seed (random / numpy / torch; the reference sets none), --test_batch_size (images per forward pass of --mode test;
1 as in the reference).  Build-only artefact: --mode train also writes init_net.pth, the weights before the first iteration, beside
latest_net.pth (as siamese.py does), so that a run can be restated from its start.  --display_id is accepted and plots nothing (no
visdom here).  One process drives one GPU.
"""
import argparse
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from compute_inception_score import MEAN, STD      # transforms.Normalize of the reference's get_transform (classification.py:319-320)

RESNETS = ('resnet18', 'resnet34', 'resnet50')


# ---------------------------------------------------------------------------- options
# (flag, argparse keywords): the reference's names and defaults (classification.py:30-67), then the build-only flags
_FLAGS = [
    ('--mode', dict(type=str, default='train', help='train | test')),
    ('--name', dict(type=str, default='exp')),
    ('--dataroot', dict(required=True, help='image folder')),
    ('--datafile', dict(type=str, default='', help='listing of image names under --dataroot (default: the folder, sorted)')),
    ('--dataroot_val', dict(type=str, default='')),
    ('--datafile_val', dict(type=str, default='')),
    ('--pretrained_model_path', dict(type=str, default='pretrained_models/resnet18-5c106cde.pth', help="trunk weights; '' = none")),
    ('--checkpoint_dir', dict(type=str, default='checkpoints')),
    ('--save_epoch_freq', dict(type=int, default=10)),
    ('--num_workers', dict(type=int, default=4)),
    ('--init_type', dict(type=str, default='normal')),
    ('--num_classes', dict(type=int, default=10)),
    ('--num_epochs', dict(type=int, default=100)),
    ('--batch_size', dict(type=int, default=100)),
    ('--lr', dict(type=float, default=0.0002)),
    ('--which_epoch', dict(type=str, default='latest')),
    ('--which_model', dict(type=str, default='resnet18', help=' | '.join(RESNETS))),
    ('--n_layers', dict(type=int, default=3)),
    ('--nf', dict(type=int, default=64)),
    ('--pooling', dict(type=str, default='avg')),
    ('--loadSize', dict(type=int, default=240)),
    ('--fineSize', dict(type=int, default=224)),
    ('--gpu_ids', dict(type=str, default='0', help='the first id is used; there is no CPU path')),
    ('--attr_bins', dict(type=str, default='[]', help='lower edges of the attribute bins, one class per bin')),
    ('--weight', dict(nargs='+', type=float, default=[], help='class weights of the cross entropy')),
    ('--dropout', dict(type=float, default=0.5)),
    ('--finetune_fc_only', dict(action='store_true', help='refused (see check_refusals)')),
    ('--print_freq', dict(type=int, default=50)),
    ('--display_id', dict(type=int, default=1, help='accepted; nothing is plotted')),
    ('--display_port', dict(type=int, default=8097)),
    ('--transforms', dict(type=str, default='resize_affine_crop')),
    ('--affineScale', dict(nargs='+', type=float, default=[0.95, 1.05])),
    ('--affineDegrees', dict(type=float, default=5)),
    ('--use_color_jitter', dict(action='store_true')),
    ('--no_flip', dict(action='store_true')),
    ('--continue_train', dict(action='store_true')),
    ('--epoch_count', dict(type=int, default=1)),
    ('--result_path', dict(type=str, default='')),
    # build-only
    ('--seed', dict(type=int, default=None, help='(pcgan_amd) seed of random / numpy / torch')),
    ('--test_batch_size', dict(type=int, default=1, help='(pcgan_amd) images per forward pass of --mode test')),
]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for flag, kw in _FLAGS:
        parser.add_argument(flag, **kw)
    return parser


def options_report(parser, opt):
    """the option listing printed at start and kept as <checkpoint_dir>/<name>/opt.txt, in the layout of this project's other scripts
    (pcgan_amd/options/base_options.py): one `name: value` row per option, values that differ from the default marked"""
    rows = ['--------------- Options -----------------']
    for key in sorted(vars(opt)):
        value, default = getattr(opt, key), parser.get_default(key)
        note = '' if value == default else '\t[default: %s]' % (default,)
        rows.append('%25s: %-30s%s' % (key, value, note))
    rows.append('----------------- End -------------------')
    return '\n'.join(rows)


def get_options(argv=None, save=True):
    """parsed options plus what the rest of the script derives from them: isTrain, use_gpu, attr_bins as a list and with the open last
    bin; --weight must name every class"""
    from pcgan_amd.util.util import str2list
    parser = build_parser()
    opt = parser.parse_args(argv)
    opt.isTrain = opt.mode == 'train'
    opt.use_gpu = bool(opt.gpu_ids) and torch.cuda.is_available()
    opt.attr_bins = list(str2list(opt.attr_bins))
    opt.attr_bins_with_inf = opt.attr_bins + [float('inf')]
    assert not opt.weight or len(opt.weight) == opt.num_classes, '--weight takes one value per class'
    report = options_report(parser, opt)
    print(report)
    if save:
        folder = os.path.join(opt.checkpoint_dir, opt.name)
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, 'opt.txt'), 'w') as f:
            f.write(report + '\n')
    return opt


# ---------------------------------------------------------------------------- data
class AttributeImages(torch.utils.data.Dataset):
    """(transformed RGB image, file name) for every name in `listing` (a text file, one name per line) or, without one, every file of
    `root` in sorted order (the reference takes the directory's arbitrary order).  The attribute value is the start of the name."""

    def __init__(self, root, listing, transform):
        if listing:
            with open(listing) as f:
                names = [line.rstrip('\n') for line in f]
        else:
            names = sorted(os.listdir(root))
        self.root, self.names, self.transform = root, [n for n in names if n], transform

    def __len__(self):
        return len(self.names)

    def __getitem__(self, i):
        from PIL import Image
        with Image.open(os.path.join(self.root, self.names[i])) as f:
            img = f.convert('RGB')
        return self.transform(img), self.names[i]


def get_transform(opt):
    """reference classification.py:282-321: the PIL steps of --transforms (all seven modes; the flip in train mode unless --no_flip),
    ToTensor, Normalize with the CIFAR statistics.  --use_color_jitter adds ColorJitter() with its default arguments: the identity."""
    from pcgan_amd.data.base_dataset import TRANSFORM_MODES, pil_steps, to_tensor
    if opt.transforms not in TRANSFORM_MODES:
        raise ValueError('--resize_or_crop %s is not a valid option.' % opt.transforms)
    mean = torch.tensor(MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(3, 1, 1)
    return lambda img: (to_tensor(pil_steps(opt, img)) - mean) / std


def labels_of(names, opt):
    """class index of every file name (classification.py:367), checked HERE, on the host: the kernel never sees a label outside
    [0, num_classes)"""
    from pcgan_amd.util.util import get_attr_label, get_attr_value
    labels = [get_attr_label(get_attr_value(name), opt.attr_bins_with_inf) for name in names]
    for name, lab in zip(names, labels):
        if lab is None or not 0 <= lab < opt.num_classes:
            raise ValueError('%r falls into bin %r of --attr_bins %r, outside the %d classes of --num_classes'
                             % (name.rstrip('\n'), lab, opt.attr_bins, opt.num_classes))
    return labels


def make_loader(opt, train=True, val=False):
    """the reference's loaders (classification.py:510-516, 526-527): training shuffles batches of --batch_size, validation shuffles
    single images, testing walks the files in order.  The shuffles draw from a generator of their own seeded by --seed."""
    root, listing = (opt.dataroot_val, opt.datafile_val) if val else (opt.dataroot, opt.datafile)
    data = AttributeImages(root, listing, get_transform(opt))
    gen = None
    if opt.seed is not None:
        gen = torch.Generator().manual_seed(opt.seed + (1 if val else 0))
    if val:
        return torch.utils.data.DataLoader(data, shuffle=True, num_workers=0, batch_size=1, generator=gen)
    if train:
        return torch.utils.data.DataLoader(data, shuffle=True, num_workers=min(opt.num_workers, 16), batch_size=opt.batch_size,
                                           generator=gen)
    return torch.utils.data.DataLoader(data, shuffle=False, num_workers=0, batch_size=max(1, opt.test_batch_size))


# ---------------------------------------------------------------------------- model
def init_like_reference(net):
    """the initialisation classification.py's trainer starts from: every convolution and the fc weight ~ N(0, 0.02), every BatchNorm
    scale ~ N(1, 0.02) with a zero shift; the fc bias keeps nn.Linear's own.  Layers are visited in registration order, so the draws
    come out of torch's generator in the reference's order (pinned by tests/golden/classification_step.npz: <trunk>/init/*)."""
    with torch.no_grad():
        for m in net.modules():
            kind = type(m).__name__
            if 'Conv' in kind or 'Linear' in kind:
                m.weight.normal_(0.0, 0.02)
            elif 'BatchNorm2d' in kind:
                m.weight.normal_(1.0, 0.02)
                m.bias.zero_()


def check_refusals(opt):
    """what this build does not run, raised before anything touches the device"""
    if opt.mode not in ('train', 'test'):
        raise NotImplementedError('Mode [%s] is not implemented.' % opt.mode)
    which = opt.which_model
    if which in ('alexnet', 'alexnet_lite') or 'vgg' in which:
        raise NotImplementedError('pcgan_amd: classifier [%s] is outside the HIP path (%s)' % (which, ', '.join(RESNETS)))
    if 'resnet' not in which:
        raise NotImplementedError('Model [%s] is not implemented.' % which)
    if opt.finetune_fc_only:
        raise AttributeError("--finetune_fc_only calls net.get_finetune_parameters(), which the reference's networks.ResNet does not "
                             'define (classification.py:338-342): the flag cannot work there and is refused here')


def get_model(opt):
    """reference classification.py:249-279 (on the CPU; the caller moves it)"""
    from pcgan_amd.hip import ops
    from pcgan_amd.models import networks
    check_refusals(opt)
    net = networks.ResNet(3, opt.num_classes, opt.which_model)       # resnet101 / resnet152 raise NotImplementedError here
    if opt.mode == 'train' and not opt.continue_train:
        init_like_reference(net)
        if opt.pretrained_model_path:      # '' trains from the initialisation above (no ImageNet file is fetched)
            net.load_pretrained(opt.pretrained_model_path)
    else:
        path = os.path.join(opt.checkpoint_dir, opt.name, '{}_net.pth'.format(opt.which_epoch))
        net.load_state_dict(torch.load(path, map_location='cpu'))
    ops.invalidate_packed_weights()
    if opt.mode != 'train':
        net.eval()
    return net


def device_of(opt):
    gpu = int(opt.gpu_ids.split(',')[0]) if opt.gpu_ids else -1
    if gpu < 0 or not torch.cuda.is_available():
        raise RuntimeError('pcgan_amd: classification.py needs an MI355X (no CPU fallback)')
    device = torch.device('cuda', gpu)
    torch.cuda.set_device(device)
    return device


def seed_everything(seed):
    if seed is not None:
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)


def save(net, path):
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, path)


# ---------------------------------------------------------------------------- train / test
def train(opt, net, loader, loader_val=None):
    """reference classification.py:325-469"""
    from pcgan_amd.hip.optim import FusedAdam
    device = device_of(opt)
    net = net.to(device)
    weight = torch.tensor(opt.weight, dtype=torch.float32, device=device) if len(opt.weight) else None      # :326-332
    save_dir = os.path.join(opt.checkpoint_dir, opt.name)
    os.makedirs(os.path.join(save_dir, 'img'), exist_ok=True)
    optimizer = FusedAdam(net.parameters(), lr=opt.lr)         # optim.Adam(param, lr=opt.lr): betas (0.9, 0.999)
    save(net, os.path.join(save_dir, 'init_net.pth'))
    dataset_size = len(loader.dataset)
    iters_per_epoch = math.ceil(dataset_size / opt.batch_size)
    loss_history, total_iter = [], 0
    seed_everything(opt.seed)      # the augmentation draws of the first epoch start from the seed, whatever the initialisation consumed
    for epoch in range(opt.epoch_count, opt.num_epochs + opt.epoch_count):
        step_losses = []                                                     # device scalars: read once, when the epoch ends
        hits = torch.zeros((), dtype=torch.int32, device=device)
        for img0, path0 in loader:
            label = torch.tensor(labels_of(path0, opt), dtype=torch.int64).to(device)
            img0 = img0.to(device)
            total_iter += 1
            optimizer.zero_grad()
            loss, _, _, correct = net.classify(img0, label, weight)         # :376-380, one node: head + loss + predictions
            loss.backward()
            optimizer.step()
            step_losses.append(loss.detach())
            hits += correct
            if total_iter % opt.print_freq == 0:
                print('epoch %02d, iter %06d, loss: %.4f' % (epoch, total_iter, loss.item()))
        assert len(step_losses) == iters_per_epoch
        loss_history += torch.stack(step_losses).cpu().tolist()
        curr_acc = {'train': int(hits) / dataset_size}                       # 1 - err_train (:426-427)
        if loader_val is not None:
            # as in the reference (:429-443) eval mode is NOT entered: BatchNorm normalises each validation image with its own
            # statistics and the running statistics keep moving.  Kept on purpose; only autograd's bookkeeping is switched off.
            hits_val = torch.zeros((), dtype=torch.int32, device=device)
            with torch.no_grad():
                for img0, path0 in loader_val:
                    label = torch.tensor(labels_of(path0, opt), dtype=torch.int64).to(device)
                    hits_val += net.classify(img0.to(device), label)[3]
            curr_acc['val'] = int(hits_val) / len(loader_val.dataset)
        print('epoch %02d: ' % epoch + ', '.join('%s accuracy %.4f' % kv for kv in curr_acc.items()))
        save(net, os.path.join(save_dir, 'latest_net.pth'))
        if epoch % opt.save_epoch_freq == 0:
            save(net, os.path.join(save_dir, '{}_net.pth'.format(epoch)))
    with open(os.path.join(save_dir, 'loss.txt'), 'w') as f:
        for value in loss_history:
            f.write(str(value) + '\n')
    return loss_history


def test(opt, net, loader):
    """reference classification.py:473-494: images in file order, one line per image, the accuracy in percent"""
    device = device_of(opt)
    net = net.to(device).eval()
    pred, target = [], []
    with torch.no_grad():
        for img0, path0 in loader:
            label = torch.tensor(labels_of(path0, opt), dtype=torch.int64)
            p = net.classify(img0.to(device), label.to(device))[2]           # first arg-max of every row, as numpy's argmax
            pred += p.cpu().tolist()
            target += label.tolist()
    acc = 0
    for i, (t, p) in enumerate(zip(target, pred)):
        acc += int(t == p)
        print('--> image #%d: target %d   pred %d' % (i + 1, t, p))
    accuracy = 100. * acc / len(pred)
    print('================================================================================')
    print('accuracy: %.4f' % accuracy)
    if opt.result_path:
        with open(opt.result_path, 'w') as f:
            f.write('%f\n' % accuracy)
    return accuracy


def main(argv=None):
    opt = get_options(argv)
    seed_everything(opt.seed)
    net = get_model(opt)
    if opt.mode == 'train':
        loader = make_loader(opt, train=True)
        loader_val = make_loader(opt, val=True) if opt.dataroot_val else None
        print('dataset size = %d' % len(loader.dataset))
        return train(opt, net, loader, loader_val)
    return test(opt, net, make_loader(opt, train=False))


if __name__ == '__main__':
    main()
