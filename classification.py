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
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

from pcgan_amd.util.script import (MEAN, STD, checkpoint_file, first_gpu, init_like_reference, normalized_transform, options_report,
                                   run_epochs, seed_everything, write_report)

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
        write_report(report, os.path.join(opt.checkpoint_dir, opt.name))
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
    from pcgan_amd.data.base_dataset import TRANSFORM_MODES
    return normalized_transform(opt, TRANSFORM_MODES)


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
        init_like_reference(net, linear=True)
        if opt.pretrained_model_path:      # '' trains from the initialisation above (no ImageNet file is fetched)
            net.load_pretrained(opt.pretrained_model_path)
    else:
        net.load_state_dict(torch.load(checkpoint_file(opt, opt.which_epoch), map_location='cpu'))
    ops.invalidate_packed_weights()
    if opt.mode != 'train':
        net.eval()
    return net


# ---------------------------------------------------------------------------- train / test
def train(opt, net, loader, loader_val=None):
    """reference classification.py:325-469"""
    device = first_gpu(opt, 'classification.py')
    net = net.to(device)
    weight = torch.tensor(opt.weight, dtype=torch.float32, device=device) if len(opt.weight) else None      # :326-332
    save_dir = os.path.join(opt.checkpoint_dir, opt.name)
    os.makedirs(os.path.join(save_dir, 'img'), exist_ok=True)

    def forward(img, label):       # :376-380, one node: head + loss + predictions; the validation pass (:429-443) takes no class weights
        loss, _, _, correct = net.classify(img, label, weight if torch.is_grad_enabled() else None)
        return loss, correct
    return run_epochs(opt, net, loader, loader_val, lambda names: torch.tensor(labels_of(names, opt), dtype=torch.int64).to(device),
                      forward, lambda loss: loss.backward(), save_dir)


def test(opt, net, loader):
    """reference classification.py:473-494: images in file order, one line per image, the accuracy in percent"""
    device = first_gpu(opt, 'classification.py')
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
