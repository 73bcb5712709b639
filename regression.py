#!/usr/bin/env python
"""Attribute regressor on the HIP path (reference regression.py): `--mode train` writes the checkpoint the continuous-label CGAN
baseline loads as pretrained_models/auxiliary_regresser.pth, `--mode embedding` writes the per-image predictions (features.npy) and
attribute values (labels.npy) that are plotted against the Elo ratings.

    python regression.py --mode train --name reg_utk --dataroot datasets/UTKFace --datafile train.txt --which_model resnet18 \
        --embedding_mean 33 --embedding_std 20 --pretrained_model_path pretrained_models/resnet18-5c106cde.pth
    python regression.py --mode embedding --name reg_utk --dataroot datasets/UTKFace --datafile test.txt --which_model resnet18 \
        --which_epoch latest

Same option names and defaults as the reference (regression.py:28-65).  The label of an image is the float its file name starts with
(`get_attr`), normalised by --embedding_mean / --embedding_std.  The net is networks.RegressionNetwork (alexnet / resnet18 / 34 / 50
trunk, the 3x3 conv head of --cnn_dim, global pooling); one training iteration is the HIP trunk and conv head with train-mode
BatchNorm, then pooling + MSELoss + the "within --delta" count + the loss gradient as one kernel (pcgan_pool_mse_fwd), the backward
passes and one fused Adam launch.  The loss is read on the host where the reference prints it (--print_freq) and once per epoch for
loss.txt; the hit count stays on the device until the epoch ends.

Dataset, loader and transforms are classification.py's, the epoch loop is shared with it (util/script.py).  Build-only flag: --seed (random / numpy / torch;
the reference sets none).  Build-only artefact: --mode train also writes init_net.pth, the weights before the first iteration.
loss.txt has one line per iteration (the reference appends only at --print_freq).  The validation loader takes single images, as
classification.py's.  --display_id is accepted and plots nothing (no visdom here).  One process drives one GPU.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

import classification as K      # the dataset and loader, transforms
from pcgan_amd.util.script import checkpoint_file, first_gpu, init_like_reference, options_report, run_epochs, write_report
from pcgan_amd.util.util import get_attr_value as get_attr      # reference regression.py:182-183

BASES = ('alexnet', 'resnet18', 'resnet34', 'resnet50')
SCRIPT = 'classification.py'      # the name in the "needs an MI355X" error, unchanged since the device helper was classification.py's


# ---------------------------------------------------------------------------- options
# (flag, argparse keywords): the reference's names and defaults (regression.py:28-65), then the build-only flag
_FLAGS = [
    ('--mode', dict(type=str, default='train', help='train | embedding')),
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
    ('--which_model', dict(type=str, default='alexnet', help=' | '.join(BASES))),
    ('--n_layers', dict(type=int, default=3)),
    ('--nf', dict(type=int, default=64)),
    ('--pooling', dict(type=str, default='avg', help='avg | max')),
    ('--loadSize', dict(type=int, default=240)),
    ('--fineSize', dict(type=int, default=224)),
    ('--gpu_ids', dict(type=str, default='0', help='the first id is used; there is no CPU path')),
    ('--print_freq', dict(type=int, default=50)),
    ('--display_id', dict(type=int, default=1, help='accepted; nothing is plotted')),
    ('--display_port', dict(type=int, default=8097)),
    ('--delta', dict(type=float, default=0.05, help='a prediction within delta of its (normalised) label counts as accurate')),
    ('--embedding_mean', dict(type=float, default=0)),
    ('--embedding_std', dict(type=float, default=1)),
    ('--cnn_dim', dict(type=int, nargs='+', default=[64, 1], help='channels of the 3x3 conv head; the last is the feature dimension')),
    ('--cnn_pad', dict(type=int, default=1)),
    ('--cnn_relu_slope', dict(type=float, default=0.7)),
    ('--transforms', dict(type=str, default='resize_affine_crop')),
    ('--affineScale', dict(nargs='+', type=float, default=[0.95, 1.05])),
    ('--affineDegrees', dict(type=float, default=5)),
    ('--use_color_jitter', dict(action='store_true')),
    ('--no_flip', dict(action='store_true')),
    ('--epoch_count', dict(type=int, default=1)),
    # build-only
    ('--seed', dict(type=int, default=None, help='(pcgan_amd) seed of random / numpy / torch')),
]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for flag, kw in _FLAGS:
        parser.add_argument(flag, **kw)
    return parser


def get_options(argv=None, save=True):
    """parsed options plus what the rest of the script derives from them: isTrain, use_gpu, embedding_normalize, and test_batch_size = 1
    for classification.py's loader (--mode embedding takes one image per pass, as the reference)"""
    parser = build_parser()
    opt = parser.parse_args(argv)
    opt.isTrain = opt.mode == 'train'
    opt.use_gpu = bool(opt.gpu_ids) and torch.cuda.is_available()
    opt.test_batch_size = 1
    report = options_report(parser, opt)
    print(report)
    if save:
        write_report(report, os.path.join(opt.checkpoint_dir, opt.name))
    mean, std = opt.embedding_mean, opt.embedding_std
    opt.embedding_normalize = lambda x: (x - mean) / std
    return opt


# ---------------------------------------------------------------------------- labels
def labels_of(names, opt, feature_dim):
    """the fp32 (B, feature_dim, 1, 1) label tensor of a batch of file names (regression.py:346-350): the float each name starts with,
    normalised by --embedding_mean / --embedding_std.  As in the reference the view only fits feature_dim = 1."""
    label = torch.FloatTensor([get_attr(name) for name in names]).view(len(names), feature_dim, 1, 1)
    return opt.embedding_normalize(label)


# ---------------------------------------------------------------------------- model
def check_refusals(opt):
    """what this build does not run, raised before anything touches the device"""
    if opt.mode not in ('train', 'embedding'):
        raise NotImplementedError('Mode [%s] is not implemented.' % opt.mode)
    which = opt.which_model
    if which != 'alexnet' and 'resnet' not in which:
        raise NotImplementedError('Model [%s] is not implemented.' % which)
    if which not in BASES:
        raise NotImplementedError('pcgan_amd: regressor base [%s] is outside the HIP path (%s)' % (which, ', '.join(BASES)))


def get_model(opt):
    """reference regression.py:245-274 (on the CPU; the caller moves it)"""
    from pcgan_amd.hip import ops
    from pcgan_amd.models import networks
    check_refusals(opt)
    if opt.which_model == 'alexnet':
        base = networks.AlexNetFeature(3, pooling='')
    else:
        base = networks.ResNetFeature(3, opt.which_model)
    net = networks.RegressionNetwork(base, pooling=opt.pooling, cnn_dim=opt.cnn_dim, cnn_pad=opt.cnn_pad,
                                     cnn_relu_slope=opt.cnn_relu_slope)
    if opt.mode == 'train':
        init_like_reference(net, linear=True)
        if opt.pretrained_model_path:      # '' trains from the initialisation above (no ImageNet file is fetched)
            net.load_pretrained(opt.pretrained_model_path)
    else:
        net.load_state_dict(torch.load(checkpoint_file(opt, opt.which_epoch), map_location='cpu'), strict=False)   # "HACK" (:268-269)
        net.eval()
    ops.invalidate_packed_weights()
    return net


# ---------------------------------------------------------------------------- train / embedding
def train(opt, net, loader, loader_val=None):
    """reference regression.py:320-428"""
    from pcgan_amd.hip import functional as HF
    device = first_gpu(opt, SCRIPT)
    net = net.to(device)
    save_dir = os.path.join(opt.checkpoint_dir, opt.name)
    os.makedirs(save_dir, exist_ok=True)

    def forward(img, label):       # :359-363, one node: pooling + loss + accuracy
        loss, _, within = net.regress(img, label, opt.delta)
        return loss, within
    # backward: the gradient the forward launch wrote, handed on as it is
    return run_epochs(opt, net, loader, loader_val, lambda names: labels_of(names, opt, net.feature_dim).to(device),
                      forward, lambda loss: loss.backward(HF.unit_gradient(loss)), save_dir)


def embedding(opt, net, loader):
    """reference regression.py:432-448: images in file order, one per pass, in eval mode"""
    device = first_gpu(opt, SCRIPT)
    net = net.to(device).eval()
    features, labels = [], []
    with torch.no_grad():
        for img0, path0 in loader:
            feature = net.forward(img0.to(device)).cpu().numpy()
            features.append(feature.reshape([1, net.feature_dim]))
            labels.append(get_attr(path0[0]))
            print('--> %s' % path0[0])
    X = np.concatenate(features, axis=0)
    labels = np.array(labels)
    np.save(os.path.join(opt.checkpoint_dir, opt.name, 'features.npy'), X)
    np.save(os.path.join(opt.checkpoint_dir, opt.name, 'labels.npy'), labels)
    return X, labels


def main(argv=None):
    opt = get_options(argv)
    K.seed_everything(opt.seed)
    net = get_model(opt)
    if opt.mode == 'train':
        loader = K.make_loader(opt, train=True)
        loader_val = K.make_loader(opt, val=True) if opt.dataroot_val else None
        print('dataset size = %d' % len(loader.dataset))
        return train(opt, net, loader, loader_val)
    return embedding(opt, net, K.make_loader(opt, train=False))


if __name__ == '__main__':
    main()
