#!/usr/bin/env python
"""Inception Score of a set of images (reference compute_inception_score.py; the IS of eval_emb.py:96-106).

    python compute_inception_score.py --dataroot gen_dir --inception_weights inception_v3_google.pth      # --which_model_IS inception_v3
    python compute_inception_score.py --dataroot gen_dir --num_classes 5 --which_model_IS resnet18 \
        --pretrained_model_path_IS checkpoints/class_<dataset>/latest_net.pth --loadSize 224 --fineSize 224 --batchSize 32 \
        --batchSize_IS 32 --splits 10 --result_path res_is.txt                                         # eval_emb.py's call

The reference's options (TestOptions) and semantics: the files of --dataroot (sorted), or the --sourcefile_A list under it, shuffled
with `random` (seeded by --seed when given), the first --how_many kept; the reference's transform (--transforms resize_and_crop, crop,
resize_affine_crop or resize_affine_center, no flip, ToTensor, Normalize with the CIFAR statistics); a bilinear resize
(align_corners=False) to 299 x 299 (inception_v3) or 224 x 224 (resnet*); softmax class probabilities in batches of --batchSize_IS;
the score of pcgan_amd/util/inception_score.py over --splits splits.  The classifiers run on the HIP path: torchvision's inception_v3
(transform_input=False) from a state_dict you supply with --inception_weights -- the reference downloads it, nothing is downloaded
here, and IS from random weights is not IS -- or the reference's networks.ResNet classifier from classification.py's checkpoint
(resnet18 / 34 / 50).  Prints `IS: mean %f, std %f` and writes '%f %f' to --result_path.
"""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pcgan_amd.util.script import MEAN, STD, normalized_transform      # (Normalize of the reference's get_transform, :74-75)

MODES = ('resize_and_crop', 'crop', 'resize_affine_crop', 'resize_affine_center')
RESNETS = ('resnet18', 'resnet34', 'resnet50')
INPUT_SIZE = {'inception_v3': 299, 'resnet': 224}


def options(argv=None):
    """(options object, flags) from argv (default: the command line); nothing touches the device"""
    from pcgan_amd.options.test_options import TestOptions

    class ISOptions(TestOptions):
        def initialize(self, parser):
            parser = TestOptions.initialize(self, parser)
            # build-only: the torchvision inception_v3 state_dict for --which_model_IS inception_v3 (the reference downloads it)
            parser.add_argument('--inception_weights', type=str, default='', help='torchvision inception_v3 state_dict (.pth)')
            return parser

        # the script builds neither a model nor a data loader: no --model / --dataset_mode plugin flags
        def gather_options(self):
            self.parser = self.initialize(argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter))
            return self.parser.parse_args(argv)

    o = ISOptions()
    opt = o.gather_options()
    opt.isTrain = False
    return o, opt


def classifier_spec(opt):
    """the refusals of the command line, on the host before any device use: (which, num_classes, weights) with weights the validated
    Inception state_dict, or the networks.ResNet classifier (CPU) with classification.py's checkpoint loaded strictly"""
    import torch
    which = opt.which_model_IS
    if 'vgg' in which:
        raise NotImplementedError('--which_model_IS %s: the VGG classifiers are outside the HIP path (inception_v3, %s)'
                                  % (which, ', '.join(RESNETS)))
    if which == 'inception_v3':
        if not opt.inception_weights:
            raise ValueError('--which_model_IS inception_v3 needs --inception_weights PATH (a torchvision inception_v3 state_dict): '
                             'the weights are not downloaded, and IS from random weights is not IS')
        from pcgan_amd.models import inception as M
        sd = M.load_state_dict_file(opt.inception_weights)
        classes = M.check_classifier_state_dict(sd)
        if opt.num_classes is not None and opt.num_classes != classes:
            raise ValueError('--num_classes %d, but the Inception head (fc.weight) has %d classes' % (opt.num_classes, classes))
        return which, classes, sd
    if 'resnet' in which:
        if which not in RESNETS:
            raise NotImplementedError('--which_model_IS %s is outside the HIP path (%s)' % (which, ', '.join(RESNETS)))
        if opt.num_classes is None:
            raise ValueError('--which_model_IS %s needs --num_classes (the class count of the classifier)' % which)
        if not opt.pretrained_model_path_IS:
            raise ValueError('--which_model_IS %s needs --pretrained_model_path_IS (the checkpoint classification.py saved)' % which)
        from pcgan_amd.models import networks
        net = networks.ResNet(3, opt.num_classes, which)
        print('loading the model from %s...' % opt.pretrained_model_path_IS)
        net.load_state_dict(torch.load(opt.pretrained_model_path_IS, map_location='cpu'), strict=True)
        return which, opt.num_classes, net
    raise NotImplementedError('--which_model_IS %s: unknown classifier (inception_v3, %s)' % (which, ', '.join(RESNETS)))


def predictor(which, weights, device):
    """batch (b, 3, H, W) float32 -> (b, classes) softmax probabilities on the device"""
    import torch
    if which == 'inception_v3':
        from pcgan_amd.models.inception import InceptionV3Classifier
        net = InceptionV3Classifier(weights=weights, gpu_ids=[device.index])      # its input pass: the resize to 299, no normalisation
        return lambda batch: net(batch.float(), probs=True)[1]
    from pcgan_amd.hip import inception as I
    net = weights.to(device).eval()
    size = INPUT_SIZE['resnet']

    def predict(batch):
        with torch.no_grad(), torch.cuda.device(device):
            x = I.prep(batch.to(device, torch.float32).contiguous(), (size, size))
            return net(x, probs=True)[1]
    return predict


def get_transform(opt):
    """the reference's transform (compute_inception_score.py:47-76): PIL image -> normalised (3, fineSize, fineSize) float32"""
    return normalized_transform(opt, MODES)


def image_paths(opt):
    """the --sourcefile_A list under --dataroot, or the files of --dataroot in sorted order; shuffled with `random`, first --how_many"""
    if opt.sourcefile_A:
        with open(opt.sourcefile_A, 'r') as f:
            paths = [os.path.join(opt.dataroot, x.rstrip('\n')) for x in f.readlines()]
    else:
        paths = [os.path.join(opt.dataroot, x) for x in sorted(os.listdir(opt.dataroot))]
    random.shuffle(paths)
    return paths[:min(int(opt.how_many), len(paths))]


class ImageFolderDataset(object):
    """compute_inception_score.py:81-99: image i = transform(RGB image of paths[i]); transforms draw from `random` in index order"""

    def __init__(self, paths, transform):
        self.paths = paths
        self.transform = transform

    def __getitem__(self, index):
        from PIL import Image
        return self.transform(Image.open(self.paths[index]).convert('RGB'))

    def __len__(self):
        return len(self.paths)


def main(argv=None):
    o, opt = options(argv)
    transform = get_transform(opt)
    which, num_classes, weights = classifier_spec(opt)
    opt = o.parse()      # the reference's parse: prints the options, seeds random / numpy / torch (--seed), selects the device
    if not opt.gpu_ids:
        raise RuntimeError('the classifier runs on the GPU only (HIP path): --gpu_ids must name a device')
    import torch
    from pcgan_amd.util.inception_score import inception_score
    dataset = ImageFolderDataset(image_paths(opt), transform)
    print('[%d] # of images found' % len(dataset))
    predict = predictor(which, weights, torch.device('cuda', opt.gpu_ids[0]))
    score_mu, score_std = inception_score(dataset, predict, num_classes=num_classes, batch_size=opt.batchSize_IS, splits=opt.splits)
    print('IS: mean %f, std %f' % (score_mu, score_std))
    if opt.result_path:
        with open(opt.result_path, 'w') as f:
            f.write('%f %f\n' % (score_mu, score_std))
    return score_mu, score_std


if __name__ == '__main__':
    main()
