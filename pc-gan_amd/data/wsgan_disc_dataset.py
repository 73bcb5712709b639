"""Class-grouped dataset of the class-label baseline (reference data/wsgan_disc_dataset.py:10-77): each line of `--sourcefile_A` is
"<file> [<attr>]"; the attribute (parsed from the file name "<attr>_<rest>" when the line has none) is binned by `--attr_bins` into one
of `--num_classes` classes -- or, under `--label_as_group`, the second column IS the class.  One id list per class; a sample holds one
image of EVERY class, the index taken modulo each class's list: int keys 0 .. K-1 (C,S,S) and 'path_<L>'.  The model draws the two
classes of a step after the batch is made, so all K images are decoded per index, as in the reference.

`--dataroot synthetic` short-circuits to seeded synthetic samples of the same dict layout (U[-1,1) images)."""
import os.path
import random

import torch

from .base_dataset import BaseDataset, get_transform, decode_raw
from ..util.util import get_attr_label, get_attr_value


class WSGANDiscDataset(BaseDataset):
    @staticmethod
    def modify_commandline_options(parser, is_train):
        return parser

    def name(self):
        return 'WSGANDiscDataset'

    def initialize(self, opt):
        self.opt = opt
        self.num_classes = opt.num_classes
        self.attr_bins = opt.attr_bins
        self.attr_bins_with_inf = opt.attr_bins + [float('inf')]
        self.root = self.dir = opt.dataroot
        self.synthetic = (opt.dataroot == 'synthetic')
        self.label_as_group = bool(getattr(opt, 'label_as_group', False))   # a training flag of the model: absent at test time
        if self.synthetic:
            self.size = int(min(opt.max_dataset_size, 64 * opt.batchSize))
            return
        with open(opt.sourcefile_A, 'r') as f:
            self.sourcefile = [line.rstrip('\n') for line in f.readlines()]
        self.create_attr_group_list()
        self.size = min(self.size, opt.max_dataset_size)
        self.transform = get_transform(opt)
        self.raw = bool(getattr(opt, 'gpu_transform', False))     # workers decode, the loader finishes the batch on the GPU

    def create_attr_group_list(self):
        """attr_group_list[L]: ids (line numbers) of the images of class L (reference :31-52)"""
        attr_group_list = [[] for _ in range(self.num_classes)]
        attrs, paths = [], []
        for id, line in enumerate(self.sourcefile):
            parts = line.split()
            attr = float(parts[1]) if len(parts) > 1 else get_attr_value(parts[0])
            attrs.append(attr)
            label = int(parts[1]) if self.label_as_group else get_attr_label(attr, self.attr_bins_with_inf)
            attr_group_list[label].append(id)
            paths.append(os.path.join(self.dir, parts[0]))
        self.attr_group_list = attr_group_list
        self.attr_group_list_len = [len(ls) for ls in attr_group_list]
        self.size = max(self.attr_group_list_len)
        self.attrs, self.paths = attrs, paths

    def _synthetic(self, index):
        o = self.opt
        g = torch.Generator().manual_seed(97531 + index)
        ret = {}
        for L in range(self.num_classes):
            ret[L] = torch.rand(o.input_nc, o.fineSize, o.fineSize, generator=g) * 2 - 1
            ret['path_' + str(L)] = '%d_synthetic_%d_%d' % (int(self.attr_bins[L]) if L < len(self.attr_bins) else L, L, index)
        return ret

    def __getitem__(self, index):
        if self.synthetic:
            return self._synthetic(index)
        from PIL import Image
        ret = {}
        for L in range(self.num_classes):
            id = self.attr_group_list[L][index % self.attr_group_list_len[L]]
            img = Image.open(self.paths[id]).convert('RGB')
            if self.raw:
                # same draws, same order as the PIL path; the per-pixel work and the gray mix are one launch per class in the loader
                ret['%d_raw' % L], ret['%d_aug' % L] = decode_raw(img, self.opt)
            else:
                img = self.transform(img)
                if self.opt.input_nc == 1:      # RGB to gray
                    img = (img[0, ...] * 0.299 + img[1, ...] * 0.587 + img[2, ...] * 0.114).unsqueeze(0)
                ret[L] = img
            ret['path_' + str(L)] = self.paths[id]
        return ret

    def reshuffle(self, rng=random):
        """the reference's per-class reshuffle (wsgan_disc_dataset.py:54-56), with the generator given"""
        if self.synthetic:
            return
        for L in range(self.num_classes):
            rng.shuffle(self.attr_group_list[L])

    def __len__(self):
        # the reference reshuffles its class lists every time len() is taken; a loader that shuffles for all ranks alike sets
        # `external_shuffle` (data/__init__.py) and len() leaves the lists alone
        if not getattr(self, 'external_shuffle', False):
            self.reshuffle()
        return self.size
