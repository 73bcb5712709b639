"""Pair dataset of the continuous-label baseline (reference data/wsgan_cont_dataset.py:11-92): each line of `--sourcefile_A` is
"<fileA> <fileB> <label>" with label 0: A<B, 1: A=B, 2: A>B, and each image's attribute value (an age, say) is parsed from its file
name ("<attr>_<rest>").  Batch dict: 'A', 'B' (C,S,S), 'A_attr', 'B_attr' (1,1,1), 'label', 'A_paths', 'B_paths'; under
`--no_mixed_label_D` one such set per label present, keyed '<L>_A' ..., index taken modulo each label's list.

`--dataroot synthetic` short-circuits to seeded synthetic samples of the same dict layout (U[-1,1) images, attributes U[0,60),
labels 0, 1 and 2)."""
import os.path
import random

import torch

from .base_dataset import BaseDataset, get_transform, decode_raw
from ..util.util import get_attr_value


class WSGANContDataset(BaseDataset):
    @staticmethod
    def modify_commandline_options(parser, is_train):
        return parser

    def name(self):
        return 'WSGANContDataset'

    def initialize(self, opt):
        self.opt = opt
        self.root = opt.dataroot
        self.synthetic = (opt.dataroot == 'synthetic')
        self.per_label = bool(getattr(opt, 'no_mixed_label_D', False))      # a training flag of the model: absent at test time
        if self.synthetic:
            self.size = int(min(opt.max_dataset_size, 64 * opt.batchSize))
            return
        with open(opt.sourcefile_A, 'r') as f:
            self.sourcefile = [line.rstrip('\n') for line in f.readlines()]
        if self.per_label:
            per = {L: [] for L in range(len(opt.relabel_D))}
            for line in self.sourcefile:
                per[int(line.split()[2])].append(line)
            self.sourcefiles = {L: v for L, v in per.items() if v}
            self.size = min(max(len(v) for v in self.sourcefiles.values()), opt.max_dataset_size)
        else:
            self.size = min(len(self.sourcefile), opt.max_dataset_size)
        self.transform = get_transform(opt)
        self.raw = bool(getattr(opt, 'gpu_transform', False))     # workers decode, the loader finishes the batch on the GPU

    def _pair(self, line, prefix=''):
        """the entries of one pair line, keys prefixed ('' or '<L>_'); the label entry is the caller's"""
        from PIL import Image
        fa, fb = line.split()[:2]
        pa, pb = os.path.join(self.root, fa), os.path.join(self.root, fb)
        ret = {prefix + 'A_attr': torch.Tensor([get_attr_value(fa)]).reshape(1, 1, 1),
               prefix + 'B_attr': torch.Tensor([get_attr_value(fb)]).reshape(1, 1, 1),
               prefix + 'A_paths': pa, prefix + 'B_paths': pb}
        if self.raw:
            # same draws, same order as the PIL path; the per-pixel work and the gray mix are one launch per batch in the loader
            ret[prefix + 'A_raw'], ret[prefix + 'A_aug'] = decode_raw(Image.open(pa).convert('RGB'), self.opt)
            ret[prefix + 'B_raw'], ret[prefix + 'B_aug'] = decode_raw(Image.open(pb).convert('RGB'), self.opt)
            return ret
        A = self.transform(Image.open(pa).convert('RGB'))
        B = self.transform(Image.open(pb).convert('RGB'))
        if self.opt.input_nc == 1:
            A = (A[0] * 0.299 + A[1] * 0.587 + A[2] * 0.114).unsqueeze(0)
        if self.opt.output_nc == 1:
            B = (B[0] * 0.299 + B[1] * 0.587 + B[2] * 0.114).unsqueeze(0)
        ret[prefix + 'A'], ret[prefix + 'B'] = A, B
        return ret

    def _synthetic(self, index, prefix=''):
        o = self.opt
        g = torch.Generator().manual_seed(2468 + index)
        s = o.fineSize
        A = torch.rand(o.input_nc, s, s, generator=g) * 2 - 1
        B = torch.rand(o.output_nc, s, s, generator=g) * 2 - 1
        attr = torch.rand(2, generator=g) * 60.0
        label = int(torch.randint(0, 3, (1,), generator=g))
        return {prefix + 'A': A, prefix + 'B': B, prefix + 'A_attr': attr[0].reshape(1, 1, 1), prefix + 'B_attr': attr[1].reshape(1, 1, 1),
                prefix + 'A_paths': '%d_synthetic_A_%d' % (int(attr[0]), index),
                prefix + 'B_paths': '%d_synthetic_B_%d' % (int(attr[1]), index)}, label

    def __getitem__(self, index):
        o = self.opt
        if self.synthetic:
            if not self.per_label:
                ret, label = self._synthetic(index)
                ret['label'] = label
                return ret
            ret = {}
            for L in range(len(o.relabel_D)):
                ret.update(self._synthetic(index * len(o.relabel_D) + L, str(L) + '_')[0])
            return ret
        if not self.per_label:
            line = self.sourcefile[index]
            ret = self._pair(line)
            ret['label'] = int(line.split()[2])
            return ret
        ret = {}
        for L, lines in self.sourcefiles.items():
            ret.update(self._pair(lines[index % len(lines)], str(L) + '_'))
        return ret

    def reshuffle(self, rng=random):
        """the reference's pair-list reshuffle (wsgan_cont_dataset.py:82-89), with the generator given"""
        if self.synthetic:
            return
        if not self.per_label:
            rng.shuffle(self.sourcefile)
        else:
            for L in self.sourcefiles:
                rng.shuffle(self.sourcefiles[L])

    def __len__(self):
        # the reference reshuffles its pair list every time len() is taken; under torch.distributed the loader does it once per epoch
        # with a generator shared by all ranks (`external_shuffle`, data/__init__.py) and len() leaves the list alone
        if not getattr(self, 'external_shuffle', False):
            self.reshuffle()
        return self.size
