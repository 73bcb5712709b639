#!/usr/bin/env python
"""Elo-rating encoder trainer with ONLINE PAIR SELECTION on the HIP path (reference siamese_online.py, `--mode train | embedding`).

One pass over the pair list.  Every batch is rated by `networks.SiameseNetwork` (ResNet trunk + 3x3 conv head, global pooling, ONE rating
per image), the pairs are ordered by squared rating distance, only the `--max_kept` hardest (`--pair_selector_type hard`: smallest
distance) or easiest (`easy`: largest) are trained on with the draw-aware binary cross entropy (+ `--lambda_regularization` times the
mean squared ratings), and the kept pairs are appended to <checkpoint_dir>/<name>/online.txt -- the list of pairs an annotator would be
asked about.  With `--use_pseudo_label` the same number of pairs from the OTHER end of the order follow, labelled with the net's own
prediction ("<a> <b> <pred>").  Ordering, selection, loss, regularizer, gradient and predictions are ONE launch (csrc/online_pair.hip via
functional.online_pair_bce); the host reads `picks` back once per iteration, AFTER optimizer.step() has been queued, where the reference
stalls three times before backward() can start.

LABEL CONVENTION: here label 0 means "the FIRST image rates higher", 1 a draw, 2 "the second rates higher" (target = (1, 0.5, 0)[label],
reference :329) -- the REVERSE of siamese.py, whose BinaryNLLLoss uses (0, 0.5, 1).  `--dataroot synthetic` follows this script's
convention: siamese.py's synthetic pairs with the labels 0 and 2 exchanged.

Flags and defaults are the reference's (:28-80), except `--display_id` (-1: no visdom here); `--gpu_transform`, `--seed` and
`--max_dataset_size` are siamese.py's.  `--num_epochs` is forced to 1 and an existing online.txt is removed when training starts, as in the
reference.  Accepted without effect, as in the reference's runnable path: `--min_kept` (with one rating channel every pair is "valid",
so the number kept is min(batch, max_kept)), `--lambda_contrastive` (its loss is commented out there), `--dropout` (the conv head's drop
layer only exists in its fc variant) and the validation set flags (display_val_acc is hard-wired off).

What the reference's own loop cannot run raises here: `--pair_selector_type random | softmax_hard | softmax_easy` (its loss unpacks two
values from selectors that return one), `--mode test` (test() is not defined), several rating channels or no global pooling
(LUT[label].view(N, -1) / dist2.reshape(N) need a (B, 1, 1, 1) score).  `--mode embedding` writes features_<epoch>.npy / labels_<epoch>.npy
through siamese.embedding, with the net in eval() as this script's get_model leaves it (:484).

    python siamese_online.py --dataroot synthetic --name online --pair_selector_type hard --max_kept 25 --pretrained_model_path ''
    python siamese_online.py --mode embedding --dataroot synthetic --name online
"""
import argparse
import os

import numpy as np
import torch

import siamese as S
from pcgan_amd.hip import parallel
from pcgan_amd.hip.optim import FusedAdam
from pcgan_amd.util.script import checkpoint_file, first_gpu, options_report, save_state, write_report

SELECTORS = {'hard': False, 'easy': True}       # -> descending: hard keeps the SMALLEST squared distances (:227-228)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    add = ap.add_argument
    add('--mode', type=str, default='train', help='train | embedding')
    add('--name', type=str, default='exp', help='experiment name')
    add('--dataroot', required=True, help='path to images, or `synthetic`')
    add('--datafile', type=str, default='', help='text file listing "<imageA> <imageB> <label>"')
    add('--dataroot_val', type=str, default='')
    add('--datafile_val', type=str, default='')
    add('--pretrained_model_path', type=str, default='', help='path to pretrained models')
    add('--checkpoint_dir', type=str, default='checkpoints')
    add('--save_epoch_freq', type=int, default=5, help='frequency of saving checkpoints')
    add('--num_workers', type=int, default=4, help='number of workers for data loader')
    add('--init_type', type=str, default='kaiming')
    add('--num_classes', type=int, default=3)
    add('--num_epochs', type=int, default=1, help='forced to 1')
    add('--batch_size', type=int, default=100)
    add('--lr', type=float, default=0.0002)
    add('--which_epoch', type=str, default='latest')
    add('--which_model', type=str, default='resnet18')
    add('--n_layers', type=int, default=3)
    add('--nf', type=int, default=64)
    add('--pooling', type=str, default='avg')
    add('--loadSize', type=int, default=224)
    add('--fineSize', type=int, default=224)
    add('--gpu_ids', type=str, default='0')
    add('--weight', nargs='+', type=float, default=[])
    add('--dropout', type=float, default=0.05)
    add('--finetune_fc_only', action='store_true')
    add('--fc_dim', type=int, nargs='+', default=[])
    add('--fc_relu_slope', type=float, default=0.3)
    add('--fc_residual', action='store_true')
    add('--cnn_dim', type=int, nargs='+', default=[64, 1])
    add('--cnn_pad', type=int, default=1)
    add('--cnn_relu_slope', type=float, default=0.7)
    add('--use_cxn', action='store_true')
    add('--lambda_regularization', type=float, default=0.0, help='weight for feature regularization loss')
    add('--lambda_contrastive', type=float, default=0.0)
    add('--print_freq', type=int, default=50)
    add('--display_id', type=int, default=-1)
    add('--display_port', type=int, default=8097)
    add('--transforms', type=str, default='resize_affine_crop')
    add('--affineScale', nargs='+', type=float, default=[0.95, 1.05])
    add('--affineDegrees', type=float, default=5)
    add('--use_color_jitter', action='store_true')
    add('--no_flip', action='store_true')
    add('--continue_train', action='store_true')
    add('--epoch_count', type=int, default=1)
    add('--min_kept', type=int, default=1)
    add('--max_kept', type=int, default=-1, help='pairs kept per batch (-1: --batch_size)')
    add('--save_latest_freq', type=int, default=10)
    add('--pair_selector_type', type=str, default='random', help='hard | easy (random, the default, cannot run in the reference either)')
    add('--serial_batches', action='store_true')
    add('--draw_prob_thresh', type=float, default=0.16)
    add('--a', type=float, default=1.0)
    add('--use_pseudo_label', action='store_true')
    add('--gpu_transform', action='store_true', help='(pcgan_amd) the image pipeline on the GPU, as in siamese.py')
    add('--seed', type=int, default=0)
    add('--max_dataset_size', type=int, default=1 << 30)
    return ap


def check_options(opt):
    """everything the reference's own loop cannot run, or that lies outside the HIP path, before any work is done"""
    if opt.mode == 'test':
        raise NotImplementedError('pcgan_amd: siamese_online.py --mode test is outside the MI355X hot path (the reference never defines '
                                  'its test(); use siamese.py --mode test)')
    if opt.mode not in ('train', 'embedding'):
        raise NotImplementedError('pcgan_amd: siamese_online.py --mode %s is outside the MI355X hot path (train | embedding)' % opt.mode)
    if 'resnet' not in opt.which_model:
        raise NotImplementedError('pcgan_amd: rating trunk [%s] is outside the MI355X hot path' % opt.which_model)
    if opt.finetune_fc_only:
        raise NotImplementedError('pcgan_amd: siamese_online.py --finetune_fc_only is outside the MI355X hot path')
    if opt.fc_dim or opt.use_cxn:
        raise NotImplementedError('pcgan_amd: SiameseNetwork with fc_dim / use_cxn is outside the MI355X hot path')
    if opt.use_color_jitter:
        raise NotImplementedError('pcgan_amd: siamese_online.py --use_color_jitter is outside the MI355X hot path')
    if opt.pooling not in ('avg', 'max') or not opt.cnn_dim or opt.cnn_dim[-1] != 1:
        raise NotImplementedError("pcgan_amd: siamese_online.py needs ONE rating per image (global --pooling avg | max and a last --cnn_dim "
                                  "of 1): the reference's loss and selector cannot run on any other score shape")
    if opt.mode == 'train' and opt.pair_selector_type not in SELECTORS:
        raise NotImplementedError("pcgan_amd: siamese_online.py --pair_selector_type %s is outside the MI355X hot path (hard | easy): the "
                                  "reference's own loop cannot run it -- its loss unpacks two values from a selector that returns one"
                                  % opt.pair_selector_type)
    if parallel.env_world()[0] > 1:
        raise NotImplementedError('pcgan_amd: siamese_online.py runs as ONE process: the reference does not define the selection over a '
                                  'batch that is sharded between processes')


def get_options(argv=None, save=True):
    """reference Options.get_options (:84-103); save=False neither removes online.txt nor writes opt.txt"""
    parser = build_parser()
    opt = parser.parse_args(argv)
    opt.isTrain = opt.mode == 'train'
    if opt.weight:
        assert len(opt.weight) == opt.num_classes
    if opt.max_kept < 0:
        opt.max_kept = opt.batch_size
    opt.num_epochs = 1
    check_options(opt)
    # what siamese.py's pieces read beside the flags above: the plain (not noisy, not Bayesian) encoder
    opt.noisy, opt.bayesian, opt.bnn_dropout, opt.rsample, opt.no_cnn, opt.T = False, False, 0.0, True, False, 1
    if opt.mode == 'train' and save:
        online = os.path.join(opt.checkpoint_dir, opt.name, 'online.txt')
        if os.path.exists(online):
            os.remove(online)
        report = options_report(parser, opt)       # the reference's option dump (:105-124), printed and kept as opt.txt
        print(report)
        write_report(report, os.path.join(opt.checkpoint_dir, opt.name))
    return opt


def parse_pair_lines(path, limit):
    """the non-empty lines of a pair list, newline-terminated; a label outside 0 .. 2 is an error HERE, not a wrong target later"""
    text = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            if not line.strip():
                continue
            fields = line.split()
            if len(fields) < 3 or fields[2] not in ('0', '1', '2'):
                raise ValueError('%s, line %d: "<imageA> <imageB> <label>" with a label of 0, 1 or 2 expected, got %r'
                                 % (path, number, line.rstrip('\n')))
            text.append(line if line.endswith('\n') else line + '\n')
    return text[:limit]


class OnlinePairDataset(S.PairDataset):
    """siamese.PairDataset whose items end in (label, index): `text[index]` is the pair's line, which stays on the host.  The synthetic
    pairs are siamese.py's with this script's label convention (0: the first hidden score is higher)."""

    def __init__(self, opt, root, listing):
        if root != 'synthetic':
            self.text = parse_pair_lines(listing, opt.max_dataset_size)
        super().__init__(opt, root, listing)
        if self.synthetic:
            self.text = ['syn_%05d_A.png syn_%05d_B.png %d\n' % (i, i, self.synthetic_label(i)) for i in range(self.n)]
        assert len(self.text) == self.n

    @staticmethod
    def synthetic_label(i):
        level = torch.rand(2, generator=torch.Generator().manual_seed(9000 + i))      # the first draw of PairDataset.__getitem__
        d = float(level[0] - level[1])
        return 1 if abs(d) < 0.1 else (0 if d > 0 else 2)

    def __getitem__(self, i):
        item = super().__getitem__(i)
        label = torch.tensor(self.synthetic_label(i)) if self.synthetic else item[-1]
        return item[:-1] + (label, torch.tensor(i))


def fetch_batch(batch, tf, device):
    """(img0, img1, label) on the device, and the labels and dataset indices of the batch on the host"""
    *rest, index = batch
    img0, img1, label = S.pair_batch(rest, tf, device)
    return img0, img1, label, rest[-1], index


def forward_loss(opt, net, img0, img1, label):
    """(total, loss3, picks) of one batch: the two ratings SiameseNetwork.forward returns go through the one-launch node"""
    from pcgan_amd.hip import functional as HF
    feat1, feat2 = net(img0, img1)[:2]
    k = min(feat1.numel(), opt.max_kept)
    return HF.online_pair_bce(feat1, feat2, label, k, SELECTORS[opt.pair_selector_type], opt.draw_prob_thresh, opt.lambda_regularization)


def backward_step(total, optimizer):
    """queue the backward pass (the node hands its stored gradient on: no launch for the factor) and the Adam step"""
    from pcgan_amd.hip import functional as HF
    total.backward(HF.unit_gradient(total))
    optimizer.step()


class OnlineLog:
    """online.txt and the counters of the reference's loop (:615-627, 638-639, 668)"""

    def __init__(self, opt, text):
        self.opt, self.text = opt, text
        self.path = os.path.join(opt.checkpoint_dir, opt.name, 'online.txt')
        self.cnt_online = self.cnt_online_diff = self.wrong = 0

    def record(self, picks, label, index):
        """picks: the node's buffer on the host (sel[k], pseudo[k], pred[N]); label, index: the batch's, on the host"""
        picks, label, index = np.asarray(picks), np.asarray(label).reshape(-1), np.asarray(index).reshape(-1)
        N = label.size
        k = (picks.size - N) // 2
        sel, pseudo, pred = picks[:k], picks[k:2 * k], picks[2 * k:]
        self.cnt_online += k
        with open(self.path, 'a') as f:
            for j in sel:
                line = self.text[index[j]]
                f.write(line)
                self.cnt_online_diff += int(line.split()[2]) != 1
            if self.opt.use_pseudo_label:
                for j in pseudo:
                    a, b = self.text[index[j]].split()[:2]
                    f.write('%s %s %d\n' % (a, b, pred[j]))
                    self.cnt_online_diff += int(pred[j]) != 1
        self.wrong += int(np.count_nonzero(pred - label))


def build_optimizer(opt, net):
    return FusedAdam(net.parameters(), lr=opt.lr)                              # optim.Adam(net.parameters(), lr) of the reference (:571)


def train(opt):
    torch.manual_seed(opt.seed)
    device = first_gpu(opt, 'siamese.py')      # (the error names the script whose device helper this was)
    net = S.build_net(opt, device)
    optimizer = build_optimizer(opt, net)
    data = OnlinePairDataset(opt, opt.dataroot, opt.datafile)
    print('dataset size = %d' % len(data))
    tf = S.gpu_pipeline(opt, data, device)
    loader = S.make_loader(opt, data, tf, batch_size=opt.batch_size, shuffle=not opt.serial_batches)
    save_dir = os.path.join(opt.checkpoint_dir, opt.name)
    os.makedirs(save_dir, exist_ok=True)
    log = OnlineLog(opt, data.text)
    history, total_iter = [], 0
    for epoch in range(opt.epoch_count, opt.num_epochs + opt.epoch_count):
        for batch in loader:
            img0, img1, label, label_host, index = fetch_batch(batch, tf, device)
            total_iter += 1
            optimizer.zero_grad()
            total, loss3, picks = forward_loss(opt, net, img0, img1, label)
            backward_step(total, optimizer)
            log.record(picks.cpu(), label_host, index)                          # THE device-to-host copy of the iteration
            if total_iter % opt.print_freq == 0:
                value = float(loss3[2])
                history.append(value)
                print('epoch %02d, iter %06d, loss: %.4f' % (epoch, total_iter, value))
            if total_iter % opt.save_latest_freq == 0:
                save_state(net, checkpoint_file(opt, 'latest'))
                if epoch % opt.save_epoch_freq == 0:
                    save_state(net, checkpoint_file(opt, epoch))
        print('epoch %02d: train accuracy %.4f' % (epoch, 1.0 - log.wrong / len(data)))
    with open(os.path.join(save_dir, 'loss.txt'), 'w') as f:
        f.writelines('%r\n' % v for v in history)
    print('!!! #labeled pairs %d #diff labeld pairs %d, ratio %.2f%%'
          % (log.cnt_online, log.cnt_online_diff, log.cnt_online_diff / log.cnt_online * 100))
    return log


def embedding(opt):
    device = first_gpu(opt, 'siamese.py')      # (the error names the script whose device helper this was)
    net = S.build_feature_net(opt, device).eval()
    return S.embedding(opt, net=net)


def main(argv=None):
    opt = get_options(argv)
    if opt.mode == 'train':
        return train(opt)
    return embedding(opt)


if __name__ == '__main__':
    main()
