"""What the stand-alone scripts share (classification.py, regression.py, siamese.py, siamese_online.py, compute_inception_score.py): the
option report, the device, the reference's initialisation, checkpoints and their paths, seeding, the normalising transform and the epoch
loop of the two attribute trainers.  Each script imports the names it publishes from here.
"""
import math
import os
import random

import numpy as np
import torch

from ..hip import parallel

MEAN = (0.4914, 0.4822, 0.4465)      # transforms.Normalize of the reference's get_transform: the CIFAR statistics
STD = (0.2023, 0.1994, 0.2010)


def options_report(parser, opt, header='--------------- Options -----------------'):
    """the reference's option dump: one `name: value` row per option in sorted order, values that differ from the parser's default
    marked, between `header` and the End rule"""
    rows = [header]
    for key, value in sorted(vars(opt).items()):
        default = parser.get_default(key)
        note = '\t[default: %s]' % (default,) if value != default else ''
        rows.append('%25s: %-30s%s' % (key, value, note))
    rows.append('----------------- End -------------------')
    return '\n'.join(rows)


def write_report(report, folder):
    """keep the report as <folder>/opt.txt"""
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, 'opt.txt'), 'w') as f:
        f.write(report + '\n')


def first_gpu(opt, script, index=None):
    """the device of the first id of --gpu_ids (of `index`, where the caller knows better: one process per GPU), made current"""
    gpu = int(opt.gpu_ids.split(',')[0]) if opt.gpu_ids else -1
    if gpu < 0 or not torch.cuda.is_available():
        raise RuntimeError('pcgan_amd: %s needs an MI355X (no CPU fallback)' % script)
    device = torch.device('cuda', gpu if index is None else index)
    torch.cuda.set_device(device)
    return device


def init_like_reference(net, linear):
    """weights_init of the reference's scripts: every convolution (and, with `linear`, every Linear weight) ~ N(0, 0.02), every
    BatchNorm2d scale ~ N(1, 0.02) with a zero shift; a Linear bias keeps nn.Linear's own.  Layers are visited in registration order, so
    the draws come out of torch's generator in the reference's order (pinned by tests/golden/classification_step.npz: <trunk>/init/*)."""
    with torch.no_grad():
        for m in net.modules():
            kind = type(m).__name__
            if 'Conv' in kind or (linear and 'Linear' in kind):
                m.weight.normal_(0.0, 0.02)
            elif 'BatchNorm2d' in kind:
                m.weight.normal_(1.0, 0.02)
                m.bias.zero_()


def seed_everything(seed):
    if seed is not None:
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)


def checkpoint_file(opt, epoch):
    """<checkpoint_dir>/<name>/<epoch>_net.pth; epoch: a number, 'latest' or 'init'"""
    return os.path.join(opt.checkpoint_dir, opt.name, '%s_net.pth' % epoch)


def save_state(net, path):
    """the state dict on the host, written by rank 0 alone"""
    if not parallel.is_distributed() or torch.distributed.get_rank() == 0:
        torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, path)


def normalized_transform(opt, modes):
    """PIL image -> the PIL steps of --transforms (one of `modes`), ToTensor, Normalize with MEAN and STD"""
    from ..data.base_dataset import pil_steps, to_tensor
    if opt.transforms not in modes:
        raise ValueError('--resize_or_crop %s is not a valid option.' % opt.transforms)
    mean = torch.tensor(MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(3, 1, 1)
    return lambda img: (to_tensor(pil_steps(opt, img)) - mean) / std


def run_epochs(opt, net, loader, loader_val, label_of, forward, backward, save_dir):
    """the epoch loop of classification.py and regression.py (reference classification.py:344-469, regression.py:336-428) for a net that
    is on its device.  label_of(names) -> the batch's labels on the device; forward(img, label) -> (loss, hits), one node, device
    scalars; backward(loss).  Writes init_net.pth (the weights before the first iteration), latest_net.pth after every epoch,
    <epoch>_net.pth every --save_epoch_freq and <save_dir>/loss.txt, one line per iteration; returns those losses.  The loss is read on
    the host at --print_freq and once per epoch, the hit count once per epoch."""
    from ..hip.optim import FusedAdam
    device = next(net.parameters()).device
    optimizer = FusedAdam(net.parameters(), lr=opt.lr)         # optim.Adam(net.parameters(), lr=opt.lr): betas (0.9, 0.999)
    save_state(net, checkpoint_file(opt, 'init'))
    dataset_size = len(loader.dataset)
    iters_per_epoch = math.ceil(dataset_size / opt.batch_size)
    loss_history, total_iter = [], 0
    seed_everything(opt.seed)      # the augmentation draws of the first epoch start from the seed, whatever the initialisation consumed
    for epoch in range(opt.epoch_count, opt.num_epochs + opt.epoch_count):
        step_losses = []                                                     # device scalars: read once, when the epoch ends
        hits = torch.zeros((), dtype=torch.int32, device=device)
        for img0, path0 in loader:
            label = label_of(path0)
            img0 = img0.to(device)
            total_iter += 1
            optimizer.zero_grad()
            loss, correct = forward(img0, label)
            backward(loss)
            optimizer.step()
            step_losses.append(loss.detach())
            hits += correct
            if total_iter % opt.print_freq == 0:
                print('epoch %02d, iter %06d, loss: %.4f' % (epoch, total_iter, loss.item()))
        assert len(step_losses) == iters_per_epoch
        loss_history += torch.stack(step_losses).cpu().tolist()
        curr_acc = {'train': int(hits) / dataset_size}                       # 1 - err_train
        if loader_val is not None:
            # as in the reference eval mode is NOT entered: BatchNorm normalises each validation image with its own statistics and the
            # running statistics keep moving.  Kept on purpose; only autograd's bookkeeping is switched off.
            hits_val = torch.zeros((), dtype=torch.int32, device=device)
            with torch.no_grad():
                for img0, path0 in loader_val:
                    label = label_of(path0)
                    hits_val += forward(img0.to(device), label)[1]
            curr_acc['val'] = int(hits_val) / len(loader_val.dataset)
        print('epoch %02d: ' % epoch + ', '.join('%s accuracy %.4f' % kv for kv in curr_acc.items()))
        save_state(net, checkpoint_file(opt, 'latest'))
        if epoch % opt.save_epoch_freq == 0:
            save_state(net, checkpoint_file(opt, epoch))
    with open(os.path.join(save_dir, 'loss.txt'), 'w') as f:
        for value in loss_history:
            f.write(str(value) + '\n')
    return loss_history
