"""Fixture generator of the attribute classifier (test infrastructure).  Run ONCE where the reference is present:

    python scripts/make_classification_golden.py            # writes tests/golden/classification_step.npz

Like oracle/make_golden.py (whose reference import with the torchvision stub it reuses) it IMPORTS the reference's models/networks.py on
the CPU, fills networks.ResNet with the deterministic weights of oracle/weights.py and records what ONE training step of the reference's
classification.py computes (criterion(net.forward(x), y).backward(); Adam.step(), :374-384) for resnet18 and resnet50: logits, the loss
with and without class weights, predictions, parameter gradients, running statistics and parameters after the step -- statistics plus a
strided sample for the trunk tensors, `fc` in full.  It also records the reference's seeded initialisation (net.apply(weights_init),
:177-185; the function is read out of the reference's script, which as a whole needs plotting packages that are not installed).
Only the .npz is committed; nothing that runs in the tests reads the reference.
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import weights as W  # noqa: E402

STRIDE = 997
CASES = (('resnet18', 64, 70), ('resnet50', 96, 71))       # (trunk, image size, weight seed); batch 6, 5 classes
LABELS = (0, 4, 2, 2, 1, 3)
CLASS_WEIGHT = (1.0, 0.5, 2.0, 1.0, 0.25)
LR = 2e-4
INIT_SEED = 5


def summary(named, prefix, out):
    """per tensor (sum, abs-sum, l2) in float64 and every STRIDE-th element; `fc` tensors in full"""
    for k, t in named:
        a = G.t2n(t).astype(np.float64)
        out['%s/stat/%s' % (prefix, k)] = np.array([a.sum(), np.abs(a).sum(), np.sqrt((a * a).sum())])
        if '.fc.' in k:
            out['%s/full/%s' % (prefix, k)] = G.t2n(t)
        else:
            out['%s/samp/%s' % (prefix, k)] = G.t2n(t).reshape(-1)[::STRIDE].copy()


def reference_weights_init():
    """the reference's weights_init, cut out of its classification.py"""
    path = os.path.join(G.REF, 'classification.py')
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'weights_init'][0]
    scope = {}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, 'exec'), scope)
    return scope['weights_init']


def main():
    rn = G.import_reference()
    out = {'labels': np.array(LABELS), 'class_weight': np.array(CLASS_WEIGHT, dtype=np.float32), 'lr': np.array(LR),
           'stride': np.array(STRIDE), 'init_seed': np.array(INIT_SEED)}
    y = torch.tensor(LABELS)
    wgt = torch.tensor(CLASS_WEIGHT)
    for which, size, seed in CASES:
        net = rn.ResNet(3, len(CLASS_WEIGHT), which)
        net.load_state_dict(W.fill_state_dict(net.state_dict(), seed))
        net.train()
        x = W.seeded_tensor((len(LABELS), 3, size, size), 100 + seed)
        opt = torch.optim.Adam(net.parameters(), lr=LR)
        opt.zero_grad()
        logits = net.forward(x)
        loss = torch.nn.CrossEntropyLoss(weight=wgt)(logits, y)
        out['%s/loss_plain' % which] = G.t2n(torch.nn.CrossEntropyLoss()(logits, y))
        loss.backward()
        out['%s/case' % which] = np.array([size, seed])
        out['%s/logits' % which] = G.t2n(logits)
        out['%s/loss' % which] = G.t2n(loss)
        out['%s/pred' % which] = logits.detach().numpy().argmax(axis=1)
        summary([(k, p.grad) for k, p in net.named_parameters()], which + '/dparam', out)
        opt.step()
        summary(list(net.named_parameters()), which + '/param_after', out)
        for k, b in net.named_buffers():
            if 'running' in k:
                a = G.t2n(b).astype(np.float64)
                out['%s/buf/%s' % (which, k)] = np.array([a.sum(), np.abs(a).sum()])
            else:
                out['%s/buf/%s' % (which, k)] = G.t2n(b)
    # the seeded initialisation of classification.py's get_model
    init = reference_weights_init()
    for which in ('resnet18', 'resnet50'):
        torch.manual_seed(INIT_SEED)
        net = rn.ResNet(3, 5, which)
        net.apply(init)
        for k, t in net.state_dict().items():
            if 'num_batches' not in k:
                a = G.t2n(t).astype(np.float64)
                out['%s/init/%s' % (which, k)] = np.array([a.sum(), np.abs(a).sum()])
    path = os.path.join(ROOT, 'tests', 'golden', 'classification_step.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d arrays, %.1f KB' % (path, len(out), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
