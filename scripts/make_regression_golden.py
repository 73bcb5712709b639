"""Fixture generator of the attribute regressor (test infrastructure).  Run ONCE where the reference is present:

    python scripts/make_regression_golden.py            # writes tests/golden/regression_step.npz

Like scripts/make_classification_golden.py it IMPORTS the reference's models/networks.py on the CPU (oracle.make_golden's import with
the torchvision stub), fills networks.RegressionNetwork with the deterministic weights of oracle/weights.py and records what ONE
training step of the reference's regression.py computes (criterion(net.forward(x), label).backward(); Adam.step(), :357-366) for
  resnet18 + cnn_dim [64, 1] + avg at 64 x 64        (a 2 x 2 map under the pooling)
  alexnet  + cnn_dim [64, 1] + max at 63 x 63        (the smallest input the stride-4 stem and the three 3/2 poolings allow: 1 x 1)
batch 6: the output, the loss, the within-delta flags of get_accuracy, parameter gradients, parameters after the step and running
statistics -- statistics plus a strided sample per tensor, the conv head's last layer in full -- and the state_dict key list.  It also
records the reference's seeded initialisation (net.apply(weights_init), :171-179; the function is read out of the reference's script,
which as a whole needs plotting packages that are not installed).  Only the .npz is committed; nothing that runs in the tests reads
the reference.
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
CASES = (('resnet18', 'avg', 64, 170), ('alexnet', 'max', 63, 171))       # (trunk, pooling, image size, weight seed); batch 6
CNN_DIM = [64, 1]
# one target per image, chosen beside the recorded outputs so that get_accuracy finds some inside DELTA and some outside
TARGETS = {'resnet18': (-0.25, 0.15, 0.30, -0.17, 0.90, -0.30), 'alexnet': (-0.02, 0.40, 0.12, -0.30, 0.10, 0.45)}
DELTA = 0.05
LR = 2e-4
INIT_SEED = 5


def summary(named, prefix, out):
    """per tensor (sum, abs-sum, l2) in float64 and every STRIDE-th element; the last layer of the conv head in full"""
    for k, t in named:
        a = G.t2n(t).astype(np.float64)
        out['%s/stat/%s' % (prefix, k)] = np.array([a.sum(), np.abs(a).sum(), np.sqrt((a * a).sum())])
        if k.startswith('cnn.3.'):
            out['%s/full/%s' % (prefix, k)] = G.t2n(t)
        else:
            out['%s/samp/%s' % (prefix, k)] = G.t2n(t).reshape(-1)[::STRIDE].copy()


def reference_function(name):
    """a top-level function cut out of the reference's regression.py"""
    path = os.path.join(G.REF, 'regression.py')
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name][0]
    scope = {'torch': torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, 'exec'), scope)
    return scope[name]


def build(rn, which, pooling):
    base = rn.AlexNetFeature(3, pooling='') if which == 'alexnet' else rn.ResNetFeature(3, which)      # regression.py:248-251
    return rn.RegressionNetwork(base, pooling=pooling, cnn_dim=CNN_DIM, cnn_pad=1, cnn_relu_slope=0.7)


def main():
    rn = G.import_reference()
    get_accuracy = reference_function('get_accuracy')
    out = {'delta': np.array(DELTA), 'lr': np.array(LR), 'stride': np.array(STRIDE),
           'init_seed': np.array(INIT_SEED), 'cnn_dim': np.array(CNN_DIM)}
    for which, pooling, size, seed in CASES:
        TARGET = TARGETS[which]
        out['%s/target' % which] = np.array(TARGET, dtype=np.float32)
        net = build(rn, which, pooling)
        net.load_state_dict(W.fill_state_dict(net.state_dict(), seed))
        net.train()
        x = W.seeded_tensor((len(TARGET), 3, size, size), 100 + seed)
        label = torch.tensor(TARGET).view(len(TARGET), net.feature_dim, 1, 1)
        opt = torch.optim.Adam(net.parameters(), lr=LR)
        opt.zero_grad()
        output = net.forward(x)
        loss = torch.nn.MSELoss()(output, label)
        flags = get_accuracy(output, label, DELTA)
        loss.backward()
        out['%s/case' % which] = np.array([size, seed])
        out['%s/pooling' % which] = np.array(pooling)
        out['%s/keys' % which] = np.array(list(net.state_dict().keys()))
        out['%s/out' % which] = G.t2n(output)
        out['%s/loss' % which] = G.t2n(loss)
        out['%s/within' % which] = np.asarray(flags)
        summary([(k, p.grad) for k, p in net.named_parameters()], which + '/dparam', out)
        opt.step()
        summary(list(net.named_parameters()), which + '/param_after', out)
        for k, b in net.named_buffers():
            if 'running' in k:
                a = G.t2n(b).astype(np.float64)
                out['%s/buf/%s' % (which, k)] = np.array([a.sum(), np.abs(a).sum()])
            else:
                out['%s/buf/%s' % (which, k)] = G.t2n(b)
    # the seeded initialisation of regression.py's get_model
    init = reference_function('weights_init')
    for which, pooling, _, _ in CASES:
        torch.manual_seed(INIT_SEED)
        net = build(rn, which, pooling)
        net.apply(init)
        for k, t in net.state_dict().items():
            if 'num_batches' not in k:
                a = G.t2n(t).astype(np.float64)
                out['%s/init/%s' % (which, k)] = np.array([a.sum(), np.abs(a).sum()])
    path = os.path.join(ROOT, 'tests', 'golden', 'regression_step.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d arrays, %.1f KB' % (path, len(out), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
