"""Fixture generator of the online pair selection (test infrastructure).  Run ONCE where the reference is present:

    python scripts/make_online_golden.py            # writes tests/golden/online_select.npz

Like scripts/make_regression_golden.py it cuts what it needs out of the reference's script with `ast` at run time (the script as a whole
needs plotting packages that are not installed): PairSelector, EmbeddingDistancePairSelector and OnlineBinaryCrossEntropyLoss of
siamese_online.py.  The constructor's unconditional `.cuda()` (:329) is neutralised by patching torch.Tensor.cuda to the identity for
the duration of the run.  For (N, max_kept) in CASES, hard and easy, on seeded fp32 ratings with |f1 - f2| <= 30 (so that no fp32
intermediate of the reference's logsigmoid is subnormal: at |s| ~ 100 the CPU build of torch flushes them and relative errors explode)
it records the inputs, selected_pairs, pseudo_pairs, the loss, the autograd gradients of feat1 and feat2, and the regularization terms
of :631-633 as the two torch fp32 expressions compute them.  It asserts that no two keys are equal: numpy's default argsort, which the
reference uses, is not stable.  Only the .npz is committed; nothing that runs in the tests reads the reference.
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402

CASES = ((1, 1), (2, 5), (12, 5), (100, 100), (100, 37), (1024, 300), (4096, 4096))
CLASSES = ('PairSelector', 'EmbeddingDistancePairSelector', 'OnlineBinaryCrossEntropyLoss')
LAMBDA = 0.3


def reference_classes():
    path = os.path.join(G.REF, 'siamese_online.py')
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
    assert [n.name for n in body] == list(CLASSES)
    scope = {'torch': torch, 'nn': torch.nn, 'F': torch.nn.functional, 'np': np}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, 'exec'), scope)
    return scope


def ratings(N, seed):
    """fp32 ratings with |f1 - f2| <= 30 and pairwise distinct (f1 - f2)^2"""
    g = torch.Generator().manual_seed(seed)
    for _ in range(100):
        f2 = torch.randn(N, generator=g) * 3.0
        s = (torch.rand(N, generator=g) * 2.0 - 1.0) * 29.0
        f1 = f2 + s
        key = (f1 - f2).pow(2).numpy()
        if float((f1 - f2).abs().max()) <= 30.0 and np.unique(key).size == N:
            return f1, f2
    raise AssertionError('no tie-free draw for N = %d' % N)


def main():
    scope = reference_classes()
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {'cases': np.array(CASES), 'lambda_reg': np.array(LAMBDA, dtype=np.float32)}
    try:
        for N, max_kept in CASES:
            for hard in (True, False):
                tag = '%d_%d_%s' % (N, max_kept, 'hard' if hard else 'easy')
                f1, f2 = ratings(N, 1000 * N + max_kept + int(hard))
                label = torch.randint(0, 3, (N,), generator=torch.Generator().manual_seed(N + max_kept))
                feat1 = f1.view(N, 1, 1, 1).clone().requires_grad_(True)
                feat2 = f2.view(N, 1, 1, 1).clone().requires_grad_(True)
                selector = scope['EmbeddingDistancePairSelector'](min_kept=1, max_kept=max_kept, hard=hard)
                criterion = scope['OnlineBinaryCrossEntropyLoss'](pair_selector=selector)
                loss, selected, pseudo = criterion(feat1 - feat2, label, feat1, feat2)
                loss.backward()
                key = (feat1.detach() - feat2.detach()).pow(2).numpy().reshape(N)
                assert np.unique(key).size == N, tag + ': equal keys'
                reg1, reg2 = feat1.detach().pow(2).mean(), feat2.detach().pow(2).mean()       # :631-632
                out[tag + '/f1'] = f1.numpy()
                out[tag + '/f2'] = f2.numpy()
                out[tag + '/label'] = label.numpy().astype(np.int8)
                out[tag + '/sel'] = np.asarray(selected).astype(np.int16)
                out[tag + '/pseudo'] = np.asarray(pseudo).astype(np.int16)
                out[tag + '/loss'] = G.t2n(loss)
                out[tag + '/df1'] = G.t2n(feat1.grad).reshape(N)
                out[tag + '/df2'] = G.t2n(feat2.grad).reshape(N)
                out[tag + '/reg'] = np.array([float(reg1), float(reg2), float((reg1 + reg2) * LAMBDA)], dtype=np.float32)
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(ROOT, 'tests', 'golden', 'online_select.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d arrays, %.1f KB' % (path, len(out), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
