"""Inception Score (reference util/inception_score.py:13-67, used by compute_inception_score.py).

The class probabilities come from a classifier on the HIP path (pcgan_amd/models/inception.py: InceptionV3Classifier, or
pcgan_amd/models/networks.py: ResNet), batch by batch; the score itself is host code in float64, as in the reference: per split of
N // splits rows, py = the split's mean row, the mean of scipy.stats.entropy(pyx, py) over its rows -- both arguments renormalised,
rel_entr with 0 log 0 = 0 -- exponentiated; the trailing N % splits rows are dropped.  It is an (N x classes) problem solved once per
evaluation, not a hot path."""
import numpy as np
from scipy.special import rel_entr


def predictions(imgs, predict, num_classes=1000, batch_size=32, verbose=True):
    """(N, num_classes) float64 probabilities of the dataset `imgs` (len / indexing, items (3, H, W) tensors), in batches of
    batch_size taken in index order (the last one may be partial) -- the reference's unshuffled DataLoader.  predict(batch) returns the
    (b, num_classes) probabilities of a (b, 3, H, W) float32 batch (a tensor on any device, or an array)."""
    import torch
    N = len(imgs)
    preds = np.zeros((N, num_classes))
    for i, start in enumerate(range(0, N, batch_size)):
        batch = torch.stack([imgs[j] for j in range(start, min(N, start + batch_size))])
        p = predict(batch)
        p = p.detach().double().cpu().numpy() if torch.is_tensor(p) else np.asarray(p, dtype=np.float64)
        if p.shape != (batch.shape[0], num_classes):
            raise ValueError('predict returned %s for a batch of %d images and %d classes' % (p.shape, batch.shape[0], num_classes))
        preds[start:start + batch.shape[0]] = p
        if verbose:
            print('--> batch #%d' % (i + 1))
    return preds


def score(preds, splits=1):
    """(mean, std) over `splits` splits of exp(mean_i KL(p(y|x_i) || p(y))) for an (N, classes) matrix of probabilities"""
    preds = np.asarray(preds, dtype=np.float64)
    N = preds.shape[0]
    split_scores = []
    for k in range(splits):
        part = preds[k * (N // splits): (k + 1) * (N // splits), :]
        py = np.mean(part, axis=0)
        # scipy.stats.entropy(pyx, py) for every row at once: both arguments normalised to sum 1, then sum(rel_entr)
        pk = part / np.sum(part, axis=1, keepdims=True)
        qk = py / np.sum(py)
        kl = np.sum(rel_entr(pk, qk[None, :]), axis=1)
        split_scores.append(np.exp(np.mean(kl)))
    return np.mean(split_scores), np.std(split_scores)


def inception_score(imgs, predict, num_classes=1000, batch_size=32, splits=1, verbose=True):
    """the reference's inception_score(imgs, model, num_classes, cuda, batch_size, resize, splits): `predict` stands for
    softmax(model(resize(batch)))"""
    N = len(imgs)
    assert batch_size > 0
    assert N > batch_size
    return score(predictions(imgs, predict, num_classes, batch_size, verbose), splits)
