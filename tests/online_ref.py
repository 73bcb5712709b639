"""float64 numpy restatement of pcgan_online_pair_bce (include/pcgan_hip.h; reference siamese_online.py:218-265, 324-342, 385-394,
630-635): the order, sel, pseudo, the three losses, the gradients and the predictions, plus the quantities the tests' bounds are stated in.

The rules, the same as the header's:
  s = f1 - f2 and key = s * s in fp32 (the bits of the reference's (A - B).pow(2)) unless a key is given; ascending by key, equal keys by
  ascending index (a stable sort; -0 == +0, NaN after +inf as numpy sorts); descending = the exact reverse of that list; sel = the first
  k, pseudo = the last k; target = (1, 0.5, 0)[label] -- label 0: the FIRST rates higher; everything after the key in float64 from the
  fp32 inputs; draw_thresh, lambda_reg and gscale are the fp32 values the C-ABI carries, widened.
"""
import numpy as np

TARGET = np.array([1.0, 0.5, 0.0])


def order_of(key, descending):
    """indices in the order of the rules above; key: fp32"""
    key = np.asarray(key, dtype=np.float32)
    order = np.argsort(key, kind='stable')
    return order[::-1].copy() if descending else order


def logsigmoid(x):
    return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def online_pair_bce(f1, f2, label, k, descending, draw_thresh, lambda_reg, gscale=1.0, key=None):
    """dict(order, sel, pseudo, pred, loss[3] (float64), df1, df2 (float64), and the bound quantities: mean_abs_term (mean |term| over
    sel), min_key_gap (smallest gap between adjacent sorted keys, inf for N = 1), min_p_margin (smallest distance of any p to 0.5 and to
    0.5 +- draw_thresh))"""
    f1 = np.asarray(f1, dtype=np.float32).reshape(-1)
    f2 = np.asarray(f2, dtype=np.float32).reshape(-1)
    label = np.clip(np.asarray(label).reshape(-1).astype(np.int64), 0, 2)
    N, k = f1.size, int(k)
    assert f2.size == N and label.size == N and 1 <= k <= N
    thr, lam, gs = (float(np.float32(v)) for v in (draw_thresh, lambda_reg, gscale))
    s32 = f1 - f2                                                           # fp32
    key32 = s32 * s32 if key is None else np.asarray(key, dtype=np.float32).reshape(-1)
    order = order_of(key32, descending)
    sel, pseudo = order[:k], order[N - k:]
    kept = np.zeros(N, dtype=bool)
    kept[sel] = True
    s = s32.astype(np.float64)
    t = TARGET[label]
    with np.errstate(over='ignore', invalid='ignore'):
        term = -(t * logsigmoid(s) + (1.0 - t) * logsigmoid(-s))
        p = sigmoid(s)
    a, b = f1.astype(np.float64), f2.astype(np.float64)
    l0 = float(np.sum(term[kept])) / k
    l1 = lam * (float(np.sum(a * a)) / N + float(np.sum(b * b)) / N) if lam != 0.0 else 0.0
    pt = np.where(label == 0, -sigmoid(-s), np.where(label == 1, p - 0.5, p))       # p - t; for t = 1 as -sigmoid(-s): no cancellation
    g = np.where(kept, pt / k, 0.0)
    df1 = gs * (g + lam * 2.0 * a / N)
    df2 = gs * (-g + lam * 2.0 * b / N)
    draw = np.abs(0.5 - p) < thr
    pred = np.where(draw, 1, np.where(p > 0.5, 0, 2)).astype(np.int32)
    sk = np.sort(key32[~np.isnan(key32)].astype(np.float64))
    with np.errstate(invalid='ignore'):
        gaps = np.diff(sk)
    margin = np.minimum(np.abs(p - 0.5), np.minimum(np.abs(p - (0.5 + thr)), np.abs(p - (0.5 - thr))))
    return dict(order=order, sel=sel.astype(np.int32), pseudo=pseudo.astype(np.int32), pred=pred, loss=np.array([l0, l1, l0 + l1]),
                df1=df1, df2=df2, p=p, mean_abs_term=float(np.mean(np.abs(term[kept]))),
                min_key_gap=float(gaps.min()) if gaps.size else float('inf'), min_p_margin=float(margin.min()))


def picks_of(ref):
    """the kernel's picks buffer: sel, pseudo, pred"""
    return np.concatenate([ref['sel'], ref['pseudo'], ref['pred']]).astype(np.int32)
