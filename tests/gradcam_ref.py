"""Float64 restatements of `siamese.py --mode attention`'s device steps, written from the formulas of include/pcgan_hip.h: the four map
types of util/gradcam.py: generate, the `input` type (d rating / d image) and the heat-map overlay with its hi == lo rule.  Every
function also returns the quantity the tests' error bounds are stated in."""
import numpy as np
import torch
import torch.nn.functional as F

MAP_TYPES = ('raw', 'pw', 'cw_pos', 'pw_cw')


def _f64(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def plane_weights(g):
    """w[n, c] = the mean over the plane of relu(g[n, c])"""
    return np.maximum(_f64(g), 0.0).mean(axis=(2, 3))


def terms(act, grad, kind):
    """the (N, C, H, W) float64 terms the map sums over c"""
    A = _f64(act)
    if kind == 'raw':
        return A
    g = _f64(grad)
    if kind == 'pw':
        return g * A
    w = plane_weights(g)[:, :, None, None]
    return w * A if kind == 'cw_pos' else w * g * A


def gradcam_map(act, grad, kind):
    """(map (N, 1, H, W), mass = sum_c |term| (N, 1, H, W)) in float64"""
    t = terms(act, grad, kind)
    s = t.sum(axis=1, keepdims=True)
    return (np.abs(s) if kind == 'raw' else np.maximum(s, 0.0)), np.abs(t).sum(axis=1, keepdims=True)


def gradcam_map_conv3d(act, grad, kind):
    """the weighted types as the reference writes them (util/gradcam.py:233-249): AvgPool2d of relu(g) as the weight of a grouped conv3d
    with groups = N over the batch laid out as channels; float64 torch"""
    A, g = torch.from_numpy(_f64(act)), torch.from_numpy(_f64(grad))
    x = g * A if kind == 'pw_cw' else A
    weights = F.avg_pool2d(F.relu(g), tuple(g.shape[2:]))[:, None, :, :, :]
    out = F.relu(F.conv3d(x[None], weights, padding=0, groups=len(weights)))
    return out.squeeze(0).numpy()


def input_gradient(net, image):
    """d sum(rating) / d image of a float64 torch twin (the first output is the rating)"""
    x = image.detach().clone().requires_grad_(True)
    out = net(x)
    rating = out[0] if isinstance(out, (tuple, list)) else out
    (g,) = torch.autograd.grad(rating.sum(), x)
    return g


def overlay(hmap, img, mean, std, alpha):
    """(out (N, 3, H, W), lohi (N, 2), pix = (img * std + mean) * 255) in float64; mean, std and alpha are taken at their fp32 values,
    which is what the kernel receives.  Where hi == lo the heat term is 0."""
    m, x = _f64(hmap), _f64(img)
    mean = np.asarray(mean, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    std = np.asarray(std, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    alpha = float(np.float32(alpha))
    N = m.shape[0]
    lo = m.reshape(N, -1).min(axis=1)
    hi = m.reshape(N, -1).max(axis=1)
    heat = np.zeros_like(x)
    for n in range(N):
        if hi[n] > lo[n]:
            heat[n] = np.broadcast_to((m[n] - lo[n]) / (hi[n] - lo[n]) * 255.0, x[n].shape)
    pix = (x * std + mean) * 255.0
    return heat * (1.0 - alpha) + pix * alpha, np.stack([lo, hi], axis=1), pix
