"""Float64 restatement of Pillow's `Image.transform(size, Image.AFFINE, m, Image.BICUBIC, fillcolor=127)` on RGB images -- the
warp of the loader's two affine modes (reference data/base_dataset.py:41-52, RandomAffine with BICUBIC and fillcolor=127) -- and of
the whole affine pipeline of get_transform after the draws (resize -> warp -> crop -> flip -> ToTensor -> Normalize).

Pillow (libImaging/Geometry.c: affine_transform, bicubic_filter32RGB), per output pixel (x, y) and channel:
  xi = (m0 * (x + .5) + m1 * (y + .5)) + m2,  yi = (m3 * (x + .5) + m4 * (y + .5)) + m5   (double, no fma)
  outside [0, W) x [0, H): the fill -- Image.new('RGB', ..., 127) is (127, 0, 0)
  else xi -= .5, yi -= .5; x0 = floor(xi), y0 = floor(yi); dx, dy the fractions; the 4 x 4 neighbourhood at columns x0 - 1 .. x0 + 2,
  rows y0 - 1 .. y0 + 2, clamped into the image; the a = -1 cubic along x per row, then along y over the four row results;
  stored as 0 if v <= 0, 255 if v >= 255, else int(v) (truncation).
numpy's float64 element-wise operations are single IEEE operations, so evaluating in the same order gives Pillow's bytes."""
import numpy as np
import torch

FILL = (127, 0, 0)


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def warp_at(arr, m, xs, ys):
    """uint8 (H, W, 3) image warped by the inverse matrix m, sampled at the output pixels (xs, ys) (integer arrays of one shape S):
    uint8 (*S, 3)"""
    H, W = arr.shape[:2]
    xo = np.asarray(xs, dtype=np.float64) + 0.5
    yo = np.asarray(ys, dtype=np.float64) + 0.5
    xi = m[0] * xo + m[1] * yo
    xi = xi + m[2]
    yi = m[3] * xo + m[4] * yo
    yi = yi + m[5]
    inside = (xi >= 0.0) & (xi < W) & (yi >= 0.0) & (yi < H)
    xi = np.where(inside, xi, 0.5) - 0.5
    yi = np.where(inside, yi, 0.5) - 0.5
    fx, fy = np.floor(xi), np.floor(yi)
    dx, dy = xi - fx, yi - fy
    x0, y0 = fx.astype(np.int64) - 1, fy.astype(np.int64) - 1
    a = arr.astype(np.float64)
    cols = [np.clip(x0 + k, 0, W - 1) for k in range(4)]
    rows = []
    for j in range(4):
        r = np.clip(y0 + j, 0, H - 1)
        rows.append(_cubic(a[r, cols[0]], a[r, cols[1]], a[r, cols[2]], a[r, cols[3]], dx[..., None]))
    v = _cubic(rows[0], rows[1], rows[2], rows[3], dy[..., None])
    out = np.where(v <= 0.0, 0.0, np.where(v >= 255.0, 255.0, v))
    out = np.trunc(out).astype(np.uint8)
    out[~inside] = FILL
    return out


def warp(arr, m):
    """the whole warped image: Image.fromarray(arr).transform((W, H), AFFINE, m, BICUBIC, fillcolor=127) as uint8 (H, W, 3)"""
    H, W = arr.shape[:2]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    return warp_at(arr, m, xs, ys)


def normalise(u8, channels=3):
    """ToTensor -> Normalize(.5, .5) of the PIL path (float32), with the pair dataset's gray mix for one channel"""
    t = torch.from_numpy((np.asarray(u8, dtype=np.float32) / 255.0).transpose(2, 0, 1).copy())
    t = (t - 0.5) / 0.5
    if channels == 1:
        t = (t[0] * 0.299 + t[1] * 0.587 + t[2] * 0.114).unsqueeze(0)
    return t


def pipeline(resized, m, x0, y0, fine, flip, channels=3):
    """warp -> crop (x0, y0, fine) -> flip -> normalise of an already resized uint8 image"""
    crop = warp(resized, m)[y0:y0 + fine, x0:x0 + fine]
    if flip:
        crop = crop[:, ::-1]
    return normalise(crop, channels)
