"""An fp64 statement of the image terms of csrc/image_terms.hip, written from the formulas in include/d4gs.h with explicit window loops
- no F.max_pool2d, no F.interpolate, no autograd.  tests/test_image_terms_ref.py pins it to torch's own CPU ops; the GPU tests compare
the kernels against it.  NumPy arrays in, NumPy arrays (or Python floats) out."""
import numpy as np


def dilate(mask, r):
    """mask [B,H,W] -> the maximum over the (2r+1)^2 window clipped to the image (max-pool's -inf padding).  Keeps the dtype."""
    mask = np.asarray(mask)
    B, H, W = mask.shape
    out = np.empty_like(mask)
    for y in range(H):
        for x in range(W):
            out[:, y, x] = mask[:, max(y - r, 0):min(y + r, H - 1) + 1, max(x - r, 0):min(x + r, W - 1) + 1].reshape(B, -1).max(axis=1)
    return out


def windows(L, factor):
    """The Lo = L // factor windows [lo, hi) of an axis of length L: lo = floor(i L / Lo), hi = ceil((i + 1) L / Lo)."""
    Lo = L // factor
    return [((i * L) // Lo, -((-(i + 1) * L) // Lo)) for i in range(Lo)]


def area_mean(a, factor):
    """a [B,H,W,C] -> [B,Ho,Wo,C], the mean of every window."""
    a = np.asarray(a, np.float64)
    B, H, W, C = a.shape
    wy, wx = windows(H, factor), windows(W, factor)
    out = np.empty((B, len(wy), len(wx), C))
    for i, (y0, y1) in enumerate(wy):
        for j, (x0, x1) in enumerate(wx):
            out[:, i, j] = a[:, y0:y1, x0:x1].sum(axis=(1, 2)) / ((y1 - y0) * (x1 - x0))
    return out


def keep_elements(pred, target, mask, factor):
    """-> (d, mbar): d = pbar mbar - tbar mbar [B,Ho,Wo,C] and mbar [B,Ho,Wo,1]; a target that already has d's shape is taken as tbar."""
    pred, target = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    B, H, W, C = pred.shape
    mb = area_mean(np.asarray(mask, np.float64).reshape(B, H, W, 1), factor)
    pb = area_mean(pred, factor)
    tb = target if target.shape == pb.shape else area_mean(target, factor)
    return pb * mb - tb * mb, mb


def sharp_keep(pred, target, mask, factor):
    """-> (loss, dloss/dpred): loss = mean |d|; every window hands sign(d) mbar / (area n) to each of its pixels, sign(0) = 0."""
    d, mb = keep_elements(pred, target, mask, factor)
    B, H, W, C = np.asarray(pred).shape
    grad = np.zeros((B, H, W, C))
    for i, (y0, y1) in enumerate(windows(H, factor)):
        for j, (x0, x1) in enumerate(windows(W, factor)):
            grad[:, y0:y1, x0:x1] += (np.sign(d[:, i, j]) * mb[:, i, j] / ((y1 - y0) * (x1 - x0) * d.size))[:, None, None]
    return float(np.abs(d).sum() / d.size), grad


def mse(a, target=None):
    """-> (mean((a - t)^2), its gradient 2 (a - t) / n); target None: the constant 1."""
    a = np.asarray(a, np.float64)
    diff = a - (1.0 if target is None else np.asarray(target, np.float64).reshape(a.shape))
    return float((diff * diff).sum() / a.size), 2.0 * diff / a.size
