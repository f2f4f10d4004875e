"""NumPy / float64 statements of the three operations of deblur4dgs_amd/observations.py, in this repository's own words (DESIGN.md
section 26).  The tests hold the kernels to these and hold these to the reference's recorded outputs (tests/golden/observations.npz)."""
import numpy as np


def masked_median_blur(image, mask, k, per_image=False):
    """image, mask [n,H,W] -> [n,H,W] in image's dtype; every output is one of the inputs, or lo / hi.

    The window is k x k, zero-padded: a position outside the image has value 0 and mask 0.  An entry is valid iff its mask equals 1.
    lo = min(min(image), 0), hi = max(max(image), 0).  The invalid entries, enumerated in (image, h, w, ky k + kx) order, count
    alternately as lo and hi; so for one pixel, with p the parity of the invalid entries before it, its own invalid entries start
    with lo if p = 0 and with hi if p = 1.  The result is the lower median, rank (k k - 1) / 2 of the k k entries: lo if rank < n_lo
    (the pixel's entries sent to lo), else the (rank - n_lo)-th smallest valid value if there is one, else hi.
    per_image: lo, hi and the enumeration restart at every image."""
    image, mask = np.asarray(image), np.asarray(mask)
    n, H, W = image.shape
    if per_image and n > 1:
        return np.concatenate([masked_median_blur(image[i:i + 1], mask[i:i + 1], k) for i in range(n)])
    r, kk = k // 2, k * k
    rank = (kk - 1) // 2
    lo, hi = min(image.min(), image.dtype.type(0)), max(image.max(), image.dtype.type(0))
    pad = ((0, 0), (r, r), (r, r))
    values = np.lib.stride_tricks.sliding_window_view(np.pad(image, pad), (k, k), axis=(1, 2)).reshape(n, H, W, kk)
    valid = np.lib.stride_tricks.sliding_window_view(np.pad(mask == 1, pad), (k, k), axis=(1, 2)).reshape(n, H, W, kk)
    n_valid = valid.sum(-1)
    n_inv = kk - n_valid
    before = np.cumsum(n_inv.reshape(-1)) - n_inv.reshape(-1)  # invalid entries before each pixel, in (image, h, w) order
    p = (before % 2).reshape(n, H, W)
    n_lo = np.where(p == 0, (n_inv + 1) // 2, n_inv // 2)
    ordered = np.sort(np.where(valid, values, np.inf), axis=-1)
    j = rank - n_lo
    picked = np.take_along_axis(ordered, np.clip(j, 0, kk - 1)[..., None], -1)[..., 0]
    return np.where(j < 0, lo, np.where(j >= n_valid, hi, picked)).astype(image.dtype)


def blend(median, old, mask):
    """the dataset's depth * mask + old * (1 - mask), every operation rounded in the arrays' dtype"""
    return median * mask + old * (1 - mask)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def parse_tapir_track_info(occ, dist):
    vis, conf = 1.0 - _sigmoid(occ), 1.0 - _sigmoid(dist)
    visible, invisible = vis * conf > 0.5, (1.0 - vis) * conf > 0.5
    return visible, invisible, conf * (visible | invisible)


def bilinear_border(img, x, y):
    """img [H,W] or [H,W,C], x, y [...]: bilinear, the coordinates clamped to the image"""
    H, W = img.shape[:2]
    x, y = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    ax, ay = x - x0, y - y0
    if img.ndim == 3:
        ax, ay = ax[..., None], ay[..., None]
    return (img[y0, x0] * (1 - ax) * (1 - ay) + img[y0, x1] * ax * (1 - ay) + img[y1, x0] * (1 - ax) * ay + img[y1, x1] * ax * ay)


def corners_in_mask(mask, x, y):
    """mask [H,W], x, y [...] -> bool: every bilinear corner with a non-zero weight lies in the image and has mask == 1.  The corner
    floor(x) always weighs; floor(x) + 1 weighs iff x is no integer; the same in y."""
    H, W = mask.shape
    x0, y0 = np.floor(x), np.floor(y)
    ok = np.ones(np.shape(x), bool)
    for dy in (0, 1):
        for dx in (0, 1):
            weighs = ((x != x0) | (dx == 0)) & ((y != y0) | (dy == 0))
            cx, cy = x0 + dx, y0 + dy
            inside = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
            value = mask[np.clip(cy, 0, H - 1).astype(int), np.clip(cx, 0, W - 1).astype(int)]
            ok &= ~weighs | (inside & (value == 1))
    return ok


def lift_tracks(query, query_img, tracks_2d, depths, masks, inv_Ks, c2ws):
    """tracks_2d [N,T,4] ... -> dict, everything in float64 (see d4gs_lift_tracks in include/d4gs.h)"""
    tr = np.asarray(tracks_2d, np.float64)
    N, T, _ = tr.shape
    x, y = tr[..., 0], tr[..., 1]
    visible, invisible, conf = parse_tapir_track_info(tr[..., 2], tr[..., 3])
    depth = np.stack([bilinear_border(np.asarray(depths[t], np.float64), x[:, t], y[:, t]) for t in range(T)], 1)
    in_mask = np.stack([corners_in_mask(np.asarray(masks[t]), x[:, t], y[:, t]) for t in range(T)], 1)
    cam = np.einsum("tij,ntj->nti", np.asarray(inv_Ks, np.float64), np.stack([x, y, np.ones_like(x)], -1)) * depth[..., None]
    c2w = np.asarray(c2ws, np.float64)
    xyz = np.einsum("tij,ntj->nti", c2w[:, :3, :3], cam) + c2w[None, :, :3, 3]
    visible, invisible, conf = visible & in_mask, invisible & in_mask, conf * in_mask
    count = visible.sum(1).astype(np.int32)
    return dict(xyz=xyz, visibles=visible, invisibles=invisible, confidences=conf, in_mask=in_mask,
                colors=bilinear_border(np.asarray(query_img, np.float64), x[:, query], y[:, query]), visible_count=count,
                hist=np.bincount(count, minlength=T + 1).astype(np.int32))


def quantile_threshold(count, frames):
    """min(int(0.05 frames), the 0.1 quantile (linear) of the visible counts)"""
    return min(int(0.05 * frames), float(np.quantile(np.asarray(count, np.float64), 0.1))) if len(count) else float(int(0.05 * frames))


def bkgd_dense(depth, mask, valid_mask, inv_K, c2w):
    """one frame [H,W] -> (points [H,W,3], normals [H,W,3], keep [H,W]) in float64"""
    d = np.asarray(depth, np.float64)
    H, W = d.shape
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    cam = (np.stack([gx, gy, np.ones_like(gx)], -1) @ np.asarray(inv_K, np.float64).T) * d[..., None]
    c2w = np.asarray(c2w, np.float64)
    pts = cam @ c2w[:3, :3].T + c2w[:3, 3]
    normals = np.zeros_like(pts)
    n = np.cross(pts[1:-1, 2:] - pts[1:-1, :-2], pts[:-2, 1:-1] - pts[2:, 1:-1])  # right - left, top - bottom
    normals[1:-1, 1:-1] = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-12)
    keep = ((1 - np.asarray(mask, np.float64)) * np.asarray(valid_mask, np.float64) * (d > 0)) != 0
    return pts, normals, keep
