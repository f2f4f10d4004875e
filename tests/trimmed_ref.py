"""The quantile-trimmed losses restated in torch on the CPU (fp64 unless told otherwise): what csrc/trimmed.hip must compute.

Written from the description in DESIGN.md section 14, not from the reference's source; tests/test_trimmed_ref.py pins it to values
recorded from the reference's own functions (tests/golden/trimmed_losses.npz).  Differentiable with respect to `pred` through
torch autograd: the kept set enters through torch.where, which carries no gradient for the comparison and gives elements outside
it a gradient of exactly zero - also when nothing is kept and the loss itself is 0 / 0 (the reference's `x[keep].mean()` does the
same).

    elements   v_i = mean over the last axis of |pred - gt|
    threshold  t = lerp(v_(floor r), v_(ceil r), frac r),  r = q (n - 1), over ALL n elements in ascending order
    kept       v_i < t   (strictly)

`rank_dtype` is the precision r is evaluated in: torch.quantile forms it in the dtype of its input, so the fp32 product path is
compared with rank_dtype=torch.float32 and the fp64 fixture with torch.float64."""
import torch


def elements(pred, gt):
    return (pred - gt).abs().mean(dim=-1)


def rank(q, n, rank_dtype=torch.float64):
    """-> (floor r, ceil r, frac r) with r = q (n - 1) rounded as torch.quantile does for input of `rank_dtype`."""
    r = torch.tensor(q, dtype=rank_dtype) * (n - 1)
    lo = torch.floor(r)
    return int(lo), int(torch.ceil(r)), float(r - lo)


def threshold(v, q, rank_dtype=torch.float64):
    """The linearly interpolated q-quantile of the flattened v (detached)."""
    s = torch.sort(v.detach().reshape(-1)).values
    lo, hi, frac = rank(q, s.numel(), rank_dtype)
    return s[lo] + (s[hi] - s[lo]) * frac


def kept(v, q, rank_dtype=torch.float64):
    return v.detach() < threshold(v, q, rank_dtype)


def _sum_over(keep, x):
    return torch.where(keep, x, torch.zeros_like(x)).sum()


def _trimmed_mean(v, q, rank_dtype):
    if v.numel() == 0:
        return v.sum() * float("nan")  # the reference raises here; the HIP path cannot
    k = kept(v, q, rank_dtype)
    return _sum_over(k, v) / k.sum()  # nothing kept: 0 / 0 = NaN


def trimmed_l1_loss(pred, gt, quantile=0.9, rank_dtype=torch.float64):
    v = elements(pred, gt).reshape(-1)
    return _trimmed_mean(v, quantile, rank_dtype)


def masked_l1_loss(pred, gt, mask=None, normalize=True, quantile=1.0, rank_dtype=torch.float64):
    if mask is None:
        return trimmed_l1_loss(pred, gt, quantile, rank_dtype)
    v = elements(pred, gt).reshape(-1)
    m = mask.to(v.dtype).reshape(-1)
    k = kept(v, quantile, rank_dtype) if quantile < 1 else torch.ones_like(v, dtype=torch.bool)
    return _sum_over(k, v * m) / (_sum_over(k, m) + 1e-8 if normalize else k.sum())


def compute_gradient_loss(pred, gt, mask, quantile=0.98, rank_dtype=torch.float64):
    if pred.dim() == 4:
        if pred.shape[-1] != 1:
            raise NotImplementedError("one channel")
        pred, gt = pred[..., 0], gt[..., 0]
    m = mask.reshape(pred.shape) != 0
    mx, my = m[:, :, 1:] & m[:, :, :-1], m[:, 1:, :] & m[:, :-1, :]
    dx = ((pred[:, :, 1:] - pred[:, :, :-1]) - (gt[:, :, 1:] - gt[:, :, :-1])).abs()
    dy = ((pred[:, 1:, :] - pred[:, :-1, :]) - (gt[:, 1:, :] - gt[:, :-1, :])).abs()
    # (boolean indexing here is the restatement's business: it runs on the CPU)
    return _trimmed_mean(dx[mx], quantile, rank_dtype) + _trimmed_mean(dy[my], quantile, rank_dtype)


def neighbours_apart(v, q, rel=1e-5):
    """The condition under which fp32 rounding of the elements cannot change the kept set: the order statistics floor(r) - 1 ..
    ceil(r) + 1 (those that exist) are pairwise at least rel * (max v - min v) apart.  From fp64 values alone."""
    s = torch.sort(v.detach().double().reshape(-1)).values
    n = s.numel()
    if n < 2:
        return True
    lo, hi, _ = rank(q, n, torch.float64)
    w = s[max(lo - 1, 0):min(hi + 1, n - 1) + 1]
    return bool((w[1:] - w[:-1]).min() >= rel * (s[-1] - s[0]))
