"""The validator's masked PSNR sums and masked SSIM restated in torch (fp64 on the CPU unless told otherwise): what
deblur4dgs_amd.metrics.masked_image_metrics must compute.

Written from the description in DESIGN.md section 19; tests/test_metrics_ref.py pins it to values recorded from the reference's own
mPSNR and mSSIM (tests/golden/metrics.npz).  The reference builds its passes from grouped conv2d calls; here a pass is a sliding
window (`unfold`) and a weighted sum, the window is formed in double, and nothing is fp32 unless the caller asks for it.

    f[k] = exp(-((k - 5) / 1.5)^2 / 2) / sum,  k = 0..10
    pass along an axis:  cnt = sum_window mask;  out = cnt != 0 ? (sum_window f z mask) * 11 / cnt : 0;  mask' = (cnt != 0)
    F[z] = pass_y(pass_x(z, mask))            (the y pass runs on the x pass's result under the x pass's mask')
    mu0 = F[p], mu1 = F[t], s00 = max(0, F[pp] - mu0^2), s11 = max(0, F[tt] - mu1^2), s = F[pt] - mu0 mu1,
    s01 = sign(s) min(sqrt(s00 s11), |s|)
    ssim = (2 mu0 mu1 + c1)(2 s01 + c2) / ((mu0^2 + mu1^2 + c1)(s00 + s11 + c2)),  c1 = 1e-4, c2 = 9e-4

The normaliser of a pass is the COUNT of the mask under the window (times 1/11), not sum f mask: the reference's behaviour."""
import torch

TAPS = 11
C1, C2 = 1e-4, 9e-4


def window(dtype=torch.float64, device="cpu"):
    k = torch.arange(TAPS, dtype=torch.float64, device=device) - TAPS // 2
    f = torch.exp(-0.5 * (k / 1.5) ** 2)
    return (f / f.sum()).to(dtype)


def masked_pass(z, m, f, axis):
    """z [B,H,W,C], m [B,H,W]; axis 1 (y) or 2 (x) -> (filtered z, mask') with that axis shortened by 10"""
    zw = (z * m[..., None]).unfold(axis, TAPS, 1)  # [..., C, 11]
    cnt = m.unfold(axis, TAPS, 1).sum(-1)
    live = cnt != 0
    safe = torch.where(live, cnt, torch.ones_like(cnt))
    out = torch.where(live[..., None], (zw * f).sum(-1) * TAPS / safe[..., None], torch.zeros((), dtype=z.dtype, device=z.device))
    return out, live.to(z.dtype)


def masked_filter(z, m, f):
    return masked_pass(*masked_pass(z, m, f, 2), f, 1)[0]


def ssim_map(pred, target, mask, dtype=torch.float64):
    """pred, target [B,H,W,3], mask [B,H,W] -> [B,H-10,W-10,3]"""
    p, t, m = pred.to(dtype), target.to(dtype), mask.to(dtype)
    f = window(dtype, p.device)
    mu0, mu1 = masked_filter(p, m, f), masked_filter(t, m, f)
    s00 = (masked_filter(p * p, m, f) - mu0 * mu0).clamp(min=0)
    s11 = (masked_filter(t * t, m, f) - mu1 * mu1).clamp(min=0)
    s = masked_filter(p * t, m, f) - mu0 * mu1
    s01 = torch.sign(s) * torch.minimum(torch.sqrt(s00 * s11), s.abs())
    return ((2 * mu0 * mu1 + C1) * (2 * s01 + C2)) / ((mu0 * mu0 + mu1 * mu1 + C1) * (s00 + s11 + C2))


def masked_image_metrics(pred, target, masks=None, ssim=True, dtype=torch.float64):
    """pred, target [B,H,W,3]; masks None, [B,H,W] or [M,B,H,W] -> (sse, mask_sum, ssim) each [M,B] (ssim None if not asked for)"""
    p, t = pred.to(dtype), target.to(dtype)
    if masks is None:
        masks = torch.ones(p.shape[:3], dtype=dtype, device=p.device)
    masks = masks.to(dtype)
    if masks.dim() == 3:
        masks = masks[None]
    sse = torch.stack([(((p - t) * m[..., None]) ** 2).sum((1, 2, 3)) for m in masks])
    msum = masks.sum((2, 3))
    val = torch.stack([ssim_map(p, t, m, dtype).mean((1, 2, 3)) for m in masks]) if ssim else None
    return sse, msum, val


def psnr(sse, total):
    """-10 log10(sse / total), total = trunc(mask sum) * 3 (the reference's int64 cast)"""
    return -10.0 * torch.log10(sse / total)
