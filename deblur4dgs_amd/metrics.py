"""The validator's image metrics as one HIP call: masked PSNR and the dycheck masked SSIM.

`from deblur4dgs_amd.metrics import PCK, mPSNR, mSSIM` replaces `from flow3d.metrics import ...`.  The reference's classes subclass
`torchmetrics`; these carry the same surface (`update`, `compute`, `reset`, `len`, and calling the object, which accumulates and
returns this batch's value) on plain Python objects.  Their state is a list of device scalars, `update` launches two kernels
(`csrc/metrics.hip`) and waits for nothing, so the trainer's per-step PSNR (flow3d/trainer.py:775-783) can sit inside a captured step.

`masked_image_metrics` is the one call underneath: the squared error under the mask, the mask sum and the mean of the masked SSIM
map, for M masks of B images at once.  `ValidationMetrics` evaluates the validator's three masks (flow3d/validator.py:460-475) with
M = 3 in one launch and returns the reference's `val/*` keys.

The masked SSIM is the reference's own (count-normalised partial convolutions), not the pytorch_msssim one of
`losses.photometric_loss`.  Images are channel-last [B,H,W,3] as the rasterizer returns them.  `mLPIPS` lives in
`deblur4dgs_amd.lpips`, because it is built around a network whose AlexNet weights the user supplies; importing the name from here
raises an ImportError that says so.  `ValidationMetrics(lpips=net)` adds the three LPIPS keys.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from ._lib import f32c, need_gpu, stream_of, vp

__all__ = ["masked_image_metrics", "compute_psnr", "mPSNR", "mSSIM", "PCK", "ValidationMetrics"]


def __getattr__(name):
    if name == "mLPIPS":
        raise ImportError("deblur4dgs_amd.metrics has no mLPIPS: the metric needs the pretrained AlexNet LPIPS weights, which this project "
                          "does not ship; use deblur4dgs_amd.lpips.mLPIPS(LPIPS(trunk, lins)) with torchvision's AlexNet weights and the "
                          "LPIPS v0.1 alex.pth")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def masked_image_metrics(preds, targets, masks=None, ssim: bool = True):
    """preds, targets [B,H,W,3]; masks None (ones), [B,H,W] (M = 1) or [M,B,H,W], a trailing axis of 1 allowed.
    -> (sse, mask_sum, ssim): float64 device tensors [M,B] - the sum of ((pred - target) * mask)^2 over pixels and channels, the sum of
    the mask, and the mean of the masked SSIM map (None when `ssim` is False; H, W >= 11 otherwise).  Any float dtype and stride is
    accepted.  Runs on the current stream, reads nothing on the host, and its outputs never require a gradient."""
    need_gpu(preds, "deblur4dgs_amd.losses")  # (the name this refusal has always carried)
    if preds.dim() != 4 or preds.shape[-1] != 3 or targets.shape != preds.shape:
        raise ValueError(f"preds and targets must both be [B,H,W,3], got {tuple(preds.shape)} and {tuple(targets.shape)}")
    B, H, W, _ = preds.shape
    p, t = f32c(preds), f32c(targets)
    m, M = None, 1
    if masks is not None:
        if masks.dim() >= 4 and masks.shape[-1] == 1 and tuple(masks.shape[-4:-1]) == (B, H, W):
            masks = masks[..., 0]
        if masks.dim() not in (3, 4) or tuple(masks.shape[-3:]) != (B, H, W):
            raise ValueError(f"masks must be [B,H,W] or [M,B,H,W] (a trailing 1 allowed) for images {tuple(preds.shape)}, got {tuple(masks.shape)}")
        m = f32c(masks.to(p.device))
        M = m.shape[0] if m.dim() == 4 else 1
    lib = L.lib()
    nb = lib.d4gs_metrics_blocks(M, B, H, W)
    if nb == 0:
        raise ValueError(f"masked_image_metrics: sizes M={M} B={B} H={H} W={W} are empty or beyond the grid")
    scratch = torch.empty(3 * nb + 3 * M * B, device=p.device, dtype=torch.float64)
    out = scratch[3 * nb:]
    L.check(lib.d4gs_masked_metrics(vp(p), vp(t), vp(m), M, B, H, W, int(bool(ssim)), vp(scratch), vp(out),
                                    stream_of(p)), "d4gs_masked_metrics")
    out = out.view(M, B, 3)
    return out[..., 0].clone(), out[..., 1].clone(), (out[..., 2].clone() if ssim else None)


def _psnr(sse, total):
    return -10.0 * torch.log(sse / total) / math.log(10.0)


def _batch_sums(preds, targets, masks):
    """preds, targets [...,3], masks [...] or None -> (sse, mask sum) of everything, two device scalars.  Images keep their [H,W]
    (the kernel's tiles are 16x16); anything flatter becomes one row."""
    H, W = (preds.shape[-3], preds.shape[-2]) if preds.dim() >= 3 else (1, preds.numel() // 3)
    p, t = preds.reshape(-1, H, W, 3), targets.reshape(-1, H, W, 3)
    sse, msum, _ = masked_image_metrics(p, t, None if masks is None else masks.reshape(-1, H, W), ssim=False)
    return sse.sum(), msum.sum()


def compute_psnr(preds, targets, masks=None) -> float:
    """flow3d/metrics.py:13-42: preds, targets [...,3], masks [...] or None -> PSNR over the whole batch as a float (one host read);
    the mask sum is clamped at 1."""
    sse, msum = _batch_sums(preds, targets, masks)
    return float(_psnr(sse, msum.clamp(min=1.0) * 3.0))


class _Metric:
    """what the reference's classes use of torchmetrics.Metric: list states, reset, and a call that accumulates and returns the
    value of this batch alone"""
    _states: tuple = ()

    def __init__(self, **kwargs):
        self.reset()

    def reset(self):
        for s in self._states:
            setattr(self, s, [])

    def forward(self, *args, **kwargs):
        kept = {s: getattr(self, s) for s in self._states}
        self.reset()
        self.update(*args, **kwargs)
        value = self.compute()
        for s in self._states:
            setattr(self, s, kept[s] + getattr(self, s))
        return value

    __call__ = forward


class mPSNR(_Metric):
    """flow3d/metrics.py:81-124.  One entry per update: the squared error of the whole batch and total = trunc(sum mask) * 3."""
    _states = ("sum_squared_error", "total")

    def __len__(self) -> int:
        return len(self.total)

    def _append(self, sse, mask_sum):
        self.sum_squared_error.append(sse.sum())
        self.total.append(mask_sum.sum().to(torch.int64) * 3)

    @torch.no_grad()
    def update(self, preds, targets, masks=None):
        """preds, targets [...,3]; masks [...] or None"""
        self._append(*_batch_sums(preds, targets, masks))

    def compute(self) -> torch.Tensor:
        """-10 log10(sse / total), averaged over the updates (an empty mask gives nan, as upstream)"""
        return _psnr(torch.stack(self.sum_squared_error), torch.stack(self.total)).mean()


class mSSIM(_Metric):
    """flow3d/metrics.py:127-217.  One entry per update: the [B] means of the masked SSIM map."""
    _states = ("similarity",)

    def __len__(self) -> int:
        return sum(s.shape[0] for s in self.similarity)

    @torch.no_grad()
    def update(self, preds, targets, masks=None):
        """preds, targets [B,H,W,3]; masks [B,H,W] or None"""
        self.similarity.append(masked_image_metrics(preds, targets, masks, ssim=True)[2][0])

    def compute(self) -> torch.Tensor:
        return torch.cat(self.similarity).mean()


class PCK(_Metric):
    """flow3d/metrics.py:282-313: the share of 2-D keypoints within `threshold` of their targets, averaged over the updates."""
    _states = ("correct", "total")

    def __len__(self) -> int:
        return len(self.total)

    @torch.no_grad()
    def update(self, preds, targets, threshold: float):
        self.correct.append((torch.linalg.norm(preds - targets, dim=-1) < threshold).sum())
        self.total.append(preds.shape[0])

    def compute(self) -> torch.Tensor:
        correct = torch.stack(self.correct)
        return (correct / torch.tensor(self.total, device=correct.device).clamp(min=1e-8)).mean()


class ValidationMetrics:
    """The image numbers of the reference's Validator (flow3d/validator.py:460-499) - six, or all nine with `lpips=` - all masks of
    a frame in one launch.
    has_bg: main = valid, fg = fg * valid, bg = (1 - fg) * valid.  Without a background the reference scores only fg * valid as the
    main mask and never updates the fg / bg metrics; their keys are nan here.
    lpips: a `deblur4dgs_amd.lpips.LPIPS` (on the images' device) makes it the reference's nine: `update` also scores the three
    masks with one `masked_sums` call, and `compute()` adds val/lpips, val/fg_lpips and val/bg_lpips (LPIPS_KEYS)."""
    KEYS = ("val/psnr", "val/ssim", "val/fg_psnr", "val/fg_ssim", "val/bg_psnr", "val/bg_ssim")
    LPIPS_KEYS = ("val/lpips", "val/fg_lpips", "val/bg_lpips")

    def __init__(self, has_bg: bool = True, lpips=None):
        self.has_bg = bool(has_bg)
        self.lpips_net = lpips
        self.reset()

    def reset(self):
        self.psnr = [mPSNR() for _ in range(3)]
        self.ssim = [mSSIM() for _ in range(3)]
        if self.lpips_net is not None:
            from .lpips import mLPIPS

            self.lpips = [mLPIPS(self.lpips_net) for _ in range(3)]

    @torch.no_grad()
    def update(self, rendered_img, img, valid_mask, fg_mask):
        """rendered_img, img [B,H,W,3]; valid_mask, fg_mask [B,H,W]"""
        B, H, W, _ = rendered_img.shape
        valid, fg = valid_mask.reshape(B, H, W).float(), fg_mask.reshape(B, H, W).float()
        masks = torch.stack((valid, fg * valid, (1 - fg) * valid)) if self.has_bg else (fg * valid)[None]
        sse, msum, ssim = masked_image_metrics(rendered_img, img, masks, ssim=True)
        for i in range(masks.shape[0]):
            self.psnr[i]._append(sse[i], msum[i])
            self.ssim[i].similarity.append(ssim[i])
        if self.lpips_net is not None:
            scores, total = self.lpips_net.masked_sums(rendered_img, img, masks)
            for i in range(masks.shape[0]):
                self.lpips[i]._append(scores[i], total[i])

    def compute(self) -> dict:
        out = {}
        for i, name in enumerate(("", "fg_", "bg_")):
            seen = len(self.psnr[i]) > 0
            out[f"val/{name}psnr"] = self.psnr[i].compute() if seen else torch.tensor(float("nan"))
            out[f"val/{name}ssim"] = self.ssim[i].compute() if seen else torch.tensor(float("nan"))
        if self.lpips_net is not None:
            for i, name in enumerate(("", "fg_", "bg_")):
                out[f"val/{name}lpips"] = self.lpips[i].compute() if len(self.lpips[i]) > 0 else torch.tensor(float("nan"))
        return out
