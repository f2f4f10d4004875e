#!/usr/bin/env python3
"""Score rendered frames the way the reference's Validator does (flow3d/validator.py:460-499), on synthetic data.

A few `mode="mid"` (sharp) views of the synthetic scene are held against the same views of a perturbed copy of it, which also
supplies the foreground mask and, as the valid mask, the pixels it covers.  `ValidationMetrics` evaluates the main, foreground and
background masks of a frame in one launch (deblur4dgs_amd.metrics) and returns the reference's `val/*` keys;
nothing is read on the host until the dict is printed.  With --lpips-trunk and --lpips-lins (torchvision's AlexNet weights and the
LPIPS v0.1 alex.pth; the project ships neither) the three LPIPS keys are scored too: nine keys, as the reference reports.
With --pose-opt every frame's camera pose is first refined against its image, as the reference's `validate_imgs_with_optimization`
does (flow3d/validator.py:400-475, the path `run_testing.py` scores through; deblur4dgs_amd.pose_refine): the
views are then rendered from a slightly wrong pose, and the refinement - one HIP graph replayed --pose-iters times - has to find
the right one.

    python examples/validate_frames.py [--frames 1 3 5] [--width 512 --height 288] [--pose-opt [--pose-iters 500]]
                                       [--lpips-trunk alexnet.pth --lpips-lins alex.pth]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deblur4dgs_amd.metrics import ValidationMetrics, mPSNR  # noqa: E402
from deblur4dgs_amd.pose_refine import validate_with_pose_refinement  # noqa: E402
from train_dynamic_step import build  # noqa: E402  (the synthetic scene of the training example)


def pose_opt(model, frames, w2c, K, W, H, iters, lpips=None):
    """Score the model's own views from a pose that is off by a small rotation and a shift, before and after refining it."""
    dev = w2c.device
    wrong = w2c[0].clone()
    wrong[:3, :3] = (torch.eye(3, device=dev) + 0.01 * torch.tensor([[0.0, -0.5, -0.7], [0.5, 0.0, -0.5], [0.7, 0.5, 0.0]], device=dev)) @ wrong[:3, :3]
    wrong[:3, 3] += torch.tensor([0.02, -0.015, 0.03], device=dev)
    batch, before = [], ValidationMetrics(has_bg=True, lpips=lpips)
    with torch.no_grad():
        for t in frames:
            gt = model.render(t, w2c, K, (W, H), return_mask=True, mode="mid")
            f = dict(t=t, w2c=wrong, K=K[0], img=gt["img"].clone(), valid_mask=torch.ones(1, H, W, device=dev),
                     fg_mask=(gt["mask"][..., 0] > 0.5).float())
            before.update(model.render(t, wrong[None], K, (W, H), mode="mid")["img"], f["img"], f["valid_mask"], f["fg_mask"])
            batch.append(f)
    print("unrefined:", {k: round(float(v), 5) for k, v in before.compute().items()})
    out = {k: float(v) for k, v in validate_with_pose_refinement(model, batch, ValidationMetrics(has_bg=True, lpips=lpips), iters=iters).items()}
    print("refined:  ", {k: round(v, 5) for k, v in out.items()})
    return out


def main(frames=(1, 3, 5), W=512, H=288, n_fg=40_000, n_bg=100_000, dev="cuda:0", seed=0, pose_iters=0, lpips_trunk=None,
         lpips_lins=None):
    model, sc = build(n_fg=n_fg, n_bg=n_bg, W=W, H=H, dev=dev, seed=seed)
    w2c, K = sc["viewmat"][None].to(dev), sc["K"][None].to(dev)
    lpips = None
    if lpips_trunk and lpips_lins:  # a path or a state dict each
        from deblur4dgs_amd.lpips import LPIPS

        lpips = LPIPS(lpips_trunk, lpips_lins).to(dev)
    if pose_iters:
        return pose_opt(model, frames, w2c, K, W, H, pose_iters, lpips)
    target, _ = build(n_fg=n_fg, n_bg=n_bg, W=W, H=H, dev=dev, seed=seed + 1)
    metrics, train_psnr = ValidationMetrics(has_bg=True, lpips=lpips), mPSNR()
    with torch.no_grad():
        for t in frames:
            rendered = model.render(t, w2c, K, (W, H), mode="mid")["img"]
            gt = target.render(t, w2c, K, (W, H), return_mask=True, mode="mid")
            fg_mask = (gt["mask"][..., 0] > 0.5).float()
            valid_mask = (gt["acc"][..., 0] > 0.5).float()
            metrics.update(rendered, gt["img"], valid_mask, fg_mask)
            print(f"frame {t}: psnr of this frame {float(train_psnr(rendered, gt['img'], valid_mask)):.3f} dB "
                  f"({int(valid_mask.sum())} valid pixels, {int((fg_mask * valid_mask).sum())} of them foreground)")
    out = {k: float(v) for k, v in metrics.compute().items()}
    print({k: round(v, 5) for k, v in out.items()})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=float, nargs="+", default=[1, 3, 5])
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--fg", type=int, default=40_000)
    ap.add_argument("--bg", type=int, default=100_000)
    ap.add_argument("--pose-opt", action="store_true", help="refine every frame's pose against its image before scoring it")
    ap.add_argument("--pose-iters", type=int, default=500, help="iterations of --pose-opt per frame (the reference's 500)")
    ap.add_argument("--lpips-trunk", default=None, help="torchvision's AlexNet state dict; with --lpips-lins: nine keys")
    ap.add_argument("--lpips-lins", default=None, help="the LPIPS v0.1 alex.pth (lin{0..4}.model.1.weight)")
    a = ap.parse_args()
    if bool(a.lpips_trunk) != bool(a.lpips_lins):
        ap.error("--lpips-trunk and --lpips-lins come together")
    main(tuple(a.frames), a.width, a.height, a.fg, a.bg, pose_iters=a.pose_iters if a.pose_opt else 0, lpips_trunk=a.lpips_trunk,
         lpips_lins=a.lpips_lins)
