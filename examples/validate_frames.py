#!/usr/bin/env python3
"""Score rendered frames the way the reference's Validator does (flow3d/validator.py:460-499), on synthetic data.

A few `mode="mid"` (sharp) views of the synthetic scene are held against the same views of a perturbed copy of it, which also
supplies the foreground mask and, as the valid mask, the pixels it covers.  `ValidationMetrics` evaluates the main, foreground and
background masks of a frame in one launch (deblur4dgs_amd.metrics) and returns the reference's `val/*` keys;
nothing is read on the host until the dict is printed.  LPIPS is not part of it (its network weights are not shipped).

    python examples/validate_frames.py [--frames 1 3 5] [--width 512 --height 288]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deblur4dgs_amd.metrics import ValidationMetrics, mPSNR  # noqa: E402
from train_dynamic_step import build  # noqa: E402  (the synthetic scene of the training example)


def main(frames=(1, 3, 5), W=512, H=288, n_fg=40_000, n_bg=100_000, dev="cuda:0", seed=0):
    model, sc = build(n_fg=n_fg, n_bg=n_bg, W=W, H=H, dev=dev, seed=seed)
    target, _ = build(n_fg=n_fg, n_bg=n_bg, W=W, H=H, dev=dev, seed=seed + 1)
    w2c, K = sc["viewmat"][None].to(dev), sc["K"][None].to(dev)
    metrics, train_psnr = ValidationMetrics(has_bg=True), mPSNR()
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
    a = ap.parse_args()
    main(tuple(a.frames), a.width, a.height, a.fg, a.bg)
