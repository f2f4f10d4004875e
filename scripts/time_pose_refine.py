#!/usr/bin/env python3
"""Time one frame of test-time pose refinement four ways, on the reference's scene shape (40 k + 100 k
Gaussians, 20 bases, 288 x 512), `--iters` iterations per frame:

  a  the eager loop written with nothing of pose_refine.py: SceneModel.render, the full backward, torch.optim.Adam and
     CosineAnnealingLR in the reference's order (flow3d/validator.py:424-455)
  b  refine_pose(graph=False): eager, pose_only + d4gs_pose_step
  c  refine_pose(graph=True): the iteration replayed from a HIP graph
  d  refine_pose(graph=True, pose_only=False): the graph with the full leaf backward (d - c = what d4gs_pose_bwd itself buys)

The variants alternate `--repeats` times in one process; each timed call ends in a device synchronise.  Medians and the spread
(max - min over the repeats) go to stdout and to `--out`.

    python scripts/time_pose_refine.py --out profiles/pose_refine_times.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from deblur4dgs_amd.pose_refine import refine_pose  # noqa: E402
from train_dynamic_step import build  # noqa: E402  (the synthetic scene of the training example)


def eager_torch_loop(model, t, w2c, K, img, iters, lr=1e-2, eta_min=1e-4):
    """Variant a: what a user of the parent commit can write."""
    H, W = img.shape[1:3]
    transR = torch.nn.Parameter(torch.eye(3, device=w2c.device))
    transT = torch.nn.Parameter(torch.zeros(3, 1, device=w2c.device))
    opt = torch.optim.Adam([{"params": [transR, transT], "lr": lr}])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=iters, eta_min=eta_min)
    loss = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scheduler.step() before optimizer.step(): the reference's order
        for _ in range(iters):
            w2c_trans = torch.zeros_like(w2c)
            w2c_trans[:, :3, :3] = transR @ w2c[:, :3, :3]
            w2c_trans[:, :3, 3:] = transT + w2c[:, :3, 3:]
            w2c_trans[:, 3, 3] = 1.0
            rendered = model.render(t, w2c_trans, K, (W, H), return_depth=True)
            loss = (rendered["img"] - img).abs().mean()
            loss.backward()
            sched.step()
            opt.step()
            opt.zero_grad(set_to_none=True)
            model.zero_grad(set_to_none=True)  # (the scene's gradients: computed, never read)
    return loss.detach()


def main(iters=500, repeats=3, W=512, H=288, n_fg=40_000, n_bg=100_000, dev="cuda:0", out=None, t=3):
    model, sc = build(n_fg=n_fg, n_bg=n_bg, W=W, H=H, dev=dev, seed=0)
    w2c, K = sc["viewmat"][None].to(dev), sc["K"][None].to(dev)
    target = w2c.clone()  # the view to find: a small rotation about a skew axis and a shift
    a = torch.tensor([0.5, -0.7, 0.5], device=dev)
    a = a / a.norm()
    Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], device=dev)
    target[0, :3, :3] = (torch.eye(3, device=dev) + 0.02 * Kx) @ w2c[0, :3, :3]
    target[0, :3, 3] += torch.tensor([0.03, -0.02, 0.04], device=dev)
    with torch.no_grad():
        img = model.render(t, target, K, (W, H))["img"].clone()
    variants = {
        "a eager torch (full backward, torch Adam)": lambda: eager_torch_loop(model, t, w2c, K, img, iters),
        "b eager pose_only + d4gs_pose_step": lambda: refine_pose(model, t, w2c[0], K[0], img, iters=iters, graph=False),
        "c graph pose_only": lambda: refine_pose(model, t, w2c[0], K[0], img, iters=iters, graph=True),
        "d graph full backward": lambda: refine_pose(model, t, w2c[0], K[0], img, iters=iters, graph=True, pose_only=False),
    }
    times = {k: [] for k in variants}
    final = {}
    for rep in range(repeats + 1):  # (round 0 is a warm-up of every variant and is not kept)
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt)
            final[name] = float(res if torch.is_tensor(res) else res["losses"][-1])
            print(f"round {rep} {name}: {dt:.3f} s  (last loss {final[name]:.5f})", flush=True)
    lines = [f"pose refinement, {iters} iterations per frame, {n_fg} + {n_bg} Gaussians, {H} x {W}; seconds per frame, {repeats} repeats"]
    for name, ts in times.items():
        lines.append(f"{name:45s} median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}  spread {max(ts) - min(ts):7.3f}"
                     f"  ms/iteration {1e3 * statistics.median(ts) / iters:7.3f}  last loss {final[name]:.5f}")
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return times


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fg", type=int, default=40_000)
    ap.add_argument("--bg", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.iters, a.repeats, a.width, a.height, a.fg, a.bg, out=a.out)
