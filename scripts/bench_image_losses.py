"""The image terms (csrc/image_terms.hip) against the reference's torch wording of the same terms - nn.MaxPool2d(9, 1, 4),
F.interpolate(scale_factor=0.25, mode="area") + F.l1_loss, F.mse_loss (flow3d/trainer.py:120,736-747,621-626) - in fp32 on the same
device and in the same process, at the training shape 288 x 512, B = 1.  The losses: forward + backward per call; the dilation:
the forward (masks are data).  Device events around windows of `--iters` calls, the two sides alternating, `--rounds` windows each;
median and spread of the windows.  Launch counts: kernels seen by torch.profiler in one call.  The HIP side is also timed as a graph
replay.

    python scripts/bench_image_losses.py [--out profiles/image_losses.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import losses as hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_image_losses.py measures on the GPU; none found")
dev = "cuda:0"
H, W = 288, 512
g = torch.Generator().manual_seed(0)
imgs = torch.rand(1, H, W, 3, generator=g).to(dev)
sharp = (imgs.cpu() + 0.05 * torch.randn(1, H, W, 3, generator=g)).to(dev)
masks = torch.zeros(1, H, W)
masks[:, 90:200, 150:380] = 1.0  # a foreground blob
masks = masks.to(dev)
acc = torch.rand(1, H, W, 1, generator=g).to(dev)
pool = torch.nn.MaxPool2d(kernel_size=9, stride=1, padding=4)


def area(x):
    return F.interpolate(x, scale_factor=0.25, mode="area")


def eager_keep(x):  # trainer.py:736-747
    m = area(masks.unsqueeze(0)).permute(0, 2, 3, 1)
    down = area(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1) * m
    blury = area(imgs.permute(0, 3, 1, 2)).permute(0, 2, 3, 1) * m
    return F.l1_loss(down, blury.detach())


# name -> (HIP call, eager call, the tensor that takes the gradient or None)
CASES = {
    "dilate_mask 9x9 (+ complement)": (lambda x: hip.dilate_mask(masks, return_complement=True)[1],
                                       lambda x: 1.0 - pool(masks.unsqueeze(0)).permute(0, 2, 3, 1), None),
    "sharp_keep_loss factor 4": (lambda x: hip.sharp_keep_loss(x, imgs, masks), eager_keep, sharp),
    "coverage_loss target None": (lambda x: hip.coverage_loss(x), lambda x: F.mse_loss(x, torch.ones_like(x)), acc),
    "coverage_loss target masks": (lambda x: hip.coverage_loss(x, masks[..., None]), lambda x: F.mse_loss(x, masks[..., None]), acc),
}


def call(fn, base):
    if base is None:
        return fn(None)
    x = base.clone().requires_grad_()
    fn(x).backward()
    return x.grad


def window(fn, base, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call(fn, base)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n  # microseconds per call


def launches(fn, base):
    try:
        from torch.profiler import ProfilerActivity, profile

        call(fn, base)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call(fn, base)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return len(names)
    except Exception as e:  # the count is a by-product: report why it is missing
        return f"not measured ({type(e).__name__})"


result = {"shape": [1, H, W, 3], "iters": a.iters, "rounds": a.rounds, "unit": "us per call (losses: forward + backward)", "cases": {}}
for name, (f_hip, f_eager, base) in CASES.items():
    for _ in range(20):
        call(f_hip, base), call(f_eager, base)
    with torch.no_grad():
        vh, ve = f_hip(base), f_eager(base)
    th, te = [], []
    for _ in range(a.rounds):
        th.append(window(f_hip, base, a.iters))
        te.append(window(f_eager, base, a.iters))
    graph = torch.cuda.CUDAGraph()
    if base is None:
        with torch.cuda.graph(graph):
            kept = f_hip(None)
    else:
        static = base.clone().requires_grad_()
        with torch.cuda.graph(graph):
            kept, = torch.autograd.grad(f_hip(static), [static])
    tg = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        tg.append(1e3 * e0.elapsed_time(e1) / a.iters)
    rec = {"first_value_hip": float(vh.reshape(-1)[0]), "first_value_eager_fp32": float(ve.reshape(-1)[0]),
           "max_abs_diff_hip_vs_eager_fp32": float((vh.reshape(-1) - ve.reshape(-1)).abs().max()),
           "hip_us": {"median": statistics.median(th), "min": min(th), "max": max(th)},
           "hip_graph_replay_us": {"median": statistics.median(tg), "min": min(tg), "max": max(tg)},
           "eager_us": {"median": statistics.median(te), "min": min(te), "max": max(te)},
           "launches_hip": launches(f_hip, base), "launches_eager": launches(f_eager, base)}
    result["cases"][name] = rec
    print(name, json.dumps(rec))
if a.out:
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
