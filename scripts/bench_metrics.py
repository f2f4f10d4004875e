"""The validator's metrics (csrc/metrics.hip) against the reference's formulation in eager torch - tests/metrics_ref.py run in fp32
on the GPU, mask by mask as the validator's six metric objects do - for the three masks of one frame (M = 3, B = 1) at 288x512 and
720x1280.  Device events around windows of `--iters` evaluations, the two sides alternating, `--rounds` windows each; median and
spread of the windows.  Launch counts: kernels seen by torch.profiler in one evaluation.  The HIP side is also timed as a graph
replay.  The achieved difference between the two sides' values is recorded beside the times.

    python scripts/bench_metrics.py [--out profiles/metrics_times.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import metrics as hip  # noqa: E402
from tests import metrics_ref as ref  # noqa: E402  (measurement script only: the eager baseline)

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_metrics.py measures on the GPU; none found")
dev = "cuda:0"


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n  # microseconds per evaluation


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return len(names)
    except Exception as e:  # the count is a by-product: report why it is missing
        return f"not measured ({type(e).__name__})"


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


result = {"M": 3, "B": 1, "iters": a.iters, "rounds": a.rounds, "unit": "us per evaluation of three masks (sse, mask sum, SSIM)", "sizes": {}}
for H, W in ((288, 512), (720, 1280)):
    g = torch.Generator().manual_seed(H)
    target = torch.rand(1, H, W, 3, generator=g)
    pred = (target + 0.1 * torch.randn(1, H, W, 3, generator=g)).clamp(0, 1).to(dev)
    target = target.to(dev)
    valid = (torch.rand(1, H, W, generator=g) < 0.9).float()
    fg = torch.zeros(1, H, W)
    fg[:, H // 4:3 * H // 4, W // 3:2 * W // 3] = 1
    masks = torch.stack((valid, fg * valid, (1 - fg) * valid)).to(dev)
    f_hip = lambda: hip.masked_image_metrics(pred, target, masks)
    f_eager = lambda: ref.masked_image_metrics(pred, target, masks, dtype=torch.float32)
    with torch.no_grad():
        for _ in range(5):
            f_hip(), f_eager()
        vh, ve = f_hip(), f_eager()
        th, te = [], []
        for _ in range(a.rounds):
            th.append(window(f_hip, a.iters))
            te.append(window(f_eager, max(a.iters // 5, 2)))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            f_hip()
        tg = [window(graph.replay, a.iters) for _ in range(a.rounds)]
        n_hip, n_eager = launches(f_hip), launches(f_eager)
    rec = {"ssim_hip": vh[2][:, 0].tolist(), "ssim_eager_fp32": ve[2][:, 0].tolist(),
           "max_abs_ssim_difference": float((vh[2] - ve[2].double()).abs().max()),
           "max_rel_sse_difference": float(((vh[0] - ve[0].double()).abs() / vh[0]).max()),
           "hip_us": spread(th), "hip_graph_replay_us": spread(tg), "eager_fp32_us": spread(te), "launches_hip": n_hip, "launches_eager": n_eager}
    result["sizes"][f"{H}x{W}"] = rec
    print(f"{H}x{W}", json.dumps(rec))
if a.out:
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
