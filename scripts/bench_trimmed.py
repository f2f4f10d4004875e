"""The trimmed losses (csrc/trimmed.hip) against the same losses in eager torch - tests/trimmed_ref.py run in fp32 on the GPU: a
torch.sort per threshold and, for the gradient loss, boolean indexing (the host waits) - at the training shape [1,288,512,1] with
the reference's quantiles.  Forward + backward per call; device events around windows of `--iters` calls, the two sides
alternating, `--rounds` windows each; median and spread of the windows.  Launch counts: kernels seen by torch.profiler in one
call.  The HIP side is also timed as a graph replay (the eager side cannot be captured).

    python scripts/bench_trimmed.py [--out profiles/trimmed_losses.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import losses as hip  # noqa: E402
from tests import trimmed_ref as ref  # noqa: E402  (measurement script only: the eager baseline)

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_trimmed.py measures on the GPU; none found")
dev = "cuda:0"
g = torch.Generator().manual_seed(0)
gt = (1.0 / (2.0 + 3.0 * torch.rand(1, 288, 512, 1, generator=g))).to(dev)
base = (gt.cpu() * (1.0 + 0.1 * torch.randn(1, 288, 512, 1, generator=g))).to(dev)
mask = (torch.rand(1, 288, 512, 1, generator=g) < 0.8).float().to(dev)
valid = mask > 0.5
F32 = torch.float32
CASES = {
    "masked_l1_loss q=0.98": (lambda x: hip.masked_l1_loss(x, gt, mask, quantile=0.98),
                              lambda x: ref.masked_l1_loss(x, gt, mask, quantile=0.98, rank_dtype=F32)),
    "trimmed_l1_loss q=0.9": (lambda x: hip.trimmed_l1_loss(x, gt, 0.9), lambda x: ref.trimmed_l1_loss(x, gt, 0.9, rank_dtype=F32)),
    "compute_gradient_loss q=0.95": (lambda x: hip.compute_gradient_loss(x, gt, valid, quantile=0.95),
                                     lambda x: ref.compute_gradient_loss(x, gt, valid, quantile=0.95, rank_dtype=F32)),
}


def call(fn):
    x = base.clone().requires_grad_()
    fn(x).backward()
    return x.grad


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call(fn)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n  # microseconds per call


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        call(fn)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call(fn)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return len(names)
    except Exception as e:  # the count is a by-product: report why it is missing
        return f"not measured ({type(e).__name__})"


result = {"shape": [1, 288, 512, 1], "iters": a.iters, "rounds": a.rounds, "unit": "us per forward + backward", "cases": {}}
for name, (f_hip, f_eager) in CASES.items():
    for _ in range(20):
        call(f_hip), call(f_eager)
    lh, le = float(f_hip(base)), float(f_eager(base))
    th, te = [], []
    for _ in range(a.rounds):
        th.append(window(f_hip, a.iters))
        te.append(window(f_eager, a.iters))
    static = base.clone().requires_grad_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grad_static, = torch.autograd.grad(f_hip(static), [static])
    tg = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        tg.append(1e3 * e0.elapsed_time(e1) / a.iters)
    n_hip, n_eager = launches(f_hip), launches(f_eager)
    rec = {"loss_hip": lh, "loss_eager_fp32": le,
           "hip_us": {"median": statistics.median(th), "min": min(th), "max": max(th)},
           "hip_graph_replay_us": {"median": statistics.median(tg), "min": min(tg), "max": max(tg)},
           "eager_us": {"median": statistics.median(te), "min": min(te), "max": max(te)},
           "launches_hip": n_hip, "launches_eager": n_eager}
    result["cases"][name] = rec
    print(name, json.dumps(rec))
if a.out:
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
