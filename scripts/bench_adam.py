#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 13 (multi-tensor Adam).  Needs an MI355X; nothing here falls back.

  python scripts/bench_adam.py steps [--steps 260] [--reps 2] [--out FILE.json]
      examples/train_dynamic_step.py in four modes, alternating, `--reps` times each: eager + torch fused Adam, eager + HIP
      Adam, graph + torch Adam (fused=False: see the example), graph + HIP Adam (inside the graph).  Per mode: median / p10 / p90
      of the per-step time over the steps after the first 40, from one timing event per step (no host sync in the loop).

  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_adam.py kernel --set train|cfg2 [--launches 300]
      nothing but `AdamGroup.step()` on the tensor set of the example's training step / of bench.py's cfg2, so that k_adam's
      row of the kernel statistics is that shape's.  Prints the bytes one launch moves (28 per element: p, g, m, v read; p, m, v
      written) - bytes / the trace's average k_adam time = achieved bytes/s.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _example():
    spec = importlib.util.spec_from_file_location("train_dynamic_step", os.path.join(ROOT, "examples", "train_dynamic_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def steps_mode(a):
    mod = _example()
    modes = {"eager_torch_fused": dict(), "eager_hip_adam": dict(hip_adam=True), "graph_torch_adam": dict(graph=True),
             "graph_hip_adam": dict(graph=True, hip_adam=True)}
    skip = 40  # warm-up: lazy state, two eager steps before the capture, the capture itself
    runs = {k: [] for k in modes}
    for rep in range(a.reps):
        for name, kw in modes.items():
            evs = []
            losses, _, _ = mod.train(steps=a.steps, verbose=False, step_events=evs, **kw)
            torch.cuda.synchronize()
            ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(skip, len(evs) - 1)]
            q = statistics.quantiles(ms, n=10)
            runs[name].append({"median_ms": statistics.median(ms), "p10_ms": q[0], "p90_ms": q[-1], "steps": len(ms),
                               "final_loss": losses[-1]})
            print(name, rep, json.dumps(runs[name][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(runs, f, indent=1)


def _tensor_set(name):
    if name == "train":  # the parameters examples/train_dynamic_step.py optimizes, in its order
        model, _ = _example().build()
        ps = [p for part in ("fg", "bg") for p in getattr(model, part).params.values()]
        ps += list(model.motion_bases.parameters()) + list(model.move_model.parameters())
        return [p.detach().clone().requires_grad_() for p in ps]
    from bench import CONFIGS
    from deblur4dgs_amd.synth import make_scene

    N, G, K, S, W, H = CONFIGS["cfg2"]  # the leaves of the benchmark's flagship render
    small = make_scene(64, 64, K, S, W, H, seed=0)
    shapes = [(N, 3), (N, 4), (N, 3), (N,), (N, 3), (G, K), tuple(small["rots"].shape), tuple(small["transls"].shape)]
    return [torch.randn(s, device="cuda:0").requires_grad_() for s in shapes]


def kernel_mode(a):
    from deblur4dgs_amd.optim import AdamGroup

    params = _tensor_set(a.set)
    group = AdamGroup()
    for p in params:
        group.adam(p, 1e-3)
        p.grad = torch.randn_like(p)
    n = sum(p.numel() for p in params)
    for _ in range(20):
        group.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.launches):
        group.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.launches
    print(json.dumps({"set": a.set, "tensors": len(params), "elements": n, "bytes_per_launch": 28 * n, "launches": a.launches,
                      "smallest": min(p.numel() for p in params), "largest": max(p.numel() for p in params),
                      "host_loop_us_per_step": 1e6 * dt}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["steps", "kernel"])
    ap.add_argument("--steps", type=int, default=260)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--set", default="train", choices=["train", "cfg2"])
    ap.add_argument("--launches", type=int, default=300)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    (steps_mode if a.mode == "steps" else kernel_mode)(a)
