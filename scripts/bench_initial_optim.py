"""ms per iteration of the warm-up fit (deblur4dgs_amd.scene_init.run_initial_optim) at the reference's size, three ways:

  graph     one iteration - schedule step, track_fit forward and backward, AdamGroup.step() - captured in a HIP graph and replayed
  eager     the same launches issued from Python
  composed  what the package could do before csrc/track_fit.hip: the six terms composed from masked_l1_loss, motion_regularizers and
            torch ops (tests/track_fit_ref.compose_terms), autograd, the four learning rates and the smoothness weight computed on the
            host, AdamGroup.sync() + step() per iteration

    python scripts/bench_initial_optim.py [--tracks 40000] [--bases 20] [--frames 24] [--iters 100] [--rounds 3] [--out FILE]
    python scripts/bench_initial_optim.py --launches     # device launches per iteration (torch.profiler), a run of its own

Protocol: the variants alternate in one process, `--rounds` rounds, each figure the time between two device
events around `--iters` iterations after 10 warm-up iterations, reported as median (min - max).  Measurement script only: not
imported by the package or the tests."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import scene_init as S  # noqa: E402
from deblur4dgs_amd.optim import AdamGroup  # noqa: E402
from deblur4dgs_amd.scene_model import GaussianParams, MotionBases  # noqa: E402
from tests import track_fit_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tracks", type=int, default=40000)
ap.add_argument("--bases", type=int, default=20)
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_initial_optim.py needs an MI355X (ROCm) device")
DEV = "cuda:0"
G, K, T, NUM_ITERS = a.tracks, a.bases, a.frames, 1000
case = {k: v.to(DEV) for k, v in R.make_case(G, K, T, 0).items()}
tracks = S.TrackObservations(case["xyz"], case["visibles"], case["invisibles"], case["confidences"], torch.zeros(G, 3, device=DEV))


def fresh():
    fg = GaussianParams(case["means"].clone(), torch.ones(G, 4, device=DEV), torch.zeros(G, 3, device=DEV), torch.zeros(G, 3, device=DEV),
                        torch.zeros(G, device=DEV), motion_coefs=case["motion_coefs"].clone())
    return fg, MotionBases(case["rots"].clone(), case["transls"].clone())


class Fused:
    def __init__(self, graph):
        fg, bases = fresh()
        self.loop = S._WarmupLoop(fg, bases, tracks, case["Ks"], case["w2cs"], NUM_ITERS)
        with torch.no_grad():
            self.loop.one()
        self.step = self.loop.capture().replay if graph else self.one

    def one(self):
        with torch.no_grad():
            self.loop.one()

    def restart(self):
        self.loop.it.zero_()  # the schedule starts over; the parameters go on from where they are


class Composed:
    def __init__(self):
        fg, bases = fresh()
        self.params = [bases.params["rots"], bases.params["transls"], fg.params["motion_coefs"], fg.params["means"]]
        self.group = AdamGroup()
        self.handles = [self.group.adam(p, lr) for p, lr in zip(self.params, R.LR0)]
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.w3, self.w2 = tracks.visibles.float() * tracks.confidences, tracks.invisibles.float() * tracks.confidences
        self.gt2d = R.project(tracks.xyz.transpose(0, 1), case["Ks"], case["w2cs"])[0].transpose(0, 1).contiguous()
        self.i = 0

    def step(self):
        rots, transls, coefs, means = self.params
        terms = R.compose_terms(means, coefs, rots, transls, tracks.xyz, self.w3, self.w2, case["Ks"], case["w2cs"], gt2d=self.gt2d)
        w = torch.tensor(R.weights(self.i, NUM_ITERS), dtype=torch.float32).to(DEV, non_blocking=True)
        for p, g in zip(self.params, torch.autograd.grad((terms * w).sum(), self.params)):
            p.grad.copy_(g)
        for h, lr0 in zip(self.handles, R.LR0):
            h.param_groups[0]["lr"] = lr0 * 0.1 ** (self.i / NUM_ITERS)
        self.group.step()  # sync(): the table goes up again, the rates have moved
        self.i += 1

    def restart(self):
        self.i = 0


def timed(v, iters):
    v.restart()
    for _ in range(10):
        v.step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        v.step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


variants = {"graph": Fused(True), "eager": Fused(False), "composed": Composed()}
lines = [f"warm-up fit, G = {G}, K = {K}, T = {T}: ms per iteration, device events around {a.iters} iterations after 10 warm-up iterations, "
         f"the variants alternating, {a.rounds} rounds: median (min - max)"]
if a.launches:
    from torch.profiler import ProfilerActivity, profile

    for name, v in variants.items():
        v.restart()
        for _ in range(3):
            v.step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(10):
                v.step()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        names = sorted({e.name for e in kernels})
        lines.append(f"{name:9s} device activities per iteration {len(kernels) / 10:.1f} ({len(names)} distinct)")
        lines += [f"    {sum(e.name == n for e in kernels) / 10:5.1f}  {n[:110]}" for n in names]
else:
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, v in variants.items():
            times[name].append(timed(v, a.iters))
    for name, t in times.items():
        lines.append(f"{name:9s} {statistics.median(t):8.3f} ({min(t):.3f} - {max(t):.3f})")
    g, c = statistics.median(times["graph"]), statistics.median(times["composed"])
    lines.append(f"graph / composed = {g / c:.3f}" + ("" if g < c else "   THE CAPTURED LOOP IS NOT FASTER THAN THE COMPOSITION"))
print("\n".join(lines))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
