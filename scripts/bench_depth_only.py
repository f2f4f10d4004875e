"""What a depth-only render costs through `rasterization()`: forward + backward of 300 k static Gaussians at 288x512 and 720x1280 by
three routes -

  D        render_mode="D" (the depth-only kernels: no colour table, one channel)
  rgbd0    the workaround: render_mode="RGB+D" with colors = zeros(N, 1) (two channels, a colour-table row per splat)
  rgbd3    render_mode="RGB+D" with 3 colours

- the whole step (event-timed) and every kernel alone (d4gs_profile_enable(1) HIP events).

  python scripts/bench_depth_only.py [--steps 200] [--rounds 5] [--out F.json]

The routes alternate `rounds` times; every number is the median over the rounds.  Measurement script only: not imported by the
package.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deblur4dgs_amd import _lib as L  # noqa: E402
from deblur4dgs_amd.rasterization import rasterization  # noqa: E402
from deblur4dgs_amd.synth import make_scene  # noqa: E402

N = 300_000
SHAPES = [(512, 288), (1280, 720)]
ROUTES = ("D", "rgbd0", "rgbd3")
DEV = "cuda:0"


def _collect(lib):
    lib.d4gs_profile_enable(0)
    buf = C.create_string_buffer(1 << 16)
    lib.d4gs_profile_collect(buf, C.c_size_t(len(buf)))
    got = {}
    for line in buf.value.decode().splitlines():
        nm, cnt, ms = line.split()
        got[nm] = (int(cnt), float(ms))
    return got


def case(W, H, steps, rounds):
    lib = L.lib()
    sc = make_scene(N, 0, 1, 1, W, H, seed=2024, dtype=torch.float32)
    leaves = dict(means=sc["means"], quats=sc["quats"], scales=torch.exp(sc["scales"]), opacities=torch.sigmoid(sc["opacities"]))
    leaves = {k: v.to(DEV).contiguous().requires_grad_() for k, v in leaves.items()}
    cols = {"D": torch.sigmoid(sc["colors"]).to(DEV), "rgbd0": torch.zeros(N, 1, device=DEV), "rgbd3": torch.sigmoid(sc["colors"]).to(DEV)}
    for c in cols.values():
        c.requires_grad_()
    V, K = sc["viewmat"].to(DEV)[None], sc["K"].to(DEV)[None]
    g = torch.Generator().manual_seed(1)
    w_d = torch.randn(1, H, W, 1, generator=g).to(DEV)  # the depth channel's cotangent: the same in every route
    w_c = torch.randn(1, H, W, 3, generator=g).to(DEV)
    w_a = torch.randn(1, H, W, 1, generator=g).to(DEV)

    def step(route):
        for v in list(leaves.values()) + [cols[route]]:
            v.grad = None
        mode = "D" if route == "D" else "RGB+D"
        rc, ra, _ = rasterization(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"], cols[route], V, K, W, H,
                                  render_mode=mode)
        loss = (rc[..., -1:] * w_d).sum() + (ra * w_a).sum()
        if route == "rgbd3":
            loss = loss + (rc[..., :3] * w_c).sum()
        loss.backward()

    def frame_ms(route):
        for _ in range(3):
            step(route)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step(route)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    def kernel_ms(route):  # -> {kernel: ms per step}
        step(route)
        torch.cuda.synchronize()
        lib.d4gs_profile_enable(1)
        step(route)
        torch.cuda.synchronize()
        _collect(lib)  # (the event machinery's first use stays out of the record)
        lib.d4gs_profile_enable(1)
        for _ in range(steps):
            step(route)
        torch.cuda.synchronize()
        return {k: ms / steps for k, (cnt, ms) in _collect(lib).items()}

    frame = {r: [] for r in ROUTES}
    kern = {r: {} for r in ROUTES}
    for _ in range(rounds):
        for r in ROUTES:
            frame[r].append(frame_ms(r))
            for k, v in kernel_ms(r).items():
                kern[r].setdefault(k, []).append(v)
    out = dict(N=N, W=W, H=H, steps=steps, rounds=rounds)
    for r in ROUTES:
        out[f"frame_ms_{r}"] = round(statistics.median(frame[r]), 4)
        out[f"kernels_ms_{r}"] = {k: round(statistics.median(v), 4) for k, v in sorted(kern[r].items())}
        out[f"kernel_sum_ms_{r}"] = round(sum(out[f"kernels_ms_{r}"].values()), 4)  # device time; the frame adds the host's
    out["D_vs_rgbd0"] = round(out["frame_ms_D"] / out["frame_ms_rgbd0"] - 1.0, 4)
    out["D_vs_rgbd0_kernels"] = round(out["kernel_sum_ms_D"] / out["kernel_sum_ms_rgbd0"] - 1.0, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_only.py measures on the GPU"
    rows = []
    for W, H in SHAPES:
        rows.append(case(W, H, a.steps, a.rounds))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
