"""What the antialiased mode (D4GS_ANTIALIASED, `rasterize_mode="antialiased"`) costs: k_project_fwd and k_gather alone
(d4gs_profile_enable(1) HIP events) and the whole fwd+bwd frame (one-call path, event-timed), with the mode off and on, on bench.py's
scenes:

  cfg2 at S = 8 and S = 1 (288x512, 3 colours + expected depth), refdefault (the reference's training shape: 16 colours + depth),
  cfg3 (720p, S = 8).

  python scripts/bench_antialias.py [--steps 20] [--rounds 3] [--out F.json]

Off and on alternate `rounds` times; every line reports the median over the rounds.  Measurement script only: not imported by
the package.
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
import bench  # noqa: E402
from deblur4dgs_amd import _lib as L  # noqa: E402
from deblur4dgs_amd.exposure import render_exposure  # noqa: E402

CASES = [("cfg2", None), ("cfg2", 1), ("refdefault", None), ("cfg3", None)]  # (bench.py config, sub-samples or None = the config's)
DEV = "cuda:0"
KERNELS = ("k_project_fwd", "k_gather")


def _collect(lib):
    lib.d4gs_profile_enable(0)
    buf = C.create_string_buffer(1 << 16)
    lib.d4gs_profile_collect(buf, C.c_size_t(len(buf)))
    got = {}
    for line in buf.value.decode().splitlines():
        nm, cnt, ms = line.split()
        got[nm] = (int(cnt), float(ms))
    return got


def case(name, S_over, steps, rounds):
    lib = L.lib()
    channels = 16 if name.startswith("refdefault") else 3
    N, G, K, S, W, H = bench.CONFIGS[name]
    sc, d, leaves, wimg, wacc = bench.make_inputs(name, DEV, channels=channels)
    if S_over is not None:
        for k in ("times", "RTs"):
            if k in leaves:
                leaves[k] = leaves[k][:S_over].detach().clone().requires_grad_()
        S = S_over
    bg = torch.ones(channels, device=DEV)

    def step(aa):
        for v in leaves.values():
            v.grad = None
        res = render_exposure(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"], leaves["colors"], 3,
                              leaves.get("motion_coefs"), leaves.get("rots"), leaves.get("transls"), leaves.get("times"), leaves["RTs"],
                              leaves["viewmat"], d["K"], W, H, background=bg, return_depth=True, fused=True, antialiased=aa)
        loss = torch.dot(res["blended"].reshape(-1), wimg.reshape(-1)) + torch.dot(res["acc"].reshape(-1), wacc.reshape(-1))
        loss.backward()

    def frame_ms(aa):
        for _ in range(3):
            step(aa)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step(aa)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    def kernel_ms(aa):  # -> {kernel: ms per call} of the two kernels the mode changes
        step(aa)
        torch.cuda.synchronize()
        lib.d4gs_profile_enable(1)
        step(aa)
        torch.cuda.synchronize()
        _collect(lib)  # (the event machinery's first use stays out of the record)
        lib.d4gs_profile_enable(1)
        for _ in range(steps):
            step(aa)
        torch.cuda.synchronize()
        got = _collect(lib)
        return {k: got[k][1] / max(got[k][0], 1) for k in KERNELS}

    keys = ("frame",) + KERNELS
    res = {flag: {k: [] for k in keys} for flag in (False, True)}
    for _ in range(rounds):
        for flag in (False, True):
            res[flag]["frame"].append(frame_ms(flag))
            for k, v in kernel_ms(flag).items():
                res[flag][k].append(v)
    out = dict(config=name, S=S, N=N, W=W, H=H, channels=channels + 1, steps=steps, rounds=rounds)
    for k in keys:
        for flag in (False, True):
            out[f"{k}_ms_{'on' if flag else 'off'}"] = round(statistics.median(res[flag][k]), 4)
        out[f"{k}_cost"] = round(out[f"{k}_ms_on"] / out[f"{k}_ms_off"] - 1.0, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_antialias.py measures on the GPU"
    rows = []
    for name, S in CASES:
        rows.append(case(name, S, a.steps, a.rounds))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
