"""What `absgrad` (D4GS_ABSGRAD) costs: the composite backward alone (k_raster_bwd*, d4gs_profile_enable(3) HIP events) and the whole
fwd+bwd frame (one-call path, event-timed), with absgrad off and on, on bench.py's scenes:

  cfg2 at S = 8 and S = 1 (288x512, 3 colours + expected depth), refdefault (16 colours + depth = 17 channels), cfg3 (720p, S = 8).

  python scripts/bench_absgrad.py [--steps 20] [--rounds 3] [--out F.json]

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

    def step(absgrad):
        for v in leaves.values():
            v.grad = None
        res = render_exposure(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"], leaves["colors"], 3,
                              leaves.get("motion_coefs"), leaves.get("rots"), leaves.get("transls"), leaves.get("times"), leaves["RTs"],
                              leaves["viewmat"], d["K"], W, H, background=bg, return_depth=True, fused=True, absgrad=absgrad)
        loss = torch.dot(res["blended"].reshape(-1), wimg.reshape(-1)) + torch.dot(res["acc"].reshape(-1), wacc.reshape(-1))
        loss.backward()

    def frame_ms(absgrad):
        for _ in range(3):
            step(absgrad)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step(absgrad)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    def bwd_kernel_ms(absgrad):
        step(absgrad)
        torch.cuda.synchronize()
        lib.d4gs_profile_enable(3)
        step(absgrad)
        torch.cuda.synchronize()
        _collect(lib)  # (the event machinery's first use stays out of the record)
        lib.d4gs_profile_enable(3)
        for _ in range(steps):
            step(absgrad)
        torch.cuda.synchronize()
        got = _collect(lib)
        n = sum(c for k, (c, _) in got.items() if k.startswith("k_raster_bwd"))
        ms = sum(t for k, (_, t) in got.items() if k.startswith("k_raster_bwd"))
        return ms / max(n, 1)

    res = {False: dict(frame=[], bwd=[]), True: dict(frame=[], bwd=[])}
    for _ in range(rounds):
        for flag in (False, True):
            res[flag]["frame"].append(frame_ms(flag))
            res[flag]["bwd"].append(bwd_kernel_ms(flag))
    out = dict(config=name, S=S, N=N, W=W, H=H, channels=channels + 1, steps=steps, rounds=rounds)
    for flag in (False, True):
        tag = "on" if flag else "off"
        out[f"bwd_kernel_ms_{tag}"] = round(statistics.median(res[flag]["bwd"]), 4)
        out[f"frame_ms_{tag}"] = round(statistics.median(res[flag]["frame"]), 4)
    out["bwd_kernel_cost"] = round(out["bwd_kernel_ms_on"] / out["bwd_kernel_ms_off"] - 1.0, 4)
    out["frame_cost"] = round(out["frame_ms_on"] / out["frame_ms_off"] - 1.0, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_absgrad.py measures on the GPU"
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
