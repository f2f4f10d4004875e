"""SH colour kernels (csrc/sh.hip): kernel time, achieved bandwidth from algorithmic bytes, the eager fp32 torch
evaluation of the same math, and what `rasterization(sh_degree=3)` adds to a frame.

  python scripts/bench_sh.py [--out F.json]        event-timed kernels, eager baseline, seam cost (no profiler)
  python scripts/bench_sh.py --kernels-only        the kernel launches alone, to run under
        rocprofv3 --kernel-trace --output-format csv -d DIR -o sh -- python scripts/bench_sh.py --kernels-only
  python scripts/bench_sh.py --trace DIR           per-kernel median time and bandwidth from that run's kernel trace

Algorithmic bytes (fp32): forward reads 12 K N coefficients + 12 N positions and writes 12 N colours; backward (the seam's
configuration: origin, clamp, v_p and v_origin requested) reads 12 K N + 24 N (coefficients, positions, v_rgb) and writes
12 K N + 12 N (v_coeffs, v_p).  Measurement script only: not imported by the package.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deblur4dgs_amd import _lib as L  # noqa: E402

CONFIGS = [(3, 16, 1 << 20), (3, 16, 4 << 20), (4, 25, 1 << 20), (4, 25, 4 << 20)]  # (degree, K, N)
COPY_CEILING = 5.5e12  # B/s: the stream-copy rate measured on the box (README.md)
DEV = "cuda:0"


def nbytes(K, N):
    return {"fwd": 12 * K * N + 12 * N + 12 * N, "bwd": (12 * K * N + 24 * N) + (12 * K * N + 12 * N)}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Bufs:
    def __init__(self, d, K, N):
        g = torch.Generator(device=DEV).manual_seed(0)
        self.d, self.K, self.N = d, K, N
        self.p = torch.randn(N, 3, device=DEV, generator=g) * 4
        self.o = torch.tensor([0.1, -0.2, -3.0], device=DEV)
        self.c = torch.randn(N, K, 3, device=DEV, generator=g) * 0.3
        self.rgb = torch.empty(N, 3, device=DEV)
        self.v_rgb = torch.randn(N, 3, device=DEV, generator=g)
        self.v_c = torch.empty(N, K, 3, device=DEV)
        self.v_p = torch.empty(N, 3, device=DEV)
        self.v_o = torch.empty(3, device=DEV)
        self.part = torch.empty(L.lib().d4gs_sh_partials_elems(N), device=DEV)
        self.stream = C.c_void_p(L.raw_stream(0))

    def fwd(self):
        L.check(L.lib().d4gs_sh_fwd(self.N, self.K, self.d, _p(self.p), _p(self.o), _p(self.c), None, 1, _p(self.rgb),
                                    self.stream), "d4gs_sh_fwd")

    def bwd(self):
        L.check(L.lib().d4gs_sh_bwd(self.N, self.K, self.d, _p(self.p), _p(self.o), _p(self.c), None, 1, _p(self.v_rgb),
                                    _p(self.v_c), _p(self.v_p), _p(self.v_o), _p(self.part), self.stream), "d4gs_sh_bwd")


def event_ms(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernels_only(iters=20):
    for d, K, N in CONFIGS:
        b = Bufs(d, K, N)
        for _ in range(iters):
            b.fwd()
        for _ in range(iters):
            b.bwd()
        torch.cuda.synchronize()
        del b


def eager_ms(d, K, N):
    """The same math as fp32 torch ops (tests/sh_ref.py on the device), fwd + bwd through autograd."""
    from tests import sh_ref

    b = Bufs(d, K, N)
    p = b.p.clone().requires_grad_()
    c = b.c.clone().requires_grad_()

    def step():
        rgb = torch.clamp_min(sh_ref.spherical_harmonics(d, p - b.o, c) + 0.5, 0.0)
        rgb.backward(b.v_rgb)

    return event_ms(step, iters=10, warmup=3)


def seam_added_ms(N=300_000, W=512, H=288, K=16, d=3, rounds=3):
    """Device time of rasterization(sh_degree=3) fwd+bwd minus rasterization with the same colours precomputed."""
    from deblur4dgs_amd.rasterization import rasterization
    from deblur4dgs_amd.sh import sh_colors
    from tests.util import static_inputs

    inp = {k: v.to(DEV) for k, v in static_inputs(N, W, H, seed=0, dtype=torch.float32).items()}
    g = torch.Generator().manual_seed(0)
    sh = (torch.randn(N, K, 3, generator=g) * 0.3).to(DEV)
    sh[:, 0] = (inp["colors"] - 0.5) / 0.28209479177387814
    leaves = {k: inp[k].clone().requires_grad_() for k in ("means", "quats", "scales", "opac")}
    sh.requires_grad_()
    V = inp["V"][None].clone().requires_grad_()
    rgb0 = sh_colors(inp["means"], inp["V"], sh.detach(), d).detach().requires_grad_()

    def frame(colors, sh_degree):
        rc, ra, _ = rasterization(leaves["means"], leaves["quats"], leaves["scales"], leaves["opac"], colors, V,
                                  inp["K"][None], W, H, sh_degree=sh_degree)
        (rc.sum() + ra.sum()).backward()

    a, b = [], []
    for _ in range(rounds):  # alternate the two, the same number of times each
        a.append(event_ms(lambda: frame(sh, d)))
        b.append(event_ms(lambda: frame(rgb0, None)))
    return statistics.median(a), statistics.median(b)


def from_trace(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {trace_dir}"
    rows = [r for f in files for r in csv.DictReader(open(f))]
    gkey = next(k for k in ("Grid_Size_X", "Grid_Size", "Grid_X") if k in rows[0])
    out = []
    for d, K, N in CONFIGS:
        blocks = (N + 255) // 256
        for kind in ("fwd", "bwd"):
            ts = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows
                  if f"k_sh_{kind}<{d}" in r["Kernel_Name"] and int(r[gkey]) in (blocks, blocks * 256)]
            if not ts:
                continue
            t = statistics.median(ts)
            bw = nbytes(K, N)[kind] / t
            out.append(dict(kernel=f"k_sh_{kind}", degree=d, K=K, N=N, dispatches=len(ts), median_us=round(t * 1e6, 2),
                            bytes=nbytes(K, N)[kind], TBps=round(bw / 1e12, 3), frac_copy_ceiling=round(bw / COPY_CEILING, 3)))
    fin = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows if "k_sh_finish" in r["Kernel_Name"]]
    if fin:
        out.append(dict(kernel="k_sh_finish", dispatches=len(fin), median_us=round(statistics.median(fin) * 1e6, 2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        res = from_trace(a.trace)
        for r in res:
            print(json.dumps(r))
    else:
        assert torch.cuda.is_available(), "bench_sh.py measures on the GPU"
        if a.kernels_only:
            kernels_only()
            return
        res = []
        for d, K, N in CONFIGS:
            b = Bufs(d, K, N)
            for kind, fn in (("fwd", b.fwd), ("bwd", b.bwd)):
                t = event_ms(fn) * 1e-3
                bw = nbytes(K, N)[kind] / t
                res.append(dict(what=f"event {kind}", degree=d, K=K, N=N, ms=round(t * 1e3, 4), TBps=round(bw / 1e12, 3),
                                frac_copy_ceiling=round(bw / COPY_CEILING, 3)))
                print(json.dumps(res[-1]), flush=True)
            del b
            torch.cuda.empty_cache()
            res.append(dict(what="eager fp32 torch fwd+bwd", degree=d, K=K, N=N, ms=round(eager_ms(d, K, N), 4)))
            print(json.dumps(res[-1]), flush=True)
            torch.cuda.empty_cache()
        with_sh, without = seam_added_ms()
        res.append(dict(what="rasterization fwd+bwd, N=300k 288x512", sh_degree3_ms=round(with_sh, 4),
                        precomputed_colors_ms=round(without, 4), added_ms=round(with_sh - without, 4)))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
