"""Times every entry of deblur4dgs_amd.scene_init at the reference's sizes (run_training_dynamic.py:118-119: 40 000 foreground tracks of
24 frames, 20 bases, 100 000 background points) and, where it imports, sklearn's NearestNeighbors on the same box for the kNN.

Each figure is the median of `--rounds` device-event windows of `--iters` calls behind a warm-up; the kNN rows also give the pair rate
N (N - 1) / time and that rate as a share of the box's own FP32 issue ceiling (d4gs_measure_peaks: v_fma_f32 lanes per second), with 8
vector operations per pair and query counted as the kernel's useful work (3 subtractions, 3 multiply-adds, a minimum and a compare;
the rest is overhead).  The wrappers allocate their outputs and workspaces inside the timed region: these are calls as a user makes them.

    python scripts/bench_scene_init.py [--out profiles/scene_init_times.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import _lib as L  # noqa: E402
from deblur4dgs_amd import scene_init as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_scene_init.py measures on the GPU; none found")
dev = "cuda:0"
G, T, K, N_BG = 40000, 24, 20, 100000
gen = torch.Generator().manual_seed(0)
motions = torch.cumsum(torch.cumsum(torch.randn(K, T, 3, generator=gen) * 0.02, 1) + torch.randn(K, 1, 3, generator=gen) * 0.05, 1)
which = torch.randint(0, K, (G,), generator=gen)
xyz = (torch.randn(G, 1, 3, generator=gen) + motions[which] + 0.01 * torch.randn(G, T, 3, generator=gen)).to(dev)
visibles = (torch.rand(G, T, generator=gen) < 0.8).to(dev)
conf = torch.rand(G, T, generator=gen).to(dev)
bg = (torch.randn(N_BG, 3, generator=gen) * torch.tensor([4.0, 1.5, 4.0])).to(dev)
cano = xyz[:, T // 2].contiguous()
_, feats = S.track_features(xyz, visibles)
labels = which.to(dev)
order = torch.argsort(labels, stable=True)
seg = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(which, minlength=K), 0)]).int().to(dev)
weights = torch.rand(G, T, generator=gen).to(dev)
centres0 = feats[:K].clone()


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n  # microseconds per call


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = [window(fn, a.iters) for _ in range(a.rounds)]
    return {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}


def kmeans_20():
    c, lab = centres0.clone(), torch.zeros(G, dtype=torch.int32, device=dev)
    S.kmeans_step(feats, c, lab, 20)


def peaks():
    try:
        scratch = torch.zeros(1 << 27, dtype=torch.uint8, device=dev)
        out = (C.c_double * 4)()
        rc = L.lib().d4gs_measure_peaks(C.c_void_p(scratch.data_ptr()), C.c_size_t(scratch.numel()), out, L.stream_of(scratch))
        torch.cuda.synchronize()
        return None if rc != 0 else {"fp32_fma_tflops": out[2], "fp32_pk_fma_tflops": out[1]}
    except Exception as e:  # context, not the measurement
        return {"error": repr(e)}


result = {"sizes": {"G": G, "T": T, "K": K, "N_bg": N_BG}, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
          "note": "one box, one run; wrappers allocate inside the timed region", "peaks_measured": peaks(), "entries": {}}
ceiling = (result["peaks_measured"] or {}).get("fp32_fma_tflops")
entries = {
    f"track_features G={G} T={T}": lambda: S.track_features(xyz, visibles),
    f"knn k=3 N={G} (foreground)": lambda: S.knn(cano, 3),
    f"knn k=3 N={N_BG} (background)": lambda: S.knn(bg, 3),
    f"kmeans_step x20 G={G} D={3 * (T - 1)} K={K}": kmeans_20,
    f"procrustes_moments G={G} T={T} K={K}": lambda: S.procrustes_moments(xyz, weights, conf, order, seg, T // 2),
}
for name, fn in entries.items():
    rec = timed(fn)
    if name.startswith("knn"):
        n = G if "foreground" in name else N_BG
        rec["splits"] = L.lib().d4gs_knn_splits(n)
        rec["pairs_per_s"] = n * (n - 1) / (rec["median_us"] * 1e-6)
        if ceiling:  # an FMA counts two flops in the ceiling: lanes per second = tflops / 2
            rec["share_of_fp32_issue_ceiling_at_8_ops_per_pair"] = 8 * rec["pairs_per_s"] / (ceiling * 1e12 / 2)
    result["entries"][name] = rec
    print(name, json.dumps(rec), flush=True)

t0 = time.perf_counter()
lab, _, iters_run = S.kmeans(feats, K, generator=torch.Generator().manual_seed(1))
torch.cuda.synchronize()
result["entries"][f"kmeans (k-means++ + Lloyd to the fixed point) G={G} K={K}"] = {"wall_ms": 1e3 * (time.perf_counter() - t0), "iterations": iters_run}
t0 = time.perf_counter()
tracks = S.TrackObservations(xyz, visibles, ~visibles, conf, torch.rand(G, 3, generator=gen).to(dev))
bases, coefs, kept = S.init_motion_params_with_procrustes(tracks, K, "6d", T // 2, generator=torch.Generator().manual_seed(1))
fg = S.init_fg_from_tracks_3d(T // 2, kept, coefs)
torch.cuda.synchronize()
result["entries"]["init_motion_params_with_procrustes + init_fg_from_tracks_3d, end to end"] = {"wall_ms": 1e3 * (time.perf_counter() - t0),
                                                                                               "kept": int(kept.xyz.shape[0])}
try:
    from sklearn.neighbors import NearestNeighbors

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for name, pts in (("foreground", cano), ("background", bg)):
        x = pts.cpu().numpy()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            NearestNeighbors(n_neighbors=4, algorithm="auto", metric="euclidean").fit(x).kneighbors(x)
            t.append(1e3 * (time.perf_counter() - t0))
        result["entries"][f"sklearn NearestNeighbors k=3 N={len(x)} ({name}, host, as the reference calls it)"] = {"median_ms": statistics.median(t)}
except ImportError:
    result["entries"]["sklearn NearestNeighbors"] = "not measured: sklearn does not import here"
for k, v in result["entries"].items():
    if "wall_ms" in str(v) or "median_ms" in str(v):
        print(k, json.dumps(v))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
