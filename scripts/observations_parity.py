"""The errors deblur4dgs_amd.observations achieves on the GPU against tests/golden/observations.npz (the reference's own functions,
recorded by tests/golden/gen_observations.py), as tests/test_gpu_observations.py bounds them.

    python scripts/observations_parity.py [--out profiles/observations_parity.md]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deblur4dgs_amd import observations as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("observations_parity.py measures on the GPU; none found")
z = np.load(os.path.join(ROOT, "tests", "golden", "observations.npz"))
g = {k: z[k] for k in z.files}
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0", torch.float32)
case = lambda p: {k[len(p) + 1:]: v for k, v in g.items() if k.startswith(p + "/")}
rel = lambda got, ref: float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-30)

lines = [f"# Observations: achieved parity on {torch.cuda.get_device_name(0)}", "",
         "Against `tests/golden/observations.npz` (the reference's functions; fp64 except the median).  Errors are max |got - ref| / max |ref|;",
         "the tests bound them by 1e-4.  `scripts/observations_parity.py`, one run.", "",
         "## Masked median blur (bit for bit)", "", "| case | shape | k | pixels that differ |", "|---|---|---|---|"]
for name in sorted({k.split("/")[1] for k in g if k.startswith("median/")}):
    c = case(f"median/{name}")
    out = O.masked_median_blur(dev(c["image"])[None], dev(c["mask"])[None], int(c["k"]))[0].cpu().numpy()
    lines.append(f"| {name} | {' x '.join(map(str, c['image'].shape))} | {int(c['k'])} | {int((out.view(np.uint32) != c['out'].view(np.uint32)).sum())} |")
lines += ["", "## Lifting", "", "| case | N x T | flags that differ | xyz | colors | confidences | samples re-drawn by the generator |", "|---|---|---|---|---|---|---|"]
for name in ("n1", "n63", "n64", "n65", "n1000", "integers", "quantile"):
    c = case(f"lift/{name}")
    got = O.lift_tracks(int(c["query"]), dev(c["img"]), dev(c["tracks_2d"]), dev(c["depths"]), dev(c["masks"]), dev(c["inv_Ks"]), dev(c["c2ws"]))
    flags = sum(int((got[k].cpu().numpy() != c[k]).sum()) for k in ("visibles", "invisibles", "in_mask"))
    N, T, _ = c["tracks_2d"].shape
    lines.append(f"| {name} | {N} x {T} | {flags} | {rel(got['xyz'], c['xyz']):.2e} | {rel(got['colors'], c['colors']):.2e} | "
                 f"{rel(got['confidences'], c['confidences']):.2e} | {int(c['redrawn'])} |")
lines += ["", "## Background points", "", "| case | H x W | points | normals |", "|---|---|---|---|"]
for name in ("flat", "rough"):
    c = case(f"normals/{name}")
    H, W = c["depth"].shape
    pts, normals, _ = O.bkgd_points_dense(dev(c["depth"])[None], torch.zeros(1, H, W, device="cuda:0"), torch.ones(1, H, W, device="cuda:0"),
                                          dev(np.linalg.inv(c["K"].astype(np.float64)))[None], dev(np.linalg.inv(c["w2c"].astype(np.float64)))[None])
    lines.append(f"| {name} | {H} x {W} | {rel(pts[0], c['points']):.2e} | {rel(normals[0], c['normals']):.2e} |")
print("\n".join(lines))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
