"""Fixture of the 2-D track loss and the mapped-depth loss: small inputs, and the two losses and the `tracks_3d` gradient of
1.7 (l2d + 3 ldepth) that the REFERENCE's own masked_l1_loss (flow3d/loss_utils.py) gives for them in float64 on the CPU.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_track_losses.py   ->  tests/golden/track_losses.npz

The two terms are inline in Trainer.compute_dynamic_losses (flow3d/trainer.py:633-667,681-689) and cannot be called on their own, so
`reference_flow` below applies, in this file's own words, the data flow the trainer wraps around masked_l1_loss: every pixel of
every target image is projected, an image mask is raised at the query pixels, the masked pixels are taken in raster order by one
boolean selection and the visible ones by a second, and the weights are the [P_all, M] product the trainer forms.  masked_l1_loss
itself is loaded from the reference (gen_trimmed_losses.load_reference).  Only data travels: the arrays below."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_trimmed_losses import load_reference  # noqa: E402

H, W = 12, 16
NAMES = ("tracks_3d", "query_tracks_2d", "target_Ks", "target_tracks_2d", "target_visibles", "track_weights", "target_track_depths")


def case(seed, N, Ps, weight_width, behind=0):
    """-> dict of NAMES; the per-batch entries are lists of len(Ps) tensors.  Distinct raster-ordered queries, continuous values."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    B = len(Ps)
    pts = torch.cat([(r(B, H, W, N, 2) - 0.5) * 4.0, 1.0 + 4.0 * r(B, H, W, N, 1)], -1)  # depths in [1, 5]
    out = {k: [] for k in NAMES[1:5] + NAMES[6:]}
    for b, P in enumerate(Ps):
        idx = torch.sort(torch.randperm(H * W, generator=g)[:P]).values
        out["query_tracks_2d"].append(torch.stack([idx % W, idx // W], -1).double() + 0.8 * r(P, 2))  # truncation is part of the flow
        K = torch.zeros(N, 3, 3, dtype=torch.float64)
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 10 + 4 * r(N), 10 + 4 * r(N), W / 2 + r(N), H / 2 + r(N), 1.0
        out["target_Ks"].append(K + 0.05 * (r(N, 3, 3) - 0.5))  # every entry takes part
        out["target_tracks_2d"].append(torch.stack([W * r(N, P), H * r(N, P)], -1))
        out["target_visibles"].append(r(N, P) < 0.7 if P > 1 else torch.ones(N, P, dtype=torch.bool))
        out["target_track_depths"].append(1.0 + 4.0 * r(N, P))
        for k in range(behind):  # points at or behind the camera plane of their target frame: the clamp
            y, x = int(idx[k] // W), int(idx[k] % W)
            pts[b, y, x, k % N, 2] = -0.5 * k
            out["target_visibles"][-1][k % N, k] = True
    n = N * sum(Ps)
    out["tracks_3d"] = pts
    # the trainer's confidences[..., None] * w_interval has width B N; width 1 is what a caller with ready-made weights passes
    out["track_weights"] = r(n, 1) * torch.exp(-2.0 * r(weight_width))[None] if weight_width > 1 else 0.1 + r(n, 1)
    return out


def cases():
    return {"n4_p65": (case(11, 4, (65,), 4), 0.98), "n1_p1": (case(12, 1, (1,), 1), 0.98),
            "b2_p7_p40": (case(13, 3, (7, 40), 6, behind=3), 0.9), "width1_weights": (case(14, 2, (20,), 1), 0.98)}


def reference_flow(masked_l1_loss, c, quantile):
    """The trainer's data flow around masked_l1_loss (module docstring) -> (2-D track loss without / max(H, W), mapped-depth loss)."""
    tracks = c["tracks_3d"]
    B, _, _, N, _ = tracks.shape
    image_points = tracks.permute(0, 3, 1, 2, 4).reshape(B * N, H * W, 3)  # one row per (batch entry, target frame)
    projected = torch.einsum("rij,rpj->rpi", torch.cat(c["target_Ks"]), image_points)
    depth = projected[..., 2:].clamp(min=1e-6)
    xy = projected[..., :2] / depth
    query_mask = torch.zeros(B, H, W, dtype=torch.float64)
    for b, q in enumerate(c["query_tracks_2d"]):
        qi = q.to(torch.int64)
        query_mask[b, qi[:, 1], qi[:, 0]] = 1.0
    at_queries = query_mask.reshape(B, 1, H * W).expand(B, N, H * W).reshape(B * N, H * W) > 0.5
    flat = lambda name, *tail: torch.cat([x.reshape(-1, *tail) for x in c[name]])
    visible, weights = flat("target_visibles"), c["track_weights"]
    l2d = masked_l1_loss(xy[at_queries][visible], flat("target_tracks_2d", 2)[visible], mask=weights[visible], quantile=quantile)
    ldepth = masked_l1_loss(1 / (depth[at_queries][visible] + 1e-5), 1 / (flat("target_track_depths")[visible, None] + 1e-5),
                            weights[visible])
    return l2d, ldepth


if __name__ == "__main__":
    ref = load_reference()
    arrays = {}
    for name, (c, q) in cases().items():
        c = dict(c, tracks_3d=c["tracks_3d"].clone().requires_grad_())
        l2d, ldepth = reference_flow(ref["masked_l1_loss"], c, q)
        (1.7 * (l2d + 3.0 * ldepth)).backward()
        for k in NAMES:
            for b, x in enumerate([c[k]] if torch.is_tensor(c[k]) else c[k]):
                arrays[f"{name}/{k}/{b}"] = x.detach().numpy()
        arrays[f"{name}/l2d"], arrays[f"{name}/ldepth"] = l2d.detach().numpy(), ldepth.detach().numpy()
        arrays[f"{name}/tracks_3d_grad"] = c["tracks_3d"].grad.numpy()
        print(name, float(l2d.detach()), float(ldepth.detach()), file=sys.stderr)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "track_losses.npz")
    np.savez_compressed(dst, **arrays)
    print(f"{len(arrays)} arrays -> {dst} ({os.path.getsize(dst)} bytes)", file=sys.stderr)
