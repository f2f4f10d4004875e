"""Times deblur4dgs_amd.observations at the training resolutions (288 x 512 and 480 x 854, T = 24 frames) against the same operations
written with torch ops on the same device: `filter_depths`, `tracks_3d` at 10 000 tracks per query frame, `bkgd_points`.

The torch side restates what the reference does, in this file's own words: the median blur unfolds the window into k k planes with an
identity convolution, calls `nonzero` on the invalid entries (a host wait), scatters the tensor's min and max into them alternately and
takes `torch.median`, frame by frame; the lifting calls `grid_sample` per query frame for depth, mask and colour and reads the
quantile on the host; the background points index with a boolean mask.  Each figure is the median of `--rounds` HIP-event windows of
one call behind a warm-up.  The wrappers allocate their outputs and workspaces inside the timed region.

    python scripts/bench_observations.py [--out profiles/observations_times.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import observations as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--tracks", type=int, default=10000)
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_observations.py measures on the GPU; none found")
dev = "cuda:0"
T, N, K = a.frames, a.tracks, 11


def timed(fn, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return statistics.median(t), min(t), max(t)


def torch_median_blur(image, mask, k):
    """[1,1,H,W]: unfold + nonzero + median"""
    _, _, H, W = image.shape
    eye = torch.eye(k * k, device=image.device).reshape(k * k, 1, k, k)
    planes = F.conv2d(image, eye, padding=k // 2).reshape(1, 1, k * k, H, W).permute(0, 1, 3, 4, 2)
    valid = F.conv2d(mask, eye, padding=k // 2).reshape(1, 1, k * k, H, W).permute(0, 1, 3, 4, 2)
    lo, hi = planes.min(), planes.max()
    idx = (1 - valid).nonzero(as_tuple=True)
    planes = planes.contiguous()
    planes[tuple(i[::2] for i in idx)] = lo
    planes[tuple(i[1::2] for i in idx)] = hi
    return planes.median(dim=-1).values


def torch_filter_depths(depths, masks, valid):
    d = depths.clamp(0, float(depths.reshape(depths.shape[0], -1).max(1).values.median() * 2.5))
    out = []
    for t in range(d.shape[0]):
        m = (masks[t] * valid[t] * (d[t] > 0))[None, None]
        blurred = torch_median_blur(d[t][None, None], m, K)[0, 0]
        out.append(blurred * masks[t] + d[t] * (1 - masks[t]))
    return torch.stack(out)


def torch_tracks_3d(raw, queries, imgs, depths, masks, Ks, w2cs):
    Tn, H, W = depths.shape
    inv_Ks, c2ws = torch.linalg.inv(Ks), torch.linalg.inv(w2cs)
    scale = torch.tensor([W - 1.0, H - 1.0], device=depths.device)
    parts = []
    for q, tr in zip(queries, raw):
        tr = tr.swapdims(0, 1)  # [T,N,4]
        xy, occ, dist = tr[..., :2], tr[..., 2], tr[..., 3]
        vis, conf = 1 - torch.sigmoid(occ), 1 - torch.sigmoid(dist)
        visible, invisible = vis * conf > 0.5, (1 - vis) * conf > 0.5
        conf = conf * (visible | invisible).float()
        grid = (xy / scale * 2 - 1)[:, None]  # [T,1,N,2]
        depth = F.grid_sample(depths[:, None], grid, align_corners=True, padding_mode="border")[:, 0, 0]
        cam = torch.einsum("tij,tnj->tni", inv_Ks, F.pad(xy, (0, 1), value=1.0)) * depth[..., None]
        xyz = torch.einsum("tij,tnj->tni", c2ws, F.pad(cam, (0, 1), value=1.0))[..., :3]
        inside = F.grid_sample(masks[:, None], grid, align_corners=True)[:, 0, 0] == 1
        visible, invisible, conf = visible & inside, invisible & inside, conf * inside.float()
        colors = F.grid_sample(imgs[q:q + 1].permute(0, 3, 1, 2), grid[q:q + 1], align_corners=True, padding_mode="border")[0, :, 0].T
        count = visible.sum(0)
        keep = count >= min(int(0.05 * Tn), count.float().quantile(0.1).item())
        parts.append((xyz[:, keep], visible[:, keep], invisible[:, keep], conf[:, keep], colors[keep]))
    return [torch.cat(x, 1 if i < 4 else 0) for i, x in enumerate(zip(*parts))]


def torch_bkgd_points(imgs, depths, masks, valid, Ks, w2cs, num_samples, generator):
    Tn, H, W = depths.shape
    gx, gy = torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float32), torch.arange(H, device=dev, dtype=torch.float32), indexing="xy")
    pix = torch.stack([gx, gy, torch.ones_like(gx)], -1)
    out = []
    for t in range(Tn):
        keep = ((1 - masks[t]) * valid[t] * (depths[t] > 0)).bool()
        c2w = torch.linalg.inv(w2cs[t])
        world = ((pix @ torch.linalg.inv(Ks[t]).T) * depths[t][..., None]) @ c2w[:3, :3].T + c2w[:3, 3]
        n = torch.linalg.cross(world[1:-1, 2:] - world[1:-1, :-2], world[:-2, 1:-1] - world[2:, 1:-1])
        normals = F.pad(F.normalize(n, dim=-1).permute(2, 0, 1), (1, 1, 1, 1)).permute(1, 2, 0)
        rows = [world[keep], normals[keep], imgs[t][keep]]
        want = num_samples // Tn if t != Tn - 1 else num_samples - (Tn - 1) * (num_samples // Tn)
        if want < rows[0].shape[0]:
            sel = torch.randperm(rows[0].shape[0], generator=generator)[:want].to(dev)
            rows = [x[sel] for x in rows]
        out.append(rows)
    return [torch.cat(x) for x in zip(*out)]


lines = [f"# deblur4dgs_amd.observations against torch ops on the same device ({torch.cuda.get_device_name(0)}): milliseconds per call,",
         f"# median (min - max) of {a.rounds} HIP-event windows behind a warm-up; T = {T} frames, k = {K}, {N} tracks per query frame",
         "# one box, one run; scripts/bench_observations.py"]
for H, W in ((288, 512), (480, 854)):
    gen = torch.Generator().manual_seed(H)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    blob = (((xx - W / 2) / (W / 4)) ** 2 + ((yy - H / 2) / (H / 3)) ** 2 < 1).float()  # a foreground blob: ~ 20 % of the image
    masks = blob[None].repeat(T, 1, 1).to(dev)
    depths = (2.0 + 3.0 * torch.rand(T, H, W, generator=gen)).to(dev)
    valid = (torch.rand(T, H, W, generator=gen) < 0.97).float().to(dev)
    imgs = torch.rand(T, H, W, 3, generator=gen).to(dev)
    Ks = torch.tensor([[0.9 * W, 0.0, W / 2], [0.0, 0.9 * W, H / 2], [0.0, 0.0, 1.0]]).repeat(T, 1, 1).to(dev)
    w2cs = torch.eye(4).repeat(T, 1, 1)
    w2cs[:, 0, 3] = torch.linspace(-0.2, 0.2, T)
    w2cs = w2cs.to(dev)
    xy = torch.rand(N, T, 2, generator=gen) * torch.tensor([W / 2, H / 1.5]) + torch.tensor([W / 4, H / 6])
    raw = [torch.cat([xy, torch.randn(N, T, 2, generator=gen) - 1.5], -1).to(dev) for _ in range(T)]
    queries = list(range(T))
    fg = ((masks * valid * (depths > 0)) > 0.5).float()
    rows = (("filter_depths", lambda: O.filter_depths(depths, masks, valid, K), lambda: torch_filter_depths(depths, masks, valid)),
            ("tracks_3d", lambda: O.tracks_3d(raw, queries, imgs, depths, fg, Ks, w2cs), lambda: torch_tracks_3d(raw, queries, imgs, depths, fg, Ks, w2cs)),
            ("bkgd_points", lambda: O.bkgd_points(imgs, depths, masks, valid, Ks, w2cs, 100000, torch.Generator().manual_seed(0)),
             lambda: torch_bkgd_points(imgs, depths, masks, valid, Ks, w2cs, 100000, torch.Generator().manual_seed(0))))
    for name, ours, theirs in rows:
        (m0, lo0, hi0), (m1, lo1, hi1) = timed(ours), timed(theirs)
        lines.append(f"{H:4d} x {W:4d}  {name:14s} HIP {m0:9.3f} ({lo0:.3f} - {hi0:.3f})   torch ops {m1:9.3f} ({lo1:.3f} - {hi1:.3f})   x {m1 / m0:.1f}")
        print(lines[-1], flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
