"""A scene from nothing but tracks: synthetic 3-D tracks and static points -> deblur4dgs_amd.scene_init -> SceneModel -> one render.

    python examples/init_scene.py [--tracks 4000] [--frames 12] [--bases 6] [--points 8000] [--from-2d] [--warmup N]

What a user with a reference-format dataset does before training: `init_motion_params_with_procrustes` clusters the tracks' velocity
directions (HIP k-means), fits an SE(3) per (basis, frame) pair (HIP moments + one batched SVD on the host), `init_fg_from_tracks_3d`
and `init_bg` size the Gaussians by their 3 nearest neighbours (HIP kNN).  Prints the shapes of what comes out.

With --from-2d the observations are not handed over but derived, as from a dataset's raw arrays: the known moving scene is drawn into
per-frame depth maps, foreground masks and TAPIR-style 2-D tracks (x, y, occlusion logit, expected-distance logit) in front of a
textured wall, and deblur4dgs_amd.observations turns those back into observations: `filter_depths` (HIP masked median blur),
`tracks_3d` (HIP lifting) and `bkgd_points` (HIP points, normals and ordered compaction).

With --warmup N the first scene is then fitted to its tracks for N iterations by `scene_init.run_initial_optim` (the reference runs
1000): schedule, loss, backward and Adam of one iteration captured in a HIP graph and replayed.  Prints the first and the last row of
the loss history (the weighted total, then track_3d, track_2d, coef_sparse, smooth_bases, smooth_tracks, z_accel)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import observations as O  # noqa: E402
from deblur4dgs_amd import scene_init as S  # noqa: E402
from deblur4dgs_amd.scene_model import SceneModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tracks", type=int, default=4000)
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--bases", type=int, default=6)
ap.add_argument("--points", type=int, default=8000)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--warmup", type=int, default=0, help="iterations of run_initial_optim on the first scene (0: none)")
ap.add_argument("--from-2d", action="store_true", help="derive the observations from synthetic depths, masks and 2-D tracks")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("init_scene.py needs an MI355X (ROCm) device")
dev = "cuda:0"
G, T, K = a.tracks, a.frames, a.bases
cano_t = T // 2
gen = torch.Generator().manual_seed(a.seed)

# K groups of tracks, each moving along its own smooth path, seen through occlusions
motions = torch.cumsum(torch.cumsum(torch.randn(K, T, 3, generator=gen) * 0.02, 1) + torch.randn(K, 1, 3, generator=gen) * 0.05, 1)
group = torch.randint(0, K, (G,), generator=gen)
xyz = torch.randn(G, 1, 3, generator=gen) * 0.6 + motions[group] + 0.005 * torch.randn(G, T, 3, generator=gen)
visibles = torch.rand(G, T, generator=gen) < 0.85
tracks = S.TrackObservations(xyz, visibles, ~visibles, torch.rand(G, T, generator=gen) * 0.5 + 0.5, torch.rand(G, 3, generator=gen) * 0.9 + 0.05).to(dev)
# a static floor with upward normals
floor = torch.rand(a.points, 3, generator=gen) * torch.tensor([6.0, 6.0, 0.05]) - torch.tensor([3.0, 3.0, 1.5])
points = S.StaticObservations(floor, torch.tensor([[0.0, 0.0, 1.0]]).expand(a.points, 3).contiguous(),
                              torch.rand(a.points, 3, generator=gen) * 0.9 + 0.05).to(dev)
W, H = 96, 64
Ks = torch.tensor([[80.0, 0.0, W / 2], [0.0, 80.0, H / 2], [0.0, 0.0, 1.0]]).repeat(T, 1, 1)
w2cs = torch.eye(4).repeat(T, 1, 1)
w2cs[:, 2, 3] = 5.0

if a.from_2d:
    # the scene as a dataset would hold it: every track is a 5 x 5 pixel patch at its own depth in front of a wall at camera z = 8
    cam = xyz @ w2cs[0, :3, :3].T + w2cs[0, :3, 3]                                # [G,T,3] (the camera does not move)
    uv = cam[..., :2] / cam[..., 2:] * Ks[0, 0, 0] + Ks[0, :2, 2]                   # [G,T,2] pixel coordinates
    depths, masks = torch.full((T, H, W), 8.0), torch.zeros(T, H, W)
    centre = uv.round().long()
    for g in torch.argsort(cam[:, cano_t, 2], descending=True).tolist():           # far to near: the nearest patch stays on top
        for t in range(T):
            cx, cy = centre[g, t].tolist()
            if 2 <= cx < W - 2 and 2 <= cy < H - 2:
                depths[t, cy - 2:cy + 3, cx - 2:cx + 3] = cam[g, t, 2]
                masks[t, cy - 2:cy + 3, cx - 2:cx + 3] = 1.0
    depths += 0.3 * (torch.rand(T, H, W, generator=gen) < 0.02) * masks              # speckle that the median blur removes
    imgs = torch.rand(T, H, W, 3, generator=gen) * 0.9 + 0.05
    logit = torch.where(visibles, -4.0, 4.0)                                         # occlusion logit: visible <=> negative
    tracks_2d = torch.cat([uv, logit[..., None], torch.full((G, T, 1), -4.0)], -1)  # [G,T,4]
    queries = [0, cano_t, T - 1]                                                    # each third of the tracks was queried in one frame
    raw = [tracks_2d[i::3].to(dev) for i in range(3)]
    valid = torch.ones(T, H, W)
    d = O.filter_depths(depths.to(dev), masks.to(dev), valid.to(dev))
    fg_masks = ((masks.to(dev) * (d > 0)) > 0.5).float()
    tracks = O.tracks_3d(raw, queries, imgs.to(dev), d, fg_masks, Ks.to(dev), w2cs.to(dev))
    points = O.bkgd_points(imgs.to(dev), d, masks.to(dev), valid.to(dev), Ks.to(dev), w2cs.to(dev), a.points,
                           generator=torch.Generator().manual_seed(a.seed))
    print(f"from 2-D: {int((d.cpu() != depths).sum())} depths changed by the blur; tracks {tracks.xyz.shape[0]} of {G} kept, "
          f"{float(tracks.visibles.float().mean()):.2f} visible; background points {points.xyz.shape[0]}")
    G = tracks.xyz.shape[0]

bases, coefs, tracks = S.init_motion_params_with_procrustes(tracks, K, "6d", cano_t, generator=torch.Generator().manual_seed(a.seed))
fg = S.init_fg_from_tracks_3d(cano_t, tracks, coefs, generator=torch.Generator().manual_seed(a.seed))
bg = S.init_bg(points)
print(f"tracks kept {tracks.xyz.shape[0]} of {G}; bases rots {tuple(bases.params['rots'].shape)} transls {tuple(bases.params['transls'].shape)}; "
      f"skipped pairs {sum(len(v) for v in bases.skipped_ts.values())}")
for name, gp in (("fg", fg), ("bg", bg)):
    print(name, {k: tuple(v.shape) for k, v in gp.params.items()}, "scene_scale", float(gp.scene_scale))

if a.warmup > 0:
    fg, bases = fg.to(dev), bases.to(dev)
    hist = S.run_initial_optim(fg, bases, tracks, Ks.to(dev), w2cs.to(dev), num_iters=a.warmup)
    for label, row in (("first", hist["losses"][0]), ("last", hist["losses"][-1])):
        print(f"warm-up {label:5s}", " ".join(f"{x:.5f}" for x in row.tolist()))

model = SceneModel(Ks, w2cs, fg, bases, bg).to(dev)
with torch.no_grad():
    out = model.render(cano_t, model.w2cs[cano_t:cano_t + 1], model.Ks[cano_t:cano_t + 1], (W, H), return_depth=True)
print("render", {k: tuple(v.shape) for k, v in out.items() if torch.is_tensor(v)}, f"mean alpha {float(out['acc'].mean()):.3f}")
