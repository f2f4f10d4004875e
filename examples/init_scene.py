"""A scene from nothing but tracks: synthetic 3-D tracks and static points -> deblur4dgs_amd.scene_init -> SceneModel -> one render.

    python examples/init_scene.py [--tracks 4000] [--frames 12] [--bases 6] [--points 8000]

What a user with a reference-format dataset does before training: `init_motion_params_with_procrustes` clusters the tracks' velocity
directions (HIP k-means), fits an SE(3) per (basis, frame) pair (HIP moments + one batched SVD on the host), `init_fg_from_tracks_3d`
and `init_bg` size the Gaussians by their 3 nearest neighbours (HIP kNN).  Prints the shapes of what comes out."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import scene_init as S  # noqa: E402
from deblur4dgs_amd.scene_model import SceneModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tracks", type=int, default=4000)
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--bases", type=int, default=6)
ap.add_argument("--points", type=int, default=8000)
ap.add_argument("--seed", type=int, default=0)
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

bases, coefs, tracks = S.init_motion_params_with_procrustes(tracks, K, "6d", cano_t, generator=torch.Generator().manual_seed(a.seed))
fg = S.init_fg_from_tracks_3d(cano_t, tracks, coefs, generator=torch.Generator().manual_seed(a.seed))
bg = S.init_bg(points)
print(f"tracks kept {tracks.xyz.shape[0]} of {G}; bases rots {tuple(bases.params['rots'].shape)} transls {tuple(bases.params['transls'].shape)}; "
      f"skipped pairs {sum(len(v) for v in bases.skipped_ts.values())}")
for name, gp in (("fg", fg), ("bg", bg)):
    print(name, {k: tuple(v.shape) for k, v in gp.params.items()}, "scene_scale", float(gp.scene_scale))

W, H = 96, 64
Ks = torch.tensor([[80.0, 0.0, W / 2], [0.0, 80.0, H / 2], [0.0, 0.0, 1.0]]).repeat(T, 1, 1)
w2cs = torch.eye(4).repeat(T, 1, 1)
w2cs[:, 2, 3] = 5.0
model = SceneModel(Ks, w2cs, fg, bases, bg).to(dev)
with torch.no_grad():
    out = model.render(cano_t, model.w2cs[cano_t:cano_t + 1], model.Ks[cano_t:cano_t + 1], (W, H), return_depth=True)
print("render", {k: tuple(v.shape) for k, v in out.items() if torch.is_tensor(v)}, f"mean alpha {float(out['acc'].mean()):.3f}")
