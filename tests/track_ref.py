"""The 2-D track loss and the mapped-depth loss restated in torch on the CPU (fp64 unless told otherwise): what
deblur4dgs_amd.losses.track_losses must compute.

Written from the description in DESIGN.md section 17: each query GATHERS its own pixel of the rendered track image (the reference
projects the whole image and pairs the i-th pixel of the queries' mask with the i-th query instead; tests/test_track_ref.py pins
this restatement to values recorded from that flow around the reference's own masked_l1_loss, tests/golden/track_losses.npz,
whose queries are distinct and raster-ordered - the case in which the two pairings are the same).  Differentiable with respect
to `tracks_3d` through torch autograd; rank, threshold and kept set come from tests/trimmed_ref.py.

    element (b, n, p), visible and inside the image:   X = tracks_3d[b, int(y_p), int(x_p), n],  P = K[b, n] X,
                                                       z = max(P_z, 1e-6),  xy = P_xy / z
    2-D term     v = mean(|xy - target|), kept where v < quantile(v) over the visible elements (quantile >= 1: all)
    depth term   v = |1 / (z + 1e-5) - 1 / (d + 1e-5)|, all kept
    each         sum_kept v w / (sum_kept w + 1e-8),  w the weights, a trailing axis summed

No visible element: the 2-D term is NaN when it selects (the reference raises), the depth term 0; the gradient is zero."""
import torch

from tests import trimmed_ref as R


def _lists(x):
    return [x] if torch.is_tensor(x) else list(x)


def elements(tracks_3d, query_tracks_2d, target_Ks, target_tracks_2d, target_visibles, track_weights, target_track_depths):
    """-> (v_2d, v_depth, weights, P_z) of the live elements, in element order, in the dtype of tracks_3d, and the boolean [n] `live`."""
    B, H, W, N, _ = tracks_3d.shape
    dt = tracks_3d.dtype
    v2d, vdep, pz, live = [], [], [], []
    for b, (q, Ks, t2d, vis, dep) in enumerate(zip(_lists(query_tracks_2d), _lists(target_Ks), _lists(target_tracks_2d),
                                                   _lists(target_visibles), _lists(target_track_depths))):
        xy = q.to(torch.int64)
        x, y = xy[:, 0], xy[:, 1]
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        pts = tracks_3d[b, y.clamp(0, H - 1), x.clamp(0, W - 1)]  # [P, N, 3] (clamped indices: masked out below)
        proj = torch.einsum("nij,pnj->npi", Ks.to(dt), pts)  # [N, P, 3]
        z = proj[..., 2].clamp(min=1e-6)
        pred = proj[..., :2] / z[..., None]
        v2d.append((pred - t2d.to(dt)).abs().mean(-1).reshape(-1))
        vdep.append((1.0 / (z + 1e-5) - 1.0 / (dep.to(dt) + 1e-5)).abs().reshape(-1))
        pz.append(proj[..., 2].reshape(-1))
        live.append(((vis != 0) & inside[None]).reshape(-1))
    live = torch.cat(live)
    w = track_weights.to(dt)
    w = w.sum(-1) if w.dim() == 2 else w
    assert w.shape == live.shape, (w.shape, live.shape)
    return torch.cat(v2d)[live], torch.cat(vdep)[live], w[live], torch.cat(pz)[live], live


def track_losses(tracks_3d, query_tracks_2d, target_Ks, target_tracks_2d, target_visibles, track_weights, target_track_depths,
                 quantile=0.98, rank_dtype=torch.float64):
    v2d, vdep, w, _, _ = elements(tracks_3d, query_tracks_2d, target_Ks, target_tracks_2d, target_visibles, track_weights,
                                  target_track_depths)
    zero = torch.zeros_like(v2d[..., None])
    if v2d.numel() == 0:  # a zero that still hangs on tracks_3d, so that the gradient is zeros and not None
        nothing = tracks_3d.sum() * 0.0
        return nothing + (float("nan") if quantile < 1 else 0.0), nothing
    return (R.masked_l1_loss(v2d[..., None], zero, w, True, quantile, rank_dtype),
            R.masked_l1_loss(vdep[..., None], zero, w, True, 1.0, rank_dtype))
