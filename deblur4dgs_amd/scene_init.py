"""A first scene from 3-D tracks and static points: what flow3d/init_utils.py builds before training starts.

The reference rests on cupy (`batched_interp_masked`), cuML (`KMeans`), sklearn on the host (`knn`) and a Python loop with one
`torch.linalg.svd` per (basis, frame) pair; here the four steps are HIP kernels (`csrc/scene_init.hip`, the "Scene initialisation"
block of include/d4gs.h) and the rest is stated in this project's own words with torch ops on the device.  There is no torch fallback
for a kernel: a CPU tensor is refused.

    tracks = TrackObservations(xyz, visibles, invisibles, confidences, colors)           # [G,T,3], [G,T] x 3, [G,3]
    bases, coefs, tracks = init_motion_params_with_procrustes(tracks, 20, "6d", cano_t)  # MotionBases, [G',K], filtered tracks
    fg = init_fg_from_tracks_3d(cano_t, tracks, coefs)
    bg = init_bg(StaticObservations(xyz, normals, colors))
    model = scene_model.SceneModel(Ks, w2cs, fg, bases, bg)

What differs from the reference, on purpose:
  * k-means starts from k-means++ centres drawn from a `torch.Generator` and runs Lloyd iterations to a fixed point (or `max_iter`);
    cuML's random initialisation cannot be matched, so the labels are a Lloyd fixed point of the seed given here, not cuML's labels;
  * the interpolation treats a row of any length as one row (the reference restarts every 64 frames) and keeps a track without a
    visible frame as it is (the reference's callers filter those out first);
  * `init_bg` restates `roma.rotvec_to_unitquat` in closed form; roma is not installed where this was written, so parity with roma
    itself is unpinned (the tests hold the closed form to an fp64 statement of the same formula);
  * the `err` / `err_before` figures that the reference logs per pair are not computed: they would cost a second pass over the tracks
    for two log lines;
  * `MotionBases` of this package holds 6-D rotations only: `rot_type="quat"` is served by `solve_motion_bases`, which returns the
    tensors, and refused by `init_motion_params_with_procrustes`.
`run_initial_optim`, the warm-up that fits the bases, the coefficients and the means to the tracks before training, is provided:
`track_fit_targets` prepares the observations once, `losses.track_fit_losses` is its loss (csrc/track_fit.hip), and the loop keeps
its schedule, its Adam state and its iteration count on the device, so one iteration is captured in a HIP graph and replayed
(DESIGN.md section 27).
Not here: the depth-range term of that warm-up (no caller of the reference sets it), the HDBSCAN mode, the viser visualisations, the
dataset readers.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math

import torch
import torch.nn.functional as F

from . import _lib as L
from ._lib import check, need_gpu, stream_of, vp

__all__ = ["TrackObservations", "StaticObservations", "track_features", "interp_tracks", "knn", "kmeans", "kmeans_step",
           "procrustes_moments", "get_weights_for_procrustes", "sample_initial_bases_centers", "solve_motion_bases",
           "init_motion_params_with_procrustes", "init_fg_from_tracks_3d", "init_bg", "TrackFitTargets", "track_fit_targets",
           "track_fit_schedule", "run_initial_optim", "FIT_LR0", "KNN_TILE", "KNN_SPLIT_MIN", "KNN_MAX_K",
           "KMEANS_MAX_K"]

KNN_TILE, KNN_SPLIT_MIN, KNN_MAX_K, KMEANS_MAX_K = L.KNN_TILE, L.KNN_SPLIT_MIN, L.KNN_MAX_K, L.KMEANS_MAX_K
WHO = "deblur4dgs_amd.scene_init"


class _Observations:
    def map(self, fn):
        return type(self)(**{f.name: fn(getattr(self, f.name)) for f in dataclasses.fields(self)})

    def to(self, device):
        return self.map(lambda x: x.to(device))

    def filter_valid(self, valid_mask):
        return self.map(lambda x: x[valid_mask])

    def __getitem__(self, key):
        return self.map(lambda x: x[key])


@dataclasses.dataclass
class TrackObservations(_Observations):
    """flow3d/tensor_dataclass.py: `xyz [G,T,3]`, `visibles`, `invisibles` [G,T] bool, `confidences [G,T]`, `colors [G,3]`."""
    xyz: torch.Tensor
    visibles: torch.Tensor
    invisibles: torch.Tensor
    confidences: torch.Tensor
    colors: torch.Tensor

    def check_sizes(self) -> bool:
        dims = self.xyz.shape[:-1]
        return (self.visibles.shape == dims and self.invisibles.shape == dims and self.confidences.shape == dims
                and self.colors.shape[:-1] == dims[:-1] and self.xyz.shape[-1] == 3 and self.colors.shape[-1] == 3)


@dataclasses.dataclass
class StaticObservations(_Observations):
    """`xyz`, `normals`, `colors`, each [N,3]."""
    xyz: torch.Tensor
    normals: torch.Tensor
    colors: torch.Tensor

    def check_sizes(self) -> bool:
        return self.normals.shape == self.xyz.shape and self.colors.shape == self.xyz.shape


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


# ---- the four kernels -----------------------------------------------------------------------------------------------------------
def track_features(xyz, visibles, want_interp: bool = True, want_vel: bool = True):
    """xyz [G,T,3], visibles [G,T] (bool or any integer / float: non-zero = visible) -> (xyz_interp [G,T,3], vel_dirs [G,3(T-1)]);
    an output that is not wanted is None.  `xyz_interp` is np.interp per track and coordinate over the visible frames, visible frames
    copied bit for bit; `vel_dirs[g, 3t + c] = v_c / (|v| + 1e-5)`, v the step of the interpolated track from frame t to t + 1."""
    need_gpu(xyz, WHO)
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or tuple(visibles.shape) != tuple(xyz.shape[:2]):
        raise ValueError(f"xyz must be [G,T,3] and visibles [G,T], got {tuple(xyz.shape)} and {tuple(visibles.shape)}")
    G, T, _ = xyz.shape
    x = _f32(xyz)
    v = (visibles != 0).to(device=x.device, dtype=torch.uint8).contiguous()
    interp = torch.empty_like(x) if want_interp else None
    vel = torch.empty(G, 3 * (T - 1), device=x.device, dtype=torch.float32) if want_vel else None
    check(L.lib().d4gs_track_features(vp(x), vp(v), G, T, vp(interp), vp(vel), stream_of(x)), "d4gs_track_features")
    return interp, vel


def interp_tracks(xyz, visibles):
    """`batched_interp_masked` (init_utils.py:594-654) for tracks: [G,T,3] with the invisible frames filled in."""
    return track_features(xyz, visibles, want_vel=False)[0]


def knn(x, k: int):
    """x [N,3] -> (dists [N,k] fp32 ascending, idx [N,k] int32): the k nearest other points of every point, exact (brute force over all
    pairs; the distance is the root of the sum of squared coordinate differences).  Self is excluded by index, so duplicates of a point
    are its neighbours at distance 0.  Both tensors stay on the device (the reference returns NumPy arrays from sklearn)."""
    need_gpu(x, WHO)
    if x.dim() != 2 or x.shape[-1] != 3:
        raise ValueError(f"x must be [N,3], got {tuple(x.shape)}")
    N = x.shape[0]
    lib = L.lib()
    nbytes = lib.d4gs_knn_workspace_bytes(N, int(k))
    if nbytes == 0:
        raise ValueError(f"knn: N={N}, k={k} (1 <= k <= {KNN_MAX_K}, k + 1 <= N <= 2^24)")
    p = _f32(x)
    dists = torch.empty(N, k, device=p.device, dtype=torch.float32)
    idx = torch.empty(N, k, device=p.device, dtype=torch.int32)
    ws = torch.empty(nbytes // 4, device=p.device, dtype=torch.float32)
    check(lib.d4gs_knn(vp(p), N, int(k), vp(dists), vp(idx), vp(ws), stream_of(p)), "d4gs_knn")
    return dists, idx


def kmeans_step(x, centres, labels, iters: int = 1, changed=None):
    """`iters` Lloyd iterations in place on `centres [K,D]` fp32 and `labels [G]` int32 (both contiguous, on x's device); returns the
    device int32 tensor [1] with the number of labels the last iteration changed.  Nothing is read on the host."""
    need_gpu(x, WHO)
    if x.dim() != 2 or centres.dim() != 2 or centres.shape[1] != x.shape[1] or labels.shape != (x.shape[0],):
        raise ValueError(f"x [G,D], centres [K,D], labels [G] expected, got {tuple(x.shape)}, {tuple(centres.shape)}, {tuple(labels.shape)}")
    if (x.dtype, centres.dtype, labels.dtype) != (torch.float32, torch.float32, torch.int32) or not (
            x.is_contiguous() and centres.is_contiguous() and labels.is_contiguous()):
        raise ValueError("kmeans_step works in place: x, centres must be contiguous fp32 and labels contiguous int32")
    G, D = x.shape
    K = centres.shape[0]
    lib = L.lib()
    nbytes = lib.d4gs_kmeans_scratch_bytes(G, D, K)
    if nbytes == 0 or iters < 1:
        raise ValueError(f"kmeans_step: G={G} D={D} K={K} iters={iters} (1 <= K <= {KMEANS_MAX_K}, K D <= 12288, iters >= 1)")
    scratch = torch.empty(nbytes // 8, device=x.device, dtype=torch.float64)
    changed = torch.empty(1, device=x.device, dtype=torch.int32) if changed is None else changed
    check(lib.d4gs_kmeans_step(vp(x), G, D, K, int(iters), vp(centres), vp(labels), vp(changed), vp(scratch), stream_of(x)),
          "d4gs_kmeans_step")
    return changed


def _kmeans_pp(x, K, generator):
    """k-means++ seeding with plain torch ops: the first centre uniformly, each further one with probability proportional to the squared
    distance to the nearest centre chosen so far.  Random numbers come from `generator` (any device); -> indices [K] into x."""
    G = x.shape[0]
    u = torch.rand(K, generator=generator, dtype=torch.float64, device=None if generator is None else generator.device).to(x.device)
    first = (u[0] * G).long().clamp(max=G - 1)
    chosen = [first]
    d2 = (x - x[first]).square().sum(-1).double()
    for k in range(1, K):
        c = torch.cumsum(d2, 0)
        nxt = torch.searchsorted(c, (u[k] * c[-1]).reshape(1), right=True).clamp(max=G - 1)[0]
        chosen.append(nxt)
        d2 = torch.minimum(d2, (x - x[nxt]).square().sum(-1).double())
    return torch.stack(chosen)


def kmeans(x, num_clusters: int, generator=None, max_iter: int = 300, chunk: int = 10):
    """Lloyd's k-means on x [G,D] -> (labels [G] int64, centres [K,D] fp32, iterations run).  Centres start from k-means++ (drawn from
    `generator`); the iterations run on the device `chunk` at a time and stop when an iteration changes no label or at `max_iter`
    (cuML's default).  The labels are a Lloyd fixed point of this seeding - not cuML's labels, whose initialisation cannot be matched.
    Bitwise reproducible for a given generator state."""
    need_gpu(x, WHO)
    x = _f32(x)
    G = x.shape[0]
    if not 1 <= num_clusters <= min(KMEANS_MAX_K, G):
        raise ValueError(f"kmeans: num_clusters={num_clusters} (1 <= K <= min({KMEANS_MAX_K}, G={G}))")
    centres = x[_kmeans_pp(x, num_clusters, generator)].contiguous()
    labels = torch.full((G,), -1, device=x.device, dtype=torch.int32)
    changed = torch.empty(1, device=x.device, dtype=torch.int32)
    done = 0
    while done < max_iter:
        n = min(chunk, max_iter - done)
        kmeans_step(x, centres, labels, n, changed)
        done += n
        if int(changed.item()) == 0:  # (a fixed point stays one: the chunk's later iterations changed nothing either)
            break
    return labels.long(), centres, done


def procrustes_moments(xyz, weights, conf, order, seg, cano_t: int):
    """The weighted sums under `solve_procrustes` for every (cluster, frame) pair in one launch -> [K,T,16] float64 on the device:
    sum u, sum u src (3), sum u dst (3), sum u dst (x) src (9, row-major), with u = w[p,cano_t] w[p,t] (conf[p,cano_t] + conf[p,t]) / 2
    over the tracks p = order[seg[n]:seg[n + 1]] of cluster n, src = xyz[p,cano_t], dst = xyz[p,t]."""
    need_gpu(xyz, WHO)
    G, T, _ = xyz.shape
    K = seg.shape[0] - 1
    if tuple(weights.shape) != (G, T) or tuple(conf.shape) != (G, T) or order.dim() != 1 or K < 1:
        raise ValueError(f"weights, conf must be [G,T] = {(G, T)}, order [n], seg [K + 1]; got {tuple(weights.shape)}, {tuple(conf.shape)}, "
                         f"{tuple(order.shape)}, {tuple(seg.shape)}")
    x, w, c = _f32(xyz), _f32(weights), _f32(conf)
    o = order.to(device=x.device, dtype=torch.int32).contiguous()
    if o.shape[0] < G:  # the kernel clamps seg to G entries of order: give it G
        o = torch.cat([o, o.new_full((G - o.shape[0],), -1)])
    s = seg.to(device=x.device, dtype=torch.int32).contiguous()
    out = torch.empty(K, T, 16, device=x.device, dtype=torch.float64)
    check(L.lib().d4gs_procrustes_moments(vp(x), vp(w), vp(c), vp(o), vp(s), G, T, K, int(cano_t), vp(out), stream_of(x)),
          "d4gs_procrustes_moments")
    return out


# ---- the reference's rules, in this project's words -------------------------------------------------------------------------------
def get_weights_for_procrustes(clusters, visibilities=None):
    """loss_utils.py:102-115 for one cluster: clusters [T,n,3], visibilities [T,n] -> weights [T,n].  Per frame, the distance of every
    track to the frame's coordinate-wise (lower) median, divided by the frame's median distance; weight = exp(-distance) over the
    frame's mean weight (+ 1e-6), times (visible + 1e-6); zero where the distance exceeds the 0.9 quantile (linear interpolation) of
    the whole cluster's distances, and where the weight is NaN."""
    centre = clusters.median(dim=-2, keepdim=True).values
    dist = torch.linalg.vector_norm(clusters - centre, dim=-1)
    dist = dist / dist.median(dim=-1, keepdim=True).values
    w = torch.exp(-dist)
    w = w / (w.mean(dim=-1, keepdim=True) + 1e-6)
    if visibilities is not None:
        w = w * (visibilities.to(w.dtype) + 1e-6)
    invalid = (dist > torch.quantile(dist.flatten(), 0.9)) | torch.isnan(w)
    return w.masked_fill(invalid, 0.0)


def _rotmat_to_quat_wxyz(R):
    """roma.rotmat_to_unitquat (1.5.0) followed by the reference's roll to wxyz, for R [..., 3, 3]: the branch is the first maximum of
    (R00, R11, R22, trace); the candidate of that branch is normalised.  (csrc/common.h states the same rule for the kernels.)"""
    flat = R.reshape(-1, 3, 3)
    tr = flat[:, 0, 0] + flat[:, 1, 1] + flat[:, 2, 2]
    choice = torch.stack([flat[:, 0, 0], flat[:, 1, 1], flat[:, 2, 2], tr], -1).argmax(-1)  # (torch.argmax: the first maximum)
    cands = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        c = [None] * 4
        c[i] = 1 - tr + 2 * flat[:, i, i]
        c[j] = flat[:, j, i] + flat[:, i, j]
        c[k] = flat[:, k, i] + flat[:, i, k]
        c[3] = flat[:, k, j] - flat[:, j, k]
        cands.append(torch.stack(c, -1))
    cands.append(torch.stack([flat[:, 2, 1] - flat[:, 1, 2], flat[:, 0, 2] - flat[:, 2, 0], flat[:, 1, 0] - flat[:, 0, 1], 1 + tr], -1))
    q = torch.stack(cands, 1)[torch.arange(flat.shape[0]), choice]  # xyzw
    q = q / torch.linalg.vector_norm(q, dim=-1, keepdim=True)
    return q.roll(1, dims=-1).reshape(*R.shape[:-2], 4)


def solve_motion_bases(xyz, visibles, confidences, labels, cano_t: int, rot_type: str = "6d", min_mean_weight: float = 0.1):
    """The loop of init_motion_params_with_procrustes (:171-240) -> (rots [K,T,6|4], transls [K,T,3], skipped, ids): for every label
    present (ids, ascending) and every frame the SE(3) transform that carries the cluster's tracks at `cano_t` onto frame t under the
    weights u = w[cano_t] w[t] (conf[cano_t] + conf[t]) / 2, w from `get_weights_for_procrustes`.  The weighted moments of all pairs
    come from one kernel launch; the 3x3 problems are solved in fp64 on a host copy of those K T 16 numbers with one batched SVD
    (R = U diag(1, 1, det U det Vh < 0 ? -1 : 1) Vh, t = dst_mean - R src_mean).  Frames are visited cano_t - 1 ... 0, then cano_t ...
    T - 1, `prev` starting at cano_t; a pair whose weight sum is below min_mean_weight * T takes the transform stored for `prev` at
    that moment (the identity while cano_t itself has not been visited) and is listed in `skipped` {label: [frames]}.  "quat": wxyz,
    the sign nearer to prev's quaternion (the reference's double-cover rule)."""
    need_gpu(xyz, WHO)
    if rot_type not in ("6d", "quat"):
        raise ValueError(f"rot_type={rot_type!r} (\"6d\" or \"quat\")")
    G, T, _ = xyz.shape
    dev = xyz.device
    labels = labels.to(dev).long()
    order = torch.argsort(labels, stable=True)
    ids, counts = torch.unique(labels, return_counts=True)
    counts_host = counts.tolist()
    seg_host = [0]
    for c in counts_host:
        seg_host.append(seg_host[-1] + c)
    K = len(counts_host)
    x = _f32(xyz)
    weights = torch.zeros(G, T, device=dev, dtype=torch.float32)
    vis = visibles.to(dev)
    for n in range(K):
        members = order[seg_host[n]:seg_host[n + 1]]
        weights[members] = get_weights_for_procrustes(x[members].transpose(0, 1), vis[members].transpose(0, 1)).transpose(0, 1)
    seg = torch.tensor(seg_host, dtype=torch.int32, device=dev)
    M = procrustes_moments(x, weights, confidences, order, seg, cano_t).cpu()  # K T 16 doubles: the only host copy
    su = M[..., 0]
    skip = su < min_mean_weight * T
    safe = torch.where(skip, torch.ones_like(su), su)[..., None]
    src_mean, dst_mean = M[..., 1:4] / safe, M[..., 4:7] / safe
    A = M[..., 7:16].reshape(K, T, 3, 3) / safe[..., None] - dst_mean[..., :, None] * src_mean[..., None, :]
    A = torch.where(skip[..., None, None], torch.eye(3, dtype=A.dtype).expand_as(A), A)
    U, _, Vh = torch.linalg.svd(A)
    S = torch.eye(3, dtype=A.dtype).repeat(K, T, 1, 1)
    S[..., 2, 2] = torch.where(torch.linalg.det(U) * torch.linalg.det(Vh) < 0, -1.0, 1.0)
    R = U @ S @ Vh
    t_all = dst_mean - (R @ src_mean[..., None])[..., 0]
    rot_all = torch.cat([R[..., 0], R[..., 1]], -1) if rot_type == "6d" else _rotmat_to_quat_wxyz(R)
    identity = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0] if rot_type == "6d" else [1.0, 0.0, 0.0, 0.0]
    rots = torch.tensor(identity, dtype=torch.float64).repeat(K, T, 1)
    transls = torch.zeros(K, T, 3, dtype=torch.float64)
    visit = list(range(cano_t - 1, -1, -1)) + list(range(cano_t, T))
    skipped = {}
    skip_host = skip.tolist()
    for n, label in enumerate(ids.tolist()):
        prev, mine = cano_t, []
        for cur in visit:
            if skip_host[n][cur]:
                rots[n, cur], transls[n, cur] = rots[n, prev].clone(), transls[n, prev].clone()
                mine.append(cur)
            else:
                r = rot_all[n, cur]
                if rot_type == "quat" and torch.linalg.vector_norm(r - rots[n, prev]) > torch.linalg.vector_norm(-r - rots[n, prev]):
                    r = -r
                rots[n, cur], transls[n, cur] = r, t_all[n, cur]
            prev = cur
        skipped[label] = mine
    return rots.to(dev, torch.float32), transls.to(dev, torch.float32), skipped, ids


def sample_initial_bases_centers(cano_t: int, tracks_3d: TrackObservations, num_bases: int, generator=None):
    """The k-means mode of init_utils.py:534-591 -> (centres [1,K,3], K, labels [G]): the tracks' velocity directions (interpolated
    over invisible frames) are clustered, K = the largest label + 1, and each centre is the coordinate-wise (lower) median of its
    cluster's points at `cano_t` (NaN for a label without points, which the caller drops)."""
    means = tracks_3d.xyz[:, cano_t]
    _, vel = track_features(tracks_3d.xyz, tracks_3d.visibles, want_interp=False)
    labels, _, _ = kmeans(vel, num_bases, generator=generator)
    K = int(labels.max().item()) + 1
    centres = torch.stack([means[labels == i].median(dim=0).values if bool((labels == i).any()) else means.new_full((3,), math.nan)
                           for i in range(K)])
    return centres[None], K, labels


def init_motion_params_with_procrustes(tracks_3d: TrackObservations, num_bases: int, rot_type: str, cano_t: int,
                                       min_mean_weight: float = 0.1, labels=None, generator=None):
    """init_utils.py:114-270 -> (MotionBases, motion_coefs [G',K], the filtered tracks).  Tracks farther from the coordinate-wise median
    of the canonical points than the 0.95 quantile of those distances, and tracks without a visible frame, are dropped first; the rest
    is clustered (`sample_initial_bases_centers`; `labels=` [G], given for the tracks BEFORE the filter, bypasses the clustering and
    takes the per-label medians as centres), labels without a track are dropped, `motion_coefs = 10 exp(-distance to each centre)`,
    and `solve_motion_bases` gives the bases.  The skipped pairs are kept on the result as `bases.skipped_ts`."""
    from .scene_model import MotionBases

    need_gpu(tracks_3d.xyz, WHO)
    if rot_type != "6d":
        raise NotImplementedError("scene_model.MotionBases holds 6-D rotations only; solve_motion_bases(..., rot_type=\"quat\") returns "
                                  "the quaternion bases as tensors")
    means = tracks_3d.xyz[:, cano_t]
    centre = means.median(dim=0).values
    dists = torch.linalg.vector_norm(means - centre, dim=-1)
    valid = (dists < torch.quantile(dists, 0.95)) & tracks_3d.visibles.any(dim=1)
    tracks_3d = tracks_3d.filter_valid(valid)
    means = means[valid]
    if labels is None:
        centres, _, labels = sample_initial_bases_centers(cano_t, tracks_3d, num_bases, generator)
        centres = centres[0]
    else:
        labels = labels.to(means.device).long()[valid]
        centres = None
    rots, transls, skipped, ids = solve_motion_bases(tracks_3d.xyz, tracks_3d.visibles, tracks_3d.confidences, labels, cano_t, rot_type,
                                                     min_mean_weight)
    if centres is None:
        centres = torch.stack([means[labels == i].median(dim=0).values for i in ids.tolist()])
    else:
        centres = centres[ids]
    motion_coefs = 10 * torch.exp(-torch.linalg.vector_norm(means[:, None] - centres[None], dim=-1))
    bases = MotionBases(rots, transls)
    bases.skipped_ts = skipped
    return bases, motion_coefs, tracks_3d


def _knn_scales(xyz):
    """the mean distance to the three nearest other points, [N,1]"""
    return knn(xyz, 3)[0].mean(dim=-1, keepdim=True)


def init_fg_from_tracks_3d(cano_t: int, tracks_3d: TrackObservations, motion_coefs, generator=None):
    """init_utils.py:32-62 -> GaussianParams: means = the tracks at `cano_t`, colours = logit(colours), scales = log of the mean 3-NN
    distance clamped to its own 5 % / 95 % quantiles (the same on all three axes), opacities = logit(0.7), quaternions `torch.rand`
    [G,4] from `generator` (uniform in [0,1)^4 and not normalised, as the reference leaves them)."""
    from .scene_model import GaussianParams

    means = _f32(tracks_3d.xyz[:, cano_t])
    need_gpu(means, WHO)
    G = means.shape[0]
    scales = _knn_scales(means)
    scales = scales.clamp(torch.quantile(scales, 0.05), torch.quantile(scales, 0.95))
    quats = torch.rand(G, 4, generator=generator, device=None if generator is None else generator.device).to(means.device)
    return GaussianParams(means, quats, torch.log(scales.repeat(1, 3)), torch.logit(tracks_3d.colors.float()),
                          torch.logit(torch.full((G,), 0.7, device=means.device)), motion_coefs)


def init_bg(points: StaticObservations):
    """init_utils.py:65-111 -> GaussianParams with `scene_center` = the mean point and `scene_scale` = half the largest extent between
    the 5 % and 95 % quantiles of the centred points per axis; scales = log of the mean 3-NN distance (no clamp, as in the reference);
    quaternions (wxyz) turn +z onto the normal: with c = z x n, axis = c / max(|c|, 1e-12), theta = acos(n_z) |axis|,
    q = [cos(theta / 2), axis sin(theta / 2) / |axis|] - the identity where the cross product vanishes (n = +z, and also n = -z, as the
    reference).  This restates `roma.rotvec_to_unitquat`, which is not installed here: parity with roma itself is unpinned."""
    from .scene_model import GaussianParams

    xyz = _f32(points.xyz)
    need_gpu(xyz, WHO)
    N = xyz.shape[0]
    center = xyz.mean(0)
    centred = xyz - center
    extent = centred.quantile(0.95, dim=0) - centred.quantile(0.05, dim=0)
    scene_scale = torch.max(extent) / 2.0
    normals = points.normals.float()
    z = normals.new_tensor([[0.0, 0.0, 1.0]]).expand_as(normals)
    rotvec = F.normalize(torch.linalg.cross(z, normals), dim=-1) * (z * normals).sum(-1, keepdim=True).acos()
    theta = torch.linalg.vector_norm(rotvec, dim=-1, keepdim=True)
    unit = torch.where(theta > 0, rotvec / theta.clamp_min(1e-30), torch.zeros_like(rotvec))
    quats = torch.cat([torch.cos(theta / 2), unit * torch.sin(theta / 2)], -1)
    return GaussianParams(xyz, quats, torch.log(_knn_scales(xyz).repeat(1, 3)), torch.logit(points.colors.float()),
                          torch.logit(torch.full((N,), 0.7, device=xyz.device)), scene_center=center, scene_scale=scene_scale)


# ---- the warm-up (init_utils.py:273-402) ----------------------------------------------------------------------------------------
FIT_LR0 = (1e-2, 3e-2, 1e-2, 1e-3)  # rots, transls, motion_coefs, means: the reference's four param groups, in its order


class TrackFitTargets:
    """What `d4gs_track_fit_prepare` leaves of the observations: `buf` (device bytes: the time-major planes of xyz, its projection and
    the two weight planes, the sum of the 3-D weights, the camera tables with their centres, 1 / fx), for G tracks and T frames."""

    def __init__(self, buf, G, T):
        self.buf, self.nbytes, self.G, self.T = buf, buf.numel(), G, T


def track_fit_targets(tracks_3d: TrackObservations, Ks, w2cs) -> TrackFitTargets:
    """tracks_3d (xyz [G,T,3], visibles, invisibles, confidences [G,T]), Ks [T,3,3], w2cs [T,4,4] -> the prepared observations
    `losses.track_fit_losses` reads.  Once per run: two launches, nothing read on the host."""
    xyz = tracks_3d.xyz
    need_gpu(xyz, WHO)
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or not tracks_3d.check_sizes():
        raise ValueError(f"tracks_3d: xyz must be [G,T,3] with visibles, invisibles, confidences [G,T]; got xyz {tuple(xyz.shape)}")
    G, T, _ = xyz.shape
    if tuple(Ks.shape) != (T, 3, 3) or tuple(w2cs.shape) != (T, 4, 4):
        raise ValueError(f"Ks {tuple(Ks.shape)} and w2cs {tuple(w2cs.shape)} must be [{T},3,3] and [{T},4,4]: one camera per frame")
    if T < 3:
        raise ValueError(f"T = {T} frames: the fit needs an interior frame (T >= 3)")
    dev = xyz.device
    nbytes = L.lib().d4gs_track_fit_targets_bytes(G, T)
    if nbytes == 0:
        raise RuntimeError(f"track_fit_targets: unsupported size G={G} T={T} (G >= 1, 3 <= T <= 65535, 9 G T <= 2^31 - 1)")
    x, c = _f32(xyz), _f32(tracks_3d.confidences).to(dev)
    vis = (tracks_3d.visibles != 0).to(device=dev, dtype=torch.uint8).contiguous()
    inv = (tracks_3d.invisibles != 0).to(device=dev, dtype=torch.uint8).contiguous()
    K3, W = _f32(Ks).to(dev), _f32(w2cs).to(dev)
    buf = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    check(L.lib().d4gs_track_fit_prepare(vp(x), vp(vis), vp(inv), vp(c), vp(K3), vp(W), G, T, vp(buf), nbytes, stream_of(x)),
          "d4gs_track_fit_prepare")
    return TrackFitTargets(buf, G, T)


def track_fit_schedule(group, it, num_iters: int, weights, lrs=None, lr0=FIT_LR0):
    """d4gs_track_fit_schedule at the head of an iteration: reads the device counter `it` [1] int32, writes this iteration's six term
    weights into `weights` [6], lr0_r 0.1^(it / num_iters) into the `lr` of the four records of `group`'s DEVICE table (handles in the
    order rots, transls, motion_coefs, means) and into `lrs[it]` ([num_iters,4], optional), and stores it + 1.  The handles' own
    `param_groups[...]["lr"]` are not touched: whatever makes `AdamGroup.sync()` upload its table again (a new gradient tensor, a
    host-side lr change) replaces the scheduled rates by the handles' - keep the `.grad` tensors in place between iterations."""
    if len(group.handles) != 4:
        raise ValueError("track_fit_schedule: an AdamGroup of four handles (rots, transls, motion_coefs, means)")
    table = group.device_table()  # (sync(): outside a capture it creates the state and uploads the table the kernel writes into)
    if table is None or table.numel() != 4 * ctypes.sizeof(L.AdamRec):
        raise RuntimeError("track_fit_schedule: every handle needs a gradient tensor (AdamGroup builds its table from them)")
    check(L.lib().d4gs_track_fit_schedule(vp(it), int(num_iters), vp(table), *[float(x) for x in lr0], vp(weights), vp(lrs),
                                          stream_of(weights)), "d4gs_track_fit_schedule")


class _WarmupLoop:
    """The state of `run_initial_optim` - parameters with their gradient buffers, the AdamGroup, the prepared observations, the
    workspace, the device counter, the weights and the two histories - and `one()`, the launches of one iteration."""

    def __init__(self, fg, bases, tracks_3d, Ks, w2cs, num_iters: int, quantile: float = 0.95):
        from .optim import AdamGroup

        self.params = [bases.params["rots"], bases.params["transls"], fg.params["motion_coefs"], fg.params["means"]]
        rots, transls, coefs, means = self.params
        for p in self.params:
            need_gpu(p, WHO, " (no CPU fallback)")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("run_initial_optim updates contiguous float32 parameters in place")
        self.G, self.K, self.T = G, K, T = means.shape[0], rots.shape[0], rots.shape[1]
        self.targets = track_fit_targets(tracks_3d, Ks, w2cs)
        if (self.targets.G, self.targets.T) != (G, T) or tuple(coefs.shape) != (G, K) or tuple(transls.shape) != (K, T, 3):
            raise ValueError(f"tracks of G = {self.targets.G}, T = {self.targets.T} for means {tuple(means.shape)}, motion_coefs "
                             f"{tuple(coefs.shape)}, rots {tuple(rots.shape)}, transls {tuple(transls.shape)}")
        self.lib, dev = L.lib(), means.device
        self.nbytes = self.lib.d4gs_track_fit_workspace_bytes(G, K, T)
        if self.nbytes == 0:
            raise RuntimeError(f"run_initial_optim: unsupported size G={G} K={K} T={T} (K <= 32, 9 G T <= 2^31 - 1)")
        self.num_iters, self.quantile = int(num_iters), float(quantile)
        self.ws = torch.empty(self.nbytes, device=dev, dtype=torch.uint8)
        self.out = torch.zeros(8, device=dev, dtype=torch.float32)
        self.weights = torch.zeros(6, device=dev, dtype=torch.float32)
        self.it = torch.zeros(1, device=dev, dtype=torch.int32)
        self.losses = torch.zeros(self.num_iters, 7, device=dev, dtype=torch.float32)
        self.lrs = torch.zeros(self.num_iters, 4, device=dev, dtype=torch.float32)
        for p in self.params:
            p.grad = torch.zeros_like(p)  # the backward writes here, the table points here: the same buffers at every iteration
        self.group = AdamGroup()
        self.handles = [self.group.adam(p, lr) for p, lr in zip(self.params, FIT_LR0)]
        self.grads = L.fill(L.LeafGrads(), v_means=means.grad, v_motion_coefs=coefs.grad, v_rots=rots.grad, v_transls=transls.grad)
        self.leaf_ptrs = [vp(means), vp(coefs), vp(rots), vp(transls)]

    def one(self):
        G, K, T, q, t, lib = self.G, self.K, self.T, self.quantile, self.targets, self.lib
        stream = stream_of(self.ws)
        track_fit_schedule(self.group, self.it, self.num_iters, self.weights, self.lrs)
        check(lib.d4gs_track_fit_fwd(*self.leaf_ptrs, G, K, T, q, vp(self.weights), vp(t.buf), t.nbytes, vp(self.ws), self.nbytes,
                                     vp(self.out), vp(self.it), vp(self.losses), self.num_iters, stream), "d4gs_track_fit_fwd")
        # the cotangents of the six terms ARE the weights: d total / d term_k
        check(lib.d4gs_track_fit_bwd(*self.leaf_ptrs, G, K, T, q, vp(t.buf), t.nbytes, vp(self.ws), self.nbytes, vp(self.weights),
                                     L.C.byref(self.grads), stream), "d4gs_track_fit_bwd")
        self.group.step()

    def capture(self):
        """one() in a HIP graph (after one eager one(), which creates the Adam state) -> the graph"""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            self.one()
        return g


def run_initial_optim(fg, bases, tracks_3d: TrackObservations, Ks, w2cs, num_iters: int = 1000, use_depth_range_loss: bool = False, *,
                      graph: bool = True) -> dict:
    """init_utils.py:273-402 with the reference's signature: `num_iters` Adam iterations (torch's defaults; lr 1e-2 rots, 3e-2 transls,
    1e-2 motion_coefs, 1e-3 means, each decayed by 0.1^(i / num_iters)) on
        track_3d + 0.5 track_2d + 0.01 coef_sparse + w(i) smooth_bases + 0.5 w(i) smooth_tracks + 0.1 z_accel
    (`losses.track_fit_losses`; w(i) = 0.01 up to i = 400, then linear to 0.1 at num_iters), updating `fg.params["means" |
    "motion_coefs"]` and `bases.params["rots" | "transls"]` IN PLACE.

    One iteration = schedule step, forward, backward, `AdamGroup.step()`, with the schedule, Adam's state and the iteration count in
    device memory.  The first iteration runs eagerly (it creates the Adam state); graph=True then captures one iteration in a HIP graph
    and replays it num_iters - 1 times - the host does nothing per iteration but launch.  graph=False launches the same kernels
    eagerly and gives the same bits.  There is no CPU fallback.

    -> dict(losses [num_iters,7]: the weighted total and the six terms of every iteration, lrs [num_iters,4]), device tensors written
    without a host wait.  The reference returns None (it prints the terms to a progress bar).  The parameters' `.grad` are left
    holding the last iteration's gradients.  use_depth_range_loss=True raises NotImplementedError: no caller of the reference sets it."""
    if use_depth_range_loss:
        raise NotImplementedError("run_initial_optim: the depth-range term is not provided (no caller of the reference sets it)")
    num_iters = int(num_iters)
    if num_iters < 1:
        raise ValueError(f"num_iters={num_iters}: at least one iteration")
    loop = _WarmupLoop(fg, bases, tracks_3d, Ks, w2cs, num_iters)
    with torch.no_grad():
        loop.one()
        if graph and num_iters > 1:
            g = loop.capture()
            for _ in range(num_iters - 1):
                g.replay()
        else:
            for _ in range(num_iters - 1):
                loop.one()
    last = 0.1 ** ((num_iters - 1) / num_iters)
    for h, lr0 in zip(loop.handles, FIT_LR0):
        h.param_groups[0]["lr"] = lr0 * last  # the rate of the last update (lrs[-1]): what the device table holds
    return dict(losses=loop.losses, lrs=loop.lrs)
