"""Fixture of the scene initialisation (deblur4dgs_amd/scene_init.py): small synthetic tracks, and what the REFERENCE's own functions
give for them in float64 on the CPU.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_scene_init.py   ->  tests/golden/scene_init.npz

Executed from the reference: `batched_interp_masked` (flow3d/init_utils.py, with numpy standing in for the module it calls `cp`), `knn`
(flow3d/loss_utils.py, through the sklearn installed here), and `init_motion_params_with_procrustes`, which calls the reference's
`get_weights_for_procrustes` and `solve_procrustes` (6d, enforce_se3) for every pair.  Its `sample_initial_bases_centers` is replaced
in its namespace by a function that returns the fixture's stored labels and their per-label medians (cuML is not installed, and its
labels are no contract).  The imports of the reference that are not installed where the generator runs are stubbed as
gen_golden._import_reference does; torch's default dtype is float64 while the reference runs, so that the tensors it creates itself
are float64 too.  The velocity directions and the synthetic tracks are this file's own words.  Only data travels: the arrays below.

Every input is rounded to fp32 before use, so the GPU sees the same numbers.  So that fp32 cannot be ill-conditioned where the
reference is not, a case's seed is advanced until (1) every solved pair has singular values s2 + s3 >= 0.1 s1, (2) no normalised
distance of get_weights_for_procrustes lies within 1e-3 (relative) of its cluster's 0.9 quantile, (3) every weight sum is at least
5 % away from the skip threshold min_mean_weight * T, and (4) no track lies within 1e-3 (relative) of the outlier radius.  The
archive is written with fixed zip timestamps: the same generator gives the same bytes."""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
from gen_motion_regs import write_npz  # noqa: E402
from gen_trimmed_losses import load_reference  # noqa: E402

MIN_MEAN_WEIGHT = 0.1
#        name             G    T   K  cano_t  seed
CASES = (("default_small", 333, 12, 5, 5, 100),
         ("edge_cano", 65, 8, 3, 0, 200),   # the descending half of the visiting order is empty
         ("skips", 130, 6, 4, 2, 300))      # cluster 1 is invisible at frame 4: that pair copies its predecessor


def import_reference():
    """-> (flow3d.init_utils, TrackObservations) with the absent imports stubbed"""
    loss_utils = types.ModuleType("flow3d.loss_utils")
    loss_utils.__dict__.update(load_reference())  # the head of flow3d/loss_utils.py (everything before its PWC-Net part)
    gen_golden.REF = os.environ["D4GS_REFERENCE"]
    gen_golden._import_reference()  # roma, pypose, jaxtyping stubs; the reference on sys.path
    sys.modules["flow3d.loss_utils"] = loss_utils
    sys.modules["cupy"] = np
    stubs = {"imageio": {}, "imageio.v3": {}, "cuml": {"HDBSCAN": None, "KMeans": None}, "viser": {"ViserServer": object},
             "loguru": {"logger": types.SimpleNamespace(info=lambda *a, **k: None)}, "flow3d.vis": {},
             "flow3d.vis.utils": {"draw_keypoints_video": None, "get_server": None, "project_2d_tracks": None}}
    for name, attrs in stubs.items():
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    sys.modules["imageio"].v3 = sys.modules["imageio.v3"]
    from flow3d import init_utils
    from flow3d.tensor_dataclass import TrackObservations

    return init_utils, TrackObservations


def _rot(axis, angle):
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def make_inputs(name, G, T, K, cano_t, seed):
    """tracks = a start point per track, carried by its cluster's rigid motion (a rotation about a fixed axis and a random-walk
    translation, the identity at cano_t), plus noise"""
    r = np.random.default_rng(seed)
    labels = r.integers(0, K, G)
    labels[:K] = np.arange(K)
    # three quarters of the start points fill a ball of radius 0.5, the rest thin out to radius 3: the 0.9 quantile of
    # get_weights_for_procrustes then falls where the distances are sparse, and condition (2) can be met at all (with ~800 evenly
    # dense distances per cluster the neighbours of the quantile are ~1e-3 apart and no seed passes)
    direction = r.normal(size=(G, 3))
    direction /= np.linalg.norm(direction, axis=-1, keepdims=True)
    far = r.uniform(size=G) >= 0.75
    radius = np.where(far, r.uniform(0.6, 3.0, G), 0.5 * r.uniform(size=G) ** (1 / 3))
    start = direction * radius[:, None]
    # a far track's radius also breathes by +-25 % from frame to frame: a rigid track has nearly the same normalised distance in all
    # T frames, and the quantile would sit inside such a clump of T values
    breathe = np.where(far[:, None], 1.0 + 0.25 * r.uniform(-1.0, 1.0, (G, T)), 1.0)
    xyz = np.zeros((G, T, 3))
    for k in range(K):
        axis, rate = r.normal(size=3), r.uniform(0.08, 0.2) * r.choice([-1.0, 1.0])
        walk = np.cumsum(r.normal(scale=0.15, size=(T, 3)), 0)
        walk -= walk[cano_t]
        for t in range(T):
            m = labels == k
            xyz[m, t] = (start[m] * breathe[m, t, None]) @ _rot(axis, rate * (t - cano_t)).T + walk[t]
    xyz += r.normal(scale=0.01, size=xyz.shape)
    visibles = r.uniform(size=(G, T)) < 0.85
    visibles[:4] = False  # tracks without a visible frame: the filter drops them
    visibles[4, :] = True
    if name == "skips":
        visibles[labels == 1, 4] = False
    conf = r.uniform(0.5, 1.0, (G, T))
    colors = r.uniform(0.05, 0.95, (G, 3))
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))  # what fp32 holds
    return dict(xyz=f(xyz), visibles=torch.from_numpy(visibles), confidences=f(conf), colors=f(colors), labels=torch.from_numpy(labels))


def outlier_filter(c, cano_t):
    """the valid mask of init_motion_params_with_procrustes and the relative gap of the nearest track to its radius"""
    means = c["xyz"][:, cano_t]
    d = torch.linalg.vector_norm(means - means.median(dim=0).values, dim=-1)
    th = torch.quantile(d, 0.95)
    return (d < th) & c["visibles"].any(dim=1), float(((d - th).abs() / th).min())


def conditions(ref, c, valid, cano_t, T, sigmas):
    """-> (ok, weight sums [K,T], weights [G',T]) on the filtered tracks"""
    xyz, vis, conf, labels = c["xyz"][valid], c["visibles"][valid], c["confidences"][valid], c["labels"][valid]
    ids = labels.unique()
    sums, weights, ok = torch.zeros(len(ids), T, dtype=torch.float64), torch.zeros(xyz.shape[0], T, dtype=torch.float64), True
    for n, i in enumerate(ids):
        m = labels == i
        cl = xyz[m].transpose(0, 1)
        w = ref.get_weights_for_procrustes(cl, vis[m].swapaxes(0, 1))
        weights[m] = w.transpose(0, 1)
        d = torch.linalg.vector_norm(cl - cl.median(dim=-2, keepdim=True)[0], dim=-1)
        d = d / d.median(dim=-1, keepdim=True)[0]
        q = np.quantile(d.numpy(), 0.9)
        ok &= float(((d - q).abs() / q).min()) >= 1e-3
        cf = conf[m].swapaxes(0, 1)
        for t in range(T):
            sums[n, t] = (w[cano_t] * w[t] * (cf[cano_t] + cf[t]) / 2).sum()
    ok &= bool(((sums / (MIN_MEAN_WEIGHT * T) - 1).abs() >= 0.05).all())
    ok &= all(float(s[1] + s[2]) >= 0.1 * float(s[0]) for s in sigmas)
    return ok, sums, weights


def run_reference(init_utils, TrackObservations, c, K, cano_t, valid):
    """init_motion_params_with_procrustes of the reference on the case -> (rots, transls, motion_coefs, filtered xyz, singular values)"""
    tracks = TrackObservations(c["xyz"].clone(), c["visibles"].clone(), ~c["visibles"], c["confidences"].clone(), c["colors"].clone())
    kept = c["labels"][valid]

    def stored_labels(mode, cano, tracks_3d, num_bases):
        assert tracks_3d.xyz.shape[0] == kept.shape[0]
        means = tracks_3d.xyz[:, cano]
        n = int(kept.max()) + 1
        return torch.stack([means[kept == i].median(dim=0).values for i in range(n)])[None], n, kept

    sigmas, svd = [], torch.linalg.svd

    def recording_svd(m):
        out = svd(m)
        sigmas.append(out[1].clone())
        return out

    init_utils.sample_initial_bases_centers = stored_labels
    torch.linalg.svd = recording_svd
    torch.set_default_dtype(torch.float64)
    try:
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            bases, coefs, out = init_utils.init_motion_params_with_procrustes(tracks, K, "6d", cano_t, min_mean_weight=MIN_MEAN_WEIGHT)
    finally:
        torch.linalg.svd = svd
        torch.set_default_dtype(torch.float32)
    return bases.params["rots"].detach(), bases.params["transls"].detach(), coefs, out.xyz, sigmas


if __name__ == "__main__":
    init_utils, TrackObservations = import_reference()
    ref = sys.modules["flow3d.loss_utils"]
    arrays = {}
    for name, G, T, K, cano_t, seed in CASES:
        for attempt in range(200):
            c = make_inputs(name, G, T, K, cano_t, seed + attempt)
            valid, gap = outlier_filter(c, cano_t)
            rots, transls, coefs, kept_xyz, sigmas = run_reference(init_utils, TrackObservations, c, K, cano_t, valid)
            ok, sums, weights = conditions(ref, c, valid, cano_t, T, sigmas)
            if ok and gap >= 1e-3:
                break
        else:
            raise SystemExit(f"{name}: no well-conditioned seed")
        assert torch.equal(kept_xyz, c["xyz"][valid]) and rots.dtype == torch.float64 and rots.shape == (K, T, 6)
        skipped = sums < MIN_MEAN_WEIGHT * T
        assert bool(skipped.any()) == (name == "skips") and len(sigmas) == int((~skipped).sum())
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            interp = init_utils.batched_interp_masked(c["xyz"][valid].numpy(), c["visibles"][valid].numpy())
        rows = [np.stack([np.interp(np.arange(T), np.flatnonzero(v), x[v, k]) for k in range(3)], -1)
                for x, v in zip(c["xyz"][valid].numpy(), c["visibles"][valid].numpy())]
        assert np.array_equal(interp, np.stack(rows))  # the reference's concatenation trick is per-row np.interp, bit for bit
        vel = interp[:, 1:] - interp[:, :-1]
        vel_dirs = (vel / (np.linalg.norm(vel, axis=-1, keepdims=True) + 1e-5)).reshape(len(vel), -1)
        knn_d, _ = ref.knn(c["xyz"][:, cano_t].float(), 3)
        arrays.update({f"{name}/xyz": c["xyz"].numpy().astype(np.float32), f"{name}/visibles": c["visibles"].numpy(),
                       f"{name}/confidences": c["confidences"].numpy().astype(np.float32),
                       f"{name}/colors": c["colors"].numpy().astype(np.float32), f"{name}/labels": c["labels"].numpy().astype(np.int32),
                       f"{name}/cano_t": np.int32(cano_t), f"{name}/valid": valid.numpy(), f"{name}/rots": rots.numpy(),
                       f"{name}/transls": transls.numpy(), f"{name}/motion_coefs": coefs.numpy(), f"{name}/skipped": skipped.numpy(),
                       f"{name}/weight_sums": sums.numpy(), f"{name}/knn3": knn_d})
        if name != "default_small":  # (the largest case would double the archive)
            arrays.update({f"{name}/interp": interp, f"{name}/vel_dirs": vel_dirs, f"{name}/weights": weights.numpy()})
        print(name, f"seed {seed + attempt}", f"kept {int(valid.sum())} of {G}", f"skipped pairs {int(skipped.sum())}", file=sys.stderr)
    dst = os.path.join(HERE, "scene_init.npz")
    write_npz(dst, arrays)
    print(f"{len(arrays)} arrays -> {dst} ({os.path.getsize(dst)} bytes)", file=sys.stderr)
