"""Fixture of the observations stage (deblur4dgs_amd/observations.py): small synthetic inputs, and what the REFERENCE's own functions
give for them on the CPU.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_observations.py   ->  tests/golden/observations.npz

Executed from the reference: flow3d/data/utils.py, loaded from its path (it needs torch and numpy only) - `masked_median_blur` in
fp32 (its output is one of its inputs, so the comparison is bitwise), `parse_tapir_track_info`, `get_tracks_3d_for_query_frame`,
`depth2point_world` and `normal_from_depth_image` in float64 with torch's default dtype set to float64 while they run.  The reference
returns the lifted tracks already filtered; so that every sample is held to it, its intermediate tensors are recorded as it computes
them (`F.grid_sample`, `torch.einsum` and its own `parse_tapir_track_info` are wrapped by recorders while it runs), and the kept
set stated here is asserted to reproduce what it returned.  Only data travels: the arrays below.

Every input is rounded to fp32 before use, so the GPU sees the same numbers.  A sample for which a discrete decision of the reference
sits at its edge is drawn again (the number of draws replaced is stored per case as `redrawn`): `vis * conf` or `(1 - vis) * conf`
within 1e-3 of 0.5; a coordinate within 1e-3 of an integer (except where the case places exact integers); the reference's
`grid_sample(mask) == 1` disagreeing with the corner rule of DESIGN.md section 26.  A case in which a visible count equals the
validity threshold while the quantile is interpolated within 1e-6 of an integer is refused (change its seed).  The depth images of
the normals are (2^a + 1) x (2^b + 1) pixels: the reference divides the pixel grid by (W - 1, H - 1) in fp32 whatever the dtype of
the depth, which is exact for those sizes.  The archive is written with fixed zip timestamps: the same generator gives the same bytes."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import observations_ref as R  # noqa: E402
from gen_motion_regs import write_npz  # noqa: E402

#               name        B*C  H   W   k   mask      seed
MEDIAN_CASES = (("small", 1, 7, 9, 11, "p70", 1),       # the image is smaller than the window
                ("odd", 1, 13, 17, 11, "p30", 2),
                ("tile", 1, 16, 16, 11, "half", 3),     # exactly one 16 x 16 tile
                ("past", 1, 17, 33, 11, "p70", 4),      # one past a tile edge both ways
                ("all", 1, 40, 50, 11, "all", 5),
                ("none", 1, 40, 50, 11, "none", 6),     # every output is lo or hi: the parity chain alone decides
                ("p30", 1, 40, 50, 11, "p30", 7),
                ("p70", 1, 40, 50, 11, "p70", 8),
                ("half", 1, 40, 50, 11, "half", 9),
                ("batch", 3, 13, 17, 11, "p70", 10),    # the parity carries across images
                ("k3", 1, 17, 33, 3, "p70", 11),
                ("k5", 1, 17, 33, 5, "p30", 12),
                ("k15", 1, 17, 33, 15, "p70", 13),
                ("negative", 2, 17, 33, 5, "p70", 14))  # values of both signs: lo < 0 < hi
#             name       N    T   H   W  query  seed
LIFT_CASES = (("n1", 1, 1, 24, 32, 0, 28),
              ("n63", 63, 2, 24, 32, 1, 22),
              ("n64", 64, 6, 24, 32, 3, 23),
              ("n65", 65, 6, 24, 32, 0, 24),
              ("n1000", 1000, 6, 24, 32, 2, 25),   # tracks outside the image on every side; frame 4 has an empty mask
              ("integers", 65, 2, 24, 32, 0, 26),  # exact integer coordinates at the query frame, on a mask with holes
              ("quantile", 200, 40, 12, 16, 5, 27))  # int(0.05 T) = 2: the visible-count rule drops tracks
NORMAL_CASES = (("flat", 9, 17, 31), ("rough", 17, 9, 32))


def f32(a):
    return np.asarray(a, np.float32)


def load_utils():
    spec = importlib.util.spec_from_file_location("reference_data_utils", os.path.join(os.environ["D4GS_REFERENCE"], "flow3d", "data", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_mask(kind, n, H, W, r):
    if kind == "all":
        return np.ones((n, H, W), np.uint8)
    if kind == "none":
        return np.zeros((n, H, W), np.uint8)
    if kind == "half":
        return np.broadcast_to((np.arange(W) >= W // 2).astype(np.uint8), (n, H, W)).copy()
    return (r.uniform(size=(n, H, W)) < {"p30": 0.3, "p70": 0.7}[kind]).astype(np.uint8)


def median_inputs(name, n, H, W, k, kind, seed):
    r = np.random.default_rng(seed)
    image = f32(r.uniform(0.5, 4.0, (n, H, W)))
    if name == "negative":
        image = f32(r.normal(size=(n, H, W)))
    image[:, ::5, ::3] = image[:, 0:1, 0:1]  # ties
    return image, make_mask(kind, n, H, W, r)


def cameras(T, r):
    """K with a principal point off the centre, w2c a rotation and translation per frame"""
    Ks, w2cs = np.zeros((T, 3, 3)), np.zeros((T, 4, 4))
    for t in range(T):
        Ks[t] = [[30.0 + t, 0.3, 15.5 + 0.2 * t], [0.0, 28.0 - 0.5 * t, 11.0], [0.0, 0.0, 1.0]]
        axis = r.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = 0.3 + 0.1 * t
        X = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        w2cs[t, :3, :3] = np.eye(3) + np.sin(a) * X + (1 - np.cos(a)) * X @ X
        w2cs[t, :3, 3] = r.normal(size=3)
        w2cs[t, 3, 3] = 1.0
    return f32(Ks), f32(w2cs)


def draw_tracks(name, N, T, H, W, query, r, n=None):
    """[n,T,4] fresh samples"""
    n = N if n is None else n
    x, y = r.uniform(0, W - 1, (n, T)), r.uniform(0, H - 1, (n, T))
    if name == "n1000":  # a fifth of the samples lie outside, on every side
        out = r.uniform(size=(n, T)) < 0.2
        side = r.integers(0, 4, (n, T))
        x = np.where(out & (side == 0), r.uniform(-6, -0.1, (n, T)), np.where(out & (side == 1), r.uniform(W - 0.9, W + 6, (n, T)), x))
        y = np.where(out & (side == 2), r.uniform(-6, -0.1, (n, T)), np.where(out & (side == 3), r.uniform(H - 0.9, H + 6, (n, T)), y))
    if name == "integers":
        x[:, query], y[:, query] = r.integers(0, W, n), r.integers(0, H, n)
    shift = 1.5 if name == "quantile" else -1.0  # "quantile": most samples occluded
    occ, dist = r.normal(shift, 2.5, (n, T)), r.normal(-1.5, 2.0, (n, T))
    return f32(np.stack([x, y, occ, dist], -1))


def lift_inputs(name, N, T, H, W, query, seed):
    r = np.random.default_rng(seed)
    gy, gx = np.mgrid[0:H, 0:W]
    depths = f32(2.0 + 0.05 * gx + 0.03 * gy + r.uniform(0, 0.5, (T, H, W)))
    masks = (r.uniform(size=(T, H, W)) < 0.1).astype(np.uint8)  # holes ...
    masks = 1 - masks                                            # ... in a full mask
    masks[:, :, :3] = 0
    if name == "n1000":
        masks[4] = 0
    Ks, w2cs = cameras(T, r)
    return dict(depths=depths, masks=masks, img=f32(r.uniform(0, 1, (H, W, 3))), Ks=Ks, w2cs=w2cs), r


class Recorder:
    """wraps a callable and keeps what it returned, call by call"""

    def __init__(self, fn):
        self.fn, self.out = fn, []

    def __call__(self, *a, **k):
        out = self.fn(*a, **k)
        self.out.append(out)
        return out


def run_lift(utils, c, tracks, query):
    """the reference on float64 copies of the fp32 inputs -> (its five returned tensors, its unfiltered intermediates)"""
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    inv_Ks, c2ws = torch.linalg.inv(t64(c["Ks"])), torch.linalg.inv(t64(c["w2cs"]))
    gs, es, parse = Recorder(F.grid_sample), Recorder(torch.einsum), Recorder(utils.parse_tapir_track_info)
    torch.set_default_dtype(torch.float64)
    F.grid_sample, torch.einsum, utils.parse_tapir_track_info = gs, es, parse
    try:
        with torch.no_grad():
            out = utils.get_tracks_3d_for_query_frame(query, t64(c["img"]), t64(tracks), t64(c["depths"]), t64(c["masks"]), inv_Ks, c2ws)
    finally:
        F.grid_sample, torch.einsum, utils.parse_tapir_track_info = gs.fn, es.fn, parse.fn
        torch.set_default_dtype(torch.float32)
    assert len(gs.out) == 3 and len(es.out) == 2 and len(parse.out) == 1
    vis, invis, conf = parse.out[0]  # [T,N], after the reference multiplied them by its mask test in place
    full = dict(xyz=es.out[1][..., :3].swapdims(0, 1), in_ref=(gs.out[1][:, 0, 0] == 1).swapdims(0, 1), visibles=vis.swapdims(0, 1),
                invisibles=invis.swapdims(0, 1), confidences=conf.swapdims(0, 1), colors=gs.out[2][0, :, 0].T)
    return out, {k: v.numpy() for k, v in full.items()}, (inv_Ks.numpy(), c2ws.numpy())


def edge_samples(name, tracks, query, masks, in_ref):
    """[N,T] bool: the samples to draw again"""
    tr = tracks.astype(np.float64)
    vis, conf = 1 - 1 / (1 + np.exp(-tr[..., 2])), 1 - 1 / (1 + np.exp(-tr[..., 3]))
    bad = (np.abs(vis * conf - 0.5) < 1e-3) | (np.abs((1 - vis) * conf - 0.5) < 1e-3)
    near = (np.abs(tr[..., 0] - np.round(tr[..., 0])) < 1e-3) | (np.abs(tr[..., 1] - np.round(tr[..., 1])) < 1e-3)
    if name == "integers":
        near[:, query] = False
    T = tr.shape[1]
    mine = np.stack([R.corners_in_mask(masks[t], tr[:, t, 0], tr[:, t, 1]) for t in range(T)], 1)
    return bad | near | (mine != in_ref)


if __name__ == "__main__":
    utils = load_utils()
    arrays = {}
    for name, n, H, W, k, kind, seed in MEDIAN_CASES:
        image, mask = median_inputs(name, n, H, W, k, kind, seed)
        with torch.no_grad():
            out = utils.masked_median_blur(torch.from_numpy(image)[None], torch.from_numpy(mask.astype(np.float32))[None], k)[0].numpy()
        assert out.dtype == np.float32 and out.shape == image.shape
        arrays.update({f"median/{name}/image": image, f"median/{name}/mask": mask, f"median/{name}/k": np.int32(k), f"median/{name}/out": out})
        print("median", name, f"{n} x {H} x {W}, k = {k}, valid {mask.mean():.2f}", file=sys.stderr)

    r = np.random.default_rng(40)
    occ, dist = f32(r.normal(0, 3, (50, 7))), f32(r.normal(-1, 3, (50, 7)))
    for _ in range(50):
        v, c = 1 - 1 / (1 + np.exp(-occ.astype(np.float64))), 1 - 1 / (1 + np.exp(-dist.astype(np.float64)))
        bad = (np.abs(v * c - 0.5) < 1e-3) | (np.abs((1 - v) * c - 0.5) < 1e-3)
        if not bad.any():
            break
        occ[bad], dist[bad] = f32(r.normal(0, 3, int(bad.sum()))), f32(r.normal(-1, 3, int(bad.sum())))
    with torch.no_grad():
        pv, pi, pc = utils.parse_tapir_track_info(torch.from_numpy(occ.astype(np.float64)), torch.from_numpy(dist.astype(np.float64)))
    arrays.update({"tapir/occ": occ, "tapir/dist": dist, "tapir/visible": pv.numpy(), "tapir/invisible": pi.numpy(), "tapir/confidence": pc.numpy()})

    for name, N, T, H, W, query, seed in LIFT_CASES:
        c, r = lift_inputs(name, N, T, H, W, query, seed)
        tracks = draw_tracks(name, N, T, H, W, query, r)
        redrawn = 0
        for attempt in range(100):
            out, full, (inv_Ks, c2ws) = run_lift(utils, c, tracks, query)
            bad = edge_samples(name, tracks, query, c["masks"], full["in_ref"])
            if not bad.any():
                break
            redrawn += int(bad.sum())
            fresh = draw_tracks(name, N, T, H, W, query, r)
            tracks[bad] = fresh[bad]
        else:
            raise SystemExit(f"{name}: samples stay at an edge")
        assert redrawn <= 0.1 * N * T, (name, redrawn)
        count = full["visibles"].sum(1)
        q = float(torch.from_numpy(count).float().quantile(0.1))
        th = min(int(0.05 * T), q)
        ranked, pos = np.sort(count), 0.1 * (N - 1)
        interpolated = ranked[int(np.floor(pos))] != ranked[int(np.ceil(pos))]
        assert not (interpolated and abs(q - round(q)) < 1e-6 and (count == round(q)).any()), f"{name}: the threshold sits at an edge"
        valid = full["in_ref"][:, query] & (count >= th)
        for got, key in zip(out, ("xyz", "colors", "visibles", "invisibles", "confidences")):  # the kept set is the reference's
            assert got.shape[0] == valid.sum() and np.array_equal(got.numpy(), full[key][valid]), (name, key)
        ours = R.lift_tracks(query, c["img"], tracks, c["depths"], c["masks"], inv_Ks, c2ws)
        assert np.array_equal(ours["in_mask"], full["in_ref"])
        arrays.update({f"lift/{name}/{k}": v for k, v in c.items()})
        arrays.update({f"lift/{name}/tracks_2d": tracks, f"lift/{name}/query": np.int32(query), f"lift/{name}/inv_Ks": inv_Ks,
                       f"lift/{name}/c2ws": c2ws, f"lift/{name}/xyz": full["xyz"], f"lift/{name}/colors": full["colors"],
                       f"lift/{name}/visibles": full["visibles"], f"lift/{name}/invisibles": full["invisibles"],
                       f"lift/{name}/confidences": full["confidences"], f"lift/{name}/in_mask": full["in_ref"], f"lift/{name}/valid": valid,
                       f"lift/{name}/redrawn": np.int32(redrawn)})
        print("lift", name, f"re-drawn {redrawn} of {N * T} ({100 * redrawn / (N * T):.1f} %), in mask {full['in_ref'].mean():.2f}, "
              f"kept {int(valid.sum())} of {N}, threshold {th}", file=sys.stderr)

    for name, H, W, seed in NORMAL_CASES:
        r = np.random.default_rng(seed)
        gy, gx = np.mgrid[0:H, 0:W]
        depth = f32(3.0 + 0.0 * gx) if name == "flat" else f32(2.0 + 0.1 * gx + 0.05 * gy + r.uniform(0, 0.3, (H, W)))
        Ks, w2cs = cameras(1, r)
        t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        torch.set_default_dtype(torch.float64)
        try:
            with torch.no_grad():
                normals = utils.normal_from_depth_image(t64(depth), t64(Ks[0]), t64(w2cs[0])).numpy()
                points = utils.depth2point_world(t64(depth), t64(Ks[0]), t64(w2cs[0])).numpy().reshape(H, W, 3)
        finally:
            torch.set_default_dtype(torch.float32)
        assert normals.dtype == np.float64 and normals.shape == (H, W, 3)
        arrays.update({f"normals/{name}/depth": depth, f"normals/{name}/K": Ks[0], f"normals/{name}/w2c": w2cs[0],
                       f"normals/{name}/normals": normals, f"normals/{name}/points": points})
    dst = os.path.join(HERE, "observations.npz")
    write_npz(dst, arrays)
    print(f"{len(arrays)} arrays -> {dst} ({os.path.getsize(dst)} bytes)", file=sys.stderr)
