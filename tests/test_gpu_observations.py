"""The observations stage on the GPU (csrc/observations.hip through deblur4dgs_amd.observations) against tests/golden/observations.npz,
which tests/golden/gen_observations.py records from the reference's own functions, and against tests/observations_ref.py, this
repository's NumPy / float64 statement of the same rules (tests/test_observations_ref.py holds that statement to the fixture).

Inputs are fp32 and every statement sees the same numbers.  The bounds:
  median      bit for bit: the output is one of the inputs, or lo / hi.  The kernel works on 16 x 16 pixel tiles with a (k - 1) / 2
              halo and scans parities in chunks of 1024 pixels, so the sizes are: 7 x 9 (smaller than the window and the tile),
              13 x 17 (one past a tile edge in x), 16 x 16 (exactly one tile), 17 x 33 (one past a tile edge both ways), 40 x 50
              (nine tiles, two chunks: the chunk carry is used), and 3 x 13 x 17 (the chain crosses images inside one chunk's range)
  lifting     every flag, in_mask, visible_count, the histogram and the kept set EQUAL (the fixture's samples stay 1e-3 away from
              every decision's edge); xyz, colors, confidences within 1e-4 max|ref| of the fp64 fixture (the project's standing bound)
  background  points and normals within 1e-4 max|ref|; border normals exactly zero; the compacted rows equal boolean indexing
The errors achieved are in profiles/observations_parity.md."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import observations_ref as R
from deblur4dgs_amd import observations as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIAN = ("small", "odd", "tile", "past", "all", "none", "p30", "p70", "half", "batch", "k3", "k5", "k15", "negative")
LIFT = ("n1", "n63", "n64", "n65", "n1000", "integers", "quantile")
SIZES = ((7, 9), (13, 17), (16, 16), (17, 33), (40, 50))
MASKS = ("all", "none", "p30", "p70", "half")
TOL = 1e-4


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "observations.npz"))
    return {k: z[k] for k in z.files}


def case(prefix):
    return {k[len(prefix) + 1:]: v for k, v in golden().items() if k.startswith(prefix + "/")}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def same_bits(t, a):
    return np.array_equal(t.detach().cpu().numpy().view(np.uint32), np.ascontiguousarray(a, np.float32).view(np.uint32))


def err(got, ref):
    """max |got - ref| / max |ref|"""
    ref = np.asarray(ref, np.float64)
    e = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-30)
    print(f"relative error {e:.3e}")
    return e


def make_mask(kind, n, H, W, r):
    if kind == "all":
        return np.ones((n, H, W), np.float32)
    if kind == "none":
        return np.zeros((n, H, W), np.float32)
    if kind == "half":
        return np.broadcast_to((np.arange(W) >= W // 2).astype(np.float32), (n, H, W)).copy()
    return (r.uniform(size=(n, H, W)) < {"p30": 0.3, "p70": 0.7}[kind]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------- median

@pytest.mark.parametrize("name", MEDIAN)
def test_median_equals_the_fixture_bit_for_bit(name):
    c = case(f"median/{name}")
    image, mask = dev(c["image"])[None], dev(c["mask"])[None]
    before = image.clone()
    out = O.masked_median_blur(image, mask, int(c["k"]))
    assert out.shape == image.shape and out.dtype == torch.float32 and same_bits(out[0], c["out"])
    assert torch.equal(image, before)  # the input is unchanged
    assert torch.equal(out, O.masked_median_blur(image, mask, int(c["k"])))  # and a second call gives the same bits


@pytest.mark.parametrize("H,W", SIZES)
def test_median_equals_the_statement_for_every_mask_and_window(H, W):
    r = np.random.default_rng(H * 100 + W)
    for n, kind, k in [(1, kind, 11) for kind in MASKS] + [(3, "p70", 11), (3, "none", 5)] + [(1, "p30", k) for k in (3, 5, 15)]:
        image = r.normal(1.0, 2.0, (n, H, W)).astype(np.float32)  # negative values present
        image[:, ::3, ::4] = image[:, :1, :1]                       # and ties
        mask = make_mask(kind, n, H, W, r)
        mask[:, H // 2, W // 3] = 0.5  # not 1: invalid
        out = O.masked_median_blur(dev(image)[None], dev(mask)[None], k)[0]
        assert same_bits(out, R.masked_median_blur(image, mask, k)), (n, kind, k)


def test_median_blend_and_filter_depths_frame_by_frame():
    r = np.random.default_rng(5)
    T, H, W = 3, 33, 41
    depths = r.uniform(0.0, 5.0, (T, H, W)).astype(np.float32)
    depths[1] *= 3.0   # the clamp at 2.5 x the median of the maxima cuts this frame
    depths[:, ::7, ::5] = 0.0  # depth 0: invalid
    masks = (r.uniform(size=(T, H, W)) < 0.4).astype(np.float32)
    valid = (r.uniform(size=(T, H, W)) < 0.9).astype(np.float32)
    d, m, v = dev(depths), dev(masks), dev(valid)
    out = O.filter_depths(d, m, v, 5)
    top = np.float32(np.median(depths.reshape(T, -1).max(1)) * np.float32(2.5))
    clamped = np.clip(depths, np.float32(0), top)
    assert clamped.max() < depths.max()
    ref = R.blend(R.masked_median_blur(clamped, masks * valid * (clamped > 0), 5, per_image=True), clamped, masks)
    assert same_bits(out, ref)
    o = out.cpu().numpy()
    assert np.array_equal(o[masks == 0], clamped[masks == 0]) and not np.array_equal(o, clamped)
    # three frames in one call = three calls of one frame (on the clamped depths: a frame alone is not clamped again)
    c = dev(clamped)
    for t in range(T):
        assert torch.equal(O.filter_depths(c[t:t + 1], m[t:t + 1], v[t:t + 1], 5)[0], out[t]), t


# --------------------------------------------------------------------------------------------------------------------- lifting

@pytest.mark.parametrize("name", LIFT)
def test_lifting_equals_the_fixture(name):
    c = case(f"lift/{name}")
    q, (N, T, _) = int(c["query"]), c["tracks_2d"].shape
    args = (q, dev(c["img"]), dev(c["tracks_2d"]), dev(c["depths"]), dev(c["masks"]), dev(c["inv_Ks"]), dev(c["c2ws"]))
    got = O.lift_tracks(*args)
    for k in ("visibles", "invisibles", "in_mask"):
        assert np.array_equal(got[k].cpu().numpy(), c[k]), k
    count = c["visibles"].sum(1)
    assert np.array_equal(got["visible_count"].cpu().numpy(), count)
    assert np.array_equal(got["hist"].cpu().numpy(), np.bincount(count, minlength=T + 1))
    for k in ("xyz", "colors", "confidences"):
        assert err(got[k], c[k]) <= TOL, k
    xyz, colors, vis, invis, conf = O.tracks_3d_for_query_frame(*args)
    valid = torch.from_numpy(c["valid"]).to(DEV)
    assert xyz.shape == (int(c["valid"].sum()), T, 3)
    assert torch.equal(xyz, got["xyz"][valid]) and torch.equal(colors, got["colors"][valid]) and torch.equal(vis, got["visibles"][valid])
    assert torch.equal(invis, got["invisibles"][valid]) and torch.equal(conf, got["confidences"][valid])


def test_tapir_flags_and_tracks_3d_over_query_frames():
    c = case("tapir")
    visible, invisible, conf = O.parse_tapir_track_info(dev(c["occ"]), dev(c["dist"]))
    assert np.array_equal(visible.cpu().numpy(), c["visible"]) and np.array_equal(invisible.cpu().numpy(), c["invisible"])
    assert err(conf, c["confidence"]) <= TOL
    c = case("lift/quantile")
    T = c["tracks_2d"].shape[1]
    Ks, w2cs = dev(c["Ks"]), dev(c["w2cs"])
    imgs = dev(c["img"])[None].repeat(T, 1, 1, 1)
    halves = [dev(c["tracks_2d"][:120]), dev(c["tracks_2d"][120:])]
    obs = O.tracks_3d(halves, [int(c["query"]), 7], imgs, dev(c["depths"]), dev(c["masks"]), Ks, w2cs, num_dyn_frames=T)
    assert obs.check_sizes()
    kept = []
    for lo, hi in ((0, 120), (120, 200)):  # the rule without the query-frame mask term, per query frame
        count = c["visibles"][lo:hi].sum(1)
        kept.append(np.flatnonzero(count >= R.quantile_threshold(count, T)) + lo)
    kept = np.concatenate(kept)
    assert 0 < len(kept) < 200 and obs.xyz.shape[0] == len(kept)
    assert np.array_equal(obs.visibles.cpu().numpy(), c["visibles"][kept]) and err(obs.xyz, c["xyz"][kept]) <= TOL
    assert err(obs.confidences, c["confidences"][kept]) <= TOL


# ------------------------------------------------------------------------------------------------------------ background points

@pytest.mark.parametrize("name", ("flat", "rough"))
def test_points_and_normals_equal_the_fixture(name):
    c = case(f"normals/{name}")
    H, W = c["depth"].shape
    inv_K, c2w = np.linalg.inv(c["K"].astype(np.float64)), np.linalg.inv(c["w2c"].astype(np.float64))
    zeros, ones = torch.zeros(1, H, W, device=DEV), torch.ones(1, H, W, device=DEV)
    pts, normals, keep = O.bkgd_points_dense(dev(c["depth"])[None], zeros, ones, dev(inv_K)[None], dev(c2w)[None])
    assert err(pts[0], c["points"]) <= TOL and err(normals[0], c["normals"]) <= TOL and bool(keep.all())
    border = torch.ones(H, W, dtype=torch.bool, device=DEV)
    border[1:-1, 1:-1] = False
    assert not normals[0][border].any()  # exact zeros
    if name == "flat":  # a fronto-parallel plane: right - left is the camera's +x, top - bottom its -y, so the normal is its -z in world axes
        n = -c2w[:3, 2]
        assert np.abs(normals[0][~border].cpu().numpy() - n).max() <= TOL


def test_bkgd_points_compaction_order_share_and_seed():
    r = np.random.default_rng(9)
    T, H, W = 3, 19, 23
    depths = r.uniform(0.5, 3.0, (T, H, W)).astype(np.float32)
    depths[:, ::4, ::3] = 0.0
    masks = (r.uniform(size=(T, H, W)) < 0.3).astype(np.float32)
    valid = (r.uniform(size=(T, H, W)) < 0.9).astype(np.float32)
    imgs = r.uniform(size=(T, H, W, 3)).astype(np.float32)
    c = case("normals/rough")
    Ks, w2cs = dev(c["K"])[None].repeat(T, 1, 1), dev(c["w2c"])[None].repeat(T, 1, 1)
    w2cs[1, 0, 3] += 0.5
    d, m, v, im = dev(depths), dev(masks), dev(valid), dev(imgs)
    inv_Ks, c2ws = torch.linalg.inv(Ks), torch.linalg.inv(w2cs)
    pts, normals, keep = O.bkgd_points_dense(d, m, v, inv_Ks, c2ws)
    for t in range(T):
        p64, n64, k64 = R.bkgd_dense(depths[t], masks[t], valid[t], inv_Ks[t].cpu().numpy(), c2ws[t].cpu().numpy())
        assert np.array_equal(keep[t].cpu().numpy(), k64) and err(pts[t], p64) <= TOL and err(normals[t], n64) <= TOL
    kept = [int(keep[t].sum()) for t in range(T)]
    assert all(0 < k < H * W for k in kept)
    # more samples than there are points: everything, in the order of boolean indexing
    obs = O.bkgd_points(im, d, m, v, Ks, w2cs, 10 ** 6)
    assert obs.check_sizes() and obs.xyz.shape[0] == sum(kept)
    assert torch.equal(obs.xyz, torch.cat([pts[t][keep[t]] for t in range(T)])) and torch.equal(obs.normals, torch.cat([normals[t][keep[t]] for t in range(T)]))
    assert torch.equal(obs.colors, torch.cat([im[t][keep[t]] for t in range(T)]))
    # fewer: floor(100 / 3) per frame, the last takes the remainder; rows of the frame, no row twice; the seed decides
    a = O.bkgd_points(im, d, m, v, Ks, w2cs, 100, generator=torch.Generator().manual_seed(3))
    b = O.bkgd_points(im, d, m, v, Ks, w2cs, 100, generator=torch.Generator().manual_seed(3))
    other = O.bkgd_points(im, d, m, v, Ks, w2cs, 100, generator=torch.Generator().manual_seed(4))
    assert a.xyz.shape == (100, 3) and torch.equal(a.xyz, b.xyz) and torch.equal(a.colors, b.colors) and not torch.equal(a.xyz, other.xyz)
    for t, (lo, hi) in enumerate(((0, 33), (33, 66), (66, 100))):
        rows = {tuple(x) for x in pts[t][keep[t]].cpu().numpy().tolist()}
        mine = [tuple(x) for x in a.xyz[lo:hi].cpu().numpy().tolist()]
        assert set(mine) <= rows and len(set(mine)) == len(mine), t


def test_the_example_runs_from_2d_inputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "init_scene.py"), "--from-2d", "--tracks", "300", "--frames", "6",
                          "--bases", "2", "--points", "500"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "from 2-D" in out.stdout and "render" in out.stdout
