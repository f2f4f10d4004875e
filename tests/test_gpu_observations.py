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
Past one turn of the single-block loops: k_mm_carry scans 256 chunk parities per turn, so 5 x 230 x 231 (260 chunks over all images)
and 512 x 513 (257 chunks per image, filter_depths) carry a parity into a second turn; k_bkgd_compact walks 1 024 pixels per turn, so
32 x 33 (a second turn of 32 px) and 47 x 45 (three turns) carry its running count; and with N = 1 track of T = 256 or 512 frames
k_lift_samples has exactly T lanes for its T + 1 histogram bins, so the last bin is zeroed in a second turn.
The errors achieved are in profiles/observations_parity.md."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import observations_ref as R
from deblur4dgs_amd import _lib as L
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


MM_CHUNK, MM_NT = 1024, 256  # observations.hip: constexpr int MM_CHUNK = 1024; MM_NT = MM_TILE * MM_TILE = 256 chunk parities per turn


def flip_parity_early(mask):
    """The same mask with one more invalid entry at an interior pixel of image 0, row 1: it lies in k x k windows, an odd number, so the
    parity of the invalid entries before every pixel behind those windows is flipped - what a lost carry does to them."""
    flipped = mask.copy()
    x = int(np.flatnonzero(mask[0, 1, 1:-1] == 1)[0]) + 1
    flipped[0, 1, x] = 0.0
    return flipped


def carry_case(n, H, W, seed):
    r = np.random.default_rng(seed)
    image = r.normal(1.0, 2.0, (n, H, W)).astype(np.float32)
    image[:, ::3, ::4] = image[:, :1, :1]
    mask = make_mask("p70", n, H, W, r)
    mask[:, H // 2, W // 3] = 0.5
    return image, mask


def test_median_carries_the_parity_into_the_second_turn_over_all_images():
    """5 x 230 x 231: 52 chunks per image, 260 in all, so the one block of k_mm_carry scans 256 chunk parities, carries their parity
    and scans 4 more (pixels 49 152.. of the last image)."""
    n, H, W, k = 5, 230, 231, 3
    cpi = -(-H * W // MM_CHUNK)
    assert cpi == 52 and MM_NT < n * cpi <= 2 * MM_NT and (n - 1) * cpi < MM_NT  # the second turn begins inside the last image
    image, mask = carry_case(n, H, W, 230231)
    ref = R.masked_median_blur(image, mask, k)
    tail = slice((MM_NT - (n - 1) * cpi) * MM_CHUNK, None)  # the last image's pixels of chunks 256..259
    lost = R.masked_median_blur(image, flip_parity_early(mask), k)
    differ = int((ref[-1].reshape(-1)[tail] != lost[-1].reshape(-1)[tail]).sum())
    print("pixels behind chunk 256 that a flipped parity changes:", differ, "of", ref[-1].reshape(-1)[tail].size)
    assert differ > 100  # the inputs see the carry
    out = O.masked_median_blur(dev(image)[None], dev(mask)[None], k)[0]
    assert same_bits(out, ref)


def test_filter_depths_carries_the_parity_into_the_second_turn_of_every_image():
    """512 x 513: 257 chunks per image, so every block of the per-image k_mm_carry takes a second turn for the last chunk (512 px)."""
    T, H, W, k = 2, 512, 513, 3
    cpi = -(-H * W // MM_CHUNK)
    assert cpi == MM_NT + 1
    r = np.random.default_rng(512513)
    depths = r.uniform(0.0, 5.0, (T, H, W)).astype(np.float32)
    depths[1] *= 3.0
    depths[:, ::7, ::5] = 0.0
    masks = (r.uniform(size=(T, H, W)) < 0.4).astype(np.float32)
    valid = (r.uniform(size=(T, H, W)) < 0.7).astype(np.float32)
    top = np.sort(depths.reshape(T, -1).max(1))[(T - 1) // 2] * np.float32(2.5)  # torch's median: of two values the lower
    clamped = np.clip(depths, np.float32(0), top)
    assert clamped.max() < depths.max()
    inner = masks * valid * (clamped > 0)
    ref = R.blend(R.masked_median_blur(clamped, inner, k, per_image=True), clamped, masks)
    for t in range(T):  # the inputs see the carry: a flipped parity changes pixels of the last chunk where the blend keeps the median
        lost = R.blend(R.masked_median_blur(clamped[t:t + 1], flip_parity_early(inner[t:t + 1]), k), clamped[t:t + 1], masks[t:t + 1])
        differ = int((ref[t].reshape(-1)[MM_NT * MM_CHUNK:] != lost[0].reshape(-1)[MM_NT * MM_CHUNK:]).sum())
        print("frame", t, "pixels of chunk 256 that a flipped parity changes:", differ)
        assert differ > 10
    d, m, v = dev(depths), dev(masks), dev(valid)
    out = O.filter_depths(d, m, v, k)
    assert same_bits(out, ref)
    c = dev(clamped)
    for t in range(T):  # one frame of 257 chunks alone (on the clamped depths: a frame alone is not clamped again)
        alone = O.filter_depths(c[t:t + 1], m[t:t + 1], v[t:t + 1], k)
        assert torch.equal(alone[0], out[t]) and same_bits(alone[0], ref[t]), t


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


@pytest.mark.parametrize("T", (256, 300, 512))
def test_lifting_zeroes_every_bin_of_a_used_histogram(T):
    """k_lift_samples zeroes the T + 1 bins with `h <= T` strided over its N T lanes.  With N = 1 and T = 256 (one block) or 512 (two)
    the grid has exactly T lanes and bin T is written in a second turn; T = 300 has 512 lanes and one turn.  The wrapper hands in
    torch.zeros, which hides the zeroing, so this calls the library with a histogram full of 7s."""
    lanes = -(-T // 256) * 256  # observations.hip: dim3((total + 255) / 256) blocks of 256, total = N T
    assert (T + 1 > lanes) == (T != 300)
    r = np.random.default_rng(T)
    H, W = 6, 7
    tracks = np.stack([r.uniform(0.5, W - 1.5, (1, T)), r.uniform(0.5, H - 1.5, (1, T)), r.normal(0.0, 3.0, (1, T)), r.normal(-3.0, 1.0, (1, T))],
                      -1).astype(np.float32)
    depths, masks = r.uniform(1.0, 2.0, (T, H, W)).astype(np.float32), np.ones((T, H, W), np.float32)
    eye3, eye4 = np.broadcast_to(np.eye(3, dtype=np.float32), (T, 3, 3)), np.broadcast_to(np.eye(4, dtype=np.float32), (T, 4, 4))
    want = R.lift_tracks(0, np.zeros((H, W, 3)), tracks, depths, masks, eye3, eye4)
    assert 0 < int(want["visible_count"][0]) < T  # a bin in the middle, and bin T must end at zero
    vis, conf = 1 - 1 / (1 + np.exp(-tracks[..., 2].astype(np.float64))), 1 - 1 / (1 + np.exp(-tracks[..., 3].astype(np.float64)))
    assert min(np.abs(vis * conf - 0.5).min(), np.abs((1 - vis) * conf - 0.5).min()) > 1e-4  # no flag at its edge: fp32 decides alike
    tr, d, m, q, ik, cw = dev(tracks), dev(depths), dev(masks), torch.zeros(H, W, 3, device=DEV), dev(eye3), dev(eye4)
    u8 = lambda: torch.empty(1, T, device=DEV, dtype=torch.uint8)
    xyz, conf, colors = torch.empty(1, T, 3, device=DEV), torch.empty(1, T, device=DEV), torch.empty(1, 3, device=DEV)
    vis, invis, in_mask = u8(), u8(), u8()
    count, hist = torch.empty(1, device=DEV, dtype=torch.int32), torch.full((T + 1,), 7, device=DEV, dtype=torch.int32)
    L.check(L.lib().d4gs_lift_tracks(L.vp(tr), L.vp(d), L.vp(m), L.vp(q), L.vp(ik), L.vp(cw), 1, T, H, W, 0, L.vp(xyz), L.vp(vis), L.vp(invis),
                                     L.vp(conf), L.vp(in_mask), L.vp(colors), L.vp(count), L.vp(hist), L.stream_of(tr)), "d4gs_lift_tracks")
    assert np.array_equal(vis.cpu().numpy().astype(bool), want["visibles"]) and int(count[0]) == int(want["visible_count"][0])
    assert np.array_equal(hist.cpu().numpy(), np.bincount(count.cpu().numpy(), minlength=T + 1))
    assert np.array_equal(hist.cpu().numpy(), want["hist"])


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


BK_NT = 1024  # observations.hip: constexpr int BK_NT = 1024, the pixels of one turn of k_bkgd_compact


@pytest.mark.parametrize("H,W,turns,last", ((32, 33, 2, 32), (47, 45, 3, 67)))
def test_bkgd_points_compaction_carries_its_base_from_turn_to_turn(H, W, turns, last):
    """One block per frame walks 1 024 pixels per turn and carries the kept count: 32 x 33 has a second turn of 32 px, 47 x 45 three
    turns.  Two frames with about half of the pixels kept; then one whose kept pixels all lie behind pixel 1 024 and one with none
    behind it.  Everything is taken: the rows equal boolean indexing in row-major order."""
    assert -(-H * W // BK_NT) == turns and H * W - (turns - 1) * BK_NT == last
    r = np.random.default_rng(H * 100 + W)
    T = 2
    c = case("normals/rough")
    Ks, w2cs = dev(c["K"])[None].repeat(T, 1, 1), dev(c["w2c"])[None].repeat(T, 1, 1)
    w2cs[1, 0, 3] += 0.5
    inv_Ks, c2ws = torch.linalg.inv(Ks), torch.linalg.inv(w2cs)
    behind = (np.arange(H * W) >= BK_NT).reshape(H, W)
    random = (r.uniform(size=(T, H, W)) < 0.5).astype(np.float32)
    for name, masks in (("half", random), ("only behind / none behind", np.stack([np.where(behind, random[0], 1.0), np.where(behind, 1.0, random[1])]))):
        depths = r.uniform(0.5, 3.0, (T, H, W)).astype(np.float32)
        valid = np.ones((T, H, W), np.float32)
        imgs = r.uniform(size=(T, H, W, 3)).astype(np.float32)
        d, m, v, im = dev(depths), dev(masks.astype(np.float32)), dev(valid), dev(imgs)
        pts, normals, keep = O.bkgd_points_dense(d, m, v, inv_Ks, c2ws)
        k64 = masks == 0
        assert np.array_equal(keep.cpu().numpy(), k64), name
        if name == "half":
            assert all(0.4 < k64[t].mean() < 0.6 and k64[t].reshape(-1)[BK_NT:].any() for t in range(T))
        else:
            assert k64[0].any() and not k64[0].reshape(-1)[:BK_NT].any() and k64[1].any() and not k64[1].reshape(-1)[BK_NT:].any()
        obs = O.bkgd_points(im, d, m, v, Ks, w2cs, 10 ** 6)
        assert obs.check_sizes() and obs.xyz.shape[0] == int(k64.sum()), name
        assert torch.equal(obs.xyz, torch.cat([pts[t][keep[t]] for t in range(T)])), name
        assert torch.equal(obs.normals, torch.cat([normals[t][keep[t]] for t in range(T)])), name
        assert torch.equal(obs.colors, torch.cat([im[t][keep[t]] for t in range(T)])), name


def test_the_example_runs_from_2d_inputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "init_scene.py"), "--from-2d", "--tracks", "300", "--frames", "6",
                          "--bases", "2", "--points", "500"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "from 2-D" in out.stdout and "render" in out.stdout
