"""Scene initialisation on the GPU (csrc/scene_init.hip through deblur4dgs_amd.scene_init) against fp64 statements written here and
against tests/golden/scene_init.npz, which tests/golden/gen_scene_init.py records from the reference's own functions in fp64.

Inputs are fp32 and every statement sees the same numbers in fp64, so the two sides differ in arithmetic only.  The bounds:
  interp     visible frames bit for bit; elsewhere 1e-6 max|xyz| (the kernel interpolates in double and rounds once: 6e-8 of the
             value); vel_dirs 1e-6 absolute (components <= 1, one rounding)
  kNN        1e-6 relative (three squares, two adds and a root in fp32: 2e-7), exact zeros, no index flip allowance
  k-means    labels equal to fp64 argmin outside points whose best two squared distances differ by < 1e-4 relative (fp32 sums of up
             to 69 squares err by ~4e-6), at most 1 % such points; centres 1e-5 max|centre| (sums in double, one rounding).
             G = 777, 2 000 and 4 097 are 4, 8 and 17 blocks; G = 65 793 = 256 x 257 + 1 is past the cap of 256 blocks: the rows
             are strided over (257 of them in a second turn) and every cluster's total is taken over exactly 256 partials
  Procrustes moments 1e-12 of the sum of the terms' magnitudes (double sums of <= 257 terms); bases 1e-4 max|ref|
"""
import functools
import os

import numpy as np
import pytest
import torch

from deblur4dgs_amd import scene_init as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("default_small", "edge_cano", "skips")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN, "scene_init.npz"))
    return {k: z[k] for k in z.files}


def golden_case(name):
    g = golden()
    return {k.split("/", 1)[1]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(name + "/")}


# ------------------------------------------------------------------------------------------------------------------ interp

def visibility(G, T, shift, gen):
    """rows cycle through: all visible, one visible frame, only the first, only the last, alternating, none, random, random"""
    vis = torch.rand(G, T, generator=gen) < 0.6
    for g in range(G):
        kind = (g + shift) % 8
        if kind == 0:
            vis[g] = True
        elif kind == 1:
            vis[g] = False
            vis[g, int(torch.randint(0, T, (1,), generator=gen))] = True
        elif kind == 2:
            vis[g] = False
            vis[g, 0] = True
        elif kind == 3:
            vis[g] = False
            vis[g, T - 1] = True
        elif kind == 4:
            vis[g] = torch.arange(T) % 2 == (g // 8) % 2
        elif kind == 5:
            vis[g] = False
    return vis


def interp_f64(xyz, vis):
    """per-row np.interp over the visible frames in fp64; a row without one is kept; and the velocity directions of the result"""
    x, v = xyz.double().numpy(), vis.numpy()
    T = x.shape[1]
    out = x.copy()
    for g in range(x.shape[0]):
        if v[g].any():
            for c in range(3):
                out[g, :, c] = np.interp(np.arange(T), np.flatnonzero(v[g]), x[g, v[g], c])
    vel = out[:, 1:] - out[:, :-1]
    dirs = vel / (np.linalg.norm(vel, axis=-1, keepdims=True) + 1e-5)
    return torch.from_numpy(out), torch.from_numpy(dirs.reshape(x.shape[0], -1))


def check_interp(xyz, vis, want, want_dirs, got, got_dirs):
    assert got.dtype == got_dirs.dtype == torch.float32 and got.shape == xyz.shape and tuple(got_dirs.shape) == (xyz.shape[0], 3 * (xyz.shape[1] - 1))
    got, got_dirs = got.cpu(), got_dirs.cpu()
    assert torch.equal(bits(got[vis]), bits(xyz[vis]))  # a visible frame is copied bit for bit
    err, err_dirs = (got.double() - want).abs().max().item(), (got_dirs.double() - want_dirs).abs().max().item()
    print(f"interp err {err:.3e} (bound {1e-6 * xyz.abs().max().item():.3e}), vel_dirs err {err_dirs:.3e} (bound 1e-6)")
    assert err <= 1e-6 * xyz.abs().max().item()
    assert err_dirs <= 1e-6 and got_dirs.abs().max().item() <= 1.0


@pytest.mark.parametrize("T", (2, 3, 24, 65))
@pytest.mark.parametrize("G", (1, 63, 64, 65, 257))
def test_track_features_are_np_interp_and_its_velocity_directions(G, T):
    gen = torch.Generator().manual_seed(1000 * G + T)
    for shift in (range(8) if G == 1 else (0,)):
        xyz = torch.randn(G, T, 3, generator=gen) * 2.0 + torch.randn(G, 1, 3, generator=gen)
        vis = visibility(G, T, shift, gen)
        want, want_dirs = interp_f64(xyz, vis)
        got, got_dirs = S.track_features(xyz.to(DEV), vis.to(DEV))
        check_interp(xyz, vis, want, want_dirs, got, got_dirs)
        assert torch.equal(bits(S.interp_tracks(xyz.to(DEV), vis.to(DEV))), bits(got))
        only_dirs = S.track_features(xyz.to(DEV), vis.to(DEV), want_interp=False)
        assert only_dirs[0] is None and torch.equal(bits(only_dirs[1]), bits(got_dirs))


@pytest.mark.parametrize("name", ("edge_cano", "skips"))
def test_track_features_match_the_reference(name):
    c = golden_case(name)
    xyz, vis = c["xyz"][c["valid"]], c["visibles"][c["valid"]]
    got, got_dirs = S.track_features(xyz.to(DEV), vis.to(DEV))
    check_interp(xyz, vis, c["interp"], c["vel_dirs"], got, got_dirs)


# --------------------------------------------------------------------------------------------------------------------- kNN

def knn_f64(x, k):
    """fp64 brute force on the device: -> (the full distance matrix with an infinite diagonal, its k smallest per row ascending)"""
    p = x.double()
    d2 = torch.zeros(len(p), len(p), dtype=torch.float64, device=p.device)
    for c in range(3):
        d2 += (p[:, None, c] - p[None, :, c]).square()
    d = d2.sqrt()
    d.fill_diagonal_(float("inf"))
    return d, torch.topk(d, k, dim=1, largest=False, sorted=True).values


def check_knn(x, k):
    N = len(x)
    dists, idx = S.knn(x, k)
    assert dists.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(dists.shape) == tuple(idx.shape) == (N, k)
    full, want = knn_f64(x, k)
    err = ((dists.double() - want).abs() / want.clamp_min(1e-300)).masked_fill(want == 0, 0.0).max().item()
    print(f"N={N} k={k}: max relative error {err:.3e} (bound 1e-6), zeros {int((want == 0).sum())}")
    assert err <= 1e-6
    assert bool((dists[want == 0] == 0).all())  # exact zeros where fp64 has zeros
    assert bool((dists[:, 1:] >= dists[:, :-1]).all())  # ascending
    i64 = idx.long()
    assert bool(((i64 >= 0) & (i64 < N)).all()) and not bool((i64 == torch.arange(N, device=x.device)[:, None]).any())
    assert bool((torch.sort(i64, dim=1).values.diff(dim=1) > 0).all()) if k > 1 else True  # distinct
    at = torch.gather(full, 1, i64)  # the fp64 distance to the reported neighbour is the reported distance
    assert bool(((dists.double() - at).abs() <= 1e-6 * at).all())
    return dists, idx


@pytest.mark.parametrize("k", (1, 3, 8))
def test_knn_at_every_tile_and_split_edge(k):
    sizes = [k + 1, 511, 512, 513, S.KNN_TILE - 1, S.KNN_TILE, S.KNN_TILE + 1, 2 * S.KNN_TILE + 1, S.KNN_SPLIT_MIN, S.KNN_SPLIT_MIN + 1]
    from deblur4dgs_amd import _lib as L

    assert L.lib().d4gs_knn_splits(S.KNN_SPLIT_MIN) == 1 and L.lib().d4gs_knn_splits(S.KNN_SPLIT_MIN + 1) > 1
    gen = torch.Generator().manual_seed(50 + k)
    for N in sizes:
        check_knn(torch.randn(N, 3, generator=gen).to(DEV), k)


@functools.lru_cache(maxsize=None)
def clustered_points():
    """3 000 points in 30 clusters of scales 1e-4 .. 1 at centres up to +-10 (coordinates clipped to +-10), ten exact duplicates"""
    gen = torch.Generator().manual_seed(7)
    centres = torch.rand(30, 3, generator=gen) * 20 - 10
    scales = torch.logspace(-4, 0, 30)
    which = torch.arange(3000) % 30
    x = (centres[which] + scales[which, None] * torch.randn(3000, 3, generator=gen)).clamp(-10, 10)
    x[torch.arange(10) * 97 + 1500] = x[torch.arange(10) * 31]
    return x


@pytest.mark.parametrize("k", (3, 8))
def test_knn_on_clustered_points_with_duplicates(k):
    x = clustered_points().to(DEV)
    dists, idx = check_knn(x, k)
    dup = torch.arange(10) * 97 + 1500
    assert bool((dists[dup, 0] == 0).all()) and bool((dists[torch.arange(10) * 31, 0] == 0).all())
    again = S.knn(x, k)
    assert torch.equal(bits(again[0]), bits(dists)) and torch.equal(again[1], idx)  # reproducible


@pytest.mark.parametrize("name", CASES)
def test_knn_matches_the_reference(name):
    c = golden_case(name)
    dists, _ = S.knn(c["xyz"][:, int(c["cano_t"])].to(DEV), 3)
    want = c["knn3"].double()
    err = ((dists.cpu().double() - want).abs() / want).max().item()
    print(f"{name}: max relative error against sklearn {err:.3e} (bound 1e-6)")
    assert err <= 1e-6


# ----------------------------------------------------------------------------------------------------------------- k-means
KM_CASES = ((777, 5, 3, 0.03), (2000, 12, 6, 0.05), (4097, 24, 20, 0.02), (65793, 12, 3, 0.02))
KM_CAPPED = 256 * 257 + 1  # the last case: 256 blocks of 256 rows stride; block 0 and lane 0 of block 1 take a second row each


def assert_kmeans_grid_is_capped(G):
    """the row stride of k_kmeans_assign / k_kmeans_accum is taken and k_kmeans_finish totals 256 partials per cluster, one per thread"""
    from deblur4dgs_amd import _lib as L

    assert L.lib().d4gs_kmeans_blocks(G) == 256 and G > 65536


@functools.lru_cache(maxsize=None)
def kmeans_inputs(G, T, K, noise):
    """G tracks = a random start + one of K smooth random-walk motions + noise -> their velocity directions (fp32, on the device) and
    K rows of them as first centres"""
    gen = torch.Generator().manual_seed(G + T)
    motions = torch.cumsum(torch.cumsum(torch.randn(K, T, 3, generator=gen) * 0.05, 1) + torch.randn(K, 1, 3, generator=gen) * 0.1, 1)
    which = torch.randint(0, K, (G,), generator=gen)
    xyz = torch.randn(G, 1, 3, generator=gen) + motions[which] + noise * torch.randn(G, T, 3, generator=gen)
    _, feats = S.track_features(xyz.to(DEV), torch.ones(G, T, dtype=torch.bool, device=DEV))
    rows = torch.randperm(G, generator=gen)[:K]
    return feats, feats[rows.to(DEV)].clone()


def lloyd_f64(x, centres):
    """one assignment in fp64 NumPy: -> labels (argmin: the lowest index among equals) and the relative margin of the best two"""
    d2 = np.stack([((x - c) ** 2).sum(1) for c in centres], 1)
    labels = d2.argmin(1)
    if centres.shape[0] == 1:
        return labels, np.full(len(x), np.inf)
    two = np.partition(d2, 1, axis=1)[:, :2]
    return labels, (two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)


@pytest.mark.parametrize("G,T,K,noise", KM_CASES)
def test_kmeans_steps_follow_fp64_lloyd(G, T, K, noise):
    feats, first = kmeans_inputs(G, T, K, noise)
    if G == KM_CAPPED:
        assert_kmeans_grid_is_capped(G)
    x64 = feats.cpu().double().numpy()
    centres, labels = first.clone(), torch.full((G,), -1, dtype=torch.int32, device=DEV)
    worst_share, worst_centre = 0.0, 0.0
    for it in range(20):
        before, old = centres.cpu().double().numpy(), labels.cpu().numpy()
        changed = S.kmeans_step(feats, centres, labels, 1)
        want, margin = lloyd_f64(x64, before)
        got = labels.cpu().numpy()
        sure = margin >= 1e-4
        assert (got[sure] == want[sure]).all(), it
        worst_share = max(worst_share, 1.0 - sure.mean())
        assert int(changed.item()) == int((got != old).sum()), it
        means = before.copy()  # the means of the device's own labels (checked above), in fp64; an empty cluster keeps its centre
        for k in range(K):
            if (got == k).any():
                means[k] = x64[got == k].mean(0)
        err = np.abs(centres.cpu().double().numpy() - means).max() / np.abs(means).max()
        worst_centre = max(worst_centre, err)
        assert err <= 1e-5, it
    print(f"G={G} T={T} K={K}: largest excluded share {worst_share:.2e} (cap 1e-2), largest centre error {worst_centre:.2e} (bound 1e-5)")
    assert worst_share <= 1e-2
    if G == KM_CAPPED:  # chosen on the CPU: the fp64 steps alone leave no row within the margin (the smallest is 7e-3), so every label is held
        assert worst_share == 0.0


@pytest.mark.parametrize("G,T,K,noise", KM_CASES)
def test_kmeans_iterations_in_one_call_are_the_single_calls_and_reproducible(G, T, K, noise):
    feats, first = kmeans_inputs(G, T, K, noise)
    runs = []
    for mode in ("single", "single", "batched"):
        centres, labels = first.clone(), torch.zeros(G, dtype=torch.int32, device=DEV)
        if mode == "single":
            for _ in range(20):
                changed = S.kmeans_step(feats, centres, labels, 1)
        else:
            changed = S.kmeans_step(feats, centres, labels, 20)
        runs.append((bits(centres), labels.cpu(), changed.cpu()))
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


def test_kmeans_ties_go_to_the_lower_index_and_an_empty_cluster_keeps_its_centre():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(600, 7, generator=gen).to(DEV)
    twin = torch.tensor([0.25, -0.5, 1.0, 0.0, 2.0, -1.0, 0.5])
    centres = torch.stack([twin + 9.0, twin, twin]).to(DEV)  # centre 0 far away; 1 and 2 identical: every row ties between them
    x[:5] += 9.0  # a few rows for centre 0
    labels = torch.full((600,), 2, dtype=torch.int32, device=DEV)
    changed = S.kmeans_step(x, centres, labels, 1)
    got = labels.cpu()
    assert not bool((got == 2).any()) and bool((got[:5] == 0).all()) and bool((got[5:] == 1).all())
    assert torch.equal(bits(centres[2]), bits(twin)) and int(changed.item()) == 600
    assert torch.allclose(centres[1].cpu().double(), x[5:].cpu().double().mean(0), rtol=0, atol=1e-6)
    # past the block cap: rows that only the stride reaches tie between centres 1 and 2, and cluster 3 has members among them alone
    G = KM_CAPPED
    assert_kmeans_grid_is_capped(G)
    x64 = torch.randn(G, 7, generator=gen)
    centres = torch.stack([twin + 9.0, twin, twin, twin - 9.0]).to(DEV)
    x64[:5] += 9.0
    lone = torch.tensor([65536, 65540, 65791, 65792])  # second-turn rows: lanes 0, 4 and 255 of block 0, lane 0 of block 1
    x64[lone] -= 9.0
    x, x64 = x64.to(DEV), x64.double()
    labels = torch.full((G,), 2, dtype=torch.int32, device=DEV)
    changed = S.kmeans_step(x, centres, labels, 1)
    got = labels.cpu()
    want = torch.ones(G, dtype=torch.int32)
    want[:5], want[lone] = 0, 3
    assert torch.equal(got, want) and int((got[65536:] == 1).sum()) == G - 65536 - len(lone)  # ties behind row 65 536: the lower index
    assert torch.equal(bits(centres[2]), bits(twin)) and int(changed.item()) == G
    rest = torch.ones(G, dtype=torch.bool)
    rest[:5], rest[lone] = False, False
    assert torch.allclose(centres[3].cpu().double(), x64[lone].mean(0), rtol=0, atol=1e-6)  # their mean, not "kept as empty"
    assert torch.allclose(centres[1].cpu().double(), x64[rest].mean(0), rtol=0, atol=1e-6)
    assert torch.allclose(centres[0].cpu().double(), x64[:5].mean(0), rtol=0, atol=1e-6)


@pytest.mark.parametrize("G,T,K,noise", KM_CASES)
def test_kmeans_wrapper_is_seeded_converges_and_reports_zero_changes_at_the_fixed_point(G, T, K, noise):
    feats, _ = kmeans_inputs(G, T, K, noise)
    a = S.kmeans(feats, K, generator=torch.Generator().manual_seed(11))
    b = S.kmeans(feats, K, generator=torch.Generator().manual_seed(11))
    assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
    assert a[0].dtype == torch.int64 and a[2] < 300, a[2]  # stopped before max_iter
    centres, labels = a[1].clone(), a[0].int()
    assert int(S.kmeans_step(feats, centres, labels, 1).item()) == 0  # a fixed point: nothing changes, centres included
    assert torch.equal(labels.long(), a[0]) and torch.equal(bits(centres), bits(a[1]))


# -------------------------------------------------------------------------------------------------------------- Procrustes

def moments_f64(xyz, w, conf, labels, K, cano_t):
    """-> ([K,T,16] by einsum in fp64, the same sums of the terms' magnitudes)"""
    x, w, conf = xyz.double(), w.double(), conf.double()
    T = x.shape[1]
    out, mag = torch.zeros(K, T, 16, dtype=torch.float64), torch.zeros(K, T, 16, dtype=torch.float64)
    for n in range(K):
        m = labels == n
        u = w[m, cano_t, None] * w[m] * (conf[m, cano_t, None] + conf[m]) / 2  # [p,T]
        src, dst = x[m, cano_t], x[m]
        for dest, f in ((out, lambda a: a), (mag, torch.abs)):
            dest[n, :, 0] = f(u).sum(0)
            dest[n, :, 1:4] = torch.einsum("pt,pc->tc", f(u), f(src))
            dest[n, :, 4:7] = torch.einsum("pt,ptc->tc", f(u), f(dst))
            dest[n, :, 7:] = torch.einsum("pt,pti,pj->tij", f(u), f(dst), f(src)).reshape(T, 9)
    return out, mag


@pytest.mark.parametrize("sizes", ((1, 1, 1, 1, 1), (257, 3, 40), (300,)), ids=("one-track-per-cluster", "cluster-of-257", "one-cluster"))
def test_procrustes_moments_are_the_fp64_sums(sizes):
    gen = torch.Generator().manual_seed(len(sizes))
    K, T, cano_t = len(sizes), 7, 3
    labels = torch.cat([torch.full((n,), i) for i, n in enumerate(sizes)])[torch.randperm(sum(sizes), generator=gen)]
    G = len(labels)
    xyz, w, conf = torch.randn(G, T, 3, generator=gen), torch.rand(G, T, generator=gen) * 2, torch.rand(G, T, generator=gen)
    w[torch.rand(G, T, generator=gen) < 0.1] = 0.0
    order = torch.argsort(labels, stable=True)
    seg = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32)
    got = S.procrustes_moments(xyz.to(DEV), w.to(DEV), conf.to(DEV), order.to(DEV), seg.to(DEV), cano_t)
    assert got.dtype == torch.float64 and tuple(got.shape) == (K, T, 16)
    want, mag = moments_f64(xyz, w, conf, labels, K, cano_t)
    err = ((got.cpu() - want).abs() / mag.clamp_min(1e-300)).masked_fill(mag == 0, 0.0).max().item()
    print(f"sizes {sizes}: largest error / sum of magnitudes {err:.3e} (bound 1e-12)")
    assert err <= 1e-12 and bool((got.cpu()[mag == 0] == 0).all())
    assert torch.equal(got, S.procrustes_moments(xyz.to(DEV), w.to(DEV), conf.to(DEV), order.to(DEV), seg.to(DEV), cano_t))


def tracks_of(c):
    return S.TrackObservations(c["xyz"].to(DEV), c["visibles"].to(DEV), ~c["visibles"].to(DEV), c["confidences"].to(DEV), c["colors"].to(DEV))


@pytest.mark.parametrize("name", CASES)
def test_motion_bases_match_the_reference(name):
    c = golden_case(name)
    cano_t, K = int(c["cano_t"]), c["rots"].shape[0]
    bases, coefs, kept = S.init_motion_params_with_procrustes(tracks_of(c), K, "6d", cano_t, labels=c["labels"].to(DEV))
    assert torch.equal(kept.xyz.cpu(), c["xyz"][c["valid"]]) and torch.equal(kept.visibles.cpu(), c["visibles"][c["valid"]])
    skipped = torch.zeros_like(c["skipped"])
    for n, (_, frames) in enumerate(sorted(bases.skipped_ts.items())):
        skipped[n, frames] = True
    assert torch.equal(skipped, c["skipped"]) and bool(skipped.any()) == (name == "skips")
    for what, got, want in (("rots", bases.params["rots"], c["rots"]), ("transls", bases.params["transls"], c["transls"]),
                            ("motion_coefs", coefs, c["motion_coefs"])):
        assert got.dtype == torch.float32 and got.shape == want.shape, what
        err = (got.detach().cpu().double() - want).abs().max().item() / want.abs().max().item()
        print(f"{name} {what}: max err / max|ref| {err:.3e} (bound 1e-4)")
        assert err <= 1e-4, what
    if "weights" in c:  # the restated get_weights_for_procrustes, per cluster, against the reference's
        labels, xyz, vis = c["labels"][c["valid"]], kept.xyz, kept.visibles
        for i in labels.unique():
            m = (labels == i).to(DEV)
            w = S.get_weights_for_procrustes(xyz[m].transpose(0, 1), vis[m].transpose(0, 1)).transpose(0, 1).cpu().double()
            want = c["weights"][labels == i]
            assert torch.equal(w == 0, want == 0) and (w - want).abs().max().item() <= 1e-5 * want.abs().max().item()


def test_procrustes_recovers_a_known_motion():
    gen = torch.Generator().manual_seed(5)
    G, T, cano_t = 400, 6, 2
    labels = torch.arange(G) % 2
    start = torch.randn(G, 3, generator=gen, dtype=torch.float64)
    Rs, ts = torch.zeros(2, T, 3, 3, dtype=torch.float64), torch.zeros(2, T, 3, dtype=torch.float64)
    xyz = torch.zeros(G, T, 3, dtype=torch.float64)
    for k in range(2):
        for t in range(T):
            q, r = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
            q = q * torch.sign(torch.diagonal(r))
            Rs[k, t] = torch.eye(3, dtype=torch.float64) if t == cano_t else q * torch.sign(torch.linalg.det(q))
            ts[k, t] = 0.0 if t == cano_t else torch.randn(3, generator=gen, dtype=torch.float64)
            xyz[labels == k, t] = start[labels == k] @ Rs[k, t].T + ts[k, t]
    ones = torch.ones(G, T)
    tracks = S.TrackObservations(xyz.float().to(DEV), ones.bool().to(DEV), ~ones.bool().to(DEV), ones.to(DEV), torch.rand(G, 3, generator=gen).to(DEV))
    bases, coefs, kept = S.init_motion_params_with_procrustes(tracks, 2, "6d", cano_t, labels=labels.to(DEV))
    assert kept.xyz.shape[0] == 380 and tuple(coefs.shape) == (380, 2) and all(v == [] for v in bases.skipped_ts.values())
    want = torch.cat([Rs[..., 0], Rs[..., 1]], -1)
    err_r = (bases.params["rots"].detach().cpu().double() - want).abs().max().item()
    err_t = (bases.params["transls"].detach().cpu().double() - ts).abs().max().item()
    print(f"known motion: rotation error {err_r:.3e}, translation error {err_t:.3e} (bound 1e-5)")
    assert err_r <= 1e-5 and err_t <= 1e-5
    q_rots, _, _, _ = S.solve_motion_bases(tracks.xyz, tracks.visibles, tracks.confidences, labels.to(DEV), cano_t, "quat")
    assert tuple(q_rots.shape) == (2, T, 4) and bool(((q_rots.norm(dim=-1) - 1).abs() <= 1e-6).all())
    w, x, y, z = q_rots.cpu().double().unbind(-1)
    back = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(2, T, 3, 3)
    assert (back - Rs).abs().max().item() <= 1e-5  # wxyz, the quaternion of the same rotation


# ---------------------------------------------------------------------------------------------------------------- builders

def mean_knn3_f64(x):
    return knn_f64(x, 3)[1].mean(-1, keepdim=True)


def test_fg_and_bg_builders_match_their_fp64_statements_and_the_scene_renders():
    from deblur4dgs_amd.scene_model import SceneModel

    c = golden_case("default_small")
    cano_t, K = int(c["cano_t"]), c["rots"].shape[0]
    bases, coefs, kept = S.init_motion_params_with_procrustes(tracks_of(c), K, "6d", cano_t, labels=c["labels"].to(DEV))
    fg = S.init_fg_from_tracks_3d(cano_t, kept, coefs, generator=torch.Generator().manual_seed(21))
    G = kept.xyz.shape[0]
    p = fg.params
    assert [tuple(p[k].shape) for k in ("means", "quats", "scales", "colors", "opacities", "motion_coefs")] == [(G, 3), (G, 4), (G, 3), (G, 3), (G,), (G, K)]
    assert torch.equal(p["means"].detach(), kept.xyz[:, cano_t]) and torch.equal(p["quats"].detach().cpu(), torch.rand(G, 4, generator=torch.Generator().manual_seed(21)))
    raw = mean_knn3_f64(kept.xyz[:, cano_t])
    lo, hi = torch.quantile(raw, 0.05), torch.quantile(raw, 0.95)
    want = torch.log(raw.clamp(lo, hi)).repeat(1, 3)
    got = p["scales"].detach().double()
    assert (got - want).abs().max().item() <= 1e-5
    assert abs(got.min().item() - lo.log().item()) <= 1e-5 and abs(got.max().item() - hi.log().item()) <= 1e-5  # the clamp quantiles
    assert (p["colors"].detach().double() - torch.logit(kept.colors.double())).abs().max().item() <= 1e-5
    assert (p["opacities"].detach().double() - np.log(0.7 / 0.3)).abs().max().item() <= 1e-6

    gen = torch.Generator().manual_seed(22)
    N = 500
    normals = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    normals[0], normals[1], normals[2] = torch.tensor([0.0, 0.0, 1.0]), torch.tensor([0.0, 0.0, -1.0]), torch.tensor([1.0, 0.0, 0.0])
    pts = S.StaticObservations((torch.randn(N, 3, generator=gen) * torch.tensor([3.0, 1.0, 0.5]) + 4.0).to(DEV), normals.to(DEV),
                               (torch.rand(N, 3, generator=gen) * 0.9 + 0.05).to(DEV))
    bg = S.init_bg(pts)
    x = pts.xyz.double()
    centre = x.mean(0)
    extent = (x - centre).quantile(0.95, dim=0) - (x - centre).quantile(0.05, dim=0)
    assert (bg.scene_center.double() - centre).abs().max().item() <= 1e-5 and abs(float(bg.scene_scale) - float(extent.max() / 2)) <= 1e-5
    assert (bg.params["scales"].detach().double() - torch.log(mean_knn3_f64(pts.xyz)).repeat(1, 3)).abs().max().item() <= 1e-5
    n = normals.double()
    cross = torch.stack([-n[:, 1], n[:, 0], torch.zeros(N, dtype=torch.float64)], -1)  # z x n
    norm = cross.norm(dim=-1, keepdim=True)
    axis = torch.where(norm > 0, cross / norm.clamp_min(1e-300), torch.zeros_like(cross))
    theta = torch.where(norm > 0, torch.acos(n[:, 2:3]), torch.zeros_like(norm))
    want_q = torch.cat([torch.cos(theta / 2), axis * torch.sin(theta / 2)], -1)
    got_q = bg.params["quats"].detach().cpu().double()
    assert (got_q - want_q).abs().max().item() <= 1e-6
    assert torch.equal(got_q[0], torch.tensor([1.0, 0, 0, 0], dtype=torch.float64)) and torch.equal(got_q[1], got_q[0])  # +z and -z

    W = H = 32
    Ks = torch.tensor([[[40.0, 0, 16], [0, 40.0, 16], [0, 0, 1]]]).repeat(c["xyz"].shape[1], 1, 1)
    w2cs = torch.eye(4).repeat(c["xyz"].shape[1], 1, 1)
    w2cs[:, 2, 3] = 6.0
    small_bg = S.init_bg(S.StaticObservations(pts.xyz * 0.2, pts.normals, pts.colors))
    model = SceneModel(Ks, w2cs, fg, bases, small_bg).to(DEV)
    with torch.no_grad():
        out = model.render(cano_t, model.w2cs[:1], model.Ks[:1], (W, H))
    assert tuple(out["img"].shape) == (1, H, W, 3) and bool(torch.isfinite(out["img"]).all()) and float(out["acc"].max()) > 0
    f7 = np.load(os.path.join(GOLDEN, "f7_state_dict.npz"))
    assert list(model.state_dict().keys()) == [str(k) for k in f7["full_keys"]]
