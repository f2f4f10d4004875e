"""deblur4dgs_amd.losses.track_losses on the GPU (csrc/trimmed.hip: k_track_values, the shared selection, k_track_bwd) against the
fp64 gather-by-query restatement tests/track_ref.py, which tests/test_track_ref.py pins to the reference.

Inputs are made in fp32 and the restatement gets those same values in fp64 (and forms the rank in fp32, as torch.quantile does for
fp32 input), so the two sides differ in arithmetic only.  Tolerances are those of tests/test_gpu_trimmed_losses.py: each loss at
rtol 2e-6, the gradient at 1e-5 of the restatement's maximum.  No kept-set flips are allowed for: every random case first asserts,
from the fp64 values alone, that the order statistics of the visible 2-D elements around the threshold are at least 1e-5 of the
value range apart (trimmed_ref.neighbours_apart) and that the rank's fractional part lies in [0.05, 0.95].

The cases are well conditioned by construction, not by selection: a target pixel lies 1 to 4 pixels from the projected point in
each coordinate and a target disparity differs from the predicted one by at least a fifth of it, so that an element's fp32
rounding (a few ulps of a coordinate below 40) stays a small fraction of the element and no element is a near-cancellation."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from deblur4dgs_amd.losses import track_losses
from tests import track_ref as T
from tests import trimmed_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
UP = 1.7  # upstream factor of every backward; the depth term enters with 3
PER_BATCH = ("query_tracks_2d", "target_Ks", "target_tracks_2d", "target_visibles", "target_track_depths")


def pick_q(n, candidates=(0.98, 0.9, 0.95, 0.8, 0.85, 0.77, 0.66, 0.97531)):
    """A quantile whose rank q (n - 1) has its fractional part in [0.05, 0.95] in fp64 (n <= 2 cannot: r = 0, or r = q)."""
    for q in candidates:
        if n < 2 or 0.05 <= math.modf(q * (n - 1))[0] <= 0.95:
            return q
    raise AssertionError(n)


def make_case(N, Ps, seed, visible=0.7, width=0, order="raster", identity_K=False, clamp=False):
    """-> keyword arguments of track_losses, fp32 CPU tensors (per-batch entries as lists).  The image is 12 x 16, or 32 x 40 where
    a batch entry needs more than 192 distinct pixels.  order: raster | shuffled | duplicates (query 1 repeats query 0's pixel)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    sign = lambda *s: torch.where(r(*s) < 0.5, -1.0, 1.0)
    B = len(Ps)
    H, W = (12, 16) if max(Ps) <= 192 else (32, 40)
    Ks = []
    for _ in range(B):
        K = torch.eye(3).repeat(N, 1, 1)
        if not identity_K:
            K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 10 + 4 * r(N), 10 + 4 * r(N), W / 2 + r(N), H / 2 + r(N)
            K = K + 0.02 * (r(N, 3, 3) - 0.5)  # every entry takes part
        Ks.append(K)
    # every pixel's point projects into the image of its target frame, at a depth in [1, 5]
    z = 1.0 + 4.0 * r(B, H, W, N)
    at = torch.stack([W * r(B, H, W, N), H * r(B, H, W, N), torch.ones(B, H, W, N)], -1) * z[..., None]
    tracks = torch.einsum("bnij,bhwnj->bhwni", torch.linalg.inv(torch.stack(Ks).double()), at.double()).float()
    kw = {k: [] for k in PER_BATCH}
    for b, P in enumerate(Ps):
        idx = torch.sort(torch.randperm(H * W, generator=g)[:P]).values
        if order == "shuffled":
            idx = idx[torch.randperm(P, generator=g)]
        elif order == "duplicates":
            idx[1::7] = idx[0::7][:idx[1::7].numel()]
        y, x = idx // W, idx % W
        kw["query_tracks_2d"].append(torch.stack([x, y], -1).float() + 0.8 * r(P, 2))
        vis = r(N, P) < visible
        if clamp:  # a quarter of the visible elements at or behind the camera plane (K = identity: P_z = z), fp32-exact
            assert identity_K
            zs = torch.tensor([0.0, -1.0, 1e-7])[torch.randint(0, 3, (N, P), generator=g)]
            hit = vis & (r(N, P) < 0.25)
            zq = tracks[b, y, x, :, 2].T  # [N, P]
            tracks[b, y, x, :, 2] = torch.where(hit, zs, zq).T
        proj = torch.einsum("nij,pnj->npi", Ks[b].double(), tracks[b, y, x].double())
        pz = proj[..., 2].clamp(min=1e-6)
        xy = (proj[..., :2] / pz[..., None]).float()
        behind = proj[..., 2] <= 1e-6
        # (behind the plane xy is of the order 1e6: the target is an image point, the element of that order)
        kw["target_tracks_2d"].append(torch.where(behind[..., None], torch.stack([W * r(N, P), H * r(N, P)], -1),
                                                  xy + sign(N, P, 2) * (1.0 + 3.0 * r(N, P, 2))))
        kw["target_visibles"].append(vis)
        ratio = 1.2 + 0.6 * r(N, P)
        kw["target_track_depths"].append(torch.where(behind, 1.0 + 4.0 * r(N, P), (pz * torch.where(r(N, P) < 0.5, ratio, 1.0 / ratio)).float()))
        kw["target_Ks"].append(Ks[b])
    n = N * sum(Ps)
    kw["tracks_3d"] = tracks
    kw["track_weights"] = 0.1 + r(n) if width == 0 else (0.1 + r(n, 1)) * torch.exp(-2.0 * r(width))[None]
    return kw


def n_visible(kw):
    return int(T.elements(**doubles(kw))[4].sum())


def doubles(kw):
    cast = lambda x: x.double() if x.is_floating_point() else x
    return {k: [cast(x) for x in v] if isinstance(v, list) else cast(v) for k, v in kw.items()}


def separated(kw, q):
    """The two conditions of the module docstring, from the fp64 values alone."""
    v2d = T.elements(**doubles(kw))[0]
    n = v2d.numel()
    return R.neighbours_apart(v2d, q) and (n < 3 or 0.05 <= math.modf(q * (n - 1))[0] <= 0.95)


def on_gpu(kw, q):
    dev = {k: [x.to(DEV) for x in v] if isinstance(v, list) else v.to(DEV) for k, v in kw.items()}
    t = dev["tracks_3d"].requires_grad_()
    l2d, ldepth = track_losses(**dev, quantile=q)
    (UP * (l2d + 3.0 * ldepth)).backward()
    return l2d.detach().cpu(), ldepth.detach().cpu(), t.grad.cpu()


def on_ref(kw, q):
    d = doubles(kw)
    t = d["tracks_3d"].requires_grad_()
    l2d, ldepth = T.track_losses(**d, quantile=q, rank_dtype=F32)
    (UP * (l2d + 3.0 * ldepth)).backward()
    return l2d.detach(), ldepth.detach(), t.grad


def check(got, want, what, grad_sets=None):
    gg, wg = got[2].double(), want[2]
    print(what, "2-D", float(got[0]), "restatement", float(want[0]), "| depth", float(got[1]), "restatement", float(want[1]),
          "| max |grad|", float(wg.abs().max()), "max grad diff", float((gg - wg).abs().max()))
    np.testing.assert_allclose(float(got[0]), float(want[0]), rtol=2e-6, atol=0, err_msg=what + " 2-D")  # (NaN == NaN here)
    np.testing.assert_allclose(float(got[1]), float(want[1]), rtol=2e-6, atol=0, err_msg=what + " depth")
    for name, sel in (grad_sets or {"all": torch.ones(wg.shape[:-1], dtype=torch.bool)}).items():
        print("   ", name, int(sel.sum()), "points, max |grad|", float(wg[sel].abs().max()), "max diff", float((gg[sel] - wg[sel]).abs().max()))
        np.testing.assert_allclose(gg[sel].numpy(), wg[sel].numpy(), rtol=0, atol=1e-5 * float(wg[sel].abs().max()), err_msg=f"{what} {name}")


def both(kw, q, what, **kws):
    got, want = on_gpu(kw, q), on_ref(kw, q)
    check(got, want, f"{what} q={q}", **kws)
    return got, want


# Seeds: a formula per case, replaced here where the two conditions did not hold for it (found and checked on the CPU; the
# conditions are asserted again in every test, so a wrong entry fails there and not in the comparison).  Every formula seed of the
# cases below passed, so the table is empty.
SEEDS = {}


def seed_for(*key, default):
    return SEEDS.get(key, default)


def random_case(key, default_seed, *args, **kw):
    """-> (case, quantile) with the separation and rank conditions asserted."""
    case = make_case(*args, seed=seed_for(*key, default=default_seed), **kw)
    q = pick_q(n_visible(case))
    assert separated(case, q), (key, q)
    return case, q


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_one_target_frame_at_every_size(P):
    case, q = random_case(("n1", P), 100 + P, 1, (P,))
    assert n_visible(case) >= 1
    both(case, q, f"N=1 P={P}")


@pytest.mark.parametrize("name,N,Ps,kw", [("n4_p65", 4, (65,), {}), ("b2_p7_p40", 2, (7, 40), {}), ("n3_all_visible", 3, (50,), {"visible": 2.0}),
                                           ("weights_n_1", 2, (33,), {"width": 1}), ("weights_n_4", 4, (33,), {"width": 4}),
                                           ("shuffled", 3, (70,), {"order": "shuffled"}), ("duplicates", 3, (70,), {"order": "duplicates"})])
def test_frames_batches_weights_and_query_orders(name, N, Ps, kw):
    case, q = random_case((name,), 7000 + 10 * N + sum(Ps), N, Ps, **kw)
    if name == "n3_all_visible":
        assert n_visible(case) == 3 * 50
    if name.startswith("weights"):
        assert case["track_weights"].shape == (N * sum(Ps), kw["width"])
    if name == "duplicates":
        flat = case["query_tracks_2d"][0].to(torch.int64)
        assert len({(int(a), int(b)) for a, b in flat}) < flat.shape[0]
    both(case, q, name)
    if name == "n4_p65":
        both(case, 1.0, name + " nothing trimmed")  # quantile 1 for the 2-D term as well: no selection at all


def test_clamped_depths_get_no_gradient_and_do_not_hide_the_rest():
    case, q = random_case(("clamp",), 4242, 3, (90,), identity_K=True, clamp=True)
    d = doubles(case)
    _, _, _, pz, live = T.elements(**d)
    assert {float(v) for v in pz[pz <= 1e-6].float()} == {0.0, -1.0, float(torch.tensor(1e-7))}
    assert 0.15 < float((pz <= 1e-6).double().mean()) < 0.35
    B, H, W, N, _ = case["tracks_3d"].shape
    qi = case["query_tracks_2d"][0].to(torch.int64)
    clamped = torch.zeros(B, H, W, N, dtype=torch.bool)
    unclamped = torch.zeros(B, H, W, N, dtype=torch.bool)
    live, behind = live.reshape(N, -1), torch.zeros(live.numel(), dtype=torch.bool)
    behind[live.reshape(-1)] = pz <= 1e-6
    behind = behind.reshape(N, -1)
    for n in range(N):
        clamped[0, qi[:, 1], qi[:, 0], n] = live[n] & behind[n]
        unclamped[0, qi[:, 1], qi[:, 0], n] = live[n] & ~behind[n]
    got, want = both(case, q, "clamp", grad_sets={"clamped": clamped, "unclamped": unclamped})
    assert float(want[2][clamped].abs().max()) > 1e4 * float(want[2][unclamped].abs().max())  # the 1e6-scaled set would hide the other
    assert not got[2][clamped][:, 2].any() and not want[2][clamped][:, 2].any()  # exactly zero through the clamp
    assert got[2][clamped][:, :2].any()  # x and y still divide by 1e-6


def test_no_visible_element():
    case = make_case(2, (30,), 5, visible=-1.0)
    got, want = both(case, 0.98, "nothing visible")
    assert math.isnan(float(got[0])) and float(got[1]) == 0.0 and not got[2].any()
    got = on_gpu(case, 1.0)
    assert float(got[0]) == 0.0 and float(got[1]) == 0.0 and not got[2].any()


def test_queries_outside_the_image_count_as_invisible():
    case, q = random_case(("outside",), 99, 2, (40,), visible=2.0)
    H, W = case["tracks_3d"].shape[1:3]
    masked = {**case, "target_visibles": [case["target_visibles"][0].clone()]}
    masked["target_visibles"][0][:, [3, 17]] = False
    q = pick_q(n_visible(masked))
    assert separated(masked, q)
    outside = {**case, "query_tracks_2d": [case["query_tracks_2d"][0].clone()]}
    outside["query_tracks_2d"][0][3] = torch.tensor([float(W), 2.0])
    outside["query_tracks_2d"][0][17] = torch.tensor([5.0, -1.0])
    a, b = on_gpu(outside, q), on_gpu(masked, q)
    for x, y in zip(a, b):
        assert torch.equal(x, y)  # bit for bit the result with the two masked
    check(a, on_ref(masked, q), "two queries outside")
    assert int((a[2] != 0).any(-1).sum()) == 2 * 38  # the rest of the gradient is intact


def test_the_gradient_is_zero_away_from_the_visible_queries():
    case, q = random_case(("n4_p65",), 7000 + 40 + 65, 4, (65,))
    got = on_gpu(case, q)
    B, H, W, N, _ = case["tracks_3d"].shape
    touched = torch.zeros(B, H, W, N, dtype=torch.bool)
    qi = case["query_tracks_2d"][0].to(torch.int64)
    for n in range(N):
        touched[0, qi[:, 1], qi[:, 0], n] = case["target_visibles"][0][n]
    assert not got[2][~touched].any()
    assert got[2][touched].any(-1).all()  # (the depth term is never trimmed: every visible point receives something)


def test_rejects_mismatched_shapes_and_cpu_tensors():
    case = make_case(2, (10,), 1)
    dev = {k: [x.to(DEV) for x in v] if isinstance(v, list) else v.to(DEV) for k, v in case.items()}
    for key, bad in (("target_tracks_2d", [dev["target_tracks_2d"][0][:, :9]]), ("target_visibles", [dev["target_visibles"][0][:1]]),
                     ("target_Ks", [dev["target_Ks"][0][:1]]), ("target_track_depths", [dev["target_track_depths"][0].T]),
                     ("track_weights", dev["track_weights"][:-1]), ("query_tracks_2d", dev["query_tracks_2d"] * 2),
                     ("tracks_3d", dev["tracks_3d"][..., :2])):
        with pytest.raises(ValueError):
            track_losses(**{**dev, key: bad})
    with pytest.raises(RuntimeError, match="ROCm"):
        track_losses(**case)
    with pytest.raises(RuntimeError, match="ROCm"):
        track_losses(**{**dev, "target_visibles": case["target_visibles"]})
    l2d, ldepth = track_losses(**{k: v[0] if isinstance(v, list) else v for k, v in dev.items()})  # single tensors for B = 1
    assert math.isfinite(float(l2d)) and math.isfinite(float(ldepth))


def _fwd_bwd(dev):
    t = dev["tracks_3d"]
    l2d, ldepth = track_losses(**dev, quantile=0.9)
    (grad,) = torch.autograd.grad(UP * (l2d + 3.0 * ldepth), [t])
    return torch.stack([l2d, ldepth]).detach(), grad


def _graph_inputs(seed, visible):
    case = make_case(3, (200, 120), seed, visible=visible, width=4)  # B = 2: 32 x 40 images
    return {k: [x.to(DEV) for x in v] if isinstance(v, list) else v.to(DEV) for k, v in case.items()}


def test_two_runs_are_bitwise_equal():
    runs = []
    for _ in range(2):
        dev = _graph_inputs(21, 0.7)
        dev["tracks_3d"].requires_grad_()
        runs.append(_fwd_bwd(dev))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert torch.isfinite(runs[0][0]).all() and runs[0][1].any()


def test_graph_capture_and_replay_with_a_different_visible_count():
    """Forward and backward in ONE captured graph (capture aborts on any host wait: this is the test that the path has none - the
    element tables are rebuilt from the static query tensors by torch ops inside the graph).  Replays with new data in the static
    inputs - another number of visible elements, which only the device learns - equal eager calls on the same data bit for bit
    (distinct queries: every address of the scatter receives one add onto zero)."""
    static = _graph_inputs(31, 0.7)
    static["tracks_3d"].requires_grad_()
    _fwd_bwd(static)  # warm-up: code objects loaded, nothing lazy left inside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _fwd_bwd(static)
    counts = set()
    for seed, visible in ((31, 0.7), (32, 0.35), (33, 0.95)):
        fresh = _graph_inputs(seed, visible)
        counts.add(int(sum(v.sum() for v in fresh["target_visibles"])))
        with torch.no_grad():
            for k, v in static.items():
                for s, f in zip(v if isinstance(v, list) else [v], fresh[k] if isinstance(v, list) else [fresh[k]]):
                    s.copy_(f)
        g.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in out]
        fresh["tracks_3d"].requires_grad_()
        eager = _fwd_bwd(fresh)
        for name, x, y in zip(("losses", "gradient"), replayed, eager):
            assert torch.equal(x, y), (seed, name, x.flatten()[:4], y.flatten()[:4])
        assert torch.isfinite(eager[0]).all() and eager[1].any()
    assert len(counts) == 3


def test_example_trains_with_track_losses_inside_the_graph():
    """examples/train_dynamic_step.py with track_losses=True on a small scene: the whole step (three renders, photometric and track
    losses, backward, one-launch Adam) captures after two eager steps and replays; the losses are finite, every step's loss equals
    the eager run's of the same seed within the spread the eager run shows between two seeds of the synthetic scene (the criterion
    of tests/test_gpu_trimmed_losses.py for the depth losses), and the first loss differs from the run without the flag."""
    spec = importlib.util.spec_from_file_location("train_dynamic_step_tracks", os.path.join(ROOT, "examples", "train_dynamic_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kw = dict(steps=6, W=128, H=96, n_fg=3000, n_bg=5000, K=6, verbose=False, hip_adam=True, track_losses=True)
    eager = mod.train(**kw)[0]
    eager_seed2 = mod.train(seed=2, **kw)[0]
    graph = mod.train(graph=True, **kw)[0]
    plain = mod.train(**{**kw, "track_losses": False})[0]
    spread = abs(eager[-1] - eager_seed2[-1])
    print("eager", eager, "| graph", graph, "| eager seed 2", eager_seed2[-1], "| spread", spread, "| without the track losses", plain[0])
    assert all(math.isfinite(l) for l in graph + eager)
    assert all(abs(a - b) <= spread for a, b in zip(graph, eager)), (graph, eager, spread)
    assert eager[0] != plain[0]
