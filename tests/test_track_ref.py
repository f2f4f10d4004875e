"""The track losses without a GPU: the fp64 gather-by-query restatement the GPU tests compare against (tests/track_ref.py) is pinned
to values recorded from the reference's data flow around its own masked_l1_loss (tests/golden/track_losses.npz, written by
tests/golden/gen_track_losses.py), and the two facts that do not depend on how queries and pixels are paired are checked on it."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "track_losses.npz")
PER_BATCH = ("query_tracks_2d", "target_Ks", "target_tracks_2d", "target_visibles", "target_track_depths")


def _gen():
    sys.path.insert(0, GOLDEN)  # the generator imports its neighbour gen_trimmed_losses
    try:
        spec = importlib.util.spec_from_file_location("gen_track_losses", os.path.join(GOLDEN, "gen_track_losses.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(GOLDEN)
    return mod


GEN = _gen()
CASES = GEN.cases()


def load(name):
    """-> (keyword arguments of track_losses from the fixture, quantile)"""
    z = np.load(FIXTURE)
    B = len(CASES[name][0]["query_tracks_2d"])
    kw = {k: [torch.from_numpy(z[f"{name}/{k}/{b}"]) for b in range(B)] for k in PER_BATCH}
    kw["tracks_3d"], kw["track_weights"] = torch.from_numpy(z[f"{name}/tracks_3d/0"]), torch.from_numpy(z[f"{name}/track_weights/0"])
    return kw, CASES[name][1]


def run(kw, q):
    t = kw["tracks_3d"].clone().requires_grad_()
    l2d, ldepth = T.track_losses(**{**kw, "tracks_3d": t}, quantile=q)
    (1.7 * (l2d + 3.0 * ldepth)).backward()
    return float(l2d.detach()), float(ldepth.detach()), t.grad


def test_fixture_holds_the_cases_the_feature_is_specified_by():
    z = np.load(FIXTURE)
    assert {k.split("/")[0] for k in z.files} == set(CASES) == {"n4_p65", "n1_p1", "b2_p7_p40", "width1_weights"}
    for name, (c, _) in CASES.items():  # the inputs in the file are the generator's (same seed): nothing drifted
        for k in GEN.NAMES:
            for b, x in enumerate([c[k]] if torch.is_tensor(c[k]) else c[k]):
                assert np.array_equal(z[f"{name}/{k}/{b}"], x.numpy()), (name, k, b)
    shapes = {n: (c["tracks_3d"].shape[3], tuple(q.shape[0] for q in c["query_tracks_2d"]), c["track_weights"].shape[1]) for n, (c, _) in CASES.items()}
    assert shapes["n4_p65"][:2] == (4, (65,)) and shapes["n1_p1"][:2] == (1, (1,)) and shapes["b2_p7_p40"][1] == (7, 40)
    assert shapes["width1_weights"][2] == 1 and shapes["b2_p7_p40"][2] > 1
    for c, _ in CASES.values():  # distinct, raster-ordered queries: the case in which the reference's pairing is the restatement's
        for q in c["query_tracks_2d"]:
            flat = q.to(torch.int64)[:, 1] * GEN.W + q.to(torch.int64)[:, 0]
            assert bool((flat[1:] > flat[:-1]).all())
    assert os.path.getsize(FIXTURE) < 256 * 1024


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference_fixture(name):
    z = np.load(FIXTURE)
    kw, q = load(name)
    l2d, ldepth, grad = run(kw, q)
    want_grad = z[f"{name}/tracks_3d_grad"]
    assert math.isfinite(float(z[f"{name}/l2d"])) and float(z[f"{name}/ldepth"]) > 0 and np.abs(want_grad).max() > 0
    np.testing.assert_allclose(l2d, float(z[f"{name}/l2d"]), rtol=1e-12, atol=0)
    np.testing.assert_allclose(ldepth, float(z[f"{name}/ldepth"]), rtol=1e-12, atol=0)
    np.testing.assert_allclose(grad.numpy(), want_grad, rtol=1e-12, atol=1e-12 * np.abs(want_grad).max())


def test_the_clamp_is_in_the_fixture():
    kw, _ = load("b2_p7_p40")
    pz = T.elements(**kw)[3]
    assert int((pz <= 1e-6).sum()) >= 2 and int((pz > 1e-6).sum()) > 50


@pytest.mark.parametrize("name", ["n4_p65", "b2_p7_p40"])
def test_permuting_queries_with_their_targets_changes_nothing(name):
    """Each query gathers its own pixel, so the order of the queries is immaterial (sums differ by rounding only)."""
    kw, q = load(name)
    base = run(kw, q)
    g = torch.Generator().manual_seed(5)
    perm_kw = {k: list(v) if isinstance(v, list) else v for k, v in kw.items()}
    N = kw["tracks_3d"].shape[3]
    w, start = [], 0
    for b, qs in enumerate(kw["query_tracks_2d"]):
        P = qs.shape[0]
        perm = torch.randperm(P, generator=g)
        perm_kw["query_tracks_2d"][b] = qs[perm]
        for k in ("target_tracks_2d", "target_visibles", "target_track_depths"):
            perm_kw[k][b] = kw[k][b][:, perm]
        w.append(kw["track_weights"][start:start + N * P].reshape(N, P, -1)[:, perm].reshape(N * P, -1))
        start += N * P
    perm_kw["track_weights"] = torch.cat(w)
    got = run(perm_kw, q)
    np.testing.assert_allclose(got[:2], base[:2], rtol=1e-13)
    np.testing.assert_allclose(got[2].numpy(), base[2].numpy(), rtol=0, atol=1e-13 * float(base[2].abs().max()))


def test_a_weight_matrix_equals_its_row_sum():
    kw, q = load("n4_p65")
    assert kw["track_weights"].shape[1] == 4
    base = run(kw, q)
    for w in (kw["track_weights"].sum(-1), kw["track_weights"].sum(-1, keepdim=True)):
        got = run({**kw, "track_weights": w}, q)
        np.testing.assert_allclose(got[:2], base[:2], rtol=1e-14)
        np.testing.assert_allclose(got[2].numpy(), base[2].numpy(), rtol=0, atol=1e-14 * float(base[2].abs().max()))


def test_restatement_corner_cases():
    kw, q = load("width1_weights")
    none = {**kw, "target_visibles": [torch.zeros_like(v) for v in kw["target_visibles"]]}
    l2d, ldepth, grad = run(none, q)
    assert math.isnan(l2d) and ldepth == 0.0 and not grad.any()  # no visible element (the reference raises)
    assert run(none, 1.0)[:2] == (0.0, 0.0)
    # a query outside the image counts as not visible
    qs = kw["query_tracks_2d"][0].clone()
    vis = kw["target_visibles"][0].clone()
    vis[:, :2] = True
    masked = run({**kw, "target_visibles": [torch.cat([torch.zeros_like(vis[:, :2]), vis[:, 2:]], 1)]}, q)
    qs[0], qs[1] = torch.tensor([float(GEN.W), 3.0]), torch.tensor([2.0, -1.0])
    outside = run({**kw, "query_tracks_2d": [qs], "target_visibles": [vis]}, q)
    assert outside[:2] == masked[:2] and torch.equal(outside[2], masked[2])
