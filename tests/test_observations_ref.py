"""tests/observations_ref.py - the NumPy / float64 statement of the observations stage in this repository's own words - reproduces
tests/golden/observations.npz, which tests/golden/gen_observations.py records from the reference's own functions: the median bit for
bit, every flag equal, float outputs to 1e-12.  No GPU needed; the GPU tests hold the kernels to both."""
import os

import numpy as np
import pytest

import observations_ref as R
from deblur4dgs_amd import observations as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observations.npz")
MEDIAN = ("small", "odd", "tile", "past", "all", "none", "p30", "p70", "half", "batch", "k3", "k5", "k15", "negative")
LIFT = ("n1", "n63", "n64", "n65", "n1000", "integers", "quantile")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def case(golden, prefix):
    return {k[len(prefix) + 1:]: v for k, v in golden.items() if k.startswith(prefix + "/")}


def close(a, b, tol=1e-12):
    return float(np.abs(np.asarray(a, np.float64) - b).max(initial=0.0)) <= tol * max(1.0, float(np.abs(b).max(initial=0.0)))


def test_the_fixture_holds_every_case(golden):
    assert {k.split("/")[1] for k in golden if k.startswith("median/")} == set(MEDIAN)
    assert {k.split("/")[1] for k in golden if k.startswith("lift/")} == set(LIFT)
    for name in LIFT:  # 1 - 3 % of the draws are replaced; never more than 10 %
        c = case(golden, f"lift/{name}")
        assert 0 <= int(c["redrawn"]) <= 0.1 * c["tracks_2d"].shape[0] * c["tracks_2d"].shape[1], name


@pytest.mark.parametrize("name", MEDIAN)
def test_median_is_the_reference_bit_for_bit(golden, name):
    c = case(golden, f"median/{name}")
    out = R.masked_median_blur(c["image"], c["mask"].astype(np.float32), int(c["k"]))
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), c["out"].view(np.uint32))
    if name == "none":
        lo, hi = min(c["image"].min(), 0), max(c["image"].max(), 0)
        assert set(np.unique(out)) <= {np.float32(lo), np.float32(hi)} and len(np.unique(out)) == 2


def test_median_per_image_restarts_the_chain(golden):
    c = case(golden, "median/batch")
    mask = c["mask"].astype(np.float32)
    per = R.masked_median_blur(c["image"], mask, 11, per_image=True)
    for i in range(3):
        assert np.array_equal(per[i], R.masked_median_blur(c["image"][i:i + 1], mask[i:i + 1], 11)[0])
    assert not np.array_equal(per, R.masked_median_blur(c["image"], mask, 11))  # the carried parity and the shared lo / hi show


def test_tapir_flags(golden):
    c = case(golden, "tapir")
    visible, invisible, conf = R.parse_tapir_track_info(c["occ"].astype(np.float64), c["dist"].astype(np.float64))
    assert np.array_equal(visible, c["visible"]) and np.array_equal(invisible, c["invisible"]) and close(conf, c["confidence"])
    assert visible.any() and invisible.any() and (~visible & ~invisible).any()


@pytest.mark.parametrize("name", LIFT)
def test_lifting_reproduces_the_reference(golden, name):
    c = case(golden, f"lift/{name}")
    q = int(c["query"])
    got = R.lift_tracks(q, c["img"], c["tracks_2d"], c["depths"], c["masks"], c["inv_Ks"], c["c2ws"])
    for k in ("visibles", "invisibles", "in_mask"):
        assert np.array_equal(got[k], c[k]), k
    for k in ("xyz", "colors", "confidences"):
        assert close(got[k], c[k]), k
    T = c["tracks_2d"].shape[1]
    valid = got["in_mask"][:, q] & (got["visible_count"] >= R.quantile_threshold(got["visible_count"], T))
    assert np.array_equal(valid, c["valid"])
    # the package's threshold from the histogram is the same number
    assert O.visible_count_threshold(got["hist"].tolist(), T) == pytest.approx(R.quantile_threshold(got["visible_count"], T), abs=1e-5)
    assert got["hist"].sum() == len(valid) and (got["hist"] * np.arange(T + 1)).sum() == got["visibles"].sum()


def test_the_cases_cover_what_they_claim(golden):
    c = case(golden, "lift/n1000")
    x, y = c["tracks_2d"][..., 0], c["tracks_2d"][..., 1]
    assert (x < 0).any() and (x > 31).any() and (y < 0).any() and (y > 23).any() and not c["masks"][4].any() and not c["in_mask"][:, 4].any()
    c = case(golden, "lift/integers")
    xy = c["tracks_2d"][:, 0, :2]
    assert np.array_equal(xy, np.round(xy)) and c["in_mask"][:, 0].any() and not c["in_mask"][:, 0].all()
    c = case(golden, "lift/quantile")
    assert 0 < c["valid"].sum() < c["in_mask"][:, int(c["query"])].sum()  # the visible-count rule drops tracks of its own


@pytest.mark.parametrize("name", ("flat", "rough"))
def test_points_and_normals(golden, name):
    c = case(golden, f"normals/{name}")
    H, W = c["depth"].shape
    pts, normals, keep = R.bkgd_dense(c["depth"], np.zeros((H, W)), np.ones((H, W)), np.linalg.inv(c["K"].astype(np.float64)),
                                      np.linalg.inv(c["w2c"].astype(np.float64)))
    assert close(pts, c["points"]) and close(normals, c["normals"]) and keep.all()
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert not c["normals"][border].any() and np.allclose(np.linalg.norm(c["normals"][~border], axis=-1), 1.0)
