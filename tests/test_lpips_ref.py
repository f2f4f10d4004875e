"""tests/lpips_ref.py, the fp64 statement of the LPIPS metric that the kernels of csrc/lpips.hip are held to, reproduces every array
that tests/golden/lpips.npz records of the reference's own PNetLin and mLPIPS run in float64: to fp64 rounding (rtol 1e-12; the
convolutions are the same torch calls on the same weights, everything behind them is restated).  No GPU."""
import numpy as np
import pytest
import torch

from tests import lpips_ref as R

RTOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def trunk():
    return R.seeded_trunk()


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)) if want.size else 0.0
    print(f"{what}: max error / max value {err:.2e}")
    assert err <= RTOL, (what, err)


def test_the_seeded_trunk_matches_its_checksum(fx, trunk):
    assert R.checksum(trunk) == list(fx["trunk_checksum"])
    assert [tuple(fx[f"lin{k}"].shape) for k in range(5)] == [(c,) for c in R.CHANNELS]
    assert all(fx[f"lin{k}"].dtype == np.float32 and (fx[f"lin{k}"] >= 0).all() for k in range(5))
    assert 0 < float(fx["ref_gap_map"]) < 1e-5 and 0 < float(fx["ref_gap_mean"]) < 1e-5  # fp32 against fp64: a few 2^-24, no more


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_name)
def test_alex_sizes_equal_the_recorded_map_shapes(fx, shape):
    from deblur4dgs_amd.lpips import alex_sizes

    B, H, W = shape
    recorded = tuple(tuple(fx[f"{R.shape_name(shape)}/uniform/layer{k}"].shape[1:]) for k in range(5))
    assert alex_sizes(H, W) == R.alex_sizes(H, W) == recorded
    assert alex_sizes(288, 512) == ((71, 127), (35, 63), (17, 31), (17, 31), (17, 31))
    for bad in ((30, 64), (64, 30)):
        with pytest.raises(ValueError, match="31"):
            alex_sizes(*bad)


@pytest.mark.parametrize("kind", R.IMAGES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_name)
def test_both_forms_and_the_layer_maps(fx, trunk, shape, kind):
    sname = R.shape_name(shape)
    p, t = R.images_of(fx, sname, kind)
    maps = R.layer_maps_of(p, t, trunk, R.head_weights(fx), normalize=True)
    for k, m in enumerate(maps):
        close(m, fx[f"{sname}/{kind}/layer{k}"], f"{sname}/{kind}/layer{k}")
    close(R.score_map(maps, shape[1], shape[2]), fx[f"{sname}/{kind}/map"], f"{sname}/{kind}/map")
    close(R.mean_score(maps), fx[f"{sname}/{kind}/mean"], f"{sname}/{kind}/mean")
    if kind == "same":
        assert all(float(m.abs().max()) == 0.0 for m in maps)


@pytest.mark.parametrize("kind", R.IMAGES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_name)
def test_the_entries_of_one_update_under_every_mask(fx, trunk, shape, kind):
    sname = R.shape_name(shape)
    p, t = R.images_of(fx, sname, kind)
    for mk in R.MASKS:
        s, total = R.masked_sums(p, t, R.mask_of(fx, sname, mk), trunk, R.head_weights(fx))
        close(s, fx[f"{sname}/{kind}/{mk}/sum"], f"{sname}/{kind}/{mk}/sum")
        assert int(total) == int(fx[f"{sname}/{kind}/{mk}/total"]) and total.dtype == torch.int64
    dyadic = R.mask_of(fx, sname, "dyadic")
    assert int(fx[f"{sname}/{kind}/dyadic/total"]) == int(float(dyadic.sum()))  # the truncated sum of a fractional mask


def test_the_validator_masks_and_the_three_update_sequence(fx, trunk):
    sname = R.shape_name(R.VALIDATOR_SHAPE)
    p, t = R.images_of(fx, sname, "uniform")
    for key, m in R.validator_masks(fx)[2].items():
        s, total = R.masked_sums(p, t, m, trunk, R.head_weights(fx))
        close(s, fx[f"validator/{key}/sum"], f"validator/{key}/sum")
        assert int(total) == int(fx[f"validator/{key}/total"])
    sums, totals = [], []
    for step in fx["sequence/steps"]:
        sname, kind, mk = str(step).split("/")
        s, total = R.masked_sums(*R.images_of(fx, sname, kind), R.mask_of(fx, sname, mk), trunk, R.head_weights(fx))
        sums.append(s), totals.append(total)
    close(torch.stack(sums), fx["sequence/sums"], "sequence/sums")
    assert [int(v) for v in totals] == [int(v) for v in fx["sequence/totals"]]
    close((torch.stack(sums) / torch.stack(totals)).mean(), fx["sequence/compute"], "sequence/compute")
