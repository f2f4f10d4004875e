"""CPU: the case table of the camera-path Jacobian tests (tests/camera_path_cases.py) is what it claims to be, and its fp64 reference is
usable at every case: finite, and with a rotation-rows / d phi block - the one the small-angle coefficients of csrc/camera.hip feed - that
is really there wherever the construction says so (and really zero where the construction says that)."""
import numpy as np
import pytest
import torch

from tests import camera_path_cases as cc


def test_the_table_covers_every_family_scale_and_count():
    assert {k[0] for k in cc.KEYS} == set(cc.FAMILIES)
    for fam in cc.FAMILIES:
        for S in cc.S_ALL:
            assert {k[1] for k in cc.KEYS if k[0] == fam and k[2] == S} == set(cc.SCALES), (fam, S)
    assert {0, 1e-7, 1e-6, 2e-6, 1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 0.1, 0.5} <= set(cc.SCALES)
    for fam in ("a", "b"):
        assert {k[2] for k in cc.KEYS if k[0] == fam} == set(cc.S_ALL) | {3, 6, 16, 32}
    assert len(set(cc.IDS)) == len(cc.IDS) == len(cc.KEYS)


def test_the_two_threshold_scales_straddle_the_switch_in_fp32_and_fp64():
    """|phi0|^2 of the scaled families lies 2e-4 (relative) on either side of SERIES_T2: three orders above the rounding of an fp32 dot
    product of three terms, so the kernel takes the same side as this table says."""
    for fam in ("a", "b", "d", "f1"):
        for s, above in ((cc.S_BELOW, False), (cc.S_ABOVE, True)):
            phi = cc.heads(fam, s)[0][3:]
            t2_64 = float((phi.double() ** 2).sum())
            t2_32 = float((phi * phi).sum())
            for t2 in (t2_64, t2_32):
                assert (t2 > cc.SERIES_T2) == above, (fam, s, t2)
                assert 1e-4 < abs(t2 / cc.SERIES_T2 - 1) < 4e-4, (fam, s, t2)
    assert np.float32(cc.SERIES_T2) == np.float32(1e-2)


def test_heads_are_what_the_families_say():
    b0, b1 = torch.tensor(cc.BASE0, dtype=torch.float64), torch.tensor(cc.BASE1, dtype=torch.float64)
    for s in cc.SCALES:
        d0, d1 = cc.heads("b", s)
        assert torch.equal(d0[:3], (0.05 * b0[:3]).float()) and torch.equal(d1[3:], (s * b1[3:]).float())
        d0, d1 = cc.heads("c", s)
        assert torch.equal(d0[3:], (0.05 * b0[3:]).float()) and torch.equal(d1[:3], (s * b1[:3]).float())
        d0, d1 = cc.heads("d", s)
        assert torch.equal(d0, d1) and d0.dtype == torch.float32
        for fam, base in (("e1", 1e-3), ("e2", 0.3)):
            d0, d1 = cc.heads(fam, s)
            assert torch.equal(d0, (base * b0).float())
            assert torch.equal(d1, d0 + (s * b1).float())  # the fp32 sum: a step below half an ulp of d0 vanishes, as in a real head
        assert float(cc.heads("f0", s)[0].abs().max()) == 0 and float(cc.heads("f1", s)[1].abs().max()) == 0
        if s > 0:
            assert float(cc.heads("f0", s)[1].abs().min()) > 0 and float(cc.heads("f1", s)[0].abs().min()) > 0


@pytest.mark.parametrize("key", cc.KEYS, ids=cc.IDS)
def test_reference_is_finite_and_its_rotation_dphi_block_is_there(key):
    r = cc.reference(*key)
    fam, s, S = key
    assert r["RTs"].shape == (S, 3, 4) and r["jac"].shape == (S, 12, 12)
    assert r["RTs"].dtype == r["jac"].dtype == torch.float64 and r["d0"].dtype == r["d1"].dtype == torch.float32
    assert bool(torch.isfinite(r["RTs"]).all()) and bool(torch.isfinite(r["jac"]).all())
    rot_dphi = float(np.abs(cc.block(r["jac"], "rot/dphi")).max())
    dtau = float((r["d1"].double()[:3] - r["d0"].double()[:3]).abs().max())
    if cc.rot_dphi_is_structural_zero(*key):
        # what is left is the fp64 chain's own cancellation just above its 1e-12 guards (camera_path_cases.py, THE REFERENCE): a tenth of
        # the rounding floor the GPU test grants such a block
        assert rot_dphi <= 1e-7 <= 0.11 * cc.FLOOR, rot_dphi
    elif dtau > 0:
        assert rot_dphi > 0.02 * dtau, (rot_dphi, dtau)  # ~ |tau1 - tau0| / 8
    # the other three blocks: d rotation / d tau and d translation / d phi are ~ identity-sized, never zero
    assert float(np.abs(cc.block(r["jac"], "rot/dtau")).max()) > 0.3
    assert float(np.abs(cc.block(r["jac"], "trans/dphi")).max()) > 0.3


def test_block_tolerance_is_the_stated_formula():
    r = cc.reference("e1", 1e-6, 11)
    j = r["jac"].numpy()
    for name, (rows, cols) in cc.BLOCKS.items():
        blk = j[:, rows][:, :, cols]
        assert blk.shape == (11, int(rows.sum()), int(cols.sum()))
        assert cc.block_tol(r["jac"], name) == 1e-4 * np.abs(blk).max() + 8 * 2.0 ** -23 * np.abs(j).max()
    assert int(cc.ROT_ROWS.sum()) == 9 and int(cc.TAU_COLS.sum()) == 6
