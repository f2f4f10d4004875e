"""tests/metrics_ref.py (the project's own words, fp64) against tests/golden/metrics.npz (the reference's own mPSNR and mSSIM in
fp32, recorded by tests/golden/gen_metrics.py).  No GPU.

The reference runs in fp32, so the bound is its own error: the generator measured max |reference_fp32 - restatement_fp64| over the
committed cases per image kind (`ref_gap_ssim/<kind>` absolute, `ref_gap_sse_rel/<kind>` relative) and this test allows ten times
that, for other BLAS / conv builds of torch.  Where pred == target or the mask is zero both must be exact: SSIM 1, SSE 0."""
import os
import re

import numpy as np
import pytest
import torch

from tests import metrics_ref as R
from tests.metrics_cases import CASES, HERE, IMAGES, MASKS, SHAPES, bounds, check_against_fixture, load_case, load_golden


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def test_the_fixture_holds_the_cases_of_the_issue(golden):
    for B, H, W in SHAPES:
        sname = f"{B}x{H}x{W}"
        for k in ("uniform/pred", "uniform/target", "flat/pred", "flat/target"):
            assert golden[f"{sname}/{k}"].shape == (B, H, W, 3) and golden[f"{sname}/{k}"].dtype == np.float32
        flat = golden[f"{sname}/flat/target"]
        assert 0.9 <= flat.min() and flat.max() <= 0.9021 and np.abs(golden[f"{sname}/flat/pred"] - 0.901).max() <= 0.0261
        masks = {m: golden[f"{sname}/mask/{m}"] for m in MASKS[1:]}
        assert all(v.shape == (B, H, W) and v.dtype == np.float32 for v in masks.values())
        assert masks["ones"].all() and not masks["zero"].any() and set(np.unique(masks["dyadic"])) == {0.0, 0.5, 1.0}
        assert 0.55 < masks["bernoulli"].mean() < 0.85 and set(np.unique(masks["bernoulli"])) == {0.0, 1.0}
        rows = torch.tensor(masks["rows"])
        cnt_x = rows.unfold(2, 11, 1).sum(-1)
        assert bool((cnt_x == 0).any()) and bool(((cnt_x != 0).float().unfold(1, 11, 1).sum(-1) > 0).all())  # empty along x, never along y
        if H >= 26 and W >= 26:  # the hole holds whole 11x11 windows
            blob = torch.tensor(masks["blob"])
            assert bool((blob.unfold(1, 11, 1).unfold(2, 11, 1).sum((-1, -2)) == 0).any()) and blob.sum() > 0
    assert float(golden["ref_gap_ssim"]) == max(float(golden[f"ref_gap_ssim/{k}"]) for k in IMAGES)
    assert float(golden["ref_gap_sse_rel"]) == max(float(golden[f"ref_gap_sse_rel/{k}"]) for k in IMAGES)
    assert float(golden["ref_gap_ssim/same"]) == 0.0 and 0 < float(golden["ref_gap_ssim/uniform"]) < 1e-5 and float(golden["ref_gap_ssim"]) < 1e-4
    assert 0 < float(golden["ref_gap_sse_rel"]) < 1e-6  # fp32 eps territory: the reference's error, not a free tolerance


def test_the_window_is_the_one_shared_by_the_kernels():
    text = open(os.path.join(HERE, "..", "deblur4dgs_amd", "csrc", "common.h")).read()
    body = text[text.index("#define D4GS_SSIM_WINDOW"):].split("}")[0]
    taps = [float(v) for v in re.findall(r"\d\.\d+", body)]
    assert len(taps) == 11 and float((R.window() - torch.tensor(taps, dtype=torch.float64)).abs().max()) <= 2.0 ** -52
    for f, n in (("photometric.hip", "PW"), ("metrics.hip", "MW")):  # one statement of the eleven numbers, used by both
        assert f"c_wind[{n}] = D4GS_SSIM_WINDOW;" in open(os.path.join(HERE, "..", "deblur4dgs_amd", "csrc", f)).read(), f


@pytest.mark.parametrize("sname,kind,mk", CASES, ids=["-".join(c) for c in CASES])
def test_restatement_matches_the_reference(golden, sname, kind, mk):
    pred, target, mask = load_case(golden, sname, kind, mk)
    sse, msum, ssim = R.masked_image_metrics(pred, target, mask)
    check_against_fixture(golden, f"{sname}/{kind}/{mk}", kind, sse[0], msum[0], ssim[0], exact=kind == "same" or mk == "zero")
    psnr, ref = float(R.psnr(sse.sum(), torch.trunc(msum.sum()) * 3)), float(golden[f"{sname}/{kind}/{mk}/psnr"])
    if mk == "zero":
        assert np.isnan(psnr) and np.isnan(ref)
    elif kind == "same":
        assert psnr == ref == float("inf")
    else:
        assert abs(psnr - ref) <= 1e-5 * abs(ref)  # the reference's fp32 quotient and logarithm: a few 1e-7 of 8..40 dB


def test_validator_masks_and_the_update_sequence(golden):
    pred, target, _ = load_case(golden, "1x64x48", "uniform", "none")
    valid, fg = torch.tensor(golden["validator/valid_mask"]), torch.tensor(golden["validator/fg_mask"])
    sse, msum, ssim = R.masked_image_metrics(pred, target, torch.stack((valid, fg * valid, (1 - fg) * valid)))
    for i, key in enumerate(("main", "fg", "bg")):
        check_against_fixture(golden, f"validator/{key}", "uniform", sse[i], msum[i], ssim[i], exact=False)
    assert float(msum[1] + msum[2]) == float(msum[0]) and float(msum[1]) > 0 and float(msum[2]) > 0
    psnrs, ssims = [], []
    for step in golden["sequence/steps"]:
        s = R.masked_image_metrics(*load_case(golden, *str(step).split("/")))
        psnrs.append(R.psnr(s[0].sum(), torch.trunc(s[1].sum()) * 3))
        ssims.append(s[2][0])
    assert abs(float(torch.stack(psnrs).mean()) - float(golden["sequence/psnr"])) <= 1e-5 * float(golden["sequence/psnr"])
    assert len(torch.cat(ssims)) == 4 and abs(float(torch.cat(ssims).mean()) - float(golden["sequence/ssim"])) <= bounds(golden, "flat")[0]
