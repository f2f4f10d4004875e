"""The cases of tests/golden/metrics.npz (tests/golden/gen_metrics.py) and how a result is held against the reference's recorded one:
shared by tests/test_metrics_ref.py (the fp64 restatement, CPU) and tests/test_gpu_metrics.py (the kernels)."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((1, 11, 11), (1, 26, 26), (2, 27, 38), (1, 43, 27), (1, 64, 48))
IMAGES = ("uniform", "flat", "same")
MASKS = ("none", "ones", "zero", "blob", "rows", "bernoulli", "dyadic")
CASES = [("x".join(map(str, s)), k, m) for s in SHAPES for k in IMAGES for m in MASKS]


def load_golden():
    return np.load(os.path.join(HERE, "golden", "metrics.npz"))


def load_case(golden, sname, kind, mk, device="cpu"):
    """-> pred, target [B,H,W,3] and the mask [B,H,W] or None, fp32"""
    src = "uniform" if kind == "same" else kind
    pred = torch.tensor(golden[f"{sname}/{src}/pred"], device=device)
    target = pred.clone() if kind == "same" else torch.tensor(golden[f"{sname}/{kind}/target"], device=device)
    return pred, target, (None if mk == "none" else torch.tensor(golden[f"{sname}/mask/{mk}"], device=device))


def bounds(golden, kind):
    """(SSIM absolute, SSE relative): ten times the reference's measured fp32 gap for this kind of image"""
    return 10 * float(golden[f"ref_gap_ssim/{kind}"]), 10 * float(golden[f"ref_gap_sse_rel/{kind}"])


def check_against_fixture(golden, name, kind, sse, msum, ssim, exact):
    """sse, msum [B], ssim [B] (fp64, any device) against the recorded update of the reference"""
    b_ssim, b_sse = bounds(golden, kind)
    ref_sse, ref_ssim = float(golden[f"{name}/sse"]), torch.tensor(golden[f"{name}/ssim"], dtype=torch.float64)
    got_sse, got_ssim = float(sse.sum()), ssim.detach().cpu().double()
    assert int(golden[f"{name}/total"]) == int(torch.trunc(msum.sum())) * 3, name
    if exact:
        assert got_sse == 0.0 == ref_sse and bool((got_ssim == 1).all()) and bool((ref_ssim == 1).all()), name
        return 0.0, 0.0
    e_ssim, e_sse = float((got_ssim - ref_ssim).abs().max()), abs(got_sse - ref_sse) / ref_sse
    assert e_ssim <= b_ssim, f"{name}: SSIM off by {e_ssim:.3e}, bound {b_ssim:.3e}"
    assert e_sse <= b_sse, f"{name}: SSE off by {e_sse:.3e} relative, bound {b_sse:.3e}"
    return e_ssim, e_sse
