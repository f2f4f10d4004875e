"""CPU: the fp64 absgrad reference (tests/absgrad_ref.py) that tests/test_gpu_absgrad.py measures the kernels against."""
import math

import torch

from oracle import raster
from tests.absgrad_ref import absgrad_of_composite, absgrad_of_rasterization
from tests.util import static_inputs


def _oracle_grad(inp, W, H, w_c, w_a, bg, mode):
    t = {k: v.clone().requires_grad_(k != "K") for k, v in inp.items()}
    rc, ra, info = raster.rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"], t["K"], W, H,
                                        background=bg, render_mode=mode)
    info["means2d"].retain_grad()
    loss = (rc * w_c).sum() + ((ra * w_a).sum() if w_a is not None else 0.0)
    loss.backward()
    return info["means2d"].grad


def test_signed_sum_is_the_oracles_means2d_grad():
    for mode, with_va, with_bg, D in (("RGB", True, True, 3), ("RGB+ED", True, False, 2), ("RGB+D", False, True, 4)):
        N, W, H = 250, 40, 36
        inp = static_inputs(N, W, H, seed=5 + D, dtype=torch.float64, D=D)
        bg = torch.linspace(0.2, 0.7, D, dtype=torch.float64) if with_bg else None
        g = torch.Generator().manual_seed(D)
        w_c = torch.randn(H, W, D + (mode != "RGB"), generator=g, dtype=torch.float64)
        w_a = torch.randn(H, W, 1, generator=g, dtype=torch.float64) if with_va else None
        absg, sgn, _ = absgrad_of_rasterization(inp["means"], inp["quats"], inp["scales"], inp["opac"], inp["colors"], inp["V"],
                                                inp["K"], W, H, w_c, w_a, bg, mode)
        ref = _oracle_grad(inp, W, H, w_c, w_a, bg, mode)
        den = float(ref.abs().max())
        assert den > 0
        assert float((sgn - ref).abs().max()) <= 1e-12 * den, mode
        # absgrad bounds the gradient elementwise, and is strictly larger where the pixels disagree in sign
        assert bool((absg >= ref.abs() - 1e-12 * den).all()), mode
        assert float((absg - ref.abs()).max()) > 1e-3 * den, mode


def test_one_splat_closed_form():
    W = H = 32
    m = torch.tensor([[13.3, 17.8]], dtype=torch.float64)
    a, b, c = 0.05, 0.012, 0.08
    conic = torch.tensor([[a, b, c]], dtype=torch.float64)
    col = torch.tensor([[0.7]], dtype=torch.float64)
    op = torch.tensor([0.8], dtype=torch.float64)
    ids = torch.zeros(4, dtype=torch.int64)
    offs = torch.tensor([0, 1, 2, 3, 4])
    v = torch.ones(H, W, 1, dtype=torch.float64)
    absg, sgn = absgrad_of_composite(m, conic, col, op, W, H, ids, offs, v)
    # pixel p: L_p = col * alpha_p, alpha_p = o exp(-sigma_p); dL_p / dm = -col alpha_p (a dx + b dy, b dx + c dy), dx = m - p
    py, px = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    dx, dy = m[0, 0] - px, m[0, 1] - py
    sig = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
    al = op[0] * torch.exp(-sig)
    on = (sig >= 0) & (al >= 1 / 255)
    gx = torch.where(on, -col[0, 0] * al * (a * dx + b * dy), torch.zeros_like(al))
    gy = torch.where(on, -col[0, 0] * al * (b * dx + c * dy), torch.zeros_like(al))
    want = torch.stack([gx.abs().sum(), gy.abs().sum()])
    assert torch.allclose(absg[0], want, rtol=1e-12, atol=0)
    assert torch.allclose(sgn[0], torch.stack([gx.sum(), gy.sum()]), rtol=1e-10, atol=1e-14)


def test_mirror_symmetric_scene_has_zero_grad_and_positive_absgrad():
    """An isotropic splat centred between pixel centres of a symmetric image, a uniform loss weight: the pixels' pulls cancel."""
    W = H = 32
    m = torch.tensor([[16.0, 16.0]], dtype=torch.float64)
    conic = torch.tensor([[0.06, 0.0, 0.06]], dtype=torch.float64)
    col = torch.tensor([[0.5, 0.25]], dtype=torch.float64)
    op = torch.tensor([0.9], dtype=torch.float64)
    ids = torch.zeros(4, dtype=torch.int64)
    offs = torch.tensor([0, 1, 2, 3, 4])
    v = torch.ones(H, W, 2, dtype=torch.float64)
    va = torch.full((H, W, 1), 0.3, dtype=torch.float64)
    absg, sgn = absgrad_of_composite(m, conic, col, op, W, H, ids, offs, v, va, background=torch.tensor([0.1, 0.2], dtype=torch.float64))
    assert float(sgn.abs().max()) < 1e-12
    assert float(absg.min()) > 1e-2
    assert math.isclose(float(absg[0, 0]), float(absg[0, 1]), rel_tol=1e-12)  # and symmetric under x <-> y
