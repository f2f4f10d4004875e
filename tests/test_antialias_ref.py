"""CPU checks of the fp64 antialiased reference (tests/antialias_ref.py): the conic identity the backward folds into v_conics, the
reference's gradients, and eps2d = 0."""
import torch

from oracle import raster
from tests.antialias_ref import compensation_from_conics, compensation_from_det, rasterization
from tests.util import static_inputs


def _conics(cov2d, eps2d):
    a, b, c = cov2d[:, 0, 0] + eps2d, cov2d[:, 0, 1], cov2d[:, 1, 1] + eps2d
    det = a * c - b * b
    return torch.stack([c / det, -b / det, a / det], -1)


def _covs(n, lam1, lam2, seed):
    g = torch.Generator().manual_seed(seed)
    th = torch.rand(n, generator=g, dtype=torch.float64) * torch.pi
    c, s = torch.cos(th), torch.sin(th)
    R = torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], -2)
    L = torch.diag_embed(torch.stack([lam1, lam2], -1))
    return R @ L @ R.transpose(-1, -2)


def test_conic_identity_equals_the_determinant_ratio():
    g = torch.Generator().manual_seed(0)
    n = 4000
    for eps2d in (0.3, 0.1, 1.0):
        # random covariances, and thin ones down to a 1e8 aspect ratio
        lam1 = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(-3, 6, generator=g))
        for lam2 in (torch.exp(torch.empty(n, dtype=torch.float64).uniform_(-3, 6, generator=g)), lam1 * 1e-4, lam1 * 1e-8):
            cov = _covs(n, lam1, lam2, seed=int(1000 * eps2d))
            ref = compensation_from_det(cov, eps2d)
            got = compensation_from_conics(_conics(cov, eps2d), torch.ones(n, dtype=torch.int32), eps2d)
            assert float((got - ref).abs().max()) <= 1e-7, eps2d
            iso = cov[:, 0, 0] * 0 + lam1  # isotropic: comp = s^2 / (s^2 + eps2d)
            cov_iso = torch.diag_embed(torch.stack([iso, iso], -1))
            assert torch.allclose(compensation_from_det(cov_iso, eps2d), iso / (iso + eps2d), rtol=1e-12, atol=0)


def test_culled_and_degenerate_instances_have_zero_compensation_and_gradient():
    cov = torch.tensor([[[4.0, 2.0], [2.0, 1.0]], [[2.0, 0.0], [0.0, 3.0]]], dtype=torch.float64)  # singular, regular
    con = _conics(cov, 0.3).requires_grad_()
    comp = compensation_from_conics(con, torch.tensor([3, 0], dtype=torch.int32), 0.3)
    assert float(comp[0]) <= 1e-7 and float(comp[1]) == 0.0
    comp.sum().backward()
    assert torch.isfinite(con.grad).all() and bool((con.grad[1] == 0).all())


def test_eps2d_zero_gives_compensation_one():
    N, W, H = 60, 40, 32
    inp = static_inputs(N, W, H, seed=4, dtype=torch.float64)
    rc, ra, info = rasterization(inp["means"], inp["quats"], inp["scales"], inp["opac"], inp["colors"], inp["V"], inp["K"], W, H,
                                 eps2d=0.0)
    vis = info["radii"] > 0
    assert int(vis.sum()) > 10
    assert torch.allclose(info["compensations"][vis], torch.ones(int(vis.sum()), dtype=torch.float64), rtol=0, atol=1e-12)
    rc0, ra0, _ = raster.rasterization(inp["means"], inp["quats"], inp["scales"], inp["opac"], inp["colors"], inp["V"], inp["K"],
                                       W, H, eps2d=0.0)
    assert torch.allclose(rc, rc0, rtol=0, atol=1e-12) and torch.allclose(ra, ra0, rtol=0, atol=1e-12)


def test_antialiasing_dims_small_splats():
    N, W, H = 80, 40, 32
    inp = static_inputs(N, W, H, seed=5, dtype=torch.float64, scale_mul=0.3)
    _, ra_c, _ = raster.rasterization(inp["means"], inp["quats"], inp["scales"], inp["opac"], inp["colors"], inp["V"], inp["K"], W, H)
    _, ra_a, info = rasterization(inp["means"], inp["quats"], inp["scales"], inp["opac"], inp["colors"], inp["V"], inp["K"], W, H)
    vis = info["radii"] > 0
    comp = info["compensations"]
    assert bool((comp[vis] > 0).all() and (comp[vis] < 1).all() and (comp[~vis] == 0).all())
    assert float(ra_a.sum()) < float(ra_c.sum())


def test_reference_gradcheck():
    N, W, H = 6, 16, 16
    inp = static_inputs(N, W, H, seed=11, dtype=torch.float64, scale_mul=6.0)
    names = ("means", "quats", "scales", "opac", "colors")

    def f(*xs):
        d = dict(zip(names, xs))
        rc, ra, _ = rasterization(d["means"], d["quats"], d["scales"], d["opac"], d["colors"], inp["V"], inp["K"], W, H,
                                  background=torch.tensor([0.2, 0.5, 0.7], dtype=torch.float64), render_mode="RGB+ED")
        return rc, ra

    rc, _ = f(*[inp[k] for k in names])
    assert float(rc[..., :3].abs().sum()) > 0
    args = tuple(inp[k].clone().requires_grad_() for k in names)
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-5, rtol=1e-4)
