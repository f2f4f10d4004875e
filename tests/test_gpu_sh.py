"""GPU parity of the SH colour kernels (csrc/sh.hip) and of `rasterization(sh_degree=d)` against the fp64 restatement in
tests/sh_ref.py and the fp64 oracle rasterizer.  Norm: max|a-b| <= tol * max|ref| per tensor."""
import pytest
import torch

from oracle import raster
from tests import sh_ref
from tests.util import check, static_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STOL = 1e-5  # spherical_harmonics: no allowance
TOL, FLIPS = 1e-4, 2e-3  # the seam's tolerances (tests/test_gpu_rasterization.py)


def _inputs(lead, K, seed, masked):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(*lead, 3, generator=g, dtype=torch.float64)
    r = 0.5 + 19.5 * torch.rand(*lead, 1, generator=g, dtype=torch.float64)  # |dirs| in [0.5, 20]
    dirs = u / u.norm(dim=-1, keepdim=True) * r
    coeffs = torch.randn(*lead, K, 3, generator=g, dtype=torch.float64)
    masks = torch.rand(*lead, generator=g) > 0.3 if masked else None
    return dirs, coeffs, masks


def _run(d, dirs, coeffs, masks, w, need_dirs=True):
    from deblur4dgs_amd.sh import spherical_harmonics

    a = dirs.float().to(DEV).requires_grad_(need_dirs)
    c = coeffs.float().to(DEV).requires_grad_()
    out = spherical_harmonics(d, a, c, None if masks is None else masks.to(DEV))
    (out * w.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.cpu(), None if a.grad is None else a.grad.cpu(), c.grad.cpu()


CASES = [(d, (d + 1) ** 2, (N,)) for d in range(5) for N in (1, 63, 64, 65, 100_003)] + \
        [(2, 25, (100_003,)), (2, 16, (2, 65)), (3, 16, (2, 64)), (4, 25, (2, 1000)), (1, 7, (2, 63))]


@pytest.mark.parametrize("d,K,lead", CASES)
def test_spherical_harmonics_matches_fp64(d, K, lead):
    for masked in (False, True):
        dirs, coeffs, masks = _inputs(lead, K, seed=d * 7 + K + len(lead) + lead[-1], masked=masked)
        w = torch.randn(*lead, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        rd, rc = dirs.clone().requires_grad_(), coeffs.clone().requires_grad_()
        ref = sh_ref.spherical_harmonics(d, rd, rc, masks)
        (ref * w).sum().backward()
        out, g_dirs, g_coeffs = _run(d, dirs, coeffs, masks, w)
        case = f"SH d={d} K={K} lead={lead} masked={masked}"
        assert out.shape == (*lead, 3) and g_coeffs.shape == (*lead, K, 3)
        check(case, "colors", out, ref, STOL)
        check(case, "v_dirs", g_dirs, rd.grad, STOL)
        check(case, "v_coeffs", g_coeffs, rc.grad, STOL)
    # dirs without a gradient: the kernel skips v_p, v_coeffs is unchanged
    out2, g_dirs2, g_coeffs2 = _run(d, dirs, coeffs, masks, w, need_dirs=False)
    assert g_dirs2 is None and torch.equal(out2, out) and torch.equal(g_coeffs2, g_coeffs)


def test_unused_masked_and_degenerate_entries_are_exact_zeros():
    from deblur4dgs_amd.sh import sh_colors

    N, K, d = 300, 25, 2
    dirs, coeffs, _ = _inputs((N,), K, seed=5, masked=False)
    dirs[7] = 0.0  # zero-length direction
    masks = torch.ones(N, dtype=torch.bool)
    masks[[3, 100, 299]] = False
    w = torch.randn(N, 3, dtype=torch.float64)
    out, g_dirs, g_coeffs = _run(d, dirs, coeffs, masks, w)
    assert torch.isfinite(out).all() and torch.isfinite(g_dirs).all() and torch.isfinite(g_coeffs).all()
    assert (g_coeffs[:, (d + 1) ** 2:] == 0).all()  # coefficients above the degree
    for n in (3, 7, 100, 299):
        assert (out[n] == 0).all() and (g_dirs[n] == 0).all() and (g_coeffs[n] == 0).all()
    assert (g_coeffs[0, :(d + 1) ** 2] != 0).any()
    # the rasterization colours: a Gaussian on the camera centre gets 0.5 (0 + 0.5) and zero gradients
    V = torch.eye(4, device=DEV)
    V[:3, 3] = torch.tensor([0.5, -1.0, 2.0], device=DEV)
    means = torch.randn(N, 3, device=DEV) * 3
    means[11] = -V[:3, 3]  # campos = -R^T t
    means.requires_grad_()
    V.requires_grad_()
    c = coeffs.float().to(DEV).requires_grad_()
    rgb = sh_colors(means, V, c, d)
    rgb.sum().backward()
    torch.cuda.synchronize()
    assert (rgb[11] == 0.5).all() and (means.grad[11] == 0).all() and (c.grad[11] == 0).all()
    assert torch.isfinite(V.grad).all()


def test_backward_is_bitwise_reproducible():
    """N = 300 000: 1172 blocks, so v_origin goes through the two-level ordered sum."""
    from deblur4dgs_amd.sh import SHFn

    N, K, d = 300_000, 16, 3
    dirs, coeffs, _ = _inputs((N,), K, seed=9, masked=False)
    w = torch.randn(N, 3, dtype=torch.float64).float().to(DEV)
    origin0 = torch.tensor([0.3, -0.2, 0.1], device=DEV)
    runs = []
    for _ in range(2):
        p = dirs.float().to(DEV).requires_grad_()
        o = origin0.clone().requires_grad_()
        c = coeffs.float().to(DEV).requires_grad_()
        (SHFn.apply(d, p, o, c, None, True) * w).sum().backward()
        torch.cuda.synchronize()
        runs.append((p.grad.clone(), o.grad.clone(), c.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    v_p, v_o, _ = runs[0]
    ref = -v_p.double().sum(0)
    assert (v_o.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def _sh_inputs(N, W, H, K, seed):
    inp = static_inputs(N, W, H, seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed)
    sh = torch.randn(N, K, 3, generator=g, dtype=torch.float64) * 0.35  # strongly view-dependent colours
    sh[:, 0] = (inp.pop("colors") - 0.5) / 0.28209479177387814
    inp["sh"] = sh
    # the same image from a camera away from the origin (static_inputs' viewmat is the identity): V = [R0 t0], means in
    # world space R0^T (x - t0), so campos = -R0^T t0 != 0 and every entry of the camera-position term is exercised
    A = torch.tensor([[0.0, -0.3, 0.2], [0.3, 0.0, -0.1], [-0.2, 0.1, 0.0]], dtype=torch.float64)
    R0, t0 = torch.linalg.matrix_exp(A), torch.tensor([0.8, -0.5, 1.5], dtype=torch.float64)
    inp["means"] = (inp["means"] - t0) @ R0
    V = torch.eye(4, dtype=torch.float64)
    V[:3, :3], V[:3, 3] = R0, t0
    inp["V"] = V @ inp["V"]
    return inp


# seeds: the viewmat gradient has no flip allowance, so no scene may hold a splat whose alpha / radius decision falls the
# other way in fp32 (seed 301 at degree 0 does: 9.6e-4 on the viewmat, 2e-3 on one Gaussian's means, SH not involved)
@pytest.mark.parametrize("mode,d,K,shape,seed", [("RGB", 0, 1, "NK3", 311), ("RGB+ED", 1, 4, "1NK3", 314),
                                                 ("RGB", 3, 16, "1NK3", 346), ("RGB+ED", 4, 25, "NK3", 365),
                                                 ("RGB+ED", 3, 25, "NK3", 355)])
def test_rasterization_sh_matches_oracle(mode, d, K, shape, seed):
    N, W, H = 1500, 96, 64
    sh_parity(_sh_inputs(N, W, H, K, seed=seed), mode, d, K, shape, N, W, H)


def sh_parity(inp, mode, d, K, shape, N, W, H, tag=""):
    """The body of the test above on given inputs (tests/test_gpu_camera_general.py runs it under a camera whose K is general too)."""
    from deblur4dgs_amd.rasterization import rasterization

    bg = torch.tensor([0.2, 0.5, 0.8], dtype=torch.float64)
    # reference: the projection's viewmat and the camera centre's are separate leaves, so the test can check that the
    # camera-position term is a sizeable part of the viewmat gradient
    t = {k: v.clone().requires_grad_(k != "K") for k, v in inp.items()}
    Vc = inp["V"].clone().requires_grad_()
    colors = torch.clamp_min(sh_ref.spherical_harmonics(d, t["means"] - sh_ref.campos(Vc), t["sh"]) + 0.5, 0.0)
    ref_c, ref_a, ref_info = raster.rasterization(t["means"], t["quats"], t["scales"], t["opac"], colors, t["V"], t["K"],
                                                  W, H, background=bg, render_mode=mode)
    gw = torch.Generator().manual_seed(9)
    w_c = torch.randn(ref_c.shape, generator=gw, dtype=torch.float64)
    w_a = torch.randn(ref_a.shape, generator=gw, dtype=torch.float64)
    ref_info["means2d"].retain_grad()
    ((ref_c * w_c).sum() + (ref_a * w_a).sum()).backward()
    v_campos_term = torch.zeros_like(inp["V"]) if Vc.grad is None else Vc.grad  # None at degree 0 (view-independent)
    ref_V = t["V"].grad + v_campos_term

    g = {k: v.float().to(DEV) for k, v in inp.items()}
    if shape == "1NK3":
        g["sh"] = g["sh"][None].clone()
    for k in ("means", "quats", "scales", "opac", "sh", "V"):
        g[k].requires_grad_()
    rc, ra, info = rasterization(g["means"], g["quats"], g["scales"], g["opac"], g["sh"], g["V"][None], g["K"][None], W, H,
                                 sh_degree=d, backgrounds=bg.float().to(DEV)[None], render_mode=mode)
    info["means2d"].retain_grad()
    ((rc[0] * w_c.float().to(DEV)).sum() + (ra[0] * w_a.float().to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    case = f"S1 sh_degree={d} K={K} {shape} {mode} N={N} {W}x{H}{tag}"
    check(case, "render_colors", rc[0].cpu(), ref_c, TOL, FLIPS)
    check(case, "render_alphas", ra[0].cpu(), ref_a, TOL, FLIPS)
    check(case, "means2d.grad", info["means2d"].grad[0].cpu(), ref_info["means2d"].grad, TOL, FLIPS)
    for name in ("means", "quats", "scales", "opac"):
        check(case, name, g[name].grad.cpu(), t[name].grad, TOL, FLIPS)
    check(case, "sh", g["sh"].grad.cpu().reshape(N, K, 3), t["sh"].grad, TOL, FLIPS)
    check(case, "viewmat 4x4", g["V"].grad.cpu(), ref_V, TOL, 0.0)
    if d > 0:
        # the camera-position term on its own (it is small beside the projection's): v_rgb from a run with the colours
        # precomputed (bitwise the same values), pushed through the SH colours alone
        from deblur4dgs_amd.sh import sh_colors

        rgb = sh_colors(g["means"], g["V"], g["sh"].reshape(N, K, 3), d).detach().requires_grad_()
        rc2, ra2, _ = rasterization(g["means"], g["quats"], g["scales"], g["opac"], rgb, g["V"][None], g["K"][None], W, H,
                                    backgrounds=bg.float().to(DEV)[None], render_mode=mode)
        assert torch.equal(rc2, rc) and torch.equal(ra2, ra)
        ((rc2[0] * w_c.float().to(DEV)).sum() + (ra2[0] * w_a.float().to(DEV)).sum()).backward()
        V2 = g["V"].detach().clone().requires_grad_()
        sh_colors(g["means"].detach(), V2, g["sh"].detach().reshape(N, K, 3), d).backward(rgb.grad)
        torch.cuda.synchronize()
        assert v_campos_term[3].abs().max() > 0  # the bottom row carries gradient
        check(case, "viewmat campos term", V2.grad.cpu(), v_campos_term, TOL, 0.0)


def test_rasterization_sh_is_bitwise_reproducible():
    from deblur4dgs_amd.rasterization import rasterization

    N, W, H, K = 2000, 96, 64, 16
    inp = {k: v.float().to(DEV) for k, v in _sh_inputs(N, W, H, K, seed=5).items()}
    runs = []
    for _ in range(2):
        t = {k: v.clone().requires_grad_(k != "K") for k, v in inp.items()}
        rc, ra, info = rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["sh"], t["V"][None], t["K"][None],
                                     W, H, sh_degree=3, backgrounds=torch.ones(1, 3, device=DEV), render_mode="RGB+ED")
        (rc.square().sum() + ra.sum()).backward()
        torch.cuda.synchronize()
        runs.append([rc.detach().clone(), ra.detach().clone()] + [t[k].grad.clone() for k in ("means", "quats", "scales",
                                                                                             "opac", "sh", "V")])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
