"""CPU checks of the SH colour model: the fp64 restatement in tests/sh_ref.py (orthonormal basis, gsplat's factored forms,
autograd), the closed-form camera centre's gradient, and the argument validation of the d4gs_sh_* C entry points (done
before any HIP call, so no GPU is needed)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import sh_ref


def _unit(n, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def test_basis_is_orthonormal_on_the_sphere():
    """Gauss-Legendre in cos(theta) x uniform phi integrates the products (polynomials of degree <= 8) exactly."""
    zs, wz = np.polynomial.legendre.leggauss(12)
    M = 24
    phi = 2 * math.pi * np.arange(M) / M
    z, ph = np.meshgrid(zs, phi, indexing="ij")
    s = np.sqrt(1 - z * z)
    u = torch.tensor(np.stack([s * np.cos(ph), s * np.sin(ph), z], -1).reshape(-1, 3))
    w = torch.tensor(np.repeat(wz, M) * (2 * math.pi / M))
    Y = sh_ref.basis(4, u)  # [P, 25]
    G = (Y * w[:, None]).T @ Y
    assert (G - torch.eye(25, dtype=torch.float64)).abs().max().item() < 1e-12


def test_factored_forms_match_the_table():
    """gsplat's kernel evaluates some functions in factored forms that agree with the table on unit vectors."""
    u = _unit(1000, 1)
    Y = sh_ref.basis(4, u)
    z = u[:, 2]
    assert torch.allclose(Y[:, 6], 0.9461746957575601 * z * z - 0.3153915652525201, rtol=0, atol=1e-14)
    assert torch.allclose(Y[:, 20], 1.984313483298443 * z * Y[:, 12] - 1.006230589874905 * Y[:, 6], rtol=0, atol=1e-14)


def test_restatement_gradcheck():
    g = torch.Generator().manual_seed(3)
    N, K = 6, 25
    means = (torch.randn(N, 3, generator=g, dtype=torch.float64) * 2).requires_grad_()
    coeffs = (torch.randn(N, K, 3, generator=g, dtype=torch.float64) * 0.2).requires_grad_()
    V = torch.eye(4, dtype=torch.float64)
    V[:3, :3] = torch.linalg.matrix_exp(torch.tensor([[0, -0.3, 0.2], [0.3, 0, -0.1], [-0.2, 0.1, 0]], dtype=torch.float64))
    V[:3, 3] = torch.tensor([0.4, -0.2, 3.0], dtype=torch.float64)
    V.requires_grad_()
    for d in range(5):
        assert torch.autograd.gradcheck(lambda m, v, c: sh_ref.sh_colors(m, v, c, d), (means, V, coeffs))
        assert torch.autograd.gradcheck(lambda m, c: sh_ref.spherical_harmonics(d, m, c), (means, coeffs))


def test_campos_closed_form_gradient_equals_inverse():
    """deblur4dgs_amd.sh.CamPosFn (-R^T t, no torch.inverse) against torch.inverse(V)[:3, 3]: value and the full 4x4
    gradient, bottom row included."""
    from deblur4dgs_amd.sh import CamPosFn

    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        A = torch.randn(3, 3, generator=g, dtype=torch.float64)
        V = torch.eye(4, dtype=torch.float64)
        V[:3, :3] = torch.linalg.matrix_exp(A - A.T)
        V[:3, 3] = torch.randn(3, generator=g, dtype=torch.float64) * 3
        v = torch.randn(3, generator=g, dtype=torch.float64)
        a = V.clone().requires_grad_()
        b = V.clone().requires_grad_()
        ca, cb = CamPosFn.apply(a), sh_ref.campos(b)
        assert torch.allclose(ca, cb, rtol=0, atol=1e-13)
        (ca * v).sum().backward()
        (cb * v).sum().backward()
        assert (a.grad - b.grad).abs().max().item() < 1e-13
        assert b.grad[3].abs().max().item() > 1e-3  # the bottom row carries gradient


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L
    from deblur4dgs_amd import build

    build.build()
    return L.lib()


def test_sh_entry_points_validate_arguments_before_any_hip_call(lib):
    fake = C.c_void_p(0x10000)  # never dereferenced: every case fails validation first
    null = C.c_void_p(0)
    assert lib.d4gs_sh_partials_elems(0) == 0
    assert lib.d4gs_sh_partials_elems(1) == 3 and lib.d4gs_sh_partials_elems(257) == 6
    assert lib.d4gs_sh_partials_elems(4 << 20) == 3 * (4 << 20) // 256

    def fwd(N=8, K=16, deg=3, p=fake, coeffs=fake, rgb=fake):
        return lib.d4gs_sh_fwd(N, K, deg, p, null, coeffs, null, 1, rgb, null)

    def bwd(N=8, K=16, deg=3, p=fake, origin=fake, coeffs=fake, v_rgb=fake, v_origin=null, partials=fake):
        return lib.d4gs_sh_bwd(N, K, deg, p, origin, coeffs, null, 1, v_rgb, fake, fake, v_origin, partials, null)

    cases = [
        (lambda: fwd(N=-1), b"N < 0"), (lambda: fwd(deg=5), b"degree"), (lambda: fwd(deg=-1), b"degree"),
        (lambda: fwd(K=15), b"K=15"), (lambda: fwd(deg=4, K=24), b"K=24"), (lambda: fwd(p=null), b"NULL"),
        (lambda: fwd(coeffs=null), b"NULL"), (lambda: fwd(rgb=null), b"NULL"),
        (lambda: bwd(N=-5), b"N < 0"), (lambda: bwd(deg=7), b"degree"), (lambda: bwd(K=3, deg=1), b"K=3"),
        (lambda: bwd(p=null), b"NULL"), (lambda: bwd(coeffs=null), b"NULL"), (lambda: bwd(v_rgb=null), b"NULL"),
        (lambda: bwd(v_origin=fake, partials=null), b"partials"), (lambda: bwd(v_origin=fake, origin=null), b"origin"),
    ]
    for call, word in cases:
        assert call() == -1  # D4GS_EINVAL
        assert word in lib.d4gs_last_error(), lib.d4gs_last_error()


def test_rasterization_rejects_bad_sh_arguments():
    """The seam validates the SH arguments before touching the device (CPU tensors suffice to reach the checks)."""
    from deblur4dgs_amd.rasterization import rasterization

    N = 4
    means, quats, scales, opac = torch.zeros(N, 3), torch.zeros(N, 4), torch.zeros(N, 3), torch.zeros(N)
    V, K = torch.eye(4)[None], torch.eye(3)[None]
    for d, colors, word in ((5, torch.zeros(N, 36, 3), "sh_degree"), (2, torch.zeros(N, 8, 3), "K >= 9"),
                            (1, torch.zeros(N, 4, 4), "colors"), (1, torch.zeros(2, N, 4, 3), "C == 1"),
                            (0, torch.zeros(N, 3), "colors")):
        with pytest.raises(ValueError, match=word):
            rasterization(means, quats, scales, opac, colors, V, K, 16, 16, sh_degree=d)
    with pytest.raises(NotImplementedError):
        rasterization(means, quats, scales, opac, torch.zeros(N, 4, 3), V, K, 16, 16, sh_degree=1, packed=True)
