"""tests/motion_ref.py (the project's own words) against tests/golden/motion_regs.npz (the reference's own functions, recorded by
tests/golden/gen_motion_regs.py): values and gradients to 1e-12 relative, exact zeros included.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import motion_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
LEAVES = ("means", "motion_coefs", "rots", "transls", "scales")
TERMS = ("smooth_bases", "smooth_tracks", "z_accel", "scale_var")
MIX = (1.3, 0.7, 2.1, 0.9)
CASES = ("default_small", "block_edges", "one", "many_times", "static_bases", "linear_rows")
SHAPES = {"default_small": (333, 20, 24, 1), "block_edges": (65, 5, 8, 3), "one": (1, 1, 3, 1), "many_times": (130, 12, 12, 5),
          "static_bases": (70, 5, 6, 2), "linear_rows": (40, 3, 7, 1)}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "motion_regs.npz"))


def load_case(golden, name, dtype=torch.float64, device="cpu"):
    """-> dict of the seven inputs (leaves require a gradient)"""
    c = {k: torch.tensor(golden[f"{name}/{k}"], dtype=dtype, device=device) for k in LEAVES + ("ts", "w2cs")}
    for k in LEAVES:
        c[k].requires_grad_()
    return c


def call(fn, c, **kw):
    return fn(c["means"], c["motion_coefs"], c["rots"], c["transls"], c["scales"], c["ts"], c["w2cs"], **kw)


def close(got, ref, what):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    err, den = float((got.detach().double() - ref).abs().max()), float(ref.abs().max())
    assert err <= 1e-12 * den, f"{what}: max error {err:.3e} against max|ref| {den:.3e}"


def test_the_fixture_holds_the_cases_of_the_issue(golden):
    for name, (G, K, T, B) in SHAPES.items():
        assert golden[f"{name}/means"].shape == (G, 3) and golden[f"{name}/motion_coefs"].shape == (G, K)
        assert golden[f"{name}/rots"].shape == (K, T, 6) and golden[f"{name}/transls"].shape == (K, T, 3)
        assert golden[f"{name}/ts"].shape == (B,) and golden[f"{name}/w2cs"].shape == (B, 4, 4)
        assert all(golden[f"{name}/{k}"].dtype == np.float32 for k in LEAVES + ("ts", "w2cs"))
    assert list(golden["block_edges/ts"]) == [0.0, 3.0, 7.0] and list(golden["many_times/ts"]) == [1.0, 1.0, np.float32(4.37), 10.0, 6.0]
    A = golden["block_edges/w2cs"][:, :3, :3].astype(np.float64)
    off = [np.abs(a @ a.T - np.eye(3)).max() for a in A]
    assert off[0] < 1e-6 and off[2] < 1e-6 and off[1] > 0.05  # one camera is not orthonormal


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_values_and_gradients(golden, name):
    c = load_case(golden, name)
    terms = call(M.motion_regularizers, c)
    for t_name, t in zip(TERMS, terms):
        close(t, golden[f"{name}/{t_name}"], f"{name} {t_name}")
    grads = torch.autograd.grad(sum(w * t for w, t in zip(MIX, terms)), [c[k] for k in LEAVES], retain_graph=True)
    for k, g in zip(LEAVES, grads):
        assert torch.isfinite(g).all()
        close(g, golden[f"{name}/grad/{k}"], f"{name} grad {k}")
    if name == "block_edges":  # each term on its own
        for t_name, t in zip(TERMS, terms):
            own = torch.autograd.grad(t, [c[k] for k in LEAVES], retain_graph=True, allow_unused=True)
            for k, g in zip(LEAVES, own):
                close(torch.zeros_like(c[k]) if g is None else g, golden[f"{name}/grad_{t_name}/{k}"], f"{name} grad of {t_name} wrt {k}")


def test_static_bases_give_exact_zeros(golden):
    c = load_case(golden, "static_bases")
    terms = call(M.motion_regularizers, c)
    assert all(float(golden[f"static_bases/{t}"]) == 0.0 for t in TERMS[:3]) and float(golden["static_bases/scale_var"]) > 0
    assert all(float(t.detach()) == 0.0 for t in terms[:3])
    grads = torch.autograd.grad(sum(w * t for w, t in zip(MIX, terms)), [c[k] for k in LEAVES])
    for k, g in zip(LEAVES, grads):
        assert (k == "scales") != bool((g == 0).all()), k
        assert not np.any(golden[f"static_bases/grad/{k}"]) or k == "scales"


def test_linear_rows_have_zero_norm_inside_a_nonzero_loss(golden):
    c = load_case(golden, "linear_rows")
    ar, at = M.accel_norms(c["rots"]).detach(), M.accel_norms(c["transls"]).detach()
    assert float(at[0, 1]) == 0.0 and float(ar[1, 2]) == 0.0  # (basis 0, frame 2) of transls, (basis 1, frame 3) of rots
    assert int((ar == 0).sum()) == 1 and int((at == 0).sum()) == 1 and float(golden["linear_rows/smooth_bases"]) > 1
    # in fp32 too: the rows are midpoints of dyadic rationals
    r32, t32 = torch.tensor(golden["linear_rows/rots"]), torch.tensor(golden["linear_rows/transls"])
    assert float(M.accel_norms(t32)[0, 1]) == 0.0 and float(M.accel_norms(r32)[1, 2]) == 0.0
    sb = call(M.motion_regularizers, c)[0]
    g_r, g_t = torch.autograd.grad(sb, [c["rots"], c["transls"]])
    assert torch.isfinite(g_r).all() and torch.isfinite(g_t).all()


def test_weights_scale_the_two_halves_of_smooth_bases(golden):
    c = load_case(golden, "block_edges")
    a = call(M.motion_regularizers, c, weight_rot=1.0, weight_transl=0.0)[0]
    b = call(M.motion_regularizers, c, weight_rot=0.0, weight_transl=1.0)[0]
    close(a + 2.0 * b, golden["block_edges/smooth_bases"], "defaults 1, 2")
