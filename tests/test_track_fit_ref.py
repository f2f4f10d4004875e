"""tests/track_fit_ref.py - the fp64 restatement of the warm-up's loss and loop that the GPU tests compare against - is pinned to what
the REFERENCE's own code gave (tests/golden/track_fit.npz, written by tests/golden/gen_track_fit.py): the six terms and the gradients
of a fixed mix of them at 1e-12 of each tensor's largest value, and the parameters after the reference's own run_initial_optim.  No GPU.

The trajectories are held to 1e-12 of each tensor's largest parameter change."""
import os

import numpy as np
import pytest
import torch

from tests import track_fit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("default", "general_cam", "one", "t4", "k9", "static_bases", "behind", "blind")
TRAJECTORIES = ("traj_one", "traj_small", "traj_general", "traj_ramp", "traj_ramp_k2")
SHAPES = dict(default=(333, 20, 24), general_cam=(65, 5, 8), one=(1, 1, 3), t4=(70, 3, 4), k9=(130, 9, 6), static_bases=(65, 4, 6),
              behind=(5, 2, 4), blind=(40, 3, 5))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "track_fit.npz"))


def load_case(golden, name):
    return {k: torch.tensor(golden[f"{name}/{k}"]) for k in R.LEAVES + R.DATA}


def close(a, b, tol):
    b = torch.as_tensor(b)
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_terms_and_gradients_match_the_reference(golden, name):
    case = load_case(golden, name)
    G, K, T = SHAPES[name]
    assert case["means"].shape == (G, 3) and case["motion_coefs"].shape == (G, K) and case["rots"].shape == (K, T, 6)
    assert all(v.dtype in (torch.float32, torch.bool) for v in case.values())
    detail = {}
    terms, grads = R.on_ref(case, golden["mix"], detail=detail)
    for i, t_name in enumerate(R.TERMS):
        assert abs(float(terms[i]) - float(golden[f"{name}/terms"][i])) <= 1e-12 * max(abs(float(golden[f"{name}/terms"][i])), 1e-300), t_name
    for k, g in zip(R.LEAVES, grads):
        assert close(g, golden[f"{name}/grad/{k}"], 1e-12), k
    assert float(detail["thr"]) == float(golden[f"{name}/thr"])
    assert R.gaps_ok(detail, zero_accel=name == "static_bases")  # the generator's conditions, on the stored inputs
    if name == "static_bases":  # exact zeros, not small numbers
        assert torch.equal(terms[3:], torch.zeros(3, dtype=torch.float64)) and torch.equal(torch.tensor(golden[f"{name}/terms"][3:]), torch.zeros(3, dtype=torch.float64))
    if name == "one":  # softmax of one coefficient is 1: the sparsity term and its gradient are exactly zero
        assert float(terms[2]) == 0.0 and torch.equal(grads[1], torch.zeros(1, 1, dtype=torch.float64))
    if name == "behind":
        assert float(detail["vz"][1, 0]) < 1e-5 and bool(case["invisibles"][0, 1]) and float(case["confidences"][0, 1]) > 0
    if name == "blind":
        assert not bool(case["visibles"][0].any()) and not bool(case["invisibles"][0].any())
    if name == "general_cam":
        A = case["w2cs"][1, :3, :3].double()
        assert float((A @ A.T - torch.eye(3, dtype=torch.float64)).abs().max()) > 0.05 and float(case["Ks"][0, 0, 1]) != 0.0


@pytest.mark.parametrize("name", TRAJECTORIES)
def test_the_loop_lands_where_the_references_own_loop_landed(golden, name):
    case, n = load_case(golden, name), int(golden[f"{name}/num_iters"])
    after = R.simulate(case, n)
    for k, a in zip(R.LEAVES, after):
        want = torch.tensor(golden[f"{name}/after/{k}"])
        moved = float((want - case[k].double()).abs().max())
        assert float((a - want).abs().max()) <= 1e-12 * max(moved, 1e-300) or (moved == 0.0 and torch.equal(a, want)), (k, moved)
    assert (n > 400) == name.startswith("traj_ramp")  # two cases run into the ramp of the smoothness weight, one with K > 1

