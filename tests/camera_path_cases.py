"""Inputs and the fp64 reference of the camera-path Jacobian tests, shared by the CPU test (tests/test_camera_path_cases.py) and the
GPU tests (tests/test_gpu_camera_jacobian.py) so that both see the same numbers.  Not a conftest: plain functions, cached.  Imports no
product code.

THE INPUTS.  A case is the pair of `MoveModel` head outputs `d0, d1 = [tau, phi]` (six numbers each) and a sub-sample count S.  Every
value is rounded to fp32 before either side sees it, so the kernel and the reference differentiate at the same point.

THE FAMILIES, each at every scale s of SCALES (base0, base1 are two fixed directions in general position):
  a  all six components of both heads scaled:      d0 = s base0,                        d1 = s base1
  b  tau fixed, phi scaled:                        d0 = [0.05 tau0, s phi0],            d1 = [0.05 tau1, s phi1]
  c  phi fixed, tau scaled:                        d0 = [s tau0, 0.05 phi0],            d1 = [s tau1, 0.05 phi1]
  d  equal heads (the relative rotation is exactly zero: so3_log of the slerp sits on its series branch):   d1 = d0 = s base0
  e1, e2  nearly equal heads:                      d0 = 1e-3 base0 (e1) or 0.3 base0 (e2), d1 = d0 + s base1
  f0, f1  one head exactly zero:                   d0 = 0, d1 = s base1 (f0);           d0 = s base0, d1 = 0 (f1)

THE SCALES run from the zero-initialised heads (exactly 0) through the first thousands of training steps (1e-7 .. 1e-2) to trained
heads (0.1, 0.5), plus the two scales S_BELOW / S_ABOVE that put |phi0|^2 of the scaled families 1e-4 (relative) below and above
SERIES_T2, the theta^2 at which csrc/camera.hip's left_jacobian / left_jacobian_inv coefficients change from their series to their
closed form.  No case is left out for lying near a guard: both sides of every guard have to be accurate there.

THE BLOCKS.  jac [S,12,12] is d RTs[s].flatten()[i] / d [d0, d1][j].  Rows i % 4 != 3 are rotation entries, i % 4 == 3 the translation
column; columns j % 6 < 3 are d tau, j % 6 >= 3 d phi.  The four (rows x columns) blocks differ by orders of magnitude in size (for small
heads the rotation rows depend on phi only through tau: |block| ~ |tau| beside blocks of size 1), so each is judged against its own
maximum, see `block_tol`.

THE REFERENCE.  oracle.camera's fp64 chain se3_to_SE3(SE3_log(linear_interpolation(se3_exp(d0), se3_exp(d1), linspace(0, 1, S)))) and
its torch.autograd.functional.jacobian.  The oracle keeps its own guards (theta^2 > 1e-12).  Its closed forms cancel too, with fp64's
rounding: just above its guard the derivative of (1 - cos th) / th^2 carries ~ 1e-16 / th^3 absolute, which enters the rotation-rows /
d phi block multiplied by |phi| |tau|.  Measured against the same chain with long series below theta^2 = 1e-2, over this table at S = 11:
at worst 5.4e-8 on the block of size 5.7e-3 of family b at s = 2e-6 (1e-5 of the block, 4 % of its tolerance), 1.6e-8 at s = 1e-5, below
1e-9 everywhere else, and below 1e-11 on the other three blocks.

WHAT IS ZERO BY CONSTRUCTION.  At u = 0 and u = 1 the path returns the heads themselves (left_jacobian_inv(phi) left_jacobian(phi) tau
= tau), so the rotation rows do not depend on phi there: with S = 2, and with equal heads at any S, the rotation-rows / d phi block is
zero up to the reference's own error (5.4e-8 at most, above); `rot_dphi_is_structural_zero` names those cases.  Everywhere else it is, to first order,
u (1 - u) / 2 [d phi] x (tau0 - tau1): up to |tau1 - tau0| / 8, and non-zero wherever the two tau differ.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

BASE0 = (0.31, -0.52, 0.77, 0.43, -0.61, 0.29)
BASE1 = (-0.45, 0.38, 0.66, -0.35, 0.72, 0.51)
SERIES_T2 = 1e-2  # csrc/camera.hip: left_jacobian / left_jacobian_inv switch series -> closed form at theta^2 > SERIES_T2
_PHI0_SQ = sum(v * v for v in BASE0[3:])
S_BELOW = math.sqrt(SERIES_T2 / _PHI0_SQ) * (1 - 1e-4)
S_ABOVE = math.sqrt(SERIES_T2 / _PHI0_SQ) * (1 + 1e-4)
SCALES = (0.0, 1e-7, 1e-6, 2e-6, 1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 0.1, S_BELOW, S_ABOVE, 0.5)
FAMILIES = ("a", "b", "c", "d", "e1", "e2", "f0", "f1")
S_ALL = (2, 11)  # every case
# one case (s = EXTRA_SCALE) of families a and b: the launch is 12 threads per sub-sample in blocks of 64 - S = 6 is the first count that
# needs two blocks, 16 fills three whole ones, 32 six; linspace's split s < S / 2 wants odd and even S
S_EXTRA = (3, 6, 16, 32)
EXTRA_SCALE = 1e-3
EPS32 = 2.0 ** -23
FLOOR = 8 * EPS32  # the fp32 rounding floor of a block, in units of max|J_ref| (see block_tol)

ROT_ROWS = np.array([i % 4 != 3 for i in range(12)])
TAU_COLS = np.array([j % 6 < 3 for j in range(12)])
BLOCKS = {"rot/dtau": (ROT_ROWS, TAU_COLS), "rot/dphi": (ROT_ROWS, ~TAU_COLS), "trans/dtau": (~ROT_ROWS, TAU_COLS),
          "trans/dphi": (~ROT_ROWS, ~TAU_COLS)}


def heads(family: str, s: float) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (d0, d1), fp32 [6] each."""
    b0, b1 = torch.tensor(BASE0, dtype=torch.float64), torch.tensor(BASE1, dtype=torch.float64)
    tau = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    phi = 1.0 - tau
    if family == "a":
        d0, d1 = s * b0, s * b1
    elif family == "b":
        d0, d1 = (0.05 * tau + s * phi) * b0, (0.05 * tau + s * phi) * b1
    elif family == "c":
        d0, d1 = (s * tau + 0.05 * phi) * b0, (s * tau + 0.05 * phi) * b1
    elif family == "d":
        d0 = d1 = s * b0
    elif family in ("e1", "e2"):
        d0 = (1e-3 if family == "e1" else 0.3) * b0
        # d1 is the fp32 sum of the fp32 d0 and the fp32 step: what a head that moved by s base1 holds
        return d0.float(), d0.float() + (s * b1).float()
    elif family == "f0":
        d0, d1 = 0.0 * b0, s * b1
    else:
        assert family == "f1", family
        d0, d1 = s * b0, 0.0 * b1
    return d0.float(), d1.float()


def _table():
    keys = [(fam, s, S) for fam in FAMILIES for s in SCALES for S in S_ALL]
    keys += [(fam, EXTRA_SCALE, S) for fam in ("a", "b") for S in S_EXTRA]
    assert len(set(keys)) == len(keys)
    return tuple(keys)


KEYS = _table()


def case_id(key) -> str:
    fam, s, S = key
    tag = "below" if s == S_BELOW else "above" if s == S_ABOVE else f"{s:g}"
    return f"{fam}-s{tag}-S{S}"


IDS = [case_id(k) for k in KEYS]


def path(d: torch.Tensor, S: int) -> torch.Tensor:
    """[12] = [d0, d1] -> RTs [S,3,4], in d's dtype, through the oracle."""
    from oracle import camera

    P0, P1 = camera.se3_exp(d[None, :6]), camera.se3_exp(d[None, 6:])
    u = torch.linspace(0, 1, S, dtype=d.dtype)
    return camera.se3_to_SE3(camera.SE3_log(camera.linear_interpolation(P0, P1, u)))[0]


@functools.lru_cache(maxsize=None)
def reference(family: str, s: float, S: int) -> dict:
    """Treat as read-only (cached).  d0, d1 fp32 [6]; RTs fp64 [S,3,4]; jac fp64 [S,12,12]."""
    d0, d1 = heads(family, s)
    d = torch.cat([d0, d1]).double()
    RTs = path(d, S)
    jac = torch.autograd.functional.jacobian(lambda x: path(x, S), d, vectorize=True).reshape(S, 12, 12)
    return dict(d0=d0, d1=d1, S=S, RTs=RTs, jac=jac)


def block(jac, name: str):
    """The entries of one of the four blocks of jac [S,12,12] (tensor or array) -> [S, rows, cols]."""
    rows, cols = BLOCKS[name]
    j = jac.detach().double().cpu().numpy() if torch.is_tensor(jac) else np.asarray(jac, np.float64)
    return j[:, rows][:, :, cols]


def block_tol(jac_ref, name: str) -> float:
    """1e-4 of the block's own maximum (the project's relative figure, per block) plus the fp32 rounding floor FLOOR * max|J_ref|: a block
    can be structurally tiny (8e-8 in family e1) while its entries are differences of O(max|J|) terms."""
    j = jac_ref.detach().double().cpu().numpy() if torch.is_tensor(jac_ref) else np.asarray(jac_ref, np.float64)
    return 1e-4 * float(np.abs(block(j, name)).max()) + FLOOR * float(np.abs(j).max())


def rot_dphi_is_structural_zero(family: str, s: float, S: int) -> bool:
    d0, d1 = heads(family, s)
    return S == 2 or bool((d0 == d1).all())
