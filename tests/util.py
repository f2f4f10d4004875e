import os

import numpy as np
import torch


def rel_err(a, b):
    """max|a-b| / max|b|  (the parity norm of SURVEY.md section 7 'Hard parts')."""
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    den = max(np.abs(b).max(), 1e-30)
    return float(np.abs(a - b).max() / den)


def frac_bad(a, b, tol):
    """fraction of elements whose error exceeds tol*max|b| (isolated discrete-decision flips)."""
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    den = max(np.abs(b).max(), 1e-30)
    return float((np.abs(a - b) > tol * den).mean())


def static_inputs(N, W, H, seed, dtype=torch.float32, scale_mul=3.0, D=3):
    from deblur4dgs_amd.synth import make_scene

    sc = make_scene(N, 0, 1, 1, W, H, seed, dtype=torch.float64, D=D)
    out = dict(means=sc["means"], quats=sc["quats"], scales=torch.exp(sc["scales"]) * scale_mul,
               opac=torch.sigmoid(sc["opacities"]), colors=torch.sigmoid(sc["colors"]), V=sc["viewmat"], K=sc["K"])
    return {k: v.to(dtype) for k, v in out.items()}


# ---- parity log ---------------------------------------------------------------------------------------------
# Every GPU parity test records the error it ACHIEVED (not just pass / fail) for each tensor it compares; conftest.py
# writes the table to gpurun_out/parity_table.{json,md} at the end of the session (committed under profiles/).
PARITY_LOG: list[dict] = []


def record(case: str, tensor: str, got, ref):
    """-> (rel_err, frac_bad at 1e-4) of `got` against `ref` (norm: max|a-b| / max|ref|), logged."""
    r = rel_err(got, ref)
    b4 = frac_bad(got, ref, 1e-4)
    n = int(np.prod(ref.shape)) if hasattr(ref, "shape") else 1
    PARITY_LOG.append(dict(case=case, tensor=tensor, n=n, rel_err=r, frac_bad_1e4=b4, frac_bad_1e3=frac_bad(got, ref, 1e-3)))
    return r, b4


def check(case: str, tensor: str, got, ref, tol: float = 1e-4, flips: float = 0.0):
    """Record the achieved error and assert: at most a fraction `flips` of the elements may differ from the fp64
    oracle by more than tol * max|ref| (flips > 0 only where one discrete decision - alpha >= 1/255, T <= 1e-4,
    ceil(radius) - taken differently in fp32 moves an element; the table in profiles/ shows the measured numbers)."""
    r, _ = record(case, tensor, got, ref)
    bad = frac_bad(got, ref, tol)
    PARITY_LOG[-1].update(asserted_tol=tol, asserted_flips=flips)
    if os.environ.get("D4GS_PARITY_MEASURE"):  # measurement run: log everything, judge afterwards
        return r
    assert bad <= flips, f"{case} / {tensor}: {bad:.2e} of the elements off by > {tol:g} x max|ref| (max err {r:.2e})"
    return r


def check_columns(case: str, tensor: str, got, ref, tol: float = 1e-4):
    """Like `check` with no allowance, but normalised per COLUMN (last axis; a 1-D tensor is one column): every element of column c
    within tol * max|ref[..., c]|.  A per-tensor norm lets a small column hide beside a large one (an expected-depth channel of 2 - 10
    scene units beside colours in (0, 1); a small gradient column beside a large one).  Each column is logged through `record`."""
    g = got.detach().double().cpu() if torch.is_tensor(got) else torch.as_tensor(np.asarray(got, np.float64))
    r = ref.detach().double().cpu() if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref, np.float64))
    assert g.shape == r.shape, (case, tensor, tuple(g.shape), tuple(r.shape))
    ncol = r.shape[-1] if r.dim() > 1 else 1
    g, r = g.reshape(-1, ncol), r.reshape(-1, ncol)
    worst = []
    for c in range(ncol):
        err, _ = record(case, f"{tensor}[..., {c}]" if ncol > 1 else tensor, g[:, c], r[:, c])
        PARITY_LOG[-1].update(asserted_tol=tol, asserted_flips=0.0, norm="per column")
        worst.append(err)
    if os.environ.get("D4GS_PARITY_MEASURE"):
        return max(worst)
    bad = [(c, f"{e:.2e}") for c, e in enumerate(worst) if not e <= tol]
    assert not bad, f"{case} / {tensor}: columns off by > {tol:g} x max|ref[..., c]|: {bad}"
    return max(worst)
