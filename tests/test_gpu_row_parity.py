"""Every Gaussian's gradient held to its OWN scale (tests/util.check_rows) on the scenes of tests/row_cases.py: the rasterization seam on
four random scenes and the hand-built strata, the fused exposure path on one scene per k_project_bwd instantiation.

The tensor norm of `check` (max|got - ref| / max|ref|) lets a defect confined to a subpopulation - sub-pixel splats, needles, splats beyond
the image or the Jacobian clamp, faint ones, the static rows, the ragged last group - hide beside the few large rows that set max|ref|.
Here, with the cotangents zeroed on the fragile pixels of oracle/margins.py on every side, per tensor and per named group:
  caps        the share of live rows off by more than 1e-4 / 1e-3 / 1e-2 of their own max|ref| is at most 10 % / 1 % / 0.5 %;
  yardstick   over all rows, the median and 90 % quantile of the row errors are at most 4 x those of the same oracle evaluated in fp32;
  dead rows   rows culled on both sides are exactly zero;
  backstop    every element within 1e-4 of the tensor's maximum (`check`, no allowance) - the ill-conditioned rows;
  colours     under positive cotangents nothing cancels in a colour row: EVERY live row within 1e-4 of itself;
  projection  (seam S1) means2d, conics, depths and opacities per row, so that a miss is placed before or after the projection.
Every measured figure is logged through `check_rows` into the session's parity table (tests/conftest.py), device and fp32 oracle side by
side, with the case's name, cotangent kind and row group; profiles/row_parity.json is that table's per-row entries."""
import pytest
import torch

from tests import row_cases as rc
from tests.util import check, check_rows, row_errors

pytestmark = pytest.mark.gpu
# (case, kind, tensor) -> yardstick ratio where the measured one exceeds 4 for a named cause; none so far
RATIO = {}


def _note(entry, **kw):
    entry.update(kw)  # the entry IS the parity log's: the table then says which case, kind and group a row statement is about


def _judge(name, kind, tensor, got, g64, g32, groups, dead):
    """One per-Gaussian gradient: all rows against the yardstick, every named group against the caps, the tensor norm as the backstop."""
    case = f"rows {name} {kind}"
    e = check_rows(case, tensor, got, g64, yard=g32, dead=dead, ratio=RATIO.get((name, kind, tensor), 4.0))
    _note(e, name=name, kind=kind, group="all")
    for gname, idx in groups.items():
        e = check_rows(f"{case} [{gname}]", tensor, got[idx], g64[idx], yard=g32[idx], dead=None if dead is None else dead[idx], ratio=None)
        _note(e, name=name, kind=kind, group=gname)
    check(case, tensor, got, g64, 1e-4, 0.0)
    if tensor == "colors" and kind == "positive":
        r, _ = row_errors(got, g64)
        assert r.max() <= 1e-4, f"{case} / colors: a colour row off by {r.max():.2e} of its own maximum under positive cotangents"


@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("name", rc.S1_CASES)
def test_rasterization_rows(name, kind):
    from tests.test_gpu_rasterization import _run_gpu

    case, ref = rc.s1_case(name), rc.s1_reference(name)
    assert float(ref["F"].float().mean()) <= rc.MAX_FRAGILE
    W, H, N = case["W"], case["H"], case["N"]
    rcol, ralpha, info, tg = _run_gpu(case["inp"], W, H, case["mode"], case["bg"], requires_grad=True)
    dev = rcol.device
    w_c, w_a = ref["cot"][kind]
    ((rcol[0] * w_c.float().to(dev)).sum() + (ralpha[0] * w_a.float().to(dev)).sum()).backward()
    torch.cuda.synchronize()
    radii = info["radii"].reshape(N).cpu()
    p64, p32 = ref["proj64"], ref["proj32"]
    dead = (radii == 0) & (p64["radii"] == 0)
    if kind == rc.KINDS[0]:  # the projection's own outputs, on rows visible on both sides (the same for either cotangent)
        both = (radii > 0) & (p64["radii"] > 0) & (p32["radii"] > 0)
        assert int(both.sum()) >= 0.9 * int((p64["radii"] > 0).sum())
        for t in rc.PROJ_TENSORS:
            got = info[t].detach().reshape(N, -1).cpu()
            e = check_rows(f"rows {name} projection", t, got[both], p64[t].reshape(N, -1)[both], yard=p32[t].reshape(N, -1)[both])
            _note(e, name=name, kind="-", group="visible on both sides")
    for t in rc.S1_TENSORS:
        _judge(name, kind, t, tg[t].grad.cpu(), ref["g64"][kind][t], ref["g32"][kind][t], case["groups"], dead)


@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("name", tuple(rc.FUSED))
def test_exposure_rows(name, kind):
    from deblur4dgs_amd.exposure import render_exposure

    case, ref = rc.fused_case(name), rc.fused_reference(name)
    assert float(ref["F"].float().mean()) <= rc.MAX_FRAGILE
    sc, N, G, W, H = case["sc"], case["N"], case["G"], case["W"], case["H"]
    dev = torch.device("cuda:0")
    L = {k: sc[k].float().to(dev).requires_grad_() for k in rc.FUSED_TENSORS}
    # (the shared leaves take gradients as in training - the backward then runs its whole epilogue - but have no rows to judge)
    fixed = {k: sc[k].float().to(dev).requires_grad_(k != "K") for k in ("rots", "transls", "times", "RTs", "viewmat", "K")}
    cols, bgc = L["colors"], torch.ones(3, device=dev)
    if case["mask"]:
        mk = torch.zeros(N, 1, device=dev)
        mk[:G] = 1.0
        cols, bgc = torch.cat([cols, mk], -1), torch.cat([bgc, torch.zeros(1, device=dev)])
    res = render_exposure(L["means"], L["quats"], L["scales"], L["opacities"], cols, 3, L["motion_coefs"], fixed["rots"], fixed["transls"],
                          fixed["times"], fixed["RTs"], fixed["viewmat"], fixed["K"], W, H, background=bgc, return_depth=True)
    w_b, w_a = ref["cot"][kind]
    assert res["blended"].shape == w_b.shape
    ((res["blended"] * w_b.float().to(dev)).sum() + (res["acc"] * w_a.float().to(dev)).sum()).backward()
    torch.cuda.synchronize()
    dead = (res["radii"].reshape(case["S"], N).cpu() == 0).all(0) & (ref["radii64"] == 0).all(0)
    for t in rc.FUSED_TENSORS:
        rows_dead = dead[:G] if t == "motion_coefs" else dead
        _judge(name, kind, t, L[t].grad.cpu(), ref["g64"][kind][t], ref["g32"][kind][t], rc.tensor_groups(case, t), rows_dead)
