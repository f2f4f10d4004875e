"""Test-time pose refinement on the device (csrc/pose_refine.hip, deblur4dgs_amd/pose_refine.py):
  1. d4gs_pose_bwd against fp64 autograd of the oracle's projection with respect to w2c and the camera deltas, at every dispatch
     edge, and against what d4gs_project_bwd leaves for the same cotangents;
  2. bitwise: two calls, and the eager loop against the loop replayed from a HIP graph;
  3. RenderCfg.pose_only / SceneModel.pose_only: no scene parameter is differentiated, W.grad equals the full backward's;
  4. refine_pose against the oracle's loop in fp64, by the fp32 oracle loop's own deviation;
  5. recovery from an intersection-list overflow inside the graph."""
import ctypes as C
import json
import os

import pytest
import torch

from deblur4dgs_amd import _lib as L
from deblur4dgs_amd import engine
from deblur4dgs_amd.synth import make_scene
from oracle import deform, raster
from tests import pose_refine_ref as R
from tests.camera_cases import PROBES, apply_camera
from tests.util import check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, T = 64, 48, 8
LEAF_KEYS = ("means", "quats", "scales", "opacities", "colors")


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
def _scene(N, G, K, S, camera, seed):
    sc = make_scene(N, G, max(K, 1), S, W, H, seed=seed, dtype=torch.float64, T=T, cam_jitter=0.03)
    sc["scales"] = sc["scales"] + 1.2  # Gaussians big enough to overlap several pixels
    w, h = W, H
    if N >= 8 * PROBES:  # (the clamp probes need room; the one-lane and sub-wave scenes keep the rotated camera)
        sc, w, h = apply_camera(sc, "general", w, h)
        if camera == "rolled":
            sc, w, h = apply_camera(sc, "rolled", w, h, check=False)  # cameras compose: the general camera, a quarter turn on
    else:
        sc, w, h = apply_camera(sc, "rotated", w, h, check=False)
    return sc, w, h


def _oracle_projection(sc, N, G, S, w, h, with_rts):
    """fp64: per sub-sample (radii, means2d, depths, conics) as differentiable functions of w2c and RTs."""
    leaf = lambda t: t.double().clone().requires_grad_()
    w2c = leaf(sc["viewmat"])
    RTs = leaf(sc["RTs"]) if with_rts else None
    fg = {k: sc[k][:G].double() for k in LEAF_KEYS} if G else None
    bg = {k: sc[k][G:].double() for k in LEAF_KEYS} if G < N else None
    if G:
        fg["motion_coefs"] = sc["motion_coefs"].double()
        bases = {k: sc[k].double() for k in ("rots", "transls")}
    scales = deform.act_scales(sc["scales"].double())
    outs = []
    for s in range(S):
        if G:
            m, q = deform.compute_poses_all(sc["times"][s:s + 1].double(), fg, bases, bg)
            m, q = m[:, 0], q[:, 0]
        else:
            m, q = sc["means"].double(), deform.act_quats(sc["quats"].double())
        if with_rts:
            m = deform.camera_delta(m, RTs[s])
        outs.append(raster.project(m, q, scales, w2c, sc["K"].double(), w, h))
    radii = torch.stack([o[0] for o in outs])
    return w2c, RTs, radii, [torch.stack([o[i] for o in outs]) for i in (1, 3, 2)]  # means2d, conics, depths


def _device_projection(sc, N, G, K, S, w, h, with_rts, antialiased):
    cfg = engine.RenderCfg(N=N, G=G, K=K if G else 0, T=T if G else 0, S=S, D=3, width=w, height=h, flags=L.RAW_PARAMS | L.RAW_COLORS,
                           n_sigmoid=3, antialiased=antialiased, lazy_sort=False, exact_tiles=False)
    mv = lambda k: sc[k].float().to(DEV)
    dyn = [mv(k) if G else None for k in ("motion_coefs", "rots", "transls", "times")]
    st = engine.State(cfg)
    with torch.no_grad():
        engine.ProjectFn.apply(st, *[mv(k) for k in LEAF_KEYS], *dyn, mv("RTs") if with_rts else None, mv("viewmat"), mv("K"))
    return cfg, st


def _pose_bwd(cfg, st, cot, want_rts):
    lib, dims = L.lib(), cfg.dims()
    f32 = dict(dtype=torch.float32, device=DEV)
    v_view = torch.full((4, 4), float("nan"), **f32)
    v_rts = torch.full((cfg.S, 3, 4), float("nan"), **f32) if want_rts else None
    n = lib.d4gs_pose_bwd_partials_elems(C.byref(dims))
    partials = torch.full((n,), float("nan"), **f32)
    L.check(lib.d4gs_pose_bwd(C.byref(dims), C.byref(L.fill(L.ProjIn(), **st.proj_in)), C.byref(L.fill(L.ProjOut(), **st.proj_out)),
                              *[L.vp(c) for c in cot], L.vp(v_view), L.vp(v_rts), L.vp(partials), L.stream_of(v_view)), "d4gs_pose_bwd")
    return v_view, v_rts


def _project_bwd(cfg, st, cot):
    lib, dims = L.lib(), cfg.dims()
    g = engine._leaf_grads(cfg, dims, st.proj_in, DEV, with_partials=True)
    zeros = [torch.zeros_like(st.proj_out[k]) for k in ("opac_act", "ctab")]
    L.check(lib.d4gs_project_bwd(C.byref(dims), C.byref(L.fill(L.ProjIn(), **st.proj_in)), C.byref(L.fill(L.ProjOut(), **st.proj_out)),
                                 *[L.vp(c) for c in cot], *[L.vp(z) for z in zeros], C.byref(L.fill(L.LeafGrads(), **g)),
                                 L.stream_of(zeros[0])), "d4gs_project_bwd")
    return g["v_viewmat"], g["v_RTs"]


COMBOS = {  # S, G as a share of N, K, camera, antialiased, camera deltas given
    "static": (1, 0.0, 1, "general", False, True),
    "half-dynamic": (3, 0.5, 9, "rolled", True, True),
    "all-dynamic": (3, 1.0, 1, "general", False, False),
    "one-sample": (1, 0.5, 9, "rolled", True, False),
}


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])  # one lane; wave and block edges; several blocks, a ragged tail
def test_pose_bwd_matches_fp64_autograd_and_project_bwd(N, combo):
    S, share, K, camera, antialiased, with_rts = COMBOS[combo]
    G = int(round(share * N)) if N > 1 else (N if share == 1.0 else 0)
    case = f"pose_bwd N={N} {combo}"
    sc, w, h = _scene(N, G, K, S, camera, seed=100 + N)
    w2c, RTs, radii_ref, ref_out = _oracle_projection(sc, N, G, S, w, h, with_rts)
    cfg, st = _device_projection(sc, N, G, K, S, w, h, with_rts, antialiased)
    # visibility is an input: an instance enters the comparison where both sides kept it (its cotangents are zero otherwise)
    vis = (st.proj_out["radii"].cpu() > 0) & (radii_ref > 0)
    assert vis.any() and float((vis != (radii_ref > 0)).double().mean()) <= 0.01, case
    g = torch.Generator().manual_seed(N)
    cot64 = [torch.randn(o.shape, generator=g, dtype=torch.float64) * vis.reshape(vis.shape + (1,) * (o.dim() - 2)) for o in ref_out]
    sum(((o * c).sum() for o, c in zip(ref_out, cot64))).backward()
    cot = [c.float().to(DEV).contiguous() for c in cot64]
    v_view, v_rts = _pose_bwd(cfg, st, cot, with_rts)
    again = _pose_bwd(cfg, st, cot, with_rts)
    full_view, full_rts = _project_bwd(cfg, st, cot)
    torch.cuda.synchronize()
    assert torch.equal(v_view, again[0]) and (not with_rts or torch.equal(v_rts, again[1])), case  # bitwise from call to call
    for name, got in (("pose_bwd", v_view), ("project_bwd", full_view)):
        assert not got[3].any() and got[3].signbit().logical_not().all(), (case, name)  # row 3: exact zeros
        check(case, f"{name} v_viewmat", got[:3].cpu(), w2c.grad[:3])
    if with_rts:
        check(case, "pose_bwd v_RTs", v_rts.cpu(), RTs.grad)
        check(case, "project_bwd v_RTs", full_rts.cpu(), RTs.grad)
    if camera == "general" and N >= 8 * PROBES:  # the clamp probes are in: some visible instance takes the clamped Jacobian branch
        V, Kc = sc["viewmat"].double(), sc["K"].double()
        pc = sc["means"].double()[-4 * PROBES:] @ V[:3, :3].T + V[:3, 3]
        beyond = ((pc[:, 0] / pc[:, 2]).abs() > 1.3 * 0.5 * w / Kc[0, 0]) | ((pc[:, 1] / pc[:, 2]).abs() > 1.3 * 0.5 * h / Kc[1, 1])
        assert G > 0 or int((beyond & vis[0, -4 * PROBES:]).sum()) >= 4, case


def test_pose_bwd_all_culled_is_exact_zeros():
    N, S = 300, 3
    sc = make_scene(N, 0, 1, S, W, H, seed=5, dtype=torch.float64, T=T, cam_jitter=0.03)
    sc["means"][:, 2] = -sc["means"][:, 2]  # behind the camera: the near plane culls every instance
    cfg, st = _device_projection(sc, N, 0, 1, S, W, H, True, False)
    assert not st.proj_out["radii"].any()
    g = torch.Generator().manual_seed(1)
    cot = [torch.randn(S, N, k, generator=g).squeeze(-1).to(DEV).contiguous() for k in (2, 3, 1)]
    v_view, v_rts = _pose_bwd(cfg, st, cot, True)
    assert not v_view.any() and not v_rts.any() and not v_view.isnan().any()


# ---- 2 - 5: the loop ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    """The model of tests/pose_refine_ref.py on the device, its base pose and the target image (the oracle's fp64 render from the
    offset pose)."""
    model, sc = R.build_model(DEV)
    return dict(model=model, w2c=sc["viewmat"].to(DEV), K=sc["K"].to(DEV), img=R.target_image().float().to(DEV))


def _refine(world, **kw):
    from deblur4dgs_amd.pose_refine import refine_pose

    res = refine_pose(world["model"], R.T_FRAME, world["w2c"], world["K"], world["img"], **kw)
    torch.cuda.synchronize()
    return res


def _same_bits(a, b):
    for k in ("transR", "transT", "w2c", "img", "losses", "lrs"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["state"].pmv, b["state"].pmv) and torch.equal(a["state"].step, b["state"].step)


def test_eager_and_graph_replay_agree_bit_for_bit(world):
    eager = _refine(world, iters=20, lr=R.LR, eta_min=R.ETA_MIN, graph=False, check_every=7)
    replay = _refine(world, iters=20, lr=R.LR, eta_min=R.ETA_MIN, graph=True, check_every=7)
    assert int(eager["state"].step) == int(replay["state"].step) == 20
    assert eager["recaptures"] == replay["recaptures"] == 0
    _same_bits(eager, replay)
    assert float(eager["losses"][-1]) < float(eager["losses"][0]) and bool((eager["losses"] > 0).all())
    assert float(eager["lrs"][-1]) == float(torch.tensor(R.ETA_MIN, dtype=torch.float32))
    # the flags the loop sets on the model are restored
    assert world["model"].pose_only is False and world["model"].deferred_size_check is False


def test_pose_only_differentiates_the_camera_alone(world):
    model = world["model"]
    scene_params = [p for part in (model.fg, model.bg, model.motion_bases) for p in part.parameters()]
    grads = {}
    for pose_only in (True, False):
        model.zero_grad(set_to_none=True)
        Wm = world["w2c"].clone().requires_grad_()
        model.pose_only = pose_only
        try:
            out = model.render(R.T_FRAME, Wm[None], world["K"][None], (W, H), return_depth=True)
        finally:
            model.pose_only = False
        (out["img"] - world["img"]).abs().mean().backward()
        torch.cuda.synchronize()
        grads[pose_only] = Wm.grad.clone()
        if pose_only:
            assert all(p.grad is None for p in scene_params)
        else:
            assert all(p.grad is not None for p in scene_params)
    assert not grads[True][3].any() and bool(grads[True][:3].abs().min() > 0)
    check("pose_only against the full backward", "W.grad", grads[True][:3].cpu(), grads[False][:3].cpu().double())


def test_loop_matches_the_oracle_loop(world):
    """30 iterations from the offset of tests/pose_refine_ref.py (which says why it is no rotation: the path must end short of the target
    with no gradient component changing sign) against the same loop on the oracle in fp64.  Yardstick: the deviation of the fp32 oracle loop from the fp64 one; the device's deviation of the
    parameters and of the loss curve is at most 4 x that (tests/util.py, ROW_YARD_RATIO).  Measured ratios: profiles/pose_refine_parity.json."""
    from tests.util import ROW_YARD_RATIO

    truth, yard = R.oracle_loop(torch.float64), R.oracle_loop(torch.float32)
    # conditions of the comparison, from the fp64 run alone
    g = truth["grads"]
    assert bool((torch.sign(g) == torch.sign(g[:1])).all()) and bool((g != 0).all()), "a gradient component changes sign"
    assert float(truth["losses"][-1]) <= (2.0 / 3.0) * float(truth["losses"][0]), "the loss does not fall by a third"
    res = _refine(world, iters=R.ITERS, lr=R.LR, eta_min=R.ETA_MIN, graph=True, check_every=10)
    p = torch.cat([res["transR"].reshape(-1), res["transT"].reshape(-1)]).cpu().double()
    dev_p, yard_p = float((p - truth["p"][-1]).abs().max()), float((yard["p"][-1] - truth["p"][-1]).abs().max())
    dev_l = float((res["losses"].cpu().double() - truth["losses"]).abs().max())
    yard_l = float((yard["losses"] - truth["losses"]).abs().max())
    out = dict(iters=R.ITERS, lr=R.LR, eta_min=R.ETA_MIN, p_dev=dev_p, p_yard=yard_p, p_ratio=dev_p / yard_p, loss_dev=dev_l,
               loss_yard=yard_l, loss_ratio=dev_l / yard_l, loss_first=float(truth["losses"][0]), loss_last=float(truth["losses"][-1]))
    print(out)
    with open(os.path.join(ROOT, "profiles", "pose_refine_parity.json"), "w") as f:
        json.dump(out, f, indent=1)
    assert dev_p <= ROW_YARD_RATIO * yard_p, out
    assert dev_l <= ROW_YARD_RATIO * yard_l, out


def test_overflow_inside_the_graph_is_recovered_with_the_same_bits(world):
    """The lists of the captured render are sized by the engine's guess for the shape: a guess far below what the frame needs makes
    every replay overflow (its kernels skip their work).  The first check must notice, the loop must go back to its snapshot, capture
    again at the capacity the check recorded, and end with the bits of a run that never overflowed."""
    clean = _refine(world, iters=12, lr=R.LR, eta_min=R.ETA_MIN, graph=True, check_every=5)
    assert clean["recaptures"] == 0
    key = engine._size_key(DEV, 1, R.N, W, H)
    big = [engine._guess_get(key + (xt,)) for xt in (False, True)]
    assert any(b is not None and b[0] > 64 for b in big)
    for xt in (False, True):
        engine._guess_put(key + (xt,), (64, 512))  # the engine's own hint: lists for 64 intersections
    tight = _refine(world, iters=12, lr=R.LR, eta_min=R.ETA_MIN, graph=True, check_every=5)
    assert tight["recaptures"] >= 1
    _same_bits(clean, tight)
