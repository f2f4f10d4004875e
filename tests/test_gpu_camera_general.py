"""GPU: every render path from cameras in general position (tests/camera_cases.py).

The rest of the suite looks through `viewmat = I`, `fx = fy`, a centred principal point and camera deltas of <= 0.01 rad, under which R and
R^T, fx and fy, limx and limy and the two sides of every cull are interchangeable.  Here: a rotated and translated w2c, fx != fy, cx / cy
off centre by non-integers of opposite sign, all three together, and an exact quarter roll - through

  a. the static seam `rasterization()` against oracle.raster, forward and backward, the viewmat gradient per COLUMN;
  b. the fused `render_exposure` (deformation, camera deltas of 0.03 rad, S sub-samples, blend) against oracle.scene, RTs and viewmat per
     column, rots / transls / times with no allowance;
  c. the feature paths (antialiased, absgrad, "ED", sh_degree = 3) against their restatements, and the suite's invariances (exact_cull,
     exact tiles, one-call frame = staged chain, SceneModel.render, fused control statistics) at the `general` camera;
  d. properties that need no oracle (a mistake shared by kernel and oracle): rigid-motion invariance, the quarter roll, a principal-point
     shift by one tile.

Shapes: N <= 1500, 88 x 56 (neither a multiple of the 16-pixel tile).  Every seed of a case with a no-allowance tensor was chosen with the
fp32 CPU twin (tests/test_cpu_twin.py: the same scenes, no element beyond 1e-4 there); the tolerances are the suite's."""
import pytest
import torch

from oracle import raster
from tests import camera_cases as cc
from tests.test_cpu_twin import GPU_CAMERA_CASES, GPU_STATIC_CASES, GPU_STATIC_SHAPE
from tests.util import check, check_columns, rel_err, static_inputs

pytestmark = pytest.mark.gpu
TOL, FLIPS = 1e-4, 2e-3  # tests/test_gpu_rasterization.py
STOL = 1e-4              # shared leaves: sums over all Gaussians, no allowance (tests/test_gpu_exposure.py)
DEV = torch.device("cuda:0")
LEAVES = ("means", "quats", "scales", "opac", "colors")


def _general(N, W, H, seed, D=3, scale_mul=3.0, camera="general"):
    inp = static_inputs(N, W, H, seed=seed, dtype=torch.float64, D=D, scale_mul=scale_mul)
    return cc.apply_camera(inp, camera, W, H)[0]


# ---- a. the static seam ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera,mode,D,seed", GPU_STATIC_CASES)
def test_static_seam_matches_the_oracle(camera, mode, D, seed):
    from tests.test_gpu_rasterization import _run_gpu

    N, W, H = GPU_STATIC_SHAPE
    c = cc.static_case(camera, mode, D, N, W, H, seed)
    W, H, ref_info = c["W"], c["H"], c["info"]
    rc, ra, info, tg = _run_gpu(c["inp"], W, H, mode, c["bg"], requires_grad=True)
    info["means2d"].retain_grad()
    ((rc[0] * c["w_c"].to(DEV).float()).sum() + (ra[0] * c["w_a"].to(DEV).float()).sum()).backward()
    torch.cuda.synchronize()
    assert rc.shape == (1, H, W, D + (mode != "RGB")) and ra.shape == (1, H, W, 1)
    case = f"camera {camera}: S1 {mode} D={D} N={N} {W}x{H}"
    # per-instance stage, at test_forward_matches_oracle's tolerances
    vis_ref, vis = ref_info["radii"] > 0, info["radii"][0].cpu() > 0
    assert (vis != vis_ref).float().mean() < 1e-3
    both = vis & vis_ref
    assert rel_err(info["means2d"][0].detach().cpu()[both], ref_info["means2d"].detach()[both]) < 1e-5
    assert rel_err(info["conics"][0].detach().cpu()[both], ref_info["conics"].detach()[both]) < 1e-4
    assert (info["radii"][0].cpu()[both] != ref_info["radii"][both]).float().mean() < 1e-3
    check(case, "render_colors", rc[0].detach().cpu(), c["ref_c"], TOL, FLIPS)
    check(case, "render_alphas", ra[0].detach().cpu(), c["ref_a"], TOL, FLIPS)
    check(case, "means2d.grad", info["means2d"].grad[0].cpu(), c["grads"]["means2d"], TOL, FLIPS)
    for name in LEAVES:
        check(case, name, tg[name].grad.cpu(), c["grads"][name], TOL, FLIPS)
    # rotation columns and the translation column each within 1e-4 of their OWN maximum
    check_columns(case, "viewmat", tg["V"].grad.cpu()[:3], c["grads"]["V"][:3], TOL)


# ---- b. the fused exposure render --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,G,K,S,W,H,seed,camera", GPU_CAMERA_CASES)
def test_exposure_forward_backward(N, G, K, S, W, H, seed, camera):
    """(G > 0, K = 4, S = 3); (G = N, K = 12, S = 1): k_project_bwd's sub-group mapping on the matrix pipe; (G = 0, S = 2).  Mask and
    depth channels on, camera deltas of 0.03 rad."""
    from deblur4dgs_amd.exposure import render_exposure

    c = cc.exposure_case(N, G, K, S, W, H, seed, camera)
    L, colors_in, bgc, Kmat = cc.exposure_leaves(c, DEV)
    res = render_exposure(L["means"], L["quats"], L["scales"], L["opacities"], colors_in, 3, L["motion_coefs"], L["rots"], L["transls"],
                          L["times"], L["RTs"], L["viewmat"], Kmat, W, H, background=bgc, return_depth=True)
    torch.cuda.synchronize()
    case = f"camera {camera}: fused N={N} G={G} K={K} S={S} {W}x{H}"
    for k in ("renders", "blended", "acc"):
        check(case, k, res[k].detach().cpu(), c["ref"][k], TOL, FLIPS)
    w = {k: v.float().to(DEV) for k, v in c["w"].items()}
    ((res["blended"] * w["blended"]).sum() + (res["acc"] * w["acc"]).sum() + (res["renders"] * w["renders"]).sum()).backward()
    torch.cuda.synchronize()
    g = c["grads"]
    for k in cc.LEAF_KEYS + (("motion_coefs",) if G else ()):
        check(case, k, L[k].grad.cpu(), g[k], TOL, FLIPS)
    if G:
        for k in ("rots", "transls", "times"):
            check(case, k, L[k].grad.cpu(), g[k], STOL)
    check_columns(case, "RTs", L["RTs"].grad.cpu(), g["RTs"], STOL)
    check_columns(case, "viewmat", L["viewmat"].grad.cpu()[:3], g["viewmat"][:3], STOL)


# ---- c. feature paths at the general camera ----------------------------------------------------------------------------------------
def test_antialiased_at_the_general_camera():
    from oracle import margins
    from tests import antialias_ref
    from tests.test_gpu_antialias import _backward, _render

    N, W, H, mode = 700, 88, 56, "RGB+ED"
    inp = _general(N, W, H, 511, scale_mul=1.5)
    bg = torch.linspace(0.1, 0.9, 3, dtype=torch.float64)
    t = {k: v.clone().requires_grad_(k != "K") for k, v in inp.items()}
    ref_c, ref_a, ref_info = antialias_ref.rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"], t["K"], W, H,
                                                         background=bg, render_mode=mode)
    # pixels of tiles whose list membership could toggle in float32 take no cotangent (tests/test_gpu_antialias.py)
    eff = (inp["opac"] * ref_info["compensations"].detach()).clamp(min=1e-300)
    toggles, _ = margins.gaussian_toggle_mask(inp["means"], inp["quats"], inp["scales"], eff, inp["V"], inp["K"], W, H)
    keep = (~toggles).double()[..., None]
    g = torch.Generator().manual_seed(21)
    w_c = torch.randn(ref_c.shape, generator=g, dtype=torch.float64) * keep
    w_a = torch.randn(ref_a.shape, generator=g, dtype=torch.float64) * keep
    ref_info["means2d"].retain_grad()
    ((ref_c * w_c).sum() + (ref_a * w_a).sum()).backward()
    rc, ra, info, tg = _render(inp, W, H, mode, bg)
    _backward(rc, ra, info, w_c, w_a)
    case = f"camera general: antialiased {mode} N={N} {W}x{H}"
    check(case, "render_colors", rc[0].detach().cpu(), ref_c.detach(), TOL, FLIPS)
    check(case, "render_alphas", ra[0].detach().cpu(), ref_a.detach(), TOL, FLIPS)
    check(case, "info.opacities", info["opacities"][0].cpu(), ref_info["opacities"].detach(), TOL, FLIPS)
    check(case, "means2d.grad", info["means2d"].grad[0].cpu(), ref_info["means2d"].grad, TOL, FLIPS)
    for name in LEAVES:
        check(case, name, tg[name].grad.cpu(), t[name].grad, TOL, FLIPS)
    check_columns(case, "viewmat", tg["V"].grad.cpu()[:3], t["V"].grad[:3], TOL)


def test_absgrad_at_the_general_camera():
    from tests.absgrad_ref import absgrad_of_rasterization
    from tests.test_gpu_absgrad import _backward, _render

    N, W, H, mode = 700, 88, 56, "RGB+ED"
    inp = _general(N, W, H, 311)
    bg = torch.linspace(0.1, 0.9, 3, dtype=torch.float64)
    g = torch.Generator().manual_seed(11)
    w_c = torch.randn(H, W, 4, generator=g, dtype=torch.float64)
    w_a = torch.randn(H, W, 1, generator=g, dtype=torch.float64)
    ref_abs, _, _ = absgrad_of_rasterization(inp["means"], inp["quats"], inp["scales"], inp["opac"], inp["colors"], inp["V"], inp["K"], W, H,
                                             w_c, w_a, bg, mode)
    rc, ra, info, _ = _render(inp, W, H, mode, bg)
    _backward(rc, ra, info, w_c, w_a)
    got = info["means2d"].absgrad
    assert got.shape == (1, N, 2) and bool((got >= 0).all()) and float(got.sum()) > 0
    check(f"camera general: absgrad {mode} N={N} {W}x{H}", "means2d.absgrad", got[0].cpu(), ref_abs, TOL, FLIPS)
    assert bool((got[0][info["radii"][0] == 0] == 0).all())


def test_expected_depth_only_at_the_general_camera():
    from tests.test_gpu_depth_only import _parity

    N, W, H = 700, 88, 56
    _parity("ED", 611, N, W, H, with_va=True, with_bg=False, exact_tiles=False, inp=_general(N, W, H, 611))


def test_sh_degree_3_at_the_general_camera():
    """tests/test_gpu_sh.py rotates and translates the camera under a centred, square-pixel K; here K is general too."""
    from tests.test_gpu_sh import sh_parity

    N, W, H, K = 1200, 88, 56, 16
    inp = _general(N, W, H, 346)
    g = torch.Generator().manual_seed(346)
    sh = torch.randn(N, K, 3, generator=g, dtype=torch.float64) * 0.35  # strongly view-dependent colours
    sh[:, 0] = (inp.pop("colors") - 0.5) / 0.28209479177387814
    inp["sh"] = sh
    sh_parity(inp, "RGB+ED", 3, K, "NK3", N, W, H, tag=" camera general")


def _static_run(inp, W, H, mode, D, **kw):
    from tests.test_gpu_rasterization import _run_gpu

    rc, ra, info, tg = _run_gpu(inp, W, H, mode, torch.linspace(0.2, 0.8, D), requires_grad=True, **kw)
    info["means2d"].retain_grad()
    w = torch.randn(rc.shape, generator=torch.Generator().manual_seed(3)).to(rc.device)
    ((rc * w).sum() + ra.sum()).backward()
    torch.cuda.synchronize()
    return dict(rc=rc.detach().clone(), ra=ra.detach().clone(), m2d=info["means2d"].grad.clone(), n=info["n_isect"],
                **{k: tg[k].grad.clone() for k in LEAVES + ("V",)})


@pytest.mark.parametrize("knob,scale_mul", [("exact_cull", 2.0), ("exact_tiles", 6.0)])
def test_exact_cull_and_exact_tiles_change_the_lists_and_not_the_image(knob, scale_mul, monkeypatch):
    """tests/test_gpu_rasterization.py's two invariances at the general camera: image, alpha and every gradient BITWISE, shorter lists."""
    monkeypatch.setenv("D4GS_SEG", "0")
    N, W, H, D = 1500, 88, 56, 3
    inp = _general(N, W, H, 77, D=D, scale_mul=scale_mul)
    a, b = (_static_run(inp, W, H, "RGB+ED", D, **{knob: on}) for on in (False, True))
    assert 0 < b["n"] < a["n"], (a["n"], b["n"])
    for k in a:
        if k != "n":
            assert torch.equal(a[k], b[k]), k
    assert float(a["means"].abs().max()) > 0 and float(a["V"].abs().max()) > 0


@pytest.mark.parametrize("sub_losses", [True, False])
def test_one_call_path_equals_the_staged_chain_bitwise(sub_losses):
    from deblur4dgs_amd.synth import make_scene
    from tests.test_gpu_frame import one_call_equals_the_staged_chain

    N, G, K_, S, W, H, D = 1200, 700, 4, 3, 88, 56, 3
    sc = make_scene(N, G, K_, S, W, H, seed=31, cam_jitter=0.03)
    sc["scales"] = sc["scales"] + 1.2
    sc = cc.apply_camera(sc, "general", W, H)[0]
    one_call_equals_the_staged_chain(sc, N, G, S, W, H, D, sub_losses)


def test_scene_model_render_with_general_w2cs_and_ks():
    """`SceneModel.render(mode="blury")`: the MoveModel's camera deltas are generated FROM the w2c (oracle.camera), 11 sub-samples."""
    from tests.test_gpu_scene_model import _build, _oracle

    N, G, K, W, H = 900, 500, 4, 88, 56
    model, sc = _build(N, G, K, W, H, 17, DEV)
    sc2 = cc.apply_camera(sc, "general", W, H)[0]
    with torch.no_grad():  # the model's Gaussians move with the world (the probes are background Gaussians)
        for k in ("means", "quats", "scales", "opacities"):
            model.fg.params[k].copy_(sc2[k][:G].to(DEV))
            model.bg.params[k].copy_(sc2[k][G:].to(DEV))
    ref, (fg, bg, bases, mm_sd), dT = _oracle(model, sc2, 3.0, W, H, "blury", "second", True, True, None, None)
    out = model.render(3.0, sc2["viewmat"][None].to(DEV), sc2["K"][None].to(DEV), (W, H), return_depth=True, return_mask=True,
                       mode="blury", stage="second")
    case = f"camera general: S2 render blury N={N} {W}x{H}"
    for k in ("img", "mask", "depth", "acc"):
        check(case, k, out[k].detach().cpu(), ref[k].detach(), TOL, FLIPS)
    g = torch.Generator().manual_seed(0)
    w, wd = torch.randn(1, H, W, 3, generator=g), torch.randn(1, H, W, 1, generator=g)
    ((out["img"] * w.to(DEV)).sum() + (out["depth"] * wd.to(DEV)).sum()).backward()
    ((ref["img"] * w.double()).sum() + (ref["depth"] * wd.double()).sum()).backward()
    torch.cuda.synchronize()
    for name, got_p, ref_p in (("fg.means", model.fg.params["means"], fg["means"]), ("fg.quats", model.fg.params["quats"], fg["quats"]),
                               ("bg.means", model.bg.params["means"], bg["means"]), ("bg.scales", model.bg.params["scales"], bg["scales"]),
                               ("fg.motion_coefs", model.fg.params["motion_coefs"], fg["motion_coefs"])):
        check(case, name, got_p.grad.cpu(), ref_p.grad, TOL, FLIPS)
    assert float(model.move_model.RT_head0[-1].bias.grad.abs().sum()) > 0  # the camera deltas are trained through v_RTs


@pytest.mark.parametrize("fused", [True, False])
def test_fused_control_statistics_equal_the_separate_kernel(fused):
    from deblur4dgs_amd import control
    from deblur4dgs_amd.exposure import render_exposure
    from deblur4dgs_amd.synth import make_scene

    N, G, K, S, W, H = 1200, 700, 4, 3, 88, 56
    sc = make_scene(N, G, K, S, W, H, seed=21, cam_jitter=0.03)
    sc["scales"] = sc["scales"] + 1.2
    sc = cc.apply_camera(sc, "general", W, H)[0]
    P = {k: sc[k].to(DEV).requires_grad_() for k in ("means", "quats", "scales", "opacities", "colors", "motion_coefs", "rots", "transls")}
    stats = control.new_running_stats(N, DEV)
    cs = dict(stats, batch_size=2, update_max_radii=True)
    o = render_exposure(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], 3, P["motion_coefs"], P["rots"], P["transls"],
                        sc["times"].to(DEV), sc["RTs"].to(DEV), sc["viewmat"].to(DEV), sc["K"].to(DEV), W, H,
                        background=torch.ones(3, device=DEV), return_depth=True, control_stats=cs, fused=fused)
    st = o["state"]
    assert bool(st.frame_io) == fused
    if not fused:
        o["means2d"].retain_grad()
    (o["blended"].square().sum() + o["acc"].sum()).backward()
    torch.cuda.synchronize()
    v_m2d = st.v_means2d if fused else o["means2d"].grad
    assert v_m2d is not None and v_m2d.shape == (S, N, 2)
    again = control.new_running_stats(N, DEV)
    control.accumulate_control_stats(again, v_m2d, o["radii"], (W, H), 2)
    torch.cuda.synchronize()
    for k in ("xys_grad_norm_acc", "vis_count"):
        assert torch.equal(stats[k], again[k]), k
    assert float(stats["xys_grad_norm_acc"].sum()) > 0 and int(stats["vis_count"].sum()) > 0.6 * N


# ---- d. oracle-free properties -----------------------------------------------------------------------------------------------------
def _k_general(N, W, H, seed):
    """identity view matrix, general K (anisotropic, then off centre: the probes are those of the final K)"""
    inp = static_inputs(N, W, H, seed=seed, dtype=torch.float64)
    inp = cc.apply_camera(inp, "anisotropic", W, H)[0]
    return cc.apply_camera(inp, "offcentre", W, H)[0]


def _render_for_property(inp, W, H, w_c):
    from tests.test_gpu_rasterization import _run_gpu

    rc, ra, info, tg = _run_gpu(inp, W, H, "RGB+ED", torch.tensor([0.2, 0.5, 0.8]), requires_grad=True)
    ((rc[0] * w_c.to(DEV)).sum() + ra.sum()).backward()
    torch.cuda.synchronize()
    return rc[0].detach().cpu(), ra[0].detach().cpu(), {k: tg[k].grad.cpu() for k in LEAVES}


def test_rigid_motion_of_world_and_camera_changes_nothing():
    """(means, quats, V = I) and (R0^T (means - t0), q(R0^T) (x) quats, V = [R0 | t0]) are the same scene in camera space: the same image,
    the same gradients on scales / opacities / colours, and means.grad turned by R0^T.  No oracle involved."""
    N, W, H = 1200, 88, 56
    a = _k_general(N, W, H, 2203)
    b = cc.apply_camera(a, "rotated", W, H)[0]
    assert torch.equal(a["V"], torch.eye(4, dtype=torch.float64)) and torch.equal(a["K"], b["K"])
    w_c = torch.randn(H, W, 4, generator=torch.Generator().manual_seed(5))
    ia, aa, ga = _render_for_property(a, W, H, w_c)
    ib, ab, gb = _render_for_property(b, W, H, w_c)
    case = f"camera rigid motion: N={N} {W}x{H}"
    check(case, "render_colors", ib, ia, TOL, FLIPS)
    check(case, "render_alphas", ab, aa, TOL, FLIPS)
    for k in ("scales", "opac", "colors"):
        check(case, k, gb[k], ga[k], TOL, FLIPS)
    check(case, "means (R0^T applied)", gb["means"], ga["means"].double() @ cc.R0, TOL, FLIPS)  # rows: g' = R0^T g
    assert rel_err(gb["means"], ga["means"]) > 0.05  # (and the rotation is not a detail)


def test_quarter_roll_turns_the_image_and_nothing_else():
    """The `rolled` camera of a general-K scene: fx <-> fy, (cx, cy) <- (H - cy, cx), W <-> H.  Tile rectangles and list lengths differ;
    the image turned back must be the unrolled one (1e-5: both are the same fp32 arithmetic up to the order of a few sums)."""
    N, W, H = 1200, 88, 56
    a = _k_general(N, W, H, 2203)
    b, Wb, Hb = cc.apply_camera(a, "rolled", W, H)
    assert (Wb, Hb) == (H, W) and float(b["K"][0, 0]) == float(a["K"][1, 1]) and float(b["K"][0, 2]) == H - float(a["K"][1, 2])
    w_c = torch.randn(H, W, 4, generator=torch.Generator().manual_seed(5))
    w_b = cc.unroll(cc.unroll(cc.unroll(w_c))).contiguous()  # three more quarter turns: the cotangent of the rolled image
    assert torch.equal(cc.unroll(w_b), w_c)
    ia, aa, ga = _render_for_property(a, W, H, w_c)
    ib, ab, gb = _render_for_property(b, Wb, Hb, w_b)
    case = f"camera quarter roll: N={N} {W}x{H}"
    check(case, "render_colors", cc.unroll(ib), ia, 1e-5, FLIPS)
    check(case, "render_alphas", cc.unroll(ab), aa, 1e-5, FLIPS)
    for k in LEAVES:  # the world did not move: every leaf gradient is the same
        check(case, k, gb[k], ga[k], TOL, FLIPS)


def test_principal_point_shift_by_one_tile():
    """cx += 16, W += 16: one more tile column on the left, every other tile keeps its list; the right W columns are the old image (not
    bitwise: fx x / z + cx rounds differently).  Scene without Gaussians beyond the FOV clamp - the clamp moves with W."""
    N, W, H = 1200, 88, 56
    a = cc.apply_camera(static_inputs(N, W, H, seed=2203, dtype=torch.float64), "rotated", W, H)[0]
    b = dict(a, K=a["K"].clone())
    b["K"][0, 2] += 16.0
    pc = a["means"] @ a["V"][:3, :3].T + a["V"][:3, 3]
    assert float((pc[:, 0] / pc[:, 2]).abs().max()) < 1.3 * 0.5 * W / float(a["K"][0, 0])
    w_c = torch.zeros(H, W, 4)
    ia, aa, _ = _render_for_property(a, W, H, w_c)
    ib, ab, _ = _render_for_property(b, W + 16, H, torch.zeros(H, W + 16, 4))
    case = f"camera principal point + 16: N={N} {W}x{H}"
    check(case, "render_colors", ib[:, 16:], ia, 1e-5, FLIPS)
    check(case, "render_alphas", ab[:, 16:], aa, 1e-5, FLIPS)
    assert float(ab[:, :16].max()) > 0.1  # the new columns show what was cut off
