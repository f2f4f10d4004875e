"""the CPU twins d4gs_forward_cpu / d4gs_backward_cpu (csrc/cpu_twin.hip, product code inside libd4gs.so) against
the fp64 torch oracle - no GPU needed.  BASELINE.json configs[0] (10 k static Gaussians, 1 camera, 288x512, N_exposure = 1) in
full, and small dynamic scenes through the whole seam (deformation, camera delta, S sub-samples, blend policies): images
and EVERY leaf gradient at north_star's 1e-4.  The twin is fp32 and scalar; the allowances are the ones of the device tests."""
import pytest
import torch

from deblur4dgs_amd.synth import make_scene
from oracle import scene as oscene
from tests.test_gpu_exposure import _split
from tests.util import frac_bad, rel_err

TOL, FLIPS = 1e-4, 2e-3


def _close(name, got, ref, flips=FLIPS):
    bad = frac_bad(got, ref, TOL)
    assert bad <= flips, f"{name}: {bad:.2e} of the elements off by > {TOL:g} x max|ref| (max err {rel_err(got, ref):.2e})"


@pytest.mark.parametrize("N,G,K,S,W,H,mask,depth", [(400, 250, 3, 3, 64, 48, True, True), (300, 300, 5, 2, 48, 40, False, False),
                                                    (350, 0, 1, 1, 56, 40, False, True)])
def test_cpu_twin_matches_the_oracle(N, G, K, S, W, H, mask, depth):
    from deblur4dgs_amd.cpu_twin import render_exposure_cpu

    sc = make_scene(N, G, K, S, W, H, seed=700 + N, dtype=torch.float64, cam_jitter=0.01)
    sc["scales"] = sc["scales"] + 1.2
    keys = ("means", "quats", "scales", "colors", "opacities")
    if G:
        fg, bg, bases = _split(sc, torch.float64)
    else:
        fg, bases, bg = None, None, {k: sc[k].clone().requires_grad_() for k in keys}
    times, RTs, w2c = sc["times"].clone().requires_grad_(), sc["RTs"].clone().requires_grad_(), sc["viewmat"].clone().requires_grad_()
    out = oscene.render_exposure(fg, bg, bases, times, RTs, w2c, sc["K"], (W, H), bg_color=1.0, return_depth=depth, return_mask=mask,
                                 single=(S == 1))
    blended_ref = torch.cat([out[k] for k in ("img", "mask", "depth") if k in out], -1)[0]
    g = torch.Generator().manual_seed(1)
    w_b = torch.randn(blended_ref.shape, generator=g, dtype=torch.float64)
    w_a = torch.randn(out["acc"][0].shape, generator=g, dtype=torch.float64)
    raw_stack = torch.stack(out["raw_renders"], 0)[:, 0]
    w_r = 0.1 * torch.randn(raw_stack.shape, generator=g, dtype=torch.float64)
    ((blended_ref * w_b).sum() + (out["acc"][0] * w_a).sum() + (raw_stack * w_r).sum()).backward()

    cat = lambda k: torch.cat([p[k].detach() for p in (fg, bg) if p is not None], 0).float().requires_grad_()
    P = {k: cat(k) for k in keys}
    leaf = lambda t: None if t is None else t.detach().float().requires_grad_()
    coefs = leaf(fg["motion_coefs"]) if G else None
    rots, transls = (leaf(bases["rots"]), leaf(bases["transls"])) if G else (None, None)
    tms, rts, vm = leaf(times), leaf(RTs), leaf(w2c)
    colors_in, bgc = P["colors"], torch.ones(3)
    policy = None
    if mask:
        mk = torch.zeros(N, 1)
        mk[: (G if 0 < G < N else N)] = 1.0
        colors_in, bgc = torch.cat([colors_in, mk], -1), torch.cat([bgc, torch.zeros(1)])
        policy = [0, 0, 0, 1] + ([0] if depth else [])  # the reference's channel 3 <- max (scene_model.py:390)
    res = render_exposure_cpu(P["means"], P["quats"], P["scales"], P["opacities"], colors_in, 3, coefs, rots, transls, tms, rts, vm,
                              sc["K"].float(), W, H, background=bgc, return_depth=depth, policy=policy)
    _close("renders", res["renders"], raw_stack)
    _close("blended", res["blended"], blended_ref)
    _close("acc", res["acc"], out["acc"][0, ..., 0])
    assert int(res["n_isect"][0]) > 0 and 0 < int(res["n_isect"][3]) <= int(res["n_isect"][2]) <= int(res["n_isect"][0])
    ((res["blended"] * w_b.float()).sum() + (res["acc"] * w_a[..., 0].float()).sum() + (res["renders"] * w_r.float()).sum()).backward()
    ref_cat = lambda k: torch.cat([p[k].grad for p in (fg, bg) if p is not None], 0)
    for k in keys:
        _close(k, P[k].grad, ref_cat(k))
    if G:
        _close("motion_coefs", coefs.grad, fg["motion_coefs"].grad)
        _close("rots", rots.grad, bases["rots"].grad, 0.0)
        _close("transls", transls.grad, bases["transls"].grad, 0.0)
        _close("times", tms.grad, times.grad, 0.0)
    _close("RTs", rts.grad, RTs.grad, 0.0)
    _close("viewmat", vm.grad[:3], w2c.grad[:3], 0.0)


# (N, G, K, S, W, H, seed, camera): the two scenes of the first test under the `general` camera (tests/camera_cases.py: rotated and
# translated w2c, fx != fy, principal point off centre; camera deltas of 0.03 rad instead of 0.01), then the shapes that
# tests/test_gpu_camera_general.py renders on the device.  Their seeds are chosen HERE: a GPU case's seed is acceptable when the fp32
# twin shows no element of a no-allowance tensor (rots, transls, times, RTs, viewmat) beyond 1e-4 of the fp64 oracle - then a miss on
# the device is the kernels', not the scene's (one alpha / radius decision falling the other way in fp32 moves a whole column sum).
CAMERA_CASES = [(400, 250, 3, 3, 64, 48, 1100, "general"), (350, 0, 1, 1, 56, 40, 1050, "general")]
GPU_CAMERA_CASES = [(N, G, K, S, 88, 56, seed, cam) for cam, seeds in (("general", (2102, 2101, 2103)), ("rotated", (2102, 2102, 2104)))
                    for (N, G, K, S), seed in zip(((900, 500, 4, 3), (900, 900, 12, 1), (700, 0, 1, 2)), seeds)]


@pytest.mark.parametrize("N,G,K,S,W,H,seed,camera", CAMERA_CASES + GPU_CAMERA_CASES)
def test_cpu_twin_matches_the_oracle_under_a_general_camera(N, G, K, S, W, H, seed, camera):
    """Mask and depth channels on.  Per-Gaussian tensors at TOL with FLIPS; rots, transls, times, RTs and viewmat with no allowance
    (measured: 2.2e-5 of max|ref| at worst - on viewmat - for the dynamic scene, 7.9e-6 for the static one)."""
    from deblur4dgs_amd.cpu_twin import render_exposure_cpu
    from tests import camera_cases

    case = camera_cases.exposure_case(N, G, K, S, W, H, seed, camera)
    L, colors_in, bgc, Kmat = camera_cases.exposure_leaves(case)
    res = render_exposure_cpu(L["means"], L["quats"], L["scales"], L["opacities"], colors_in, 3, L["motion_coefs"], L["rots"],
                              L["transls"], L["times"], L["RTs"], L["viewmat"], Kmat, W, H, background=bgc, return_depth=True)
    for k in ("renders", "blended", "acc"):
        _close(k, res[k], case["ref"][k])
    w = case["w"]
    ((res["blended"] * w["blended"].float()).sum() + (res["acc"] * w["acc"].float()).sum() + (res["renders"] * w["renders"].float()).sum()).backward()
    shared = ("rots", "transls", "times", "RTs", "viewmat")
    for k, want in case["grads"].items():
        got = L[k].grad
        print(f"{camera} N={N} G={G} K={K} S={S} {k}: {rel_err(got, want):.2e}")
        assert float(want.abs().max()) > 0 or (k == "times" and S == 1), k  # (S = 1 renders at the integer frame time 3.0, where the oracle's own d / d time is 0)
        if k in ("viewmat", "RTs"):  # per column, as the device test's check_columns: rotation and translation columns each on their own
            got, want = (got[:3], want[:3]) if k == "viewmat" else (got, want)
            for col in range(4):
                _close(f"{k}[..., {col}]", got[..., col], want[..., col], 0.0)
        else:
            _close(k, got, want, 0.0 if k in shared else FLIPS)


# the static seam's cases of tests/test_gpu_camera_general.py: (camera, mode, D, seed) at N = 1200, 88 x 56 (`rolled`: 56 x 88)
GPU_STATIC_CASES = [(cam, mode, D, seed) for cam in ("rotated", "anisotropic", "offcentre", "general", "rolled")
                    for mode, D, seed in (("RGB+ED", 3, 2203), ("RGB", 16, 2204))]
GPU_STATIC_SHAPE = (1200, 88, 56)


@pytest.mark.parametrize("camera,mode,D,seed", GPU_STATIC_CASES)
def test_cpu_twin_static_seam_under_every_camera(camera, mode, D, seed):
    """The seeds of the device test's static cases, by the same rule: the viewmat gradient (no allowance, per column) of the fp32 twin
    within 1e-4 of the fp64 oracle's."""
    from deblur4dgs_amd.cpu_twin import render_exposure_cpu
    from tests import camera_cases

    N, W, H = GPU_STATIC_SHAPE
    c = camera_cases.static_case(camera, mode, D, N, W, H, seed)
    W, H = c["W"], c["H"]
    P = {k: c["inp"][k].float().requires_grad_() for k in ("means", "quats", "scales", "opac", "colors", "V")}
    res = render_exposure_cpu(P["means"], P["quats"], P["scales"], P["opac"], P["colors"], 0, None, None, None, None, None, P["V"],
                              c["inp"]["K"].float(), W, H, background=c["bg"].float(), return_depth=mode == "RGB+ED", blend=False,
                              raw_params=False)
    _close("renders", res["renders"][0], c["ref_c"])
    _close("alphas", res["alphas"][0], c["ref_a"])
    ((res["renders"][0] * c["w_c"].float()).sum() + (res["alphas"][0] * c["w_a"].float()).sum()).backward()
    for k in ("means", "quats", "scales", "opac", "colors"):
        _close(k, P[k].grad, c["grads"][k])
    got, want = P["V"].grad[:3].double(), c["grads"]["V"][:3]
    for col in range(4):
        print(f"{camera} {mode} D={D} viewmat[:, {col}]: {rel_err(got[:, col], want[:, col]):.2e}")
        _close(f"viewmat[:, {col}]", got[:, col], want[:, col], 0.0)


def test_cfg1_on_the_cpu_twin_in_full():
    """BASELINE.json configs[0] on its exact workload (seed 1000, identity camera delta) - the CPU-runnable case."""
    from deblur4dgs_amd.cpu_twin import render_exposure_cpu

    N, W, H = 10_000, 512, 288
    sc = make_scene(N, 0, 1, 1, W, H, seed=1000, dtype=torch.float64, cam_jitter=0.0)
    keys = ("means", "quats", "scales", "colors", "opacities")
    bg = {k: sc[k].clone().requires_grad_() for k in keys}
    w2c = sc["viewmat"].clone().requires_grad_()
    ref = oscene.render_exposure(None, bg, None, sc["times"], sc["RTs"], w2c, sc["K"], (W, H), bg_color=1.0, return_depth=True, single=True)
    ref_img = torch.cat([ref["img"], ref["depth"]], -1)[0]
    g = torch.Generator().manual_seed(0)
    w_i = torch.randn(ref_img.shape, generator=g, dtype=torch.float64)
    w_a = torch.randn(H, W, generator=g, dtype=torch.float64)
    ((ref_img * w_i).sum() + (ref["acc"][0, ..., 0] * w_a).sum()).backward()
    P = {k: sc[k].float().requires_grad_() for k in keys}
    vm = sc["viewmat"].float().requires_grad_()
    res = render_exposure_cpu(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], 3, None, None, None, None,
                              sc["RTs"].float(), vm, sc["K"].float(), W, H, background=torch.ones(3), return_depth=True)
    assert res["renders"].shape == (1, H, W, 4) and 0 < int(res["n_isect"][0]) <= ref["info"][0]["n_isect"]
    assert ((res["radii"][0] > 0) != (ref["info"][0]["radii"] > 0)).float().mean() < 1e-3
    _close("blended", res["blended"], ref_img, 1e-4)
    _close("acc", res["acc"], ref["acc"][0, ..., 0], 1e-4)
    ((res["blended"] * w_i.float()).sum() + (res["acc"] * w_a.float()).sum()).backward()
    for k in keys:
        _close(k, P[k].grad, bg[k].grad, 1e-4)
    _close("viewmat", vm.grad[:3], w2c.grad[:3], 0.0)


def test_cpu_twin_is_an_entry_point_not_a_fallback():
    from deblur4dgs_amd import exposure
    from deblur4dgs_amd.cpu_twin import render_exposure_cpu

    sc = make_scene(50, 0, 1, 1, 32, 32, seed=5, dtype=torch.float32, cam_jitter=0.0)
    with pytest.raises(RuntimeError, match="CPU tensor"):  # the device seam still refuses CPU tensors
        exposure.render_exposure(sc["means"], sc["quats"], sc["scales"], sc["opacities"], sc["colors"], 3, None, None, None, None,
                                 sc["RTs"], sc["viewmat"], sc["K"], 32, 32)
    src = open(exposure.__file__).read() + open(exposure.__file__.replace("exposure.py", "engine.py")).read()
    assert "cpu_twin" not in src and "_cpu(" not in src  # nothing on the device path routes here


def test_cpu_twin_activated_inputs_no_background_no_blend():
    """The gsplat-seam flavour of the flags: activated scales / opacities (raw_params=False), no background, blend off."""
    from deblur4dgs_amd.cpu_twin import render_exposure_cpu
    from oracle import raster
    from tests.util import static_inputs

    W, H, N = 72, 56, 500
    inp = static_inputs(N, W, H, seed=77, dtype=torch.float64, D=3, scale_mul=3.0)
    ref = {k: v.clone().requires_grad_() for k, v in inp.items() if k in ("means", "quats", "scales", "opac", "colors")}
    rc, ra, _ = raster.rasterization(ref["means"], ref["quats"], ref["scales"], ref["opac"], ref["colors"], inp["V"], inp["K"], W, H,
                                     background=None, render_mode="RGB")
    g = torch.Generator().manual_seed(3)
    w = torch.randn(rc.shape, generator=g, dtype=torch.float64)
    ((rc * w).sum() + 0.3 * ra.sum()).backward()
    P = {k: inp[k].float().requires_grad_() for k in ref}
    res = render_exposure_cpu(P["means"], P["quats"], P["scales"], P["opac"], P["colors"], 0, None, None, None, None, None,
                              inp["V"].float(), inp["K"].float(), W, H, background=None, return_depth=False, blend=False,
                              raw_params=False)
    assert res["blended"] is None and res["renders"].shape == (1, H, W, 3)
    _close("renders", res["renders"][0], rc)
    _close("alphas", res["alphas"][0, ..., 0], ra[..., 0])
    ((res["renders"][0] * w.float()).sum() + 0.3 * res["alphas"].sum()).backward()
    for k in ref:
        _close(k, P[k].grad, ref[k].grad)


def test_cpu_twin_default_policy_is_the_reference_policy():
    """`policy=None` must mean what it means on the device path - channel 3 <- max_S, channel 16 <- min_S
    (scene_model.py:392-393) - not "mean everywhere".  S > 1 and NCH > 3 (RGB + depth), default arguments."""
    from deblur4dgs_amd.cpu_twin import render_exposure_cpu
    from deblur4dgs_amd.exposure import reference_policy

    N, G, K, S, W, H = 300, 200, 3, 3, 48, 40
    sc = make_scene(N, G, K, S, W, H, seed=911, dtype=torch.float32, cam_jitter=0.01)
    sc["scales"] = sc["scales"] + 1.2
    args = (sc["means"], sc["quats"], sc["scales"], sc["opacities"], sc["colors"], 3, sc["motion_coefs"], sc["rots"], sc["transls"],
            sc["times"], sc["RTs"], sc["viewmat"], sc["K"], W, H)
    dflt = render_exposure_cpu(*args, background=torch.ones(3), return_depth=True)
    expl = render_exposure_cpu(*args, background=torch.ones(3), return_depth=True, policy=reference_policy(4))
    mean = render_exposure_cpu(*args, background=torch.ones(3), return_depth=True, policy=[0, 0, 0, 0])
    assert torch.equal(dflt["blended"], expl["blended"])
    assert torch.equal(dflt["blended"][..., :3], mean["blended"][..., :3])
    assert not torch.equal(dflt["blended"][..., 3], mean["blended"][..., 3])  # the depth channel takes the max, not the mean
    raw = dflt["renders"][..., 3]
    want = torch.maximum(raw[:-1].amax(0), raw.mean(0))  # max{raw_0 .. raw_{S-2}, mean}: the reference's in-place quirk
    assert torch.allclose(dflt["blended"][..., 3], want, rtol=1e-6, atol=1e-6)
