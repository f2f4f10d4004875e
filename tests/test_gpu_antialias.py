"""GPU: gsplat's `rasterize_mode="antialiased"` (D4GS_ANTIALIASED): opacity * compensation from the projection kernel, the
compensation's adjoint folded into v_conics by the gather.

  - parity with the fp64 reference (tests/antialias_ref.py) over the instantiated channel counts, two channel chunks (D = 20) and
    every render mode, with and without v_alphas / background, with exact_cull on and off: images, alphas, info["opacities"] and the
    gradients of every leaf and of viewmat;
  - closed-form answers with no oracle: an isotropic splat, cov2d = s^2 I, has compensation s^2 / (s^2 + eps2d);
  - eps2d = 0: the render and every gradient are bitwise the classic ones;
  - a needle splat (pre-blur determinant 0): no NaN / Inf, and no gradient through it;
  - dense vs sparse rows, lazy vs eager lists: bitwise; depth segments: the hand-off's rounding; run-to-run bitwise;
  - with sh_degree = 3 and absgrad = True;
  - the exposure path (S = 8): one-call and staged chains bitwise, both against the exposure oracle with the antialiased rasterizer,
    and the fused densification statistics against d4gs_control_stats."""
import math

import numpy as np
import pytest
import torch

import oracle.raster
from oracle import margins
from tests import antialias_ref, ladder
from tests.util import check, rel_err, static_inputs

pytestmark = pytest.mark.gpu

TOL = 1e-4       # tests/test_gpu_absgrad.py's tolerance and flip allowance
GTOL = 1e-4
GFLIPS = 2e-3
VTOL = 1e-4      # viewmat: a sum over every Gaussian, no allowance
SEG_TOL = 2e-5   # depth-segmented vs whole-list replay (tests/test_gpu_list_edges.py)
NAMES = ("means", "quats", "scales", "opac", "colors", "V")


def _render(inp, W, H, mode="RGB", bg=None, aa=True, **kw):
    from deblur4dgs_amd.rasterization import rasterization

    dev = torch.device("cuda:0")
    t = {k: torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(torch.float32).to(dev) for k, v in inp.items()}
    for k in NAMES:
        t[k].requires_grad_()
    rc, ra, info = rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"][None], t["K"][None], W, H,
                                 backgrounds=None if bg is None else torch.as_tensor(bg).to(dev).float()[None], render_mode=mode,
                                 rasterize_mode="antialiased" if aa else "classic", **kw)
    return rc, ra, info, t


def _backward(rc, ra, info, w_c, w_a):
    dev = rc.device
    info["means2d"].retain_grad()
    loss = (rc[0] * torch.as_tensor(w_c).to(dev).float()).sum()
    if w_a is not None:
        loss = loss + (ra[0] * torch.as_tensor(w_a).to(dev).float()).sum()
    loss.backward()
    torch.cuda.synchronize()


def _grads(rc, ra, info, t):
    out = dict(rc=rc.detach(), ra=ra.detach(), opacities=info["opacities"].detach(), means2d=info["means2d"].grad)
    out.update({k: t[k].grad for k in NAMES})
    return {k: v.detach().cpu().clone() for k, v in out.items()}


PARITY = [(D, mode) for D in (1, 3, 4, 5, 8, 16, 20) for mode in ("RGB", "RGB+ED", "RGB+D")]
# D4GS_EXACT_TILES: the exact-tiles projection (tau from the compensated opacity), larger splats so that rectangles of 2 x 2 ... 8 x 8
# tiles get masks
PARITY_XT = [(3, "RGB+ED"), (4, "RGB"), (16, "RGB+D"), (20, "RGB+ED")]


@pytest.mark.parametrize("D,mode", PARITY)
def test_antialiased_matches_the_fp64_reference(D, mode):
    i = PARITY.index((D, mode))
    _parity(D, mode, i, exact_cull=i % 2 == 0, exact_tiles=False, scale_mul=1.5)


@pytest.mark.parametrize("D,mode", PARITY_XT)
def test_antialiased_exact_tiles_matches_the_fp64_reference(D, mode):
    i = PARITY_XT.index((D, mode))
    _parity(D, mode, 100 + i, exact_cull=True, exact_tiles=True, scale_mul=4.0)


def _parity(D, mode, i, exact_cull, exact_tiles, scale_mul):
    with_va, with_bg = (i % 4) in (0, 1), (i % 4) in (0, 2)
    N, W, H = 700, 72, 56
    inp = static_inputs(N, W, H, seed=500 + i, dtype=torch.float64, D=D, scale_mul=scale_mul)
    bg = torch.linspace(0.1, 0.9, D, dtype=torch.float64) if with_bg else None
    t = {k: v.clone().requires_grad_(k != "K") for k, v in inp.items()}
    ref_c, ref_a, ref_info = antialias_ref.rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"], t["K"],
                                                         W, H, background=bg, render_mode=mode)
    # pixels of tiles whose list membership could toggle in float32 take no cotangent (tests/test_gpu_flip_cause.py's argument)
    eff = (inp["opac"] * ref_info["compensations"].detach()).clamp(min=1e-300)
    toggles, _ = margins.gaussian_toggle_mask(inp["means"], inp["quats"], inp["scales"], eff, inp["V"], inp["K"], W, H)
    keep = (~toggles).double()[..., None]
    g = torch.Generator().manual_seed(21 + i)
    w_c = torch.randn(ref_c.shape, generator=g, dtype=torch.float64) * keep
    w_a = torch.randn(ref_a.shape, generator=g, dtype=torch.float64) * keep if with_va else None
    ref_info["means2d"].retain_grad()
    loss = (ref_c * w_c).sum() + ((ref_a * w_a).sum() if with_va else 0.0)
    loss.backward()

    rc, ra, info, tg = _render(inp, W, H, mode, bg, exact_cull=exact_cull, exact_tiles=exact_tiles)
    _backward(rc, ra, info, w_c, w_a)
    case = (f"antialiased {mode} D={D} N={N} {W}x{H} v_alphas={with_va} bg={with_bg} exact_cull={exact_cull}"
            f"{' exact_tiles' if exact_tiles else ''}")
    check(case, "render_colors", rc[0].detach().cpu(), ref_c.detach(), TOL, GFLIPS)
    check(case, "render_alphas", ra[0].detach().cpu(), ref_a.detach(), TOL, GFLIPS)
    assert info["opacities"].shape == (1, N)
    check(case, "info.opacities", info["opacities"][0].cpu(), ref_info["opacities"].detach(), TOL, GFLIPS)
    assert bool((info["opacities"][0][info["radii"][0] == 0] == 0).all())
    check(case, "means2d.grad", info["means2d"].grad[0].cpu(), ref_info["means2d"].grad, GTOL, GFLIPS)
    for name in ("means", "quats", "scales", "opac", "colors"):
        check(case, name, tg[name].grad.cpu(), t[name].grad, GTOL, GFLIPS)
    check(case, "viewmat", tg["V"].grad.cpu()[:3], t["V"].grad[:3], VTOL, 0.0)


@pytest.mark.parametrize("mode,D,scale_mul", [("RGB+ED", 3, 6.0), ("RGB", 4, 12.0), ("RGB+ED", 16, 8.0)])
def test_exact_tiles_change_nothing_but_the_lists(mode, D, scale_mul, monkeypatch):
    """Under the antialiased mode the exact-tiles test works from the compensated opacity: it may drop only tiles in which no pixel
    reaches alpha >= 1/255 with it, so image, alpha and every gradient are bitwise those of the whole rectangles, the lists are a
    subset of the rectangles' lists in the same depth order, and they shrink (tests/test_gpu_rasterization.py's classic check)."""
    monkeypatch.setenv("D4GS_SEG", "0")
    W, H, N = 256, 160, 6000
    inp = static_inputs(N, W, H, seed=31 + D, dtype=torch.float32, D=D, scale_mul=scale_mul)
    bg = np.linspace(0.2, 0.8, D)
    rng = np.random.default_rng(3)
    w_c, w_a = rng.standard_normal((H, W, D + (mode != "RGB"))), rng.standard_normal((H, W, 1))
    res = []
    for xt in (False, True):
        rc, ra, info, t = _render(inp, W, H, mode, bg, exact_tiles=xt, lazy_sort=False)
        _backward(rc, ra, info, w_c, w_a)
        offs = torch.cat([info["isect_offsets"].flatten().cpu().long(), torch.tensor([info["n_isect"]])])
        res.append(dict(g=_grads(rc, ra, info, t), n=info["n_isect"], tpg=info["tiles_per_gauss"].flatten().cpu().clone(),
                        ids=info["flatten_ids"].cpu().clone(), offs=offs))
    a, b = res
    for k in a["g"]:
        assert torch.equal(a["g"][k], b["g"][k]), k
    assert b["n"] < 0.93 * a["n"], (a["n"], b["n"])
    assert bool((b["tpg"] <= a["tpg"]).all()) and int(b["tpg"].sum()) == b["n"]
    for t in range(len(a["offs"]) - 1):
        fa = a["ids"][a["offs"][t]:a["offs"][t + 1]].tolist()
        fb = b["ids"][b["offs"][t]:b["offs"][t + 1]].tolist()
        it = iter(fa)
        assert all(any(x == y for y in it) for x in fb), t  # fb is a subsequence of fa


def _one_splat(s3, z, opac, W=33, H=33, f=40.0, eps2d=0.3):
    """one isotropic Gaussian on the optical axis, projected onto the centre of pixel (16, 16): cov2d = (f s3 / z)^2 I."""
    cx = cy = 16.5
    inp = dict(means=torch.tensor([[0.0, 0.0, z]]), quats=torch.tensor([[1.0, 0.0, 0.0, 0.0]]), scales=torch.full((1, 3), s3),
               opac=torch.tensor([opac]), colors=torch.tensor([[0.2, 0.6, 0.9]]), V=torch.eye(4),
               K=torch.tensor([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]]))
    s2 = (f * s3 / z) ** 2
    return inp, s2 / (s2 + eps2d)


@pytest.mark.parametrize("s3,z,opac,eps2d", [(0.02, 2.0, 0.8, 0.3), (0.005, 1.0, 0.5, 0.3), (0.1, 4.0, 0.9, 0.1), (0.3, 3.0, 0.6, 0.3)])
def test_isotropic_splat_known_answer(s3, z, opac, eps2d):
    inp, comp = _one_splat(s3, z, opac, eps2d=eps2d)
    rc, ra, info, _ = _render(inp, 33, 33, eps2d=eps2d)
    assert int(info["radii"][0, 0]) > 0
    assert math.isclose(float(info["opacities"][0, 0]), opac * comp, rel_tol=2e-6)
    # sigma = 0 at the centre pixel: alpha = opacity * compensation (render_alphas = 1 - (1 - alpha): an ulp of 1 more)
    assert math.isclose(float(ra[0, 16, 16, 0]), min(opac * comp, 0.99), rel_tol=1e-5)
    _, ra_c, info_c, _ = _render(inp, 33, 33, aa=False, eps2d=eps2d)
    assert math.isclose(float(ra_c[0, 16, 16, 0]), opac, rel_tol=1e-5)
    assert torch.equal(info["conics"], info_c["conics"]) and torch.equal(info["radii"], info_c["radii"])


@pytest.mark.parametrize("D,mode,exact_cull", [(3, "RGB+ED", True), (16, "RGB", False), (20, "RGB+D", True)])
def test_eps2d_zero_is_bitwise_classic(D, mode, exact_cull):
    N, W, H = 1500, 96, 64
    inp = static_inputs(N, W, H, seed=60 + D, dtype=torch.float32, D=D)
    bg = np.linspace(0.2, 0.8, D)
    nch = D + (mode != "RGB")
    rng = np.random.default_rng(D)
    w_c, w_a = rng.standard_normal((H, W, nch)), rng.standard_normal((H, W, 1))
    res = {}
    for aa in (False, True):
        rc, ra, info, t = _render(inp, W, H, mode, bg, aa=aa, eps2d=0.0, exact_cull=exact_cull)
        _backward(rc, ra, info, w_c, w_a)
        res[aa] = dict(_grads(rc, ra, info, t), radii=info["radii"].cpu())
    assert float(res[True]["rc"].abs().sum()) > 0
    # info["opacities"]: the activated opacities (classic) and the composited ones (antialiased: 0 for culled Gaussians)
    vis = res[False]["radii"] > 0
    assert int((~vis).sum()) > 0
    assert torch.equal(res[True]["opacities"], torch.where(vis, res[False]["opacities"], torch.zeros(())))
    for k in res[False]:
        if k != "opacities":
            assert torch.equal(res[False][k], res[True][k]), k


@pytest.mark.parametrize("exact_cull", [True, False])
def test_needle_splat_has_no_nan_and_no_gradient(exact_cull):
    N, W, H = 200, 64, 48
    g = torch.Generator().manual_seed(13)
    u = lambda *shape: torch.rand(*shape, generator=g)
    # an identity camera looking at a cloud of small splats; Gaussian 0 is a needle on the optical axis, along the camera's x axis: the
    # squares of its two short scales underflow, so its pre-blur 2-D covariance has determinant exactly 0.  (Not scales of exactly 0:
    # the classic backward divides the scale gradient by the scale.)
    inp = dict(means=torch.stack([u(N) - 0.5, 0.8 * u(N) - 0.4, 2.0 + 2.0 * u(N)], -1), quats=torch.randn(N, 4, generator=g),
               scales=0.02 + 0.06 * u(N, 3), opac=0.3 + 0.6 * u(N), colors=u(N, 3), V=torch.eye(4),
               K=torch.tensor([[60.0, 0.0, W / 2], [0.0, 60.0, H / 2], [0.0, 0.0, 1.0]]))
    inp["means"][0] = torch.tensor([0.0, 0.0, 2.0])
    inp["quats"][0] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    inp["scales"][0] = torch.tensor([0.5, 1e-25, 1e-25])
    inp["opac"][0] = 0.9
    rc, ra, info, t = _render(inp, W, H, "RGB+ED", np.array([0.3, 0.5, 0.7]), exact_cull=exact_cull)
    assert int(info["radii"][0, 0]) > 0
    assert float(info["opacities"][0, 0]) == 0.0
    rng = np.random.default_rng(1)
    _backward(rc, ra, info, rng.standard_normal((H, W, 4)), rng.standard_normal((H, W, 1)))
    for x in (rc, ra, info["opacities"], info["means2d"].grad, *[t[k].grad for k in NAMES]):
        assert bool(torch.isfinite(x).all())
    for k in ("means", "quats", "scales", "opac", "colors"):
        assert bool((t[k].grad[0] == 0).all()), k
    assert bool((info["means2d"].grad[0, 0] == 0).all())


@pytest.mark.parametrize("D", [3, 16])
def test_row_modes_lazy_lists_and_depth_segments(D, monkeypatch):
    from deblur4dgs_amd import engine

    sc = ladder.ladder_scene(48, 48, [63, 64, 65, 256, 257, 1, 2], seed=191 + D, D=D)
    W, H = sc["W"], sc["H"]
    inp = {k: sc[k] for k in ("means", "quats", "scales", "opac", "colors", "V", "K")}
    bg = np.linspace(0.1, 0.9, D)
    rng = np.random.default_rng(7)
    w_c, w_a = rng.standard_normal((H, W, D + 1)), rng.standard_normal((H, W, 1))
    got = {}
    for rows in ("dense", "sparse"):
        for seg in ("0", "1"):
            for lazy in (False, True):
                monkeypatch.setattr(engine, "BWD_ROWS", rows)
                monkeypatch.setenv("D4GS_SEG", seg)
                rc, ra, info, t = _render(inp, W, H, "RGB+ED", bg, lazy_sort=lazy, exact_tiles=False)
                _backward(rc, ra, info, w_c, w_a)
                got[(rows, seg, lazy)] = _grads(rc, ra, info, t)
    base = got[("dense", "0", False)]
    assert float(base["opac"].abs().sum()) > 0
    for key, r in got.items():
        for k in r:
            if key[1] == "0":  # row modes and lazy lists: the same bits
                assert torch.equal(r[k], base[k]), (key, k)
            else:  # depth segments: the hand-off's rounding
                assert rel_err(r[k], base[k]) <= SEG_TOL, (key, k)


def test_backward_is_run_to_run_bitwise():
    N, W, H = 2500, 128, 80
    inp = static_inputs(N, W, H, seed=8, dtype=torch.float32, D=3)
    rng = np.random.default_rng(0)
    w_c, w_a = rng.standard_normal((H, W, 4)), rng.standard_normal((H, W, 1))
    runs = []
    for _ in range(3):
        rc, ra, info, t = _render(inp, W, H, "RGB+ED", np.array([0.3, 0.5, 0.7]))
        _backward(rc, ra, info, w_c, w_a)
        runs.append(_grads(rc, ra, info, t))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k


def test_with_sh_degree_3_and_absgrad():
    from tests.absgrad_ref import absgrad_of_composite
    from tests.sh_ref import sh_colors

    N, W, H = 600, 64, 48
    inp = static_inputs(N, W, H, seed=77, dtype=torch.float64, D=3)
    g = torch.Generator().manual_seed(5)
    coeffs = 0.3 * torch.randn(N, 16, 3, generator=g, dtype=torch.float64)
    w_c = torch.randn(H, W, 3, generator=g, dtype=torch.float64)
    t = {k: v.clone().requires_grad_(k != "K") for k, v in dict(inp, colors=coeffs).items()}
    cols = sh_colors(t["means"], t["V"], t["colors"], 3)
    ref_c, _, ref_info = antialias_ref.rasterization(t["means"], t["quats"], t["scales"], t["opac"], cols, t["V"], t["K"], W, H)
    ref_info["means2d"].retain_grad()
    (ref_c * w_c).sum().backward()
    ref_abs, _ = absgrad_of_composite(ref_info["means2d"], ref_info["conics"], cols, ref_info["opacities"], W, H,
                                      ref_info["flatten_ids"], ref_info["isect_offsets"], w_c)
    rc, ra, info, tg = _render(dict(inp, colors=coeffs), W, H, sh_degree=3, absgrad=True)
    _backward(rc, ra, info, w_c, None)
    case = f"antialiased sh_degree=3 absgrad N={N} {W}x{H}"
    check(case, "render_colors", rc[0].detach().cpu(), ref_c.detach(), TOL, GFLIPS)
    check(case, "means2d.absgrad", info["means2d"].absgrad[0].cpu(), ref_abs, GTOL, GFLIPS)
    check(case, "means2d.grad", info["means2d"].grad[0].cpu(), ref_info["means2d"].grad, GTOL, GFLIPS)
    for name in ("means", "quats", "scales", "opac", "colors"):
        check(case, name, tg[name].grad.cpu(), t[name].grad, GTOL, GFLIPS)
    check(case, "viewmat", tg["V"].grad.cpu()[:3], t["V"].grad[:3], VTOL, 0.0)


@pytest.mark.parametrize("K,exact_tiles", [(6, None), (6, True), (12, True)])
def test_exposure_path_chains_oracle_and_fused_statistics(K, exact_tiles, monkeypatch):
    """exact_tiles=True runs the exact-tiles projection kernels: K = 6 blends the motion bases in LDS, K = 12 (>= 10) reads them
    from the global table (k_project_fwd's TAB instantiations)."""
    from deblur4dgs_amd import control
    from deblur4dgs_amd.exposure import render_exposure
    from deblur4dgs_amd.synth import make_scene
    from oracle import scene as oscene
    from tests.test_gpu_exposure import _split

    dev = torch.device("cuda:0")
    S, N, G, W, H = 8, 3000, 1200, 96, 64
    sc = make_scene(N, G, K, S, W, H, seed=21, dtype=torch.float64)
    if exact_tiles:  # splats a few tiles wide: rectangles of 2 x 2 ... 8 x 8 tiles get masks
        sc["scales"] = sc["scales"] + 1.0
    # the exposure oracle with the antialiased rasterizer (oracle/scene.py looks it up as raster.rasterization)
    monkeypatch.setattr(oracle.raster, "rasterization", antialias_ref.rasterization)
    fg, bgp, bases = _split(sc, torch.float64)
    times, RTs = sc["times"].clone().requires_grad_(), sc["RTs"].clone().requires_grad_()
    w2c = sc["viewmat"].clone().requires_grad_()
    out = oscene.render_exposure(fg, bgp, bases, times, RTs, w2c, sc["K"], (W, H), bg_color=1.0, return_depth=True)
    blended_ref = torch.cat([out["img"], out["depth"]], -1)[0]
    g = torch.Generator().manual_seed(2)
    w_b = torch.randn(blended_ref.shape, generator=g, dtype=torch.float64)
    w_a = torch.randn(out["acc"][0].shape, generator=g, dtype=torch.float64)
    ((blended_ref * w_b).sum() + (out["acc"][0] * w_a).sum()).backward()
    ref = {k: torch.cat([p[k].grad for p in (fg, bgp) if p is not None], 0) for k in ("means", "quats", "scales", "colors", "opacities")}

    res = {}
    for fused in (True, False):
        P = {k: sc[k].float().to(dev).requires_grad_() for k in ("means", "quats", "scales", "opacities", "colors", "motion_coefs",
                                                                  "rots", "transls")}
        vm = sc["viewmat"].float().to(dev).requires_grad_()
        stats = control.new_running_stats(N, dev)
        cs = dict(stats, batch_size=2, update_max_radii=True)
        o = render_exposure(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], 3, P["motion_coefs"], P["rots"],
                            P["transls"], sc["times"].float().to(dev), sc["RTs"].float().to(dev), vm, sc["K"].float().to(dev), W, H,
                            background=torch.ones(3, device=dev), return_depth=True, control_stats=cs, fused=fused, antialiased=True,
                            exact_tiles=exact_tiles)
        st = o["state"]
        assert bool(st.frame_io) == fused
        if exact_tiles:
            assert st.cfg.exact_tiles and st.cfg.exact_cull
            if not fused:  # the projection's per-tile test ran: it left masks
                assert bool((st.proj_out["tile_masks"] != 0).any())
        case = f"antialiased exposure fused={fused} N={N} G={G} K={K} S={S} {W}x{H} exact_tiles={exact_tiles}"
        check(case, "blended", o["blended"].detach().cpu(), blended_ref.detach(), TOL, GFLIPS)
        check(case, "acc", o["acc"].detach().cpu(), out["acc"][0, ..., 0].detach(), TOL, GFLIPS)
        if not fused:
            o["means2d"].retain_grad()
        ((o["blended"] * w_b.float().to(dev)).sum() + (o["acc"] * w_a[..., 0].float().to(dev)).sum()).backward()
        torch.cuda.synchronize()
        for k in ref:
            check(case, k, P[k].grad.cpu(), ref[k], GTOL, GFLIPS)
        check(case, "viewmat", vm.grad.cpu()[:3], w2c.grad[:3], VTOL, 0.0)
        v_m2d = st.v_means2d if fused else o["means2d"].grad
        assert v_m2d is not None and v_m2d.shape == (S, N, 2)
        # the fused statistics are d4gs_control_stats on the returned v_means2d, bit for bit
        again = control.new_running_stats(N, dev)
        control.accumulate_control_stats(again, v_m2d, o["radii"], (W, H), 2)
        torch.cuda.synchronize()
        for k in ("xys_grad_norm_acc", "vis_count"):
            assert torch.equal(stats[k], again[k]), (fused, k)
        assert float(stats["xys_grad_norm_acc"].sum()) > 0
        res[fused] = dict({k: P[k].grad.cpu().clone() for k in P}, blended=o["blended"].detach().cpu().clone(),
                          v_m2d=v_m2d.detach().cpu().clone(), viewmat=vm.grad.cpu().clone())
    for k in res[True]:
        assert torch.equal(res[True][k], res[False][k]), k
