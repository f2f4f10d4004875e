"""GPU: gsplat's `absgrad` (`rasterization(absgrad=True)`, `info["means2d"].absgrad`) from the composite backward (D4GS_ABSGRAD).

  - parity with the fp64 per-pixel reference (tests/absgrad_ref.py) over the instantiated channel counts and render modes, with and
    without v_alphas / background, and through sh_degree;
  - the flag changes nothing else: images and every other gradient are bitwise equal with it on and off;
  - dense vs sparse gradient rows, lazy vs eager lists: bitwise; depth-segmented vs whole-list replay: the hand-off's rounding;
    lists of 63..65 and 256 / 257 entries (tests/ladder.py);
  - run-to-run bitwise;
  - the exposure path (S = 8): one-call FrameFn and the staged chain agree, and their fused absgrad statistics are bitwise what
    d4gs_control_stats computes from the returned absgrad;
  - a render of more than 16 colour channels is refused."""
import numpy as np
import pytest
import torch

from oracle import cref, margins
from tests import ladder
from tests.absgrad_ref import absgrad_of_rasterization
from tests.util import check, rel_err, static_inputs

pytestmark = pytest.mark.gpu

GTOL = 1e-4    # tests/test_gpu_rasterization.py's means2d.grad norm and flip allowance
GFLIPS = 2e-3
SEG_TOL = 2e-5  # depth-segmented vs whole-list replay (tests/test_gpu_list_edges.py)
EPS = 1e-5      # ladder scenes: decision margins below this are masked (as tests/test_gpu_list_edges.py does)


def _render(inp, W, H, mode, bg, absgrad=True, sh_degree=None, **kw):
    from deblur4dgs_amd.rasterization import rasterization

    dev = torch.device("cuda:0")
    t = {k: torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(torch.float32).to(dev) for k, v in inp.items()}
    for k in ("means", "quats", "scales", "opac", "colors", "V"):
        t[k].requires_grad_()
    rc, ra, info = rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"][None], t["K"][None], W, H,
                                 backgrounds=None if bg is None else torch.as_tensor(bg).to(dev).float()[None], render_mode=mode,
                                 absgrad=absgrad, sh_degree=sh_degree, **kw)
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
    out = dict(rc=rc.detach(), ra=ra.detach(), means2d=info["means2d"].grad)
    out.update({k: t[k].grad for k in ("means", "quats", "scales", "opac", "colors", "V")})
    return {k: v.detach().cpu().clone() for k, v in out.items()}


PARITY = [(D, mode) for D in (1, 3, 4, 5, 8, 16) for mode in ("RGB", "RGB+ED", "RGB+D")]


@pytest.mark.parametrize("D,mode", PARITY)
def test_absgrad_matches_the_fp64_per_pixel_reference(D, mode):
    i = PARITY.index((D, mode))
    with_va, with_bg = (i % 4) in (0, 1), (i % 4) in (0, 2)  # the four combinations in turn
    N, W, H = 700, 72, 56
    inp = static_inputs(N, W, H, seed=300 + i, dtype=torch.float64, D=D)
    bg = torch.linspace(0.1, 0.9, D, dtype=torch.float64) if with_bg else None
    nch = D + (mode != "RGB")
    g = torch.Generator().manual_seed(11 + i)
    w_c = torch.randn(H, W, nch, generator=g, dtype=torch.float64)
    w_a = torch.randn(H, W, 1, generator=g, dtype=torch.float64) if with_va else None
    ref_abs, _, _ = absgrad_of_rasterization(inp["means"], inp["quats"], inp["scales"], inp["opac"], inp["colors"], inp["V"],
                                             inp["K"], W, H, w_c, w_a, bg, mode)
    rc, ra, info, _ = _render(inp, W, H, mode, bg)
    _backward(rc, ra, info, w_c, w_a)
    got = info["means2d"].absgrad
    assert got.shape == (1, N, 2) and got.dtype == torch.float32
    assert bool((got >= 0).all())
    case = f"absgrad {mode} D={D} N={N} {W}x{H} v_alphas={with_va} bg={with_bg}"
    check(case, "means2d.absgrad", got[0].cpu(), ref_abs, GTOL, GFLIPS)
    culled = info["radii"][0] == 0
    assert bool((got[0][culled] == 0).all())


def test_absgrad_with_sh_degree_3():
    from tests.sh_ref import sh_colors

    N, W, H = 600, 64, 48
    inp = static_inputs(N, W, H, seed=77, dtype=torch.float64, D=3)
    g = torch.Generator().manual_seed(5)
    coeffs = 0.3 * torch.randn(N, 16, 3, generator=g, dtype=torch.float64)
    w_c = torch.randn(H, W, 3, generator=g, dtype=torch.float64)
    inp_sh = dict(inp, colors=coeffs)
    rc, ra, info, t = _render(inp_sh, W, H, "RGB", None, sh_degree=3)
    _backward(rc, ra, info, w_c, None)
    cols = sh_colors(inp["means"], inp["V"], coeffs, 3)  # the colours the seam composites, in fp64
    ref_abs, _, _ = absgrad_of_rasterization(inp["means"], inp["quats"], inp["scales"], inp["opac"], cols, inp["V"], inp["K"], W, H,
                                             w_c)
    check(f"absgrad sh_degree=3 N={N} {W}x{H}", "means2d.absgrad", info["means2d"].absgrad[0].cpu(), ref_abs, GTOL, GFLIPS)


@pytest.mark.parametrize("D,mode", [(3, "RGB+ED"), (4, "RGB"), (8, "RGB+D"), (16, "RGB+ED"), (6, "RGB")])
def test_the_flag_leaves_every_other_output_bitwise_unchanged(D, mode):
    N, W, H = 1500, 96, 64
    inp = static_inputs(N, W, H, seed=40 + D, dtype=torch.float32, D=D)
    bg = np.linspace(0.2, 0.8, D)
    nch = D + (mode != "RGB")
    rng = np.random.default_rng(D)
    w_c, w_a = rng.standard_normal((H, W, nch)), rng.standard_normal((H, W, 1))
    res = {}
    for flag in (False, True):
        rc, ra, info, t = _render(inp, W, H, mode, bg, absgrad=flag)
        _backward(rc, ra, info, w_c, w_a)
        res[flag] = _grads(rc, ra, info, t)
        assert hasattr(info["means2d"], "absgrad") == flag
    for k in res[False]:
        assert torch.equal(res[False][k], res[True][k]), k


def _ladder_case(D):
    sc = ladder.ladder_scene(48, 48, [63, 64, 65, 256, 257, 1, 2], seed=91 + D, D=D)
    return sc


@pytest.mark.parametrize("D", [3, 16])
def test_row_modes_lazy_lists_and_depth_segments(D, monkeypatch):
    from deblur4dgs_amd import engine

    sc = _ladder_case(D)
    W, H = sc["W"], sc["H"]
    inp = {k: sc[k] for k in ("means", "quats", "scales", "opac", "colors", "V", "K")}
    bg = np.linspace(0.1, 0.9, D)
    out, al, ctx = cref.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opac"], sc["colors"], sc["V"], sc["K"], W, H,
                                      background=bg, render_mode="RGB+ED", dtype=np.float64)
    n = ctx["n_isect"]
    mg = margins.pixel_margins(torch.from_numpy(ctx["m2d"]), torch.from_numpy(ctx["con"]), torch.from_numpy(sc["opac"]),
                               torch.from_numpy(ctx["dep"]), torch.from_numpy(ctx["flat"][:n]).long(), torch.from_numpy(ctx["offs"]).long(),
                               W, H)
    F = margins.fragile_pixels(mg, EPS, eps_order=0.0)
    assert float(F.float().mean()) <= 0.05
    keep = (~F).double().numpy()[..., None]
    rng = np.random.default_rng(3)
    w_c, w_a = rng.standard_normal(out.shape) * keep, rng.standard_normal(al.shape) * keep
    dt = lambda k: torch.from_numpy(np.asarray(sc[k], np.float64))
    ref_abs, _, _ = absgrad_of_rasterization(dt("means"), dt("quats"), dt("scales"), dt("opac"), dt("colors"), dt("V"), dt("K"), W, H,
                                             torch.from_numpy(w_c), torch.from_numpy(w_a), torch.from_numpy(bg), "RGB+ED")
    got = {}
    for rows in ("dense", "sparse"):
        for seg in ("0", "1"):
            for lazy in (False, True):
                monkeypatch.setattr(engine, "BWD_ROWS", rows)
                monkeypatch.setenv("D4GS_SEG", seg)
                rc, ra, info, t = _render(inp, W, H, "RGB+ED", bg, lazy_sort=lazy, exact_tiles=False)
                assert info["n_isect"] == n
                _backward(rc, ra, info, w_c, w_a)
                got[(rows, seg, lazy)] = dict(_grads(rc, ra, info, t), absgrad=info["means2d"].absgrad.cpu().clone())
                check(f"absgrad ladder D={D} rows={rows} seg={seg} lazy={lazy}", "means2d.absgrad", got[(rows, seg, lazy)]["absgrad"][0],
                      ref_abs, GTOL, GFLIPS)
    base = got[("dense", "0", False)]
    for key, r in got.items():
        for k in r:
            if key[1] == "0":  # row modes and lazy lists: the same bits
                assert torch.equal(r[k], base[k]), (key, k)
            elif k == "absgrad":  # depth segments: the hand-off's rounding
                assert rel_err(r[k], got[("dense", "1", False)][k]) == 0.0, key
                assert rel_err(r[k], base[k]) <= SEG_TOL, key


def test_absgrad_is_run_to_run_bitwise():
    N, W, H = 2500, 128, 80
    inp = static_inputs(N, W, H, seed=8, dtype=torch.float32, D=3)
    rng = np.random.default_rng(0)
    w_c, w_a = rng.standard_normal((H, W, 4)), rng.standard_normal((H, W, 1))
    runs = []
    for _ in range(3):
        rc, ra, info, t = _render(inp, W, H, "RGB+ED", np.array([0.3, 0.5, 0.7]))
        _backward(rc, ra, info, w_c, w_a)
        runs.append(info["means2d"].absgrad.cpu().clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_exposure_path_fused_statistics_and_staged_chain():
    from deblur4dgs_amd import control
    from deblur4dgs_amd.exposure import render_exposure
    from deblur4dgs_amd.synth import make_scene

    dev = torch.device("cuda:0")
    S, N, G, K, W, H = 8, 3000, 1200, 6, 128, 96
    sc = make_scene(N, G, K, S, W, H, seed=21)
    res = {}
    for fused in (True, False):
        P = {k: sc[k].to(dev).requires_grad_() for k in ("means", "quats", "scales", "opacities", "colors", "motion_coefs", "rots",
                                                          "transls")}
        stats = control.new_running_stats(N, dev)
        cs = dict(stats, batch_size=2, update_max_radii=False, absgrad=True)
        out = render_exposure(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], 3, P["motion_coefs"], P["rots"],
                              P["transls"], sc["times"].to(dev), sc["RTs"].to(dev), sc["viewmat"].to(dev), sc["K"].to(dev), W, H,
                              return_depth=True, control_stats=cs, fused=fused, absgrad=True)
        st = out["state"]
        assert bool(st.frame_io) == fused
        (out["blended"].square().sum() + out["acc"].sum()).backward()
        torch.cuda.synchronize()
        ab = st.v_means2d_abs
        assert ab is not None and ab.shape == (S, N, 2)
        if not fused:
            assert torch.equal(out["means2d"].absgrad, ab)
        # the fused statistics are d4gs_control_stats on the returned absgrad, bit for bit
        again = control.new_running_stats(N, dev)
        control.accumulate_control_stats(again, ab, out["radii"], (W, H), 2)
        torch.cuda.synchronize()
        for k in ("xys_grad_norm_acc", "vis_count", "max_radii"):
            assert torch.equal(stats[k], again[k]), (fused, k)
        assert float(stats["xys_grad_norm_acc"].sum()) > 0
        res[fused] = (ab.cpu().clone(), {k: v.cpu().clone() for k, v in stats.items()}, P["means"].grad.cpu().clone())
    assert torch.equal(res[True][0], res[False][0])
    for k in res[True][1]:
        assert torch.equal(res[True][1][k], res[False][1][k]), k
    assert torch.equal(res[True][2], res[False][2])


def test_scene_model_exposes_absgrad_on_current_xys():
    from deblur4dgs_amd import control
    from tests.test_gpu_scene_model import _build

    dev = torch.device("cuda:0")
    N, G, K, W, H = 1500, 800, 3, 96, 64
    for fused in (True, False):
        model, sc = _build(N, G, K, W, H, 23, dev)
        model.fused = fused
        stats = control.new_running_stats(N, dev)
        model.attach_control_stats(stats, batch_size=1, absgrad=True)
        out = model.render(3.0, sc["viewmat"][None].to(dev), sc["K"][None].to(dev), (W, H), return_depth=True, mode="blury")
        out["img"].square().sum().backward()
        torch.cuda.synchronize()
        xs = model._current_xys
        assert all(getattr(x, "absgrad", None) is not None for x in xs)
        ab = torch.cat([x.absgrad for x in xs], 0)
        again = control.new_running_stats(N, dev)
        control.accumulate_from_model(again, model, batch_size=1, absgrad=True)
        torch.cuda.synchronize()
        for k in ("xys_grad_norm_acc", "vis_count"):
            assert torch.equal(stats[k], again[k]), (fused, k)
        assert bool((ab >= 0).all())
        model.detach_control_stats()


def test_more_than_sixteen_channels_is_refused():
    N, W, H = 300, 48, 32
    inp = static_inputs(N, W, H, seed=3, dtype=torch.float32, D=20)
    with pytest.raises(NotImplementedError, match="per-chunk sums"):
        _render(inp, W, H, "RGB", None)
    rc, ra, info, t = _render(inp, W, H, "RGB", None, absgrad=False)  # (without absgrad the same render is fine)
    assert rc.shape == (1, H, W, 20)
