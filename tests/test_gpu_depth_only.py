"""GPU: gsplat's depth-only render modes "D" / "ED" through the depth-only composite kernels (D4gsDims.D == 0 with a depth mode).

  - parity with the fp64 oracle (oracle.raster.rasterization, render_mode "D" / "ED"): image, alpha and the gradients of every leaf,
    of viewmat and of info["means2d"], with and without a background (ignored) and v_alphas, exact tiles on and off, several seeds and
    sizes, and a scene whose lists cross the 256-key depth-segment unit;
  - the antialiased mode against tests/antialias_ref.py (info["opacities"] included), absgrad against tests/absgrad_ref.py;
  - closed-form answers for one isotropic splat on a pixel centre;
  - lazy lists and dense / sparse rows: bitwise; depth segments: the image bitwise, the gradients within the hand-off's rounding;
  - the depth channel of "D" against the last channel of "RGB+D" with a zero background;
  - N == 0, and sh_degree = 3: no SH kernel launch, colors.grad stays None."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import oracle.raster
from oracle import margins
from tests import absgrad_ref, antialias_ref, ladder
from tests.util import check, rel_err, static_inputs

pytestmark = pytest.mark.gpu

TOL = 1e-4       # tests/test_gpu_antialias.py's tolerance and flip allowance
GTOL = 1e-4
GFLIPS = 2e-3
VTOL = 1e-4      # viewmat: a sum over every Gaussian, no allowance
SEG_TOL = 2e-5   # depth-segmented vs whole-list replay (tests/test_gpu_list_edges.py)
NAMES = ("means", "quats", "scales", "opac", "colors", "V")
LEAVES = ("means", "quats", "scales", "opac")


def _render(inp, W, H, mode, bg=None, aa=False, **kw):
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
    out = dict(rc=rc.detach(), ra=ra.detach(), means2d=info["means2d"].grad)
    out.update({k: t[k].grad for k in LEAVES + ("V",)})
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _ref(inp, W, H, mode, bg, aa):
    t = {k: v.clone().requires_grad_(k != "K") for k, v in inp.items()}
    fn = antialias_ref.rasterization if aa else oracle.raster.rasterization
    ref_c, ref_a, ref_info = fn(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"], t["K"], W, H, background=bg,
                                render_mode=mode)
    return t, ref_c, ref_a, ref_info


def _parity(mode, seed, N, W, H, with_va, with_bg, exact_tiles, scale_mul=3.0, aa=False, inp=None):
    inp = inp or static_inputs(N, W, H, seed=seed, dtype=torch.float64, D=3, scale_mul=scale_mul)
    N = inp["means"].shape[0]
    bg = torch.tensor([0.3, 0.5, 0.7], dtype=torch.float64) if with_bg else None
    t, ref_c, ref_a, ref_info = _ref(inp, W, H, mode, bg, aa)
    assert ref_c.shape == (H, W, 1)
    # pixels of tiles whose list membership could toggle in float32 take no cotangent (tests/test_gpu_flip_cause.py's argument)
    eff = (inp["opac"] * ref_info["compensations"].detach()).clamp(min=1e-300) if aa else inp["opac"]
    toggles, _ = margins.gaussian_toggle_mask(inp["means"], inp["quats"], inp["scales"], eff, inp["V"], inp["K"], W, H)
    keep = (~toggles).double()[..., None]
    g = torch.Generator().manual_seed(seed + 7)
    w_c = torch.randn(ref_c.shape, generator=g, dtype=torch.float64) * keep
    w_a = torch.randn(ref_a.shape, generator=g, dtype=torch.float64) * keep if with_va else None
    ref_info["means2d"].retain_grad()
    ((ref_c * w_c).sum() + ((ref_a * w_a).sum() if with_va else 0.0)).backward()

    rc, ra, info, tg = _render(inp, W, H, mode, bg.numpy() if with_bg else None, aa=aa, exact_tiles=exact_tiles)
    assert rc.shape == (1, H, W, 1) and ra.shape == (1, H, W, 1)
    _backward(rc, ra, info, w_c, w_a)
    case = (f"depth-only {mode}{' antialiased' if aa else ''} N={N} {W}x{H} v_alphas={with_va} bg={with_bg}"
            f"{' exact_tiles' if exact_tiles else ''}")
    check(case, "render_colors", rc[0].detach().cpu(), ref_c.detach(), TOL, GFLIPS)
    check(case, "render_alphas", ra[0].detach().cpu(), ref_a.detach(), TOL, GFLIPS)
    if aa:
        check(case, "info.opacities", info["opacities"][0].cpu(), ref_info["opacities"].detach(), TOL, GFLIPS)
    check(case, "means2d.grad", info["means2d"].grad[0].cpu(), ref_info["means2d"].grad, GTOL, GFLIPS)
    for name in LEAVES:
        check(case, name, tg[name].grad.cpu(), t[name].grad, GTOL, GFLIPS)
    check(case, "viewmat", tg["V"].grad.cpu()[:3], t["V"].grad[:3], VTOL, 0.0)
    assert tg["colors"].grad is None  # never composited (gsplat computes the colours and discards them)
    assert float(rc.detach().abs().sum()) > 0 and float(tg["means"].grad.abs().sum()) > 0
    return rc, ra, info


PARITY = [(mode, i) for mode in ("D", "ED") for i in range(4)]


@pytest.mark.parametrize("mode,i", PARITY)
def test_depth_only_matches_the_fp64_oracle(mode, i):
    N, W, H = ((700, 72, 56), (1500, 96, 64), (400, 40, 33), (1200, 128, 48))[i]
    _parity(mode, 600 + 10 * i + (mode == "ED"), N, W, H, with_va=i in (0, 1), with_bg=i in (0, 2), exact_tiles=i % 2 == 1,
            scale_mul=3.0 if i < 2 else 5.0)


@pytest.mark.parametrize("mode", ["D", "ED"])
def test_depth_only_lists_across_the_segment_unit_match_the_oracle(mode, monkeypatch):
    """Lists of 257 .. 513 keys: more than one depth segment of 256 (the composite backward replays them in parallel)."""
    monkeypatch.setenv("D4GS_SEG", "1")
    sc = ladder.ladder_scene(48, 48, [257, 300, 513, 64, 1, 255, 256, 20, 400], seed=41 + (mode == "ED"), D=3)
    inp = {k: torch.as_tensor(sc[k], dtype=torch.float64) for k in ("means", "quats", "scales", "opac", "colors", "V", "K")}
    rc, ra, info = _parity(mode, 77, 0, sc["W"], sc["H"], with_va=True, with_bg=False, exact_tiles=False, inp=inp)
    offs = torch.cat([info["isect_offsets"].flatten().cpu().long(), torch.tensor([info["n_isect"]])])
    assert int((offs[1:] - offs[:-1]).max()) > 256


@pytest.mark.parametrize("mode", ["D", "ED"])
def test_antialiased_depth_only_matches_the_reference(mode):
    _parity(mode, 700 + (mode == "ED"), 700, 72, 56, with_va=True, with_bg=True, exact_tiles=False, scale_mul=1.5, aa=True)
    _parity(mode, 710 + (mode == "ED"), 900, 80, 64, with_va=False, with_bg=False, exact_tiles=True, scale_mul=4.0, aa=True)


@pytest.mark.parametrize("mode", ["D", "ED"])
def test_absgrad_of_a_depth_only_render(mode):
    N, W, H = 700, 72, 56
    inp = static_inputs(N, W, H, seed=800 + (mode == "ED"), dtype=torch.float64, D=3)
    g = torch.Generator().manual_seed(3)
    w_c = torch.randn(H, W, 1, generator=g, dtype=torch.float64)
    w_a = torch.randn(H, W, 1, generator=g, dtype=torch.float64)
    with torch.no_grad():
        radii, means2d, depths, conics = oracle.raster.project(inp["means"], inp["quats"], inp["scales"], inp["V"], inp["K"], W, H)
        _, flatten_ids, isect_offsets = oracle.raster.isect_tiles(means2d, radii, depths, W, H)
    ref_abs, _ = absgrad_ref.absgrad_of_composite(means2d, conics, depths[:, None], inp["opac"], W, H, flatten_ids, isect_offsets, w_c,
                                                  w_a, None, ed=mode == "ED")
    rc, ra, info, _ = _render(inp, W, H, mode, absgrad=True)
    _backward(rc, ra, info, w_c, w_a)
    got = info["means2d"].absgrad
    assert got.shape == (1, N, 2) and bool((got >= 0).all()) and float(got.sum()) > 0
    check(f"absgrad depth-only {mode} N={N} {W}x{H}", "means2d.absgrad", got[0].cpu(), ref_abs, GTOL, GFLIPS)
    assert bool((got[0][info["radii"][0] == 0] == 0).all())


def _one_splat(s3, z, opac, W=33, H=33, f=40.0):
    """one isotropic Gaussian on the optical axis, projected onto the centre of pixel (16, 16)"""
    return dict(means=torch.tensor([[0.0, 0.0, z]]), quats=torch.tensor([[1.0, 0.0, 0.0, 0.0]]), scales=torch.full((1, 3), s3),
                opac=torch.tensor([opac]), colors=torch.tensor([[0.2, 0.6, 0.9]]), V=torch.eye(4),
                K=torch.tensor([[f, 0.0, 16.5], [0.0, f, 16.5], [0.0, 0.0, 1.0]]))


@pytest.mark.parametrize("s3,z,opac", [(0.05, 2.0, 0.8), (0.1, 4.0, 0.5), (0.3, 3.0, 0.99)])
def test_isotropic_splat_known_answers(s3, z, opac):
    inp = _one_splat(s3, z, opac)
    rc_d, ra, info, _ = _render(inp, 33, 33, "D", bg=np.array([5.0, 5.0, 5.0]))
    rc_e, ra_e, _, _ = _render(inp, 33, 33, "ED")
    assert int(info["radii"][0, 0]) > 0 and torch.equal(ra, ra_e)
    alpha = min(opac, 0.999)
    # sigma = 0 at the centre pixel: alpha = opacity; "D" = z alpha, "ED" = z (render_alphas = 1 - (1 - alpha): an ulp of 1 off)
    assert math.isclose(float(ra[0, 16, 16, 0]), alpha, rel_tol=1e-5)
    assert math.isclose(float(rc_d[0, 16, 16, 0]), z * alpha, rel_tol=1e-5)
    lit = ra[0, ..., 0] > 0
    assert int(lit.sum()) > 1 and bool((rc_d[0, ..., 0][~lit] == 0).all())  # the background is ignored
    assert torch.allclose(rc_e[0, ..., 0][lit], torch.full_like(rc_e[0, ..., 0][lit], z), rtol=1e-5, atol=0)
    assert bool((rc_e[0, ..., 0][~lit] == 0).all())


def test_row_modes_lazy_lists_and_depth_segments(monkeypatch):
    from deblur4dgs_amd import engine

    sc = ladder.ladder_scene(48, 48, [63, 64, 65, 256, 257, 600, 1, 2], seed=193, D=3)
    W, H = sc["W"], sc["H"]
    inp = {k: sc[k] for k in ("means", "quats", "scales", "opac", "colors", "V", "K")}
    rng = np.random.default_rng(9)
    w_c, w_a = rng.standard_normal((H, W, 1)), rng.standard_normal((H, W, 1))
    for mode in ("D", "ED"):
        got = {}
        for rows in ("dense", "sparse"):
            for seg in ("0", "1"):
                for lazy in (False, True):
                    monkeypatch.setattr(engine, "BWD_ROWS", rows)
                    monkeypatch.setenv("D4GS_SEG", seg)
                    rc, ra, info, t = _render(inp, W, H, mode, lazy_sort=lazy, exact_tiles=False)
                    _backward(rc, ra, info, w_c, w_a)
                    got[(rows, seg, lazy)] = _grads(rc, ra, info, t)
        base = got[("dense", "0", False)]
        assert float(base["opac"].abs().sum()) > 0
        for key, r in got.items():
            for k in r:
                if key[1] == "0" or k in ("rc", "ra"):  # row modes and lazy lists: the same bits; segments: the same image
                    assert torch.equal(r[k], base[k]), (mode, key, k)
                else:  # depth segments' gradients: the hand-off's rounding
                    assert rel_err(r[k], base[k]) <= SEG_TOL, (mode, key, k)


@pytest.mark.parametrize("exact_tiles", [False, True])
def test_depth_channel_equals_the_rgb_plus_d_render(exact_tiles):
    """The depth-only kernel composites the same depth with the same transmittance as the RGB+D kernels: the image is the last
    channel of an RGB+D render with a zero background, bit for bit (asserted to 1e-6 relative, and bitwise)."""
    N, W, H = 2500, 128, 80
    inp = static_inputs(N, W, H, seed=91, dtype=torch.float32, D=3)
    rc, ra, _, _ = _render(inp, W, H, "D", exact_tiles=exact_tiles)
    rc3, ra3, _, _ = _render(inp, W, H, "RGB+D", bg=np.zeros(3), exact_tiles=exact_tiles)
    assert rel_err(rc[..., 0], rc3[..., 3]) <= 1e-6
    assert torch.equal(rc[..., 0], rc3[..., 3]) and torch.equal(ra, ra3)


@pytest.mark.parametrize("mode", ["D", "ED"])
def test_empty_scene(mode):
    inp = dict(means=torch.zeros(0, 3), quats=torch.zeros(0, 4), scales=torch.zeros(0, 3), opac=torch.zeros(0), colors=torch.zeros(0, 3),
        V=torch.eye(4), K=torch.tensor([[30.0, 0.0, 16.0], [0.0, 30.0, 12.0], [0.0, 0.0, 1.0]]))
    rc, ra, info, t = _render(inp, 32, 24, mode, bg=np.array([0.3, 0.5, 0.7]), absgrad=True)
    assert rc.shape == (1, 24, 32, 1) and ra.shape == (1, 24, 32, 1)
    assert float(rc.abs().sum()) == 0 and float(ra.abs().sum()) == 0
    rc.sum().backward()
    assert t["means"].grad.shape == (0, 3)


def _launches(fn):
    from deblur4dgs_amd import _lib as L

    lib = L.lib()
    buf = C.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    lib.d4gs_profile_collect(buf, C.c_size_t(len(buf)))  # (drops anything recorded before)
    lib.d4gs_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.d4gs_profile_enable(0)
    lib.d4gs_profile_collect(buf, C.c_size_t(len(buf)))
    return out, {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines()}


@pytest.mark.parametrize("mode", ["D", "ED"])
def test_sh_coefficients_are_neither_evaluated_nor_differentiated(mode):
    N, W, H = 600, 64, 48
    inp = static_inputs(N, W, H, seed=55, dtype=torch.float64, D=3)
    g = torch.Generator().manual_seed(2)
    coeffs = 0.3 * torch.randn(N, 16, 3, generator=g, dtype=torch.float64)
    w_c = torch.randn(H, W, 1, generator=g, dtype=torch.float64)

    def run():
        rc, ra, info, t = _render(dict(inp, colors=coeffs), W, H, mode, sh_degree=3)
        _backward(rc, ra, info, w_c, None)
        return rc, t

    (rc, t), launches = _launches(run)
    assert not any(k.startswith("k_sh") for k in launches), launches
    assert launches.get("k_raster_fwd_r", 0) >= 1 and launches.get("k_raster_bwd_q", 0) == 1, launches
    assert t["colors"].grad is None and t["means"].grad is not None
    rc0, _, _, _ = _render(inp, W, H, mode)  # the SH coefficients change nothing
    assert torch.equal(rc, rc0)
