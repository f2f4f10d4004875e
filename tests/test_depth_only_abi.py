"""CPU: the C ABI of the depth-only render modes (D4gsDims.D == 0 with a depth mode: gsplat's render_mode "D" / "ED") - sizes and
the host-side argument checks, which all return before any HIP call (fake device addresses are never dereferenced) - and the seam's
render_mode validation."""
import ctypes as C

import pytest
import torch

from tests.test_absgrad_abi import FAKE, _frame_args, _raster_bwd_args


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def _dims(depth_mode, flags=0, **kw):
    from deblur4dgs_amd import _lib as L

    base = dict(N=1000, S=2, D=0, width=64, height=48, depth_mode=depth_mode, flags=flags)
    base.update(kw)
    return L.Dims(**base)


@pytest.mark.parametrize("mode", ["ED", "D"])
def test_query_sizes_of_a_depth_only_render(lib, mode):
    from deblur4dgs_amd import _lib as L

    depth = L.DEPTH_ED if mode == "ED" else L.DEPTH_D
    z = L.Sizes()
    assert lib.d4gs_query_sizes(C.byref(_dims(depth)), C.byref(z)) == 0, lib.d4gs_last_error()
    assert z.isect_grad_row == 7 and z.ctab == 0 and z.channels == 1
    assert z.render_colors == 2 * 48 * 64 and z.render_alphas == 2 * 48 * 64
    ref = L.Sizes()  # everything but the colour table and the channels is that of a one-colour render
    assert lib.d4gs_query_sizes(C.byref(_dims(depth, D=1)), C.byref(ref)) == 0
    for name, _ in L.Sizes._fields_:
        if name not in ("ctab", "isect_grad_row", "channels", "render_colors", "seg_state"):
            assert getattr(z, name) == getattr(ref, name), name
    assert lib.d4gs_query_sizes(C.byref(_dims(depth, L.ABSGRAD)), C.byref(z)) == 0 and z.isect_grad_row == 9


def test_zero_channels_without_a_depth_mode_are_refused(lib):
    from deblur4dgs_amd import _lib as L

    d = _dims(L.DEPTH_NONE)
    assert lib.d4gs_query_sizes(C.byref(d), C.byref(L.Sizes())) == -1
    assert b"D == 0 needs depth_mode" in lib.d4gs_last_error(), lib.d4gs_last_error()
    pout, isect, ras, ok = _raster_bwd_args()
    pin = L.ProjIn(**{n: FAKE for n, _ in L.ProjIn._fields_})
    calls = (lambda: lib.d4gs_project_fwd(C.byref(d), C.byref(pin), C.byref(pout), None),
             lambda: lib.d4gs_bin_sort(C.byref(d), C.byref(pout), C.byref(isect), None),
             lambda: lib.d4gs_raster_fwd(C.byref(d), C.byref(pout), C.byref(isect), C.byref(ras), None),
             lambda: lib.d4gs_raster_bwd(C.byref(d), C.byref(pout), C.byref(isect), C.byref(ras), C.byref(L.RasterGrads(**ok)), None))
    for call in calls:
        assert call() == -1
        assert b"D == 0 needs depth_mode" in lib.d4gs_last_error(), lib.d4gs_last_error()
    d.D = -1
    assert lib.d4gs_query_sizes(C.byref(d), C.byref(L.Sizes())) == -1


def test_staged_entry_points_take_null_colour_buffers_with_zero_channels(lib):
    """Every call below fails on purpose at a check BEHIND the NULL-buffer check (so nothing is launched); with D > 0 the same
    NULL buffers are refused there."""
    from deblur4dgs_amd import _lib as L

    pout, isect, ras, ok = _raster_bwd_args()
    pout.ctab = None
    pin = L.ProjIn(**{n: FAKE for n, _ in L.ProjIn._fields_})
    pin.colors = None
    for D, null_word in ((0, None), (3, b"NULL")):
        d = _dims(L.DEPTH_ED, D=D, N=0)  # d4gs_project_fwd: "N == 0" comes after the NULL check
        assert lib.d4gs_project_fwd(C.byref(d), C.byref(pin), C.byref(pout), None) == -1
        assert (null_word or b"N == 0") in lib.d4gs_last_error(), lib.d4gs_last_error()
        d = _dims(L.DEPTH_ED, L.EXACT_TILES, D=D)  # check_binned: the exact-tiles masks come after the NULL check
        pout.tile_masks = None
        assert lib.d4gs_bin_sort(C.byref(d), C.byref(pout), C.byref(isect), None) == -1
        assert (null_word or b"tile_masks") in lib.d4gs_last_error(), lib.d4gs_last_error()
        pout.tile_masks = FAKE
        d = _dims(L.DEPTH_D, L.ABSGRAD, D=D)  # d4gs_raster_bwd: the absgrad buffers come after the NULL check
        rg = L.RasterGrads(**{**ok, "v_ctab": None})
        assert lib.d4gs_raster_bwd(C.byref(d), C.byref(pout), C.byref(isect), C.byref(ras), C.byref(rg), None) == -1
        assert (null_word or b"needs v_means2d_abs") in lib.d4gs_last_error(), lib.d4gs_last_error()
        d = _dims(L.DEPTH_D, D=D, G=1, K=1, T=1)  # d4gs_project_bwd: the motion inputs come after the NULL check
        leaf = L.LeafGrads(**{n: FAKE for n in ("v_means", "v_quats", "v_scales", "v_opacities", "partials")})
        pin_m = L.ProjIn(**{n: FAKE for n, _ in L.ProjIn._fields_})
        pin_m.colors, pin_m.motion_coefs = None, None
        v = C.c_void_p(FAKE)
        assert lib.d4gs_project_bwd(C.byref(d), C.byref(pin_m), C.byref(pout), v, v, v, v, None, C.byref(leaf), None) == -1
        assert (null_word or b"G>0 needs") in lib.d4gs_last_error(), lib.d4gs_last_error()


def test_one_call_frame_refuses_zero_channels(lib):
    from deblur4dgs_amd import _lib as L

    d, pin, io, leaf = _frame_args(0)
    d.D = 0
    for fn in (lib.d4gs_frame_workspace_bytes, lib.d4gs_frame_workspace_bytes_fwd):
        assert fn(C.byref(d), 1000) == 0
        assert b"one-call frame" in lib.d4gs_last_error(), lib.d4gs_last_error()
    assert lib.d4gs_forward(C.byref(d), C.byref(pin), C.byref(io), C.c_void_p(FAKE), 1 << 40, 1000, 0, None) == -1
    assert b"one-call frame" in lib.d4gs_last_error(), lib.d4gs_last_error()
    fg = L.FrameGrads(v_renders=FAKE, v_means2d=FAKE)
    assert lib.d4gs_backward(C.byref(d), C.byref(pin), C.byref(io), C.byref(fg), C.byref(leaf), C.c_void_p(FAKE), 1 << 40, 1000, 0,
                             None) == -1
    assert b"one-call frame" in lib.d4gs_last_error(), lib.d4gs_last_error()


def test_cpu_twin_keeps_its_zero_channel_render():
    """The CPU twins took D == 0 with a depth mode before the depth-only kernels existed (their own loops, not the device kernels'
    instantiations); that stays as it was: the expected depth against the fp64 oracle's "ED" render."""
    import oracle.raster
    from deblur4dgs_amd.cpu_twin import render_exposure_cpu
    from tests.util import static_inputs

    N, W, H = 200, 32, 32
    inp = static_inputs(N, W, H, seed=1, dtype=torch.float32, D=3)
    out = render_exposure_cpu(inp["means"], inp["quats"], inp["scales"], inp["opac"], torch.zeros(N, 0), 0, None, None, None, None,
                              None, inp["V"], inp["K"], W, H, return_depth=True, blend=False, raw_params=False)
    ref, _, _ = oracle.raster.rasterization(*(inp[k].double() for k in ("means", "quats", "scales", "opac", "colors", "V", "K")),
                                            W, H, render_mode="ED")
    assert out["renders"].shape == (1, H, W, 1)
    assert float((out["renders"][0].double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


def test_render_cfg_of_a_depth_only_render():
    from deblur4dgs_amd import _lib as L
    from deblur4dgs_amd.engine import RenderCfg

    cfg = RenderCfg(N=10, G=0, K=0, T=0, S=1, D=0, width=16, height=16, depth_mode=L.DEPTH_ED, depth_only=True)
    assert cfg.NCH == 1 and cfg.DP == 0 and cfg.dims().D == 0 and cfg.dims().depth_mode == L.DEPTH_ED
    assert not RenderCfg(N=10, G=0, K=0, T=0, S=1, D=0, width=16, height=16).depth_only  # the older D == 0 route stays the default


@pytest.mark.parametrize("mode", ["D", "ED"])
def test_depth_only_modes_pass_validation_and_need_a_device(mode):
    from deblur4dgs_amd.rasterization import rasterization

    z = torch.zeros
    args = (z(2, 3), z(2, 4), z(2, 3), z(2), z(2, 3), torch.eye(4)[None], torch.eye(3)[None], 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rasterization(*args, render_mode=mode)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rasterization(*args, render_mode=mode, backgrounds=z(1, 3), absgrad=True, rasterize_mode="antialiased")
    # colors are validated exactly as in the other modes
    with pytest.raises(ValueError, match="sh_degree"):
        rasterization(*args[:4], z(2, 3, 3), *args[5:], render_mode=mode, sh_degree=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rasterization(*args[:4], z(2, 16, 3), *args[5:], render_mode=mode, sh_degree=3)


def test_other_render_modes_are_still_refused():
    from deblur4dgs_amd.rasterization import rasterization

    z = torch.zeros
    args = (z(2, 3), z(2, 4), z(2, 3), z(2), z(2, 3), torch.eye(4)[None], torch.eye(3)[None], 16, 16)
    for mode in ("bogus", "d", "RGB+ED+D", "DE", ""):
        with pytest.raises(ValueError, match="render_mode"):
            rasterization(*args, render_mode=mode)
