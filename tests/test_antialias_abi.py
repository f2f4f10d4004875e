"""CPU: the C ABI of the antialiased mode (D4GS_ANTIALIASED, D4gsProjOut.compensations, D4gsSizes.compensations) - sizes and the
host-side argument checks, which all return before any HIP call (fake device addresses are never dereferenced) - and the seam's
rasterize_mode validation."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_absgrad_abi import FAKE, ROOT, _fields, _frame_args, _raster_bwd_args


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def test_flag_value_and_appended_fields():
    from deblur4dgs_amd import _lib as L

    src = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    assert re.search(r"\bD4GS_ANTIALIASED\s*=\s*64\b", src)
    assert re.search(r"#define D4GS_VERSION 305\b", src)
    assert L.ANTIALIASED == 64
    names = _fields("D4gsProjOut")
    assert names == [f[0] for f in L.ProjOut._fields_] and names[-2:] == ["tile_masks", "compensations"]
    sizes = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*?)\} D4gsSizes;", sizes, re.S).group(1)
    hdr = [x.strip() for decl in body.split(";") if decl.strip()
           for x in re.sub(r"^(int32_t|int64_t)\s*", "", decl.strip()).split(",")]
    assert hdr == [f[0] for f in L.Sizes._fields_] and hdr[-2:] == ["tile_masks", "compensations"]
    assert dict(L.Sizes._fields_)["compensations"] is C.c_int64


def test_query_sizes_and_workspace_grow_by_one_float_per_instance(lib):
    from deblur4dgs_amd import _lib as L

    for N, S, flags in ((1000, 2, 0), (4097, 8, L.EXACT_CULL | L.LAZY_SORT), (77, 1, L.EXACT_CULL | L.EXACT_TILES | L.ABSGRAD)):
        z0, z1 = L.Sizes(), L.Sizes()
        d0 = L.Dims(N=N, S=S, D=3, width=64, height=48, depth_mode=1, flags=flags)
        d1 = L.Dims(N=N, S=S, D=3, width=64, height=48, depth_mode=1, flags=flags | L.ANTIALIASED)
        assert lib.d4gs_query_sizes(C.byref(d0), C.byref(z0)) == 0 and lib.d4gs_query_sizes(C.byref(d1), C.byref(z1)) == 0
        assert z0.compensations == 0 and z1.compensations == S * N
        for name, _ in L.Sizes._fields_:  # nothing else moves
            if name != "compensations":
                assert getattr(z0, name) == getattr(z1, name), name
        for fn in (lib.d4gs_frame_workspace_bytes, lib.d4gs_frame_workspace_bytes_fwd):
            for cap in (1, 100000):
                grow = fn(C.byref(d1), cap) - fn(C.byref(d0), cap)
                assert 4 * S * N <= grow <= 4 * S * N + 256, (N, S, cap, grow)  # the buffer plus the carve's 256-byte alignment


def _proj_fwd_args(comp):
    from deblur4dgs_amd import _lib as L

    pin = L.ProjIn(**{n: FAKE for n in ("means", "quats", "scales", "opacities", "colors", "viewmat", "Kmat")})
    pout = L.ProjOut(**{**{n: FAKE for n, _ in L.ProjOut._fields_}, "compensations": comp})
    return pin, pout


@pytest.mark.parametrize("flag,comp,word", [(True, 0, b"needs D4gsProjOut.compensations"),
                                            (False, FAKE, b"without D4GS_ANTIALIASED")])
def test_project_fwd_and_raster_bwd_reject_inconsistent_compensations(lib, flag, comp, word):
    from deblur4dgs_amd import _lib as L

    d = L.Dims(N=10, S=1, D=3, width=16, height=16, flags=L.ANTIALIASED if flag else 0)
    pin, pout = _proj_fwd_args(comp)
    assert lib.d4gs_project_fwd(C.byref(d), C.byref(pin), C.byref(pout), None) == -1
    assert word in lib.d4gs_last_error(), lib.d4gs_last_error()
    _, isect, ras, ok = _raster_bwd_args()
    rg = L.RasterGrads(**ok)
    assert lib.d4gs_raster_bwd(C.byref(d), C.byref(pout), C.byref(isect), C.byref(ras), C.byref(rg), None) == -1
    assert word in lib.d4gs_last_error(), lib.d4gs_last_error()


def test_raster_bwd_needs_the_activated_opacity_with_the_flag(lib):
    from deblur4dgs_amd import _lib as L

    d = L.Dims(N=10, S=1, D=3, width=16, height=16, flags=L.ANTIALIASED)
    _, pout = _proj_fwd_args(FAKE)
    pout.opac_act = 0
    _, isect, ras, ok = _raster_bwd_args()
    rg = L.RasterGrads(**ok)
    assert lib.d4gs_raster_bwd(C.byref(d), C.byref(pout), C.byref(isect), C.byref(ras), C.byref(rg), None) == -1
    assert b"opac_act" in lib.d4gs_last_error(), lib.d4gs_last_error()


def test_cpu_twins_refuse_the_flag(lib):
    from deblur4dgs_amd import _lib as L

    d, pin, io, leaf = _frame_args(L.ANTIALIASED)
    fg = L.FrameGrads(v_renders=FAKE, v_means2d=FAKE)
    assert lib.d4gs_forward_cpu(C.byref(d), C.byref(pin), C.byref(io)) == -1
    assert b"D4GS_ANTIALIASED" in lib.d4gs_last_error()
    assert lib.d4gs_backward_cpu(C.byref(d), C.byref(pin), C.byref(io), C.byref(fg), C.byref(leaf)) == -1
    assert b"D4GS_ANTIALIASED" in lib.d4gs_last_error()


def test_render_cfg_sets_the_flag():
    from deblur4dgs_amd import _lib as L
    from deblur4dgs_amd.engine import RenderCfg

    base = dict(N=10, G=0, K=0, T=0, S=1, D=3, width=16, height=16)
    assert not RenderCfg(**base).dims().flags & L.ANTIALIASED
    assert RenderCfg(**base, antialiased=True).dims().flags & L.ANTIALIASED
    assert RenderCfg(**base, antialiased=True, absgrad=True).dims().flags & (L.ANTIALIASED | L.ABSGRAD) == L.ANTIALIASED | L.ABSGRAD


def test_rasterize_mode_is_validated_before_any_work():
    from deblur4dgs_amd.rasterization import rasterization

    z = torch.zeros
    args = (z(2, 3), z(2, 4), z(2, 3), z(2), z(2, 3), torch.eye(4)[None], torch.eye(3)[None], 16, 16)
    with pytest.raises(ValueError, match="rasterize_mode"):
        rasterization(*args, rasterize_mode="bogus")
    with pytest.raises(NotImplementedError):
        rasterization(*args, rasterize_mode="antialiased", packed=True)
    with pytest.raises(NotImplementedError):
        rasterization(*args, tile_size=8)
