"""CPU: the C ABI of absgrad (D4GS_ABSGRAD, D4gsRasterGrads / D4gsFrameGrads.v_means2d_abs and .stats_absgrad) - sizes and the
host-side argument checks, which all return before any HIP call (fake device addresses are never dereferenced)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def test_flag_value_and_ctypes_mirror():
    from deblur4dgs_amd import _lib as L

    src = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    assert re.search(r"\bD4GS_ABSGRAD\s*=\s*32\b", src)
    assert L.ABSGRAD == 32


def _fields(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4gs.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            decl = re.sub(r"^(const\s+)?(float|int32_t|int64_t|uint64_t|uint8_t|void)\s*", "", decl)
            out += [x.strip().lstrip("*").strip() for x in decl.split(",")]
    return out


def test_grads_structs_match_the_header_with_the_appended_fields():
    from deblur4dgs_amd import _lib as L

    for cname, cls in (("D4gsFrameGrads", L.FrameGrads), ("D4gsRasterGrads", L.RasterGrads)):
        names = _fields(cname)
        assert names == [f[0] for f in cls._fields_], cname
        assert names[-2:] == ["v_means2d_abs", "stats_absgrad"], cname
    assert dict(L.FrameGrads._fields_)["stats_absgrad"] is C.c_int32


def test_query_sizes_row_width(lib):
    from deblur4dgs_amd import _lib as L

    for D, depth in ((3, L.DEPTH_ED), (16, L.DEPTH_D), (5, L.DEPTH_NONE), (1, L.DEPTH_NONE)):
        nch = D + (depth != L.DEPTH_NONE)
        z = L.Sizes()
        d = L.Dims(N=100, S=2, D=D, width=64, height=32, depth_mode=depth)
        assert lib.d4gs_query_sizes(C.byref(d), C.byref(z)) == 0 and z.isect_grad_row == 6 + nch
        d.flags = L.ABSGRAD
        assert lib.d4gs_query_sizes(C.byref(d), C.byref(z)) == 0 and z.isect_grad_row == 8 + nch
    d0 = L.Dims(N=1000, S=2, D=3, width=64, height=48, depth_mode=1)
    d1 = L.Dims(N=1000, S=2, D=3, width=64, height=48, depth_mode=1, flags=L.ABSGRAD)
    cap = 100000
    assert lib.d4gs_frame_workspace_bytes(C.byref(d1), cap) - lib.d4gs_frame_workspace_bytes(C.byref(d0), cap) >= 8 * cap


def _raster_bwd_args():
    from deblur4dgs_amd import _lib as L

    pout = L.ProjOut(**{n: FAKE for n, _ in L.ProjOut._fields_})
    isect = L.Isect(n_isect=4, max_tile_count=0, keys=FAKE, gid_of_emit=FAKE, sorted_gid=FAKE, sorted_emit=FAKE)
    ras = L.Raster(**{n: FAKE for n, _ in L.Raster._fields_})
    ok = dict(v_render_colors=FAKE, isect_grad=FAKE, isect_live=FAKE, v_means2d=FAKE, v_conics=FAKE, v_depths=FAKE, v_opac_act=FAKE,
              v_ctab=FAKE)
    return pout, isect, ras, ok


@pytest.mark.parametrize("flag,extra,word", [(True, {}, b"needs v_means2d_abs"),
                                             (False, dict(v_means2d_abs=FAKE), b"without D4GS_ABSGRAD"),
                                             (False, dict(stats_absgrad=1), b"without D4GS_ABSGRAD")])
def test_raster_bwd_rejects_inconsistent_absgrad_arguments(lib, flag, extra, word):
    from deblur4dgs_amd import _lib as L

    pout, isect, ras, ok = _raster_bwd_args()
    d = L.Dims(N=10, S=1, D=3, width=16, height=16, flags=L.ABSGRAD if flag else 0)
    rg = L.RasterGrads(**ok, **extra)
    assert lib.d4gs_raster_bwd(C.byref(d), C.byref(pout), C.byref(isect), C.byref(ras), C.byref(rg), None) == -1
    assert word in lib.d4gs_last_error(), lib.d4gs_last_error()


def _frame_args(flags):
    from deblur4dgs_amd import _lib as L

    d = L.Dims(N=1000, S=2, D=3, width=64, height=48, depth_mode=1, flags=flags)
    pin = L.ProjIn(**{n: FAKE for n, _ in L.ProjIn._fields_})
    io = L.FrameIO(**{n: FAKE for n in ("renders", "alphas", "means2d", "radii", "n_isect")})
    leaf = L.LeafGrads(**{n: FAKE for n in ("v_means", "v_quats", "v_scales", "v_opacities", "v_colors")})
    return d, pin, io, leaf


@pytest.mark.parametrize("flag,extra,word", [(True, {}, b"needs v_means2d_abs"),
                                             (False, dict(v_means2d_abs=FAKE), b"without D4GS_ABSGRAD"),
                                             (False, dict(stats_absgrad=1), b"without D4GS_ABSGRAD")])
def test_one_call_backward_rejects_inconsistent_absgrad_arguments(lib, flag, extra, word):
    from deblur4dgs_amd import _lib as L

    d, pin, io, leaf = _frame_args(L.ABSGRAD if flag else 0)
    ws = lib.d4gs_frame_workspace_bytes(C.byref(d), 1000)
    fg = L.FrameGrads(v_renders=FAKE, v_means2d=FAKE, **extra)
    assert lib.d4gs_backward(C.byref(d), C.byref(pin), C.byref(io), C.byref(fg), C.byref(leaf), C.c_void_p(FAKE), ws, 1000, 0,
                             None) == -1
    assert word in lib.d4gs_last_error(), lib.d4gs_last_error()


def test_cpu_twins_refuse_the_flag(lib):
    from deblur4dgs_amd import _lib as L

    d, pin, io, leaf = _frame_args(L.ABSGRAD)
    fg = L.FrameGrads(v_renders=FAKE, v_means2d=FAKE, v_means2d_abs=FAKE)
    assert lib.d4gs_forward_cpu(C.byref(d), C.byref(pin), C.byref(io)) == -1
    assert b"CPU twins" in lib.d4gs_last_error()
    assert lib.d4gs_backward_cpu(C.byref(d), C.byref(pin), C.byref(io), C.byref(fg), C.byref(leaf)) == -1
    assert b"CPU twins" in lib.d4gs_last_error()
