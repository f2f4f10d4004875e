"""The entry points of csrc/image_terms.hip (d4gs_dilate_mask, d4gs_area_keep_*, d4gs_mse_*) are declared, bound and exported, and
validate their arguments on the host before any launch: fake addresses - nothing is dereferenced; no GPU needed."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_dilate_mask", "d4gs_area_keep_map_elems", "d4gs_area_keep_blocks", "d4gs_area_keep_fwd", "d4gs_area_keep_bwd",
       "d4gs_mse_blocks", "d4gs_mse_fwd", "d4gs_mse_bwd")
A = 0x10000  # a fake, 16-byte aligned device address

# the legal call of every entry point, and the name of each pointer argument by position (True: required)
#                       mask | B H W r | out out_complement stream
CALLS = {"d4gs_dilate_mask": ([A, 2, 41, 70, 4, A, A, None], {0: (b"mask", True), 5: (b"out", True), 6: (b"out_complement", False)}),
         #                pred mask target | target_reduced | B H W C factor | map partials out stream
         "d4gs_area_keep_fwd": ([A, A, A, 0, 2, 41, 70, 3, 4, A, A, A, None],
                                {0: (b"pred", True), 1: (b"mask", True), 2: (b"target", True), 9: (b"map", True), 10: (b"partials", True),
                                 11: (b"out", True)}),
         #                map v_loss | B H W C factor | v_pred stream
         "d4gs_area_keep_bwd": ([A, A, 2, 41, 70, 3, 4, A, None], {0: (b"map", True), 1: (b"v_loss", True), 7: (b"v_pred", True)}),
         #          a t | n | partials out stream
         "d4gs_mse_fwd": ([A, A, 5740, A, A, None], {0: (b"a", True), 1: (b"t", False), 3: (b"partials", True), 4: (b"out", True)}),
         #          a t v_loss | n | v_a stream
         "d4gs_mse_bwd": ([A, A, A, 5740, A, None], {0: (b"a", True), 1: (b"t", False), 2: (b"v_loss", True), 4: (b"v_a", True)})}
DOUBLES = {("d4gs_area_keep_fwd", 10), ("d4gs_mse_fwd", 3)}  # the 8-byte aligned arguments


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def put(fn, i, v):
    base = CALLS[fn][0]
    return base[:i] + [v] + base[i + 1:]


def bad(lib, fn, args, *words):
    assert getattr(lib, fn)(*args) == -1, (fn, args)  # D4GS_EINVAL
    err = lib.d4gs_last_error()
    assert fn.encode() in err and all(w in err for w in words), err


def test_new_symbols_are_declared_bound_and_exported_and_the_version_is_305(lib):
    from deblur4dgs_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    assert lib.d4gs_version() == 305 and "#define D4GS_VERSION 305" in header and L.VERSION == 305
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert hasattr(lib, name) and name in L.EXPORTS and f"{name}(" in header, name
        assert getattr(lib, name).argtypes is not None, name
        assert f" T {name}\n" in dyn, name
    assert L.EXPORTS[-len(NEW):] == NEW  # appended behind the metrics
    for q in (lib.d4gs_area_keep_map_elems, lib.d4gs_area_keep_blocks, lib.d4gs_mse_blocks):
        assert q.restype is C.c_int64


def test_null_and_misaligned_pointers_are_refused(lib):
    for fn, (_, ptrs) in CALLS.items():
        for i, (name, required) in ptrs.items():
            if required:
                bad(lib, fn, put(fn, i, None), name, b"NULL")
            for off in ((1, 4, 6) if (fn, i) in DOUBLES else (1, 2, 3)):
                bad(lib, fn, put(fn, i, A + off), name, b"misaligned")


def test_bad_sizes_are_refused(lib):
    for i, name in ((1, b"B="), (2, b"H="), (3, b"W=")):
        for v in (0, -1, -2 ** 31):
            bad(lib, "d4gs_dilate_mask", put("d4gs_dilate_mask", i, v), b"bad size", name + str(v).encode())
    for r in (-1, -2 ** 31):
        bad(lib, "d4gs_dilate_mask", put("d4gs_dilate_mask", 4, r), b"r=" + str(r).encode())
    for b_, h, w in ((65536, 16, 16), (1, 16 * 65535 + 1, 16), (1, 1, 2 ** 30 + 1)):
        bad(lib, "d4gs_dilate_mask", [A, b_, h, w, 4, A, A, None], b"overflows the grid", f"B={b_} H={h} W={w}".encode())
    for fn, first in (("d4gs_area_keep_fwd", 4), ("d4gs_area_keep_bwd", 2)):
        for k, name in enumerate((b"B=", b"H=", b"W=", b"C=")):
            for v in (0, -1, -2 ** 31):
                bad(lib, fn, put(fn, first + k, v), b"bad size", name + str(v).encode())
        for f in (0, -4, 3, 5, 6, 16):
            bad(lib, fn, put(fn, first + 4, f), b"factor=" + str(f).encode())
        base = CALLS[fn][0]
        for h, w, f in ((3, 70, 4), (41, 3, 4), (1, 1, 2), (7, 7, 8)):  # torch: an empty tensor and a NaN loss
            args = base[:first + 1] + [h, w, 3, f] + base[first + 5:]
            bad(lib, fn, args, b"below factor", f"H={h} W={w}".encode())
        for b_, h, w, c in ((1, 32769, 8, 1), (1, 8, 32769, 1), (2, 32768, 32768, 1), (1, 32768, 32768, 3)):
            args = base[:first] + [b_, h, w, c, 4] + base[first + 5:]
            bad(lib, fn, args, b"overflows the grid", f"B={b_} H={h} W={w} C={c}".encode())
    for fn, i in (("d4gs_mse_fwd", 2), ("d4gs_mse_bwd", 3)):
        for n in (0, -1, 2 ** 31, 2 ** 40):
            bad(lib, fn, put(fn, i, n), b"bad size", f"n={n}".encode())


def test_size_queries(lib):
    blocks, elems, mse = lib.d4gs_area_keep_blocks, lib.d4gs_area_keep_map_elems, lib.d4gs_mse_blocks
    assert elems(2, 41, 70, 3, 4) == 2 * 10 * 17 * 3 and blocks(2, 41, 70, 3, 4) == 4  # 1020 elements
    assert elems(1, 288, 512, 3, 4) == 72 * 128 * 3 and blocks(1, 288, 512, 3, 4) == 108
    assert elems(1, 4, 4, 1, 4) == 1 and blocks(1, 4, 4, 1, 4) == 1 and elems(1, 7, 7, 3, 4) == 3 and elems(2, 9, 11, 3, 2) == 2 * 4 * 5 * 3
    assert elems(1, 16, 16, 1, 1) == 256 and blocks(1, 16, 16, 1, 1) == 1 and blocks(1, 16, 16, 1, 8) == 1 and elems(1, 17, 16, 1, 1) == 272
    assert elems(1, 32768, 32768, 1, 8) == 4096 * 4096 and blocks(1, 32768, 32768, 1, 8) == 65536  # the last legal size
    for bad_ in ((0, 8, 8, 3, 4), (1, 0, 8, 3, 4), (1, 8, 0, 3, 4), (1, 8, 8, 0, 4), (-1, 8, 8, 3, 4), (1, 8, 8, 3, 0), (1, 8, 8, 3, 3),
                 (1, 8, 8, 3, 16), (1, 8, 8, 3, -4), (1, 3, 8, 3, 4), (1, 8, 3, 3, 4), (1, 32769, 8, 1, 4), (2, 32768, 32768, 1, 4),
                 (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 4)):
        assert elems(*bad_) == 0 and blocks(*bad_) == 0, bad_
    assert [mse(n) for n in (1, 255, 256, 257, 5740, 288 * 512, 4096 * 256, 4096 * 256 + 1, 2 ** 31 - 1)] == [1, 1, 1, 2, 23, 576, 4096, 4096, 4096]
    assert [mse(n) for n in (0, -1, 2 ** 31, 2 ** 62)] == [0, 0, 0, 0]


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from deblur4dgs_amd import losses as Lo

    p, t, m = torch.rand(1, 8, 12, 3), torch.rand(1, 8, 12, 3), torch.ones(1, 8, 12)
    with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback, as the other losses
        Lo.dilate_mask(m)
    with pytest.raises(RuntimeError, match="ROCm"):
        Lo.sharp_keep_loss(p, t, m)
    with pytest.raises(RuntimeError, match="ROCm"):
        Lo.coverage_loss(m)
    for k in (8, 0, 2):
        with pytest.raises(ValueError, match="kernel_size"):
            Lo.dilate_mask(m, kernel_size=k)
    with pytest.raises(ValueError, match="factor"):
        Lo.sharp_keep_loss(p, t, m, factor=3)
    with pytest.raises(ValueError, match="below factor"):
        Lo.sharp_keep_loss(p[:, :3], t[:, :3], m[:, :3])
    with pytest.raises(ValueError, match="masks"):
        Lo.sharp_keep_loss(p, t, m[:, :, :11])
    with pytest.raises(ValueError, match="target"):
        Lo.sharp_keep_loss(p, t[:, :4], m)
    with pytest.raises(ValueError, match="target"):
        Lo.coverage_loss(m, torch.ones(1, 8, 11))
