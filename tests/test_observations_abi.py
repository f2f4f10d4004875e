"""The entry points of csrc/observations.hip (d4gs_masked_median_ws_bytes, d4gs_masked_median_blur, d4gs_lift_tracks, d4gs_bkgd_points)
are declared, bound and exported in a block of their own, and validate their arguments on the host before any launch: fake addresses
- nothing is dereferenced; no GPU needed."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_masked_median_ws_bytes", "d4gs_masked_median_blur", "d4gs_lift_tracks", "d4gs_bkgd_points")
A = 0x10000  # a fake, 16-byte aligned device address
B = 0x20000  # another one (out must not be image)

# the legal call of every entry point, and each pointer argument by position: (name, required, alignment)
#                                  image mask blend | n_img H W k per_image | out workspace stream
CALLS = {"d4gs_masked_median_blur": ([A, A, A, 3, 40, 50, 11, 0, B, A, None],
                                     {0: (b"image", True, 4), 1: (b"mask", True, 4), 2: (b"blend", False, 4), 8: (b"out", True, 4),
                                      9: (b"workspace", True, 16)}),
         #                   tracks depths masks img inv_Ks c2ws | N T H W query | xyz vis invis conf in_mask colors count hist stream
         "d4gs_lift_tracks": ([A, A, A, A, A, A, 1000, 6, 24, 32, 2, A, A, A, A, A, A, A, A, None],
                              {0: (b"tracks_2d", True, 4), 1: (b"depths", True, 4), 2: (b"masks", True, 4), 3: (b"query_img", True, 4),
                               4: (b"inv_Ks", True, 4), 5: (b"c2ws", True, 4), 11: (b"xyz", True, 4), 12: (b"visibles", True, 1),
                               13: (b"invisibles", True, 1), 14: (b"confidences", True, 4), 15: (b"in_mask", True, 1),
                               16: (b"colors", True, 4), 17: (b"visible_count", True, 4), 18: (b"hist", True, 4)}),
         #                   depths masks valid inv_Ks c2ws | T H W | points normals keep index counts stream
         "d4gs_bkgd_points": ([A, A, A, A, A, 3, 24, 32, A, A, A, A, A, None],
                              {0: (b"depths", True, 4), 1: (b"masks", True, 4), 2: (b"valid_masks", True, 4), 3: (b"inv_Ks", True, 4),
                               4: (b"c2ws", True, 4), 8: (b"points", True, 4), 9: (b"normals", True, 4), 10: (b"keep", True, 1),
                               11: (b"index", False, 4), 12: (b"counts", False, 4)})}


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


def test_the_block_is_declared_bound_and_exported_in_a_table_of_its_own(lib):
    from deblur4dgs_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    assert lib.d4gs_version() == 305 and "#define D4GS_VERSION 305" in header and L.VERSION == 305
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert tuple(L.DATA_PROTOTYPES) == NEW  # in the header's order
    assert not set(NEW) & (set(L.EXPORTS) | set(L.INIT_PROTOTYPES) | set(L.EVAL_PROTOTYPES))  # disjoint from the other three tables
    assert header.count("D4GS_DATA_API") >= len(NEW) + 1 and header.index("#define D4GS_DATA_API") > header.index("#define D4GS_EVAL_API")
    for name in NEW:
        assert hasattr(lib, name) and f"{name}(" in header, name
        assert getattr(lib, name).argtypes == L.DATA_PROTOTYPES[name][1] and getattr(lib, name).restype is L.DATA_PROTOTYPES[name][0], name
        assert f" T {name}\n" in dyn, name
    assert lib.d4gs_masked_median_ws_bytes.restype is C.c_int64
    # every pointer of the block is a device pointer: no [host] mark
    assert all(t is C.c_void_p or not hasattr(t, "contents") for _, a in L.DATA_PROTOTYPES.values() for t in a)


def test_the_data_block_is_parsed_as_strictly_as_the_rest():
    from deblur4dgs_amd import _lib as L

    text = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    init, ev, data = {}, {}, {}
    _, _, prototypes = L.parse(text, init, eval=ev, data=data)
    assert tuple(data) == NEW and len(prototypes) == len(L.EXPORTS) and tuple(init) == tuple(L.INIT_PROTOTYPES) and tuple(ev) == tuple(L.EVAL_PROTOTYPES)
    L.parse(text)  # the keyword is optional
    old = "D4GS_DATA_API int64_t d4gs_masked_median_ws_bytes(int64_t n_img, int64_t H, int64_t W);"
    for new, word in ((old.replace("int64_t H", "long H"), "long H"), (old[:-1], "D4GS_DATA_API prototypes"),
                      (old.replace("int64_t d4gs", "unsigned d4gs"), "d4gs_masked_median_ws_bytes")):
        assert text.count(old) == 1
        with pytest.raises(ValueError) as e:
            L.parse(text.replace(old, new))
        assert word in str(e.value), str(e.value)


def test_null_and_misaligned_pointers_are_refused(lib):
    for fn, (_, ptrs) in CALLS.items():
        for i, (name, required, align) in ptrs.items():
            if required:
                bad(lib, fn, put(fn, i, None), name, b"NULL")
            for off in {1: (), 4: (1, 2, 3), 16: (1, 4, 8)}[align]:
                bad(lib, fn, put(fn, i, A + off), name, b"misaligned")


def test_bad_sizes_and_kernel_sizes_are_refused(lib):
    fn = "d4gs_masked_median_blur"
    for i, name in ((3, b"n_img="), (4, b"H="), (5, b"W=")):
        for v in (0, -1, -2 ** 31):
            bad(lib, fn, put(fn, i, v), b"bad size", name + str(v).encode())
    for k in (1, 2, 4, 10, 12, 16, 17, 0, -3, 2 ** 31 - 1):  # even, below 3, above 15
        bad(lib, fn, put(fn, 6, k), f"kernel_size={k}".encode())
    bad(lib, fn, [A, A, A, 2 ** 11, 2 ** 10, 2 ** 10, 11, 0, B, A, None], b"overflows", b"n_img=2048 H=1024 W=1024")
    bad(lib, fn, put(fn, 8, A), b"out aliases image")
    fn = "d4gs_lift_tracks"
    for i, name in ((6, b"N="), (7, b"T="), (8, b"H="), (9, b"W=")):
        for v in (0, -1, -2 ** 31):
            bad(lib, fn, put(fn, i, v), b"bad size", name + str(v).encode())
    for q in (-1, 6, 2 ** 31 - 1):
        bad(lib, fn, put(fn, 10, q), f"query={q}".encode())
    bad(lib, fn, put(fn, 6, 2 ** 27), b"overflows", b"N=134217728 T=6")          # N T 4
    bad(lib, fn, put(fn, 8, 2 ** 24), b"overflows", b"H=16777216 W=32")          # T H W
    bad(lib, fn, [A, A, A, A, A, A, 10, 1, 2 ** 15, 2 ** 15, 0] + [A] * 8 + [None], b"overflows", b"H=32768 W=32768")  # H W 3
    fn = "d4gs_bkgd_points"
    for i, name in ((5, b"T="), (6, b"H="), (7, b"W=")):
        for v in (0, -1, -2 ** 31):
            bad(lib, fn, put(fn, i, v), b"bad size", name + str(v).encode())
    bad(lib, fn, put(fn, 5, 2 ** 20), b"overflows", b"T=1048576 H=24 W=32")  # T H W 3
    bad(lib, fn, put(fn, 11, None), b"index and counts come together")
    bad(lib, fn, put(fn, 12, None), b"index and counts come together")


def test_the_workspace_query_at_its_edges(lib):
    ws = lib.d4gs_masked_median_ws_bytes

    def expect(n, H, W):  # parities, chunk table, tile min / max, lo / hi: each rounded up to 16 bytes
        up = lambda b: (b + 15) // 16 * 16
        tiles, chunks = -(-H // 16) * -(-W // 16), -(-H * W // 1024)
        return up(n * H * W) + up(n * chunks) + up(n * tiles * 8) + up(n * 8)

    for n, H, W in ((1, 1, 1), (1, 16, 16), (1, 17, 33), (3, 40, 50), (24, 288, 512), (24, 480, 854), (1, 32, 32), (1, 32, 33)):
        assert ws(n, H, W) == expect(n, H, W) > 0 and ws(n, H, W) % 16 == 0, (n, H, W)
    assert ws(1, 2 ** 15, 2 ** 16 - 1) == expect(1, 2 ** 15, 2 ** 16 - 1)  # just below 2^31 pixels
    assert ws(1, 1, 2 ** 31 - 1) == expect(1, 1, 2 ** 31 - 1) and ws(2 ** 31 - 1, 1, 1) == expect(2 ** 31 - 1, 1, 1)  # the limit itself
    for n, H, W in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1, 2 ** 16, 2 ** 15), (2, 2 ** 15, 2 ** 15), (2 ** 40, 1, 1)):
        assert ws(n, H, W) == 0, (n, H, W)


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from deblur4dgs_amd import observations as O

    T, H, W, N = 2, 8, 9, 5
    d, m, img = torch.rand(T, H, W), torch.ones(T, H, W), torch.rand(T, H, W, 3)
    Ks, w2cs, tr = torch.eye(3).repeat(T, 1, 1), torch.eye(4).repeat(T, 1, 1), torch.rand(N, T, 4)
    for call in (lambda: O.masked_median_blur(d[None], m[None]), lambda: O.filter_depths(d, m, m),
                 lambda: O.parse_tapir_track_info(tr[..., 2], tr[..., 3]), lambda: O.lift_tracks(0, img[0], tr, d, m, Ks, w2cs),
                 lambda: O.tracks_3d_for_query_frame(0, img[0], tr, d, m, Ks, w2cs), lambda: O.tracks_3d([tr], [0], img, d, m, Ks, w2cs),
                 lambda: O.bkgd_points_dense(d, m, m, Ks, w2cs), lambda: O.bkgd_points(img, d, m, m, Ks, w2cs, 10)):
        with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback
            call()
    assert O.visible_count_threshold([0, 0, 0], 2) == 0 and O.visible_count_threshold([3, 0, 0, 5], 100) == 0.0
    assert O.visible_count_threshold([0, 0, 1, 0, 9], 100) == pytest.approx(3.8)  # 0.1 * 9 = 0.9 of the way from 2 to 4
