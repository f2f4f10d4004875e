"""The entry points of csrc/scene_init.hip (d4gs_track_features, d4gs_knn*, d4gs_kmeans_*, d4gs_procrustes_moments) are declared, bound
and exported, and validate their arguments on the host before any launch: fake addresses - nothing is dereferenced; no GPU needed."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_track_features", "d4gs_knn_splits", "d4gs_knn_workspace_bytes", "d4gs_knn", "d4gs_kmeans_blocks", "d4gs_kmeans_scratch_bytes",
       "d4gs_kmeans_step", "d4gs_procrustes_moments")
A = 0x10000  # a fake, 16-byte aligned device address

# the legal call of every entry point, and each pointer argument by position: (name, required, alignment)
#                          xyz visible | G T | xyz_interp vel_dirs stream
CALLS = {"d4gs_track_features": ([A, A, 333, 12, A, A, None],
                                 {0: (b"xyz", True, 4), 1: (b"visible", True, 1), 4: (b"xyz_interp", False, 4), 5: (b"vel_dirs", False, 4)}),
         #           points | N k | dists idx workspace stream
         "d4gs_knn": ([A, 3000, 3, A, A, A, None], {0: (b"points", True, 4), 3: (b"dists", True, 4), 4: (b"idx", False, 4),
                                                    5: (b"workspace", True, 16)}),
         #                   x | G D K iters | centres labels changed scratch stream
         "d4gs_kmeans_step": ([A, 4097, 69, 20, 1, A, A, A, A, None],
                              {0: (b"x", True, 4), 5: (b"centres", True, 4), 6: (b"labels", True, 4), 7: (b"changed", True, 4),
                               8: (b"scratch", True, 8)}),
         #                          xyz weights conf order seg | G T K cano_t | out stream
         "d4gs_procrustes_moments": ([A, A, A, A, A, 333, 12, 5, 5, A, None],
                                     {0: (b"xyz", True, 4), 1: (b"weights", True, 4), 2: (b"conf", True, 4), 3: (b"order", True, 4),
                                      4: (b"seg", True, 4), 9: (b"out", True, 8)})}


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
    assert tuple(L.INIT_PROTOTYPES) == NEW and not set(NEW) & set(L.EXPORTS)  # the block of its own, in the header's order
    for name in NEW:
        assert hasattr(lib, name) and f"D4GS_INIT_API" in header and f"{name}(" in header, name
        assert getattr(lib, name).argtypes == L.INIT_PROTOTYPES[name][1] and getattr(lib, name).restype is L.INIT_PROTOTYPES[name][0], name
        assert f" T {name}\n" in dyn, name
    assert lib.d4gs_knn_splits.restype is C.c_int32
    for q in (lib.d4gs_knn_workspace_bytes, lib.d4gs_kmeans_blocks, lib.d4gs_kmeans_scratch_bytes):
        assert q.restype is C.c_int64
    # every pointer of the block is a device pointer: no [host] mark
    assert all(t is C.c_void_p or not hasattr(t, "contents") for _, a in L.INIT_PROTOTYPES.values() for t in a)
    assert (L.KNN_MAX_K, L.KMEANS_MAX_K) == (8, 64) and L.KNN_TILE >= 64 and L.KNN_SPLIT_MIN >= L.KNN_TILE


def test_the_init_block_is_parsed_as_strictly_as_the_rest():
    from deblur4dgs_amd import _lib as L

    text = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    init = {}
    _, _, prototypes = L.parse(text, init)
    assert tuple(init) == NEW and len(prototypes) == len(L.EXPORTS)
    for old, new, word in (("D4GS_INIT_API int32_t d4gs_knn_splits(int64_t N);", "D4GS_INIT_API int32_t d4gs_knn_splits(long N);", "long N"),
                           ("D4GS_INIT_API int32_t d4gs_knn_splits(int64_t N);", "D4GS_INIT_API int32_t d4gs_knn_splits(int64_t N)",
                            "D4GS_INIT_API prototypes"),
                           ("D4GS_INIT_API int64_t d4gs_kmeans_blocks(int64_t G);", "D4GS_INIT_API unsigned d4gs_kmeans_blocks(int64_t G);",
                            "d4gs_kmeans_blocks")):
        assert text.count(old) == 1, old
        with pytest.raises(ValueError) as e:
            L.parse(text.replace(old, new))
        assert word in str(e.value), str(e.value)


def test_null_and_misaligned_pointers_are_refused(lib):
    for fn, (_, ptrs) in CALLS.items():
        for i, (name, required, align) in ptrs.items():
            if required:
                bad(lib, fn, put(fn, i, None), name, b"NULL")
            for off in {1: (), 4: (1, 2, 3), 8: (1, 4, 6), 16: (1, 4, 8)}[align]:
                bad(lib, fn, put(fn, i, A + off), name, b"misaligned")


def test_bad_sizes_are_refused(lib):
    for i, name in ((2, b"G="), (3, b"T=")):
        for v in (0, -1, -2 ** 31):
            bad(lib, "d4gs_track_features", put("d4gs_track_features", i, v), b"bad size", name + str(v).encode())
    bad(lib, "d4gs_track_features", put("d4gs_track_features", 3, 1), b"vel_dirs", b"T >= 2")
    assert lib.d4gs_track_features(A, A, 10, 1, None, None, None) == 0  # T = 1 without vel_dirs is legal (and nothing is launched)
    bad(lib, "d4gs_track_features", [A, A, 2 ** 27, 6, A, A, None], b"overflows", b"G=134217728 T=6")
    for n in (0, -1, -2 ** 31):
        bad(lib, "d4gs_knn", put("d4gs_knn", 1, n), b"bad size", f"N={n}".encode())
    for k in (0, -1, 9, 2 ** 31 - 1):
        bad(lib, "d4gs_knn", put("d4gs_knn", 2, k), f"k={k}".encode())
    for n, k in ((1, 1), (3, 3), (8, 8)):
        bad(lib, "d4gs_knn", [A, n, k, A, A, A, None], f"N={n}".encode(), b"N >= k + 1")
    bad(lib, "d4gs_knn", put("d4gs_knn", 1, 2 ** 24 + 1), b"overflows", b"2^24")
    for i, name in ((1, b"G="), (2, b"D="), (3, b"K="), (4, b"iters=")):
        for v in (0, -1, -2 ** 31):
            bad(lib, "d4gs_kmeans_step", put("d4gs_kmeans_step", i, v), b"bad size", name + str(v).encode())
    bad(lib, "d4gs_kmeans_step", put("d4gs_kmeans_step", 3, 65), b"K=65", b"K <= 64")
    bad(lib, "d4gs_kmeans_step", [A, 100, 193, 64, 1, A, A, A, A, None], b"overflows", b"K D <= 12288")  # 64 * 193 = 12352
    bad(lib, "d4gs_kmeans_step", [A, 2 ** 30, 3, 2, 1, A, A, A, A, None], b"overflows", b"G D <= 2^31 - 1")
    for i, name in ((5, b"G="), (6, b"T="), (7, b"K=")):
        for v in (0, -1, -2 ** 31):
            bad(lib, "d4gs_procrustes_moments", put("d4gs_procrustes_moments", i, v), b"bad size", name + str(v).encode())
    for cano in (-1, 12, 2 ** 31 - 1):
        bad(lib, "d4gs_procrustes_moments", put("d4gs_procrustes_moments", 8, cano), f"cano_t={cano}".encode())
    bad(lib, "d4gs_procrustes_moments", put("d4gs_procrustes_moments", 7, 65536), b"overflows the grid", b"K=65536")
    bad(lib, "d4gs_procrustes_moments", [A, A, A, A, A, 2 ** 27, 6, 5, 5, A, None], b"overflows the grid", b"G=134217728")


def test_size_queries(lib):
    from deblur4dgs_amd import _lib as L

    splits, ws, blocks, scratch = lib.d4gs_knn_splits, lib.d4gs_knn_workspace_bytes, lib.d4gs_kmeans_blocks, lib.d4gs_kmeans_scratch_bytes
    assert [splits(n) for n in (2, L.KNN_TILE, L.KNN_SPLIT_MIN)] == [1, 1, 1] and splits(L.KNN_SPLIT_MIN + 1) > 1
    for n in (L.KNN_SPLIT_MIN + 1, 40000, 100000, 300000):
        s = splits(n)
        tiles = -(-n // L.KNN_TILE)
        assert 1 < s <= min(64, tiles) and ws(n, 3) == s * n * 3 * 8, n
        assert -(-tiles // -(-tiles // s)) == s, n  # no split without a tile
    assert ws(4, 3) == ws(L.KNN_SPLIT_MIN, 8) == 16  # never 0 for a legal pair
    assert splits(2 ** 24) == 1 and ws(2 ** 24, 8) == 16  # the query blocks alone fill the machine
    assert [splits(n) for n in (1, 0, -1, 2 ** 24 + 1, 2 ** 40)] == [0] * 5
    for n, k in ((0, 1), (1, 1), (3, 3), (8, 8), (100, 0), (100, 9), (100, -1), (2 ** 24 + 1, 3), (-5, 3)):
        assert ws(n, k) == 0, (n, k)
    assert [blocks(g) for g in (1, 256, 257, 40000, 256 * 256, 256 * 256 + 1, 2 ** 31 - 1)] == [1, 1, 2, 157, 256, 256, 256]
    assert [blocks(g) for g in (0, -1, 2 ** 31, 2 ** 62)] == [0] * 4
    assert scratch(40000, 69, 20) == 157 * 20 * 72 * 8 + 632 and scratch(1, 1, 1) == 4 * 8 + 8 and scratch(777, 12, 3) == 4 * 3 * 16 * 8 + 16
    for bad_ in ((0, 69, 20), (100, 0, 20), (100, 69, 0), (100, 69, 65), (100, 193, 64), (2 ** 30, 3, 2), (-1, 3, 2), (100, -3, 2), (2 ** 31, 1, 1)):
        assert scratch(*bad_) == 0, bad_


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from deblur4dgs_amd import scene_init as S

    xyz, vis = torch.rand(10, 4, 3), torch.ones(10, 4, dtype=torch.bool)
    tracks = S.TrackObservations(xyz, vis, ~vis, torch.ones(10, 4), torch.rand(10, 3))
    assert tracks.check_sizes() and tracks.filter_valid(torch.arange(10) < 3).xyz.shape == (3, 4, 3)
    static = S.StaticObservations(torch.rand(9, 3), torch.rand(9, 3), torch.rand(9, 3))
    assert static.check_sizes() and static.filter_valid(torch.arange(9) < 2).normals.shape == (2, 3)
    for call in (lambda: S.track_features(xyz, vis), lambda: S.interp_tracks(xyz, vis), lambda: S.knn(xyz[:, 0], 3),
                 lambda: S.kmeans(xyz[:, 0], 2), lambda: S.kmeans_step(xyz[:, 0], xyz[:2, 0], torch.zeros(10, dtype=torch.int32)),
                 lambda: S.init_motion_params_with_procrustes(tracks, 2, "6d", 1), lambda: S.init_fg_from_tracks_3d(1, tracks, torch.rand(10, 2)),
                 lambda: S.init_bg(static), lambda: S.sample_initial_bases_centers(1, tracks, 2)):
        with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback
            call()
