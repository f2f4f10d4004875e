"""The entry points of csrc/feed.hip (d4gs_feed_draw, d4gs_feed_draw_cpu, d4gs_feed_batch) are declared under D4GS_FEED_API, parsed into
a table of their own (the sixth), bound and exported, and validate their arguments on the host before any launch: fake addresses -
nothing is dereferenced; no GPU needed.  The draw's CPU twin (the kernel's own functions compiled for the host) is held to what a draw
must be: distinct frames of the range, a pure function of (seed, step), every frame equally often."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_feed_draw", "d4gs_feed_draw_cpu", "d4gs_feed_batch")
A = 0x10000  # a fake, 16-byte aligned device address

#                           counter seed start end n targets stream
CALLS = {"d4gs_feed_draw": ([A, 7, 1, 5, 4, A, None], {0: (b"counter", True, 8), 5: (b"targets", True, 4)}),
         #                   imgs depths masks valid Ks w2cs time_ids tracks offsets | n_rows | index targets | F H W N P num_frames |
         "d4gs_feed_batch": ([A, A, A, A, A, A, A, A, A, 6 * 700, A, A, 6, 24, 32, 4, 257, 4,
                              # ts w2c K | img valid_mask mask depth | query target_ts target_w2cs target_Ks target_tracks_2d |
                              A, A, A, A, A, A, A, A, A, A, A, A,
                              # visibles invisibles confidences track_depths track_imgs | pix rows vis weights | n_queries status stream
                              A, A, A, A, A, A, A, A, A, A, A, None],
                             {0: (b"imgs", True, 4), 1: (b"depths", True, 4), 2: (b"masks", True, 4), 3: (b"valid_masks", True, 4),
                              4: (b"Ks", True, 4), 5: (b"w2cs", True, 4), 6: (b"time_ids", True, 8), 7: (b"tracks", True, 16),
                              8: (b"offsets", True, 8), 10: (b"index", True, 4), 11: (b"targets", True, 4), 18: (b"ts", True, 8),
                              19: (b"w2c", True, 4), 20: (b"K", True, 4), 21: (b"img", False, 4), 22: (b"valid_mask", False, 4),
                              23: (b"mask", False, 4), 24: (b"depth", False, 4), 25: (b"query_tracks_2d", True, 8),
                              26: (b"target_ts", True, 8), 27: (b"target_w2cs", True, 4), 28: (b"target_Ks", True, 4),
                              29: (b"target_tracks_2d", True, 8), 30: (b"target_visibles", True, 1), 31: (b"target_invisibles", True, 1),
                              32: (b"target_confidences", True, 4), 33: (b"target_track_depths", True, 4),
                              34: (b"target_track_imgs", True, 4), 35: (b"pix", True, 4), 36: (b"rows", True, 4), 37: (b"vis", True, 1),
                              38: (b"weights", True, 4), 39: (b"n_queries", True, 4), 40: (b"status", True, 4)})}
OFFSETS = {1: (), 4: (1, 2, 3), 8: (1, 2, 4), 16: (1, 4, 8)}


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def _header():
    return open(os.path.join(ROOT, "include", "d4gs.h")).read()


def put(fn, i, v):
    base = CALLS[fn][0]
    return base[:i] + [v] + base[i + 1:]


def bad(lib, fn, args, *words):
    assert getattr(lib, fn)(*args) == -1, (fn, args)  # D4GS_EINVAL
    err = lib.d4gs_last_error()
    assert fn.encode() in err and all(w in err for w in words), err


def host(address, ctype):
    """a typed host pointer to a fake address (None: NULL), as d4gs_feed_draw_cpu's [host] parameters take it"""
    return C.cast(address, C.POINTER(ctype)) if address else None


def test_the_block_is_declared_parsed_bound_and_exported_in_a_table_of_its_own(lib):
    from deblur4dgs_amd import _lib as L

    header = _header()
    assert lib.d4gs_version() == 305 and "#define D4GS_VERSION 305" in header and L.VERSION == 305 and len(L.EXPORTS) == 79
    init, ev, data, fit, feed = {}, {}, {}, {}, {}
    _, structs, prototypes = L.parse(header, init, eval=ev, data=data, fit=fit, feed=feed)
    assert tuple(feed) == NEW == tuple(L.FEED_PROTOTYPES)  # in the header's order
    others = (L.EXPORTS, L.INIT_PROTOTYPES, L.EVAL_PROTOTYPES, L.DATA_PROTOTYPES, L.FIT_PROTOTYPES)
    assert all(not set(NEW) & set(t) for t in others) and tuple(prototypes) == L.EXPORTS  # disjoint from the other five tables
    assert (tuple(init), tuple(ev), tuple(data), tuple(fit)) == tuple(tuple(t) for t in others[1:])
    assert set(structs) == set(L.STRUCT_NAMES.values())  # no new struct
    assert tuple(L.parse(header)[2]) == L.EXPORTS  # the keyword is optional: the block is read and counted all the same
    assert header.count("D4GS_FEED_API") >= len(NEW) + 1 and header.index("#define D4GS_FEED_API") > header.index("#define D4GS_FIT_API")
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert hasattr(lib, name) and f"{name}(" in header and f" T {name}\n" in dyn, name
        assert getattr(lib, name).argtypes == L.FEED_PROTOTYPES[name][1] and getattr(lib, name).restype is L.FEED_PROTOTYPES[name][0], name
    # the device draw takes device pointers (void*), its twin typed host pointers: the [host] marks were read; the seed is 64 bits wide
    dev, cpu = L.FEED_PROTOTYPES["d4gs_feed_draw"][1], L.FEED_PROTOTYPES["d4gs_feed_draw_cpu"][1]
    assert len(dev) == len(cpu) + 1 and dev[-1] is C.c_void_p and dev[0] is C.c_void_p and dev[5] is C.c_void_p
    assert cpu[0]._type_ is C.c_int64 and cpu[5]._type_ is C.c_int32 and dev[1] is cpu[1] is C.c_uint64
    assert all(t is C.c_void_p or not hasattr(t, "contents") for t in L.FEED_PROTOTYPES["d4gs_feed_batch"][1])  # all device pointers


@pytest.mark.parametrize("new, word", [
    ("D4GS_FEED_API int d4gs_feed_draw(int64_t *counter, uint64_t seed, int32_t start, int32_t end, int32_t n, int32_t *targets, void *stream)",
     "D4GS_FEED_API prototypes"),  # no semicolon
    ("D4GS_FEED_API int d4gs_feed_draw(int64_t *counter, unsigned long seed, int32_t start, int32_t end, int32_t n, int32_t *targets, void *stream);",
     "d4gs_feed_draw"),            # unknown type
    ("D4GS_FEED_API unsigned d4gs_feed_draw(int64_t *counter, uint64_t seed, int32_t start, int32_t end, int32_t n, int32_t *targets, void *stream);",
     "d4gs_feed_draw")])           # return type
def test_the_feed_block_is_parsed_as_strictly_as_the_rest(new, word):
    from deblur4dgs_amd import _lib as L

    old = "D4GS_FEED_API int d4gs_feed_draw(int64_t *counter, uint64_t seed, int32_t start, int32_t end, int32_t n, int32_t *targets, void *stream);"
    text = _header()
    assert text.count(old) == 1
    with pytest.raises(ValueError) as e:
        L.parse(text.replace(old, new))
    assert word in str(e.value), str(e.value)


def test_null_and_misaligned_pointers_are_refused(lib):
    for fn, (_, ptrs) in CALLS.items():
        for i, (name, required, align) in ptrs.items():
            if required:
                bad(lib, fn, put(fn, i, None), name, b"NULL")
            for off in OFFSETS[align]:
                bad(lib, fn, put(fn, i, A + off), name, b"misaligned")
    fn = "d4gs_feed_draw_cpu"
    bad(lib, fn, [None, 7, 1, 5, 4, host(A, C.c_int32)], b"counter", b"NULL")
    bad(lib, fn, [host(A, C.c_int64), 7, 1, 5, 4, None], b"targets", b"NULL")
    for off in OFFSETS[8]:
        bad(lib, fn, [host(A + off, C.c_int64), 7, 1, 5, 4, host(A, C.c_int32)], b"counter", b"misaligned")
    for off in OFFSETS[4]:
        bad(lib, fn, [host(A, C.c_int64), 7, 1, 5, 4, host(A + off, C.c_int32)], b"targets", b"misaligned")


def test_bad_sizes_are_refused(lib):
    fn = "d4gs_feed_batch"
    for i, name in ((12, b"F="), (13, b"H="), (14, b"W="), (15, b"N="), (16, b"P="), (17, b"num_frames="), (9, b"n_rows=")):
        for v in (0, -1, -2 ** 31):
            bad(lib, fn, put(fn, i, v), b"bad size", name + str(v).encode())
    bad(lib, fn, put(fn, 15, 65), b"N=65")                                       # one wave holds a draw
    bad(lib, fn, put(fn, 13, 2 ** 22), b"overflows", b"H=4194304 W=32")          # F H W 3
    bad(lib, fn, put(fn, 16, 2 ** 28), b"overflows", b"N=4 P=268435456")         # N P 3
    for i in (21, 22, 23, 24):  # the four planes: all or none
        bad(lib, fn, put(fn, i, None), b"come together")
    for fn, args in (("d4gs_feed_draw", lambda *a: [A, 7, *a, A, None]),
                     ("d4gs_feed_draw_cpu", lambda *a: [host(A, C.c_int64), 7, *a, host(A, C.c_int32)])):
        for start, end in ((-1, 5), (5, 5), (6, 5), (0, 0), (-2 ** 31, 2 ** 31 - 1)):
            bad(lib, fn, args(start, end, 1), b"bad range", f"start={start} end={end}".encode())
        for n in (0, -1, 5, 2 ** 31 - 1):  # n > end - start = 4 included
            bad(lib, fn, args(1, 5, n), f"n={n}".encode())
        bad(lib, fn, args(0, 100, 65), b"n=65")


def test_the_cpu_draw_is_distinct_in_range_and_a_function_of_seed_and_step():
    from deblur4dgs_amd.feed import draw_cpu

    seen = set()
    for seed in (0, 1, 2 ** 63 + 5, -3):
        for step in (0, 1, 2, 1000, 2 ** 40):
            for start, end, n in ((1, 5, 4), (1, 5, 1), (3, 24, 4), (0, 64, 64), (0, 1000, 64), (7, 8, 1)):
                t = draw_cpu(seed, step, start, end, n)
                assert len(t) == n == len(set(t)) and all(start <= x < end for x in t), (seed, step, start, end, n, t)
                assert t == draw_cpu(seed, step, start, end, n)
            seen.add(tuple(draw_cpu(seed, step, 0, 1000, 8)))
    assert len(seen) == 20  # another seed or step: another draw
    with pytest.raises(RuntimeError, match="n=5"):
        draw_cpu(0, 0, 1, 5, 5)


@pytest.mark.parametrize("n", (1, 4))
def test_the_cpu_draw_visits_every_frame_equally_often(n):
    """4 000 steps over an 8-frame range: a frame is expected 4 000 n / 8 times and must be drawn between 0.8 and 1.2 times that.  For
    n = 1 the count is binomial(4 000, 1 / 8): mean 500, standard deviation 20.9, so the bound is 4.8 standard deviations; for n = 4
    (mean 2 000, at most sqrt(4 000 / 4) = 31.6) it is 12."""
    from deblur4dgs_amd.feed import draw_cpu

    counts = np.zeros(8, np.int64)
    for step in range(4000):
        for t in draw_cpu(12345, step, 3, 11, n):
            counts[t - 3] += 1
    expected = 4000 * n / 8
    print("draws per frame / expected:", np.round(counts / expected, 3))
    assert counts.sum() == 4000 * n and (counts >= 0.8 * expected).all() and (counts <= 1.2 * expected).all(), counts


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from deblur4dgs_amd import feed, losses

    F, H, W = 3, 8, 9
    img, d, m = torch.rand(F, H, W, 3), torch.rand(F, H, W), torch.ones(F, H, W)
    Ks, w2cs, ids = torch.eye(3).repeat(F, 1, 1), torch.eye(4).repeat(F, 1, 1), torch.arange(F)
    with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback
        feed.DeviceClip(img, d, m, m, Ks, w2cs, ids, [torch.rand(F, 5, 4)] * F, 0, F, 2)
    tables = dict(pix=torch.zeros(4, dtype=torch.int32), rows=torch.zeros(4, dtype=torch.int32), vis=torch.ones(4, dtype=torch.uint8),
                  weights=torch.ones(4), tgt_2d=torch.zeros(4, 2), tgt_depth=torch.ones(4), Ks=torch.eye(3).reshape(1, 9).repeat(2, 1))
    with pytest.raises(RuntimeError, match="ROCm"):
        losses.track_losses_from_tables(torch.rand(1, H, W, 2, 3), tables)
    with pytest.raises(ValueError, match=r"\[1,H,W,N,3\]"):
        losses.track_losses_from_tables(torch.rand(2, H, W, 2, 3), tables)
