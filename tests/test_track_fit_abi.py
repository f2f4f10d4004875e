"""The entry points of csrc/track_fit.hip are declared under D4GS_FIT_API, parsed into a table of their own (the fifth), bound and
exported, and validate their arguments on the host before any HIP call: fake addresses - nothing is dereferenced; no GPU needed.
The schedule's CPU twin (d4gs_track_fit_schedule_cpu, the kernel's own inline function compiled for the host) is held to
torch.optim.lr_scheduler.ExponentialLR on four param groups and to the reference's w_smooth_func."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import track_fit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_track_fit_targets_bytes", "d4gs_track_fit_workspace_bytes", "d4gs_track_fit_prepare", "d4gs_track_fit_fwd",
       "d4gs_track_fit_bwd", "d4gs_track_fit_schedule", "d4gs_track_fit_schedule_cpu")
A = 0x10000  # a fake, 16-byte aligned device address
G, K, T = 333, 20, 24


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def _header():
    return open(os.path.join(ROOT, "include", "d4gs.h")).read()


def test_header_parses_with_five_blocks_counted():
    from deblur4dgs_amd import _lib as L

    init, ev, data, fit = {}, {}, {}, {}
    constants, structs, prototypes = L.parse(_header(), init, eval=ev, data=data, fit=fit)
    assert (len(prototypes), len(init), len(ev), len(data), len(structs), constants["VERSION"]) == (79, 8, 4, 4, 16, 305)
    assert tuple(fit) == NEW == tuple(L.FIT_PROTOTYPES)
    others = set(L.EXPORTS) | set(L.INIT_PROTOTYPES) | set(L.EVAL_PROTOTYPES) | set(L.DATA_PROTOTYPES)
    assert not set(NEW) & others and len(others) == 79 + 8 + 4 + 4  # a block of its own; the four tables are what they were
    assert tuple(init) == tuple(L.INIT_PROTOTYPES) and tuple(ev) == tuple(L.EVAL_PROTOTYPES) and tuple(data) == tuple(L.DATA_PROTOTYPES)
    # the older ways of calling parse keep their meaning: the fifth block is read and checked all the same
    assert tuple(L.parse(_header())[2]) == tuple(L.parse(_header(), {}, eval={}, data={})[2]) == tuple(prototypes) == L.EXPORTS
    assert "D4gsLeafGrads" in _header().split("#define D4GS_FIT_API")[1] and set(structs) == set(L.STRUCT_NAMES.values())  # no new struct


def test_new_symbols_are_declared_bound_and_exported(lib):
    from deblur4dgs_amd import _lib as L

    header = _header()
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert f"D4GS_FIT_API" in header and f"{name}(" in header and f" T {name}\n" in dyn, name
        restype, argtypes = L.FIT_PROTOTYPES[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype, name
    assert lib.d4gs_track_fit_targets_bytes.restype is C.c_size_t and lib.d4gs_track_fit_workspace_bytes.restype is C.c_size_t
    # the GPU schedule step takes device pointers (void*), its CPU twin typed host pointers: the [host] marks were read
    dev, host = L.FIT_PROTOTYPES["d4gs_track_fit_schedule"][1], L.FIT_PROTOTYPES["d4gs_track_fit_schedule_cpu"][1]
    assert len(dev) == len(host) + 1 and dev[-1] is C.c_void_p  # (the stream)
    assert host[0]._type_ is C.c_int32 and host[2]._type_ is L.AdamRec and host[7]._type_ is C.c_float and host[8]._type_ is C.c_float
    assert dev[0] is C.c_void_p and dev[2] is C.c_void_p and all(d is h for d, h in zip(dev[3:7], host[3:7]))
    assert L.FIT_PROTOTYPES["d4gs_track_fit_bwd"][1][13]._type_ is L.LeafGrads


@pytest.mark.parametrize("old, new, word", [
    ("D4GS_FIT_API size_t d4gs_track_fit_targets_bytes(int32_t G, int32_t T);",
     "D4GS_FIT_API size_t d4gs_track_fit_targets_bytes(int32_t G, int32_t T)", "D4GS_FIT_API prototypes"),    # no semicolon
    ("D4GS_FIT_API size_t d4gs_track_fit_targets_bytes(int32_t G, int32_t T);",
     "D4GS_FIT_API size_t d4gs_track_fit_targets_bytes(long G, int32_t T);", "long G"),                       # unknown type
    ("D4GS_FIT_API size_t d4gs_track_fit_targets_bytes(int32_t G, int32_t T);",
     "D4GS_FIT_API unsigned d4gs_track_fit_targets_bytes(int32_t G, int32_t T);", "d4gs_track_fit_targets_bytes"),  # return type
    ("size_t workspace_bytes, const float *v_out, const D4gsLeafGrads *grads, void *stream);",
     "size_t workspace_bytes, const float *v_out, const D4gsLeafGradz *grads, void *stream);", "D4gsLeafGradz"),
])
def test_a_damaged_fit_line_raises(old, new, word):
    from deblur4dgs_amd import _lib as L

    text = _header()
    assert text.count(old) == 1, old
    with pytest.raises(ValueError) as e:
        L.parse(text.replace(old, new))
    assert word in str(e.value), str(e.value)


def test_size_queries_are_host_arithmetic(lib):
    tb, wb = lib.d4gs_track_fit_targets_bytes, lib.d4gs_track_fit_workspace_bytes
    assert tb(G, T) > 4 * 7 * G * T and tb(G, T) % 16 == 0 and wb(G, K, T) > 4 * 7 * G * T + 4 * G * K and wb(G, K, T) % 16 == 0
    assert tb(1, 3) > 0 and wb(1, 1, 3) > 0 and wb(40000, 20, 24) > wb(40000, 1, 24) and tb(40001, 24) > tb(40000, 24)
    for g, t in ((0, 3), (-1, 3), (1, 2), (1, 0), (1, -5), (1, 65536), (2 ** 27, 8), (-2 ** 31, 3)):
        assert tb(g, t) == 0 and wb(g, 1, t) == 0, (g, t)
    for k in (0, -1, 33, 2 ** 31 - 1):
        assert wb(G, k, T) == 0, k
    assert wb(G, 32, T) > 0 and wb(2 ** 26, 32, 3) == 0  # G K past 2^31 - 1


def _calls(lib):
    tb, wb = lib.d4gs_track_fit_targets_bytes(G, T), lib.d4gs_track_fit_workspace_bytes(G, K, T)
    from deblur4dgs_amd import _lib as L

    grads = L.LeafGrads(v_means=A, v_motion_coefs=A, v_rots=A, v_transls=A)
    #            xyz vis inv conf Ks w2cs | G T | targets bytes stream
    return {"d4gs_track_fit_prepare": ([A, A, A, A, A, A, G, T, A, tb, None], dict(ptrs=(0, 1, 2, 3, 4, 5, 8), G=6, T=7, targets=(8, 9))),
            #  means coefs rots transls | G K T | q weights | targets bytes ws bytes | out | iter losses num_iters | stream
            "d4gs_track_fit_fwd": ([A, A, A, A, G, K, T, 0.95, A, A, tb, A, wb, A, A, A, 1000, None],
                                   dict(ptrs=(0, 1, 2, 3, 9, 11, 13), G=4, K=5, T=6, q=7, targets=(9, 10), ws=(11, 12))),
            #  means coefs rots transls | G K T | q | targets bytes ws bytes | v_out grads stream
            "d4gs_track_fit_bwd": ([A, A, A, A, G, K, T, 0.95, A, tb, A, wb, A, C.pointer(grads), None],
                                   dict(ptrs=(0, 1, 2, 3, 8, 10, 12, 13), G=4, K=5, T=6, q=7, targets=(8, 9), ws=(10, 11)))}, grads


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    from deblur4dgs_amd import _lib as L

    calls, grads = _calls(lib)

    def bad(fn, args, *words):
        assert getattr(lib, fn)(*args) == L.EINVAL, (fn, args)
        err = lib.d4gs_last_error()
        assert fn.encode() in err and all(w in err for w in words), err

    def put(args, i, v):
        return args[:i] + [v] + args[i + 1:]

    for fn, (good, at) in calls.items():
        for i in at["ptrs"]:
            bad(fn, put(good, i, None), b"NULL")
        for v in (0, -1, -2 ** 31):
            bad(fn, put(good, at["G"], v), b"bad size", f"G={v}".encode())
        for v in (2, 1, 0, -1, 65536):
            bad(fn, put(good, at["T"], v), b"bad size", f"T={v}".encode())
        bad(fn, put(good, at["G"], 2 ** 27), b"bad size", b"2^31 - 1")  # 9 G T overflows
        i, n = at["targets"]
        bad(fn, put(good, n, good[n] - 1), b"targets", b"needed")
        bad(fn, put(good, n, 0), b"targets")
        for off in (1, 4, 8):
            bad(fn, put(good, i, A + off), b"targets", b"aligned")
        if "K" in at:
            for v in (0, -1, 33, 2 ** 31 - 1):
                bad(fn, put(good, at["K"], v), b"bad size", f"K={v}".encode())
            i, n = at["ws"]
            bad(fn, put(good, n, good[n] - 1), b"workspace", b"needed")
            for off in (1, 4, 8):
                bad(fn, put(good, i, A + off), b"workspace", b"aligned")
            for q in (0.0, -0.5, float("nan"), float("inf")):
                bad(fn, put(good, at["q"], q), b"quantile")
    fwd = calls["d4gs_track_fit_fwd"][0]
    bad("d4gs_track_fit_fwd", put(put(put(fwd, 4, 2 ** 26), 10, 2 ** 40), 12, 2 ** 40), b"bad size")  # G K = 20 * 2^26 overflows
    # a loss history is optional; with one, the counter and a row count are required
    for i, v, word in ((14, None, b"iter"), (16, 0, b"num_iters=0"), (16, -3, b"num_iters=-3"), (15, A + 2, b"aligned"), (14, A + 1, b"aligned")):
        bad("d4gs_track_fit_fwd", put(fwd, i, v), b"loss history", word)
    # the four gradients the backward overwrites are required; the others are not read
    for k in ("v_means", "v_motion_coefs", "v_rots", "v_transls"):
        g = L.LeafGrads(v_means=A, v_motion_coefs=A, v_rots=A, v_transls=A)
        setattr(g, k, None)
        bad("d4gs_track_fit_bwd", put(calls["d4gs_track_fit_bwd"][0], 13, C.pointer(g)), b"NULL")


def test_schedule_refuses_bad_arguments_before_any_hip_call(lib):
    from deblur4dgs_amd import _lib as L

    ok = [A, 1000, A, 1e-2, 3e-2, 1e-2, 1e-3, A, A, None]
    for i, name in ((0, "iter"), (2, "table"), (7, "weights")):
        args = list(ok)
        args[i] = None
        assert lib.d4gs_track_fit_schedule(*args) == L.EINVAL and b"d4gs_track_fit_schedule:" in lib.d4gs_last_error() \
            and b"NULL" in lib.d4gs_last_error(), name
    for i in (0, 2, 7, 8):
        args = list(ok)
        args[i] = A + 2
        assert lib.d4gs_track_fit_schedule(*args) == L.EINVAL and b"misaligned" in lib.d4gs_last_error(), i
    for n in (0, -1):
        args = list(ok)
        args[1] = n
        assert lib.d4gs_track_fit_schedule(*args) == L.EINVAL and f"num_iters={n}".encode() in lib.d4gs_last_error()
    for i in (3, 4, 5, 6):
        for v in (0.0, -1e-2, float("nan"), float("inf")):
            args = list(ok)
            args[i] = v
            assert lib.d4gs_track_fit_schedule(*args) == L.EINVAL and f"lr0[{i - 3}]".encode() in lib.d4gs_last_error()


def _twin(lib, num_iters, steps, start=0):
    """`steps` calls of the CPU twin from iteration `start` -> (lrs [num_iters,4] fp32, table lrs per call [steps,4] fp64,
    weights per call [steps,6] fp32, the counter)"""
    from deblur4dgs_amd import _lib as L

    table = (L.AdamRec * 4)()
    it = C.c_int32(start)
    weights = (C.c_float * 6)()
    lrs = np.zeros((num_iters, 4), np.float32)
    tab, ws = [], []
    for _ in range(steps):
        rc = lib.d4gs_track_fit_schedule_cpu(C.byref(it), num_iters, table, *R.LR0, weights, lrs.ctypes.data_as(C.POINTER(C.c_float)))
        assert rc == 0, lib.d4gs_last_error()
        tab.append([table[r].lr for r in range(4)])
        ws.append(list(weights))
    return lrs, np.asarray(tab), np.asarray(ws, np.float32), it.value


@pytest.mark.parametrize("num_iters", [1, 7, 400, 404, 1000])
def test_schedule_twin_matches_exponential_lr_and_w_smooth_func(lib, num_iters):
    lrs, tab, ws, count = _twin(lib, num_iters, num_iters)
    assert count == num_iters
    params = [torch.zeros(1, requires_grad=True) for _ in range(4)]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(params, R.LR0)])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.1 ** (1 / num_iters))
    for i in range(num_iters):
        want = np.asarray([g["lr"] for g in opt.param_groups])  # the rates update i runs at: torch's chained product
        # 1 000 double multiplications drift by ~1e-13 relative, far below half an fp32 ulp: within one fp32 ulp of torch
        w32 = want.astype(np.float32)
        assert np.all(np.abs(lrs[i].astype(np.float64) - w32.astype(np.float64)) <= np.spacing(w32).astype(np.float64)), (i, lrs[i], w32)
        assert np.all(np.abs(tab[i] - want) <= 1e-12 * want), (i, tab[i], want)
        assert np.array_equal(ws[i], np.asarray(R.weights(i, num_iters), np.float64).astype(np.float32)), (i, ws[i])
        opt.step()
        sched.step()
    assert np.array_equal(tab[0], np.asarray(R.LR0))  # iteration 0 runs at lr0 itself


def test_schedule_twin_past_the_end_and_without_a_history(lib):
    from deblur4dgs_amd import _lib as L

    for n in (5, 400):  # no ramp at all when num_iters <= 400: a counter past the end (and past 400) still never divides by <= 0
        _, tab, ws, _ = _twin(lib, n, 4, start=399)
        assert np.isfinite(ws).all() and np.all(ws[:, 3] == np.float32(0.01)) and np.all(ws[:, 4] == np.float32(0.005)) and np.isfinite(tab).all()

    lrs, tab, ws, count = _twin(lib, 5, 3, start=4)  # iterations 4, 5, 6 of 5: only row 4 exists
    assert count == 7 and np.all(lrs[:4] == 0) and np.all(lrs[4] > 0)
    assert np.all(tab[1] < tab[0]) and np.all(tab[2] < tab[1])  # the decay goes on; nothing is written past the history
    table, it, weights = (L.AdamRec * 4)(), C.c_int32(0), (C.c_float * 6)()
    assert lib.d4gs_track_fit_schedule_cpu(C.byref(it), 10, table, *R.LR0, weights, None) == 0 and it.value == 1
    assert lib.d4gs_track_fit_schedule_cpu(None, 10, table, *R.LR0, weights, None) == L.EINVAL
    assert lib.d4gs_track_fit_schedule_cpu(C.byref(it), 0, table, *R.LR0, weights, None) == L.EINVAL


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from deblur4dgs_amd import losses
    from deblur4dgs_amd import scene_init as S
    from deblur4dgs_amd.scene_model import GaussianParams, MotionBases

    c = R.make_case(10, 2, 4, 1)
    tracks = S.TrackObservations(c["xyz"], c["visibles"], c["invisibles"], c["confidences"], torch.zeros(10, 3))
    with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback
        S.track_fit_targets(tracks, c["Ks"], c["w2cs"])
    fg = GaussianParams(c["means"], torch.randn(10, 4), torch.zeros(10, 3), torch.zeros(10, 3), torch.zeros(10), motion_coefs=c["motion_coefs"])
    bases = MotionBases(c["rots"], c["transls"])
    with pytest.raises(RuntimeError, match="ROCm"):
        S.run_initial_optim(fg, bases, tracks, c["Ks"], c["w2cs"], num_iters=3)
    with pytest.raises(NotImplementedError, match="depth-range"):
        S.run_initial_optim(fg, bases, tracks, c["Ks"], c["w2cs"], num_iters=3, use_depth_range_loss=True)
    with pytest.raises(ValueError, match="num_iters"):
        S.run_initial_optim(fg, bases, tracks, c["Ks"], c["w2cs"], num_iters=0)
    targets = S.TrackFitTargets(torch.zeros(16, dtype=torch.uint8), 10, 4)
    leaves = [c[k] for k in R.LEAVES]
    with pytest.raises(RuntimeError, match="ROCm"):
        losses.track_fit_losses(*leaves, targets)
    with pytest.raises(ValueError, match="T >= 3"):
        losses.track_fit_losses(c["means"], c["motion_coefs"], c["rots"][:, :2], c["transls"][:, :2], S.TrackFitTargets(targets.buf, 10, 2))
    with pytest.raises(ValueError, match="targets of G"):
        losses.track_fit_losses(*leaves, S.TrackFitTargets(targets.buf, 11, 4))
    with pytest.raises(ValueError, match="quantile"):
        losses.track_fit_losses(*leaves, targets, quantile=0.0)
    with pytest.raises(ValueError, match="expected"):
        losses.track_fit_losses(c["means"][:, :2], *leaves[1:], targets)
