"""The entry points of csrc/pose_refine.hip (d4gs_pose_bwd_partials_elems, d4gs_pose_bwd, d4gs_pose_step, d4gs_pose_step_cpu) are
declared under D4GS_EVAL_API, parsed into a table of their own, bound and exported, and validate their arguments on the host before
any HIP call: fake addresses - nothing is dereferenced; no GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_pose_bwd_partials_elems", "d4gs_pose_bwd", "d4gs_pose_step", "d4gs_pose_step_cpu")
A = 0x10000  # a fake, 16-byte aligned device address


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def _header():
    return open(os.path.join(ROOT, "include", "d4gs.h")).read()


def test_header_parses_with_three_blocks_counted():
    from deblur4dgs_amd import _lib as L

    init, ev = {}, {}
    constants, structs, prototypes = L.parse(_header(), init, eval=ev)
    assert (len(prototypes), len(init), len(structs), constants["VERSION"]) == (79, 8, 16, 305)
    assert tuple(ev) == NEW == tuple(L.EVAL_PROTOTYPES)
    assert not set(NEW) & (set(L.EXPORTS) | set(L.INIT_PROTOTYPES))  # a block of its own
    # the two older ways of calling parse keep their meaning: the third block is read and checked all the same
    assert tuple(L.parse(_header())[2]) == tuple(L.parse(_header(), {})[2]) == tuple(prototypes) == L.EXPORTS


def test_new_symbols_are_declared_bound_and_exported(lib):
    from deblur4dgs_amd import _lib as L

    header = _header()
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert f"{name}(" in header and f" T {name}\n" in dyn, name
        restype, argtypes = L.EVAL_PROTOTYPES[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype, name
    assert lib.d4gs_pose_bwd_partials_elems.restype is C.c_size_t
    # the GPU entry points take device pointers (void*), the CPU twin typed host pointers: the [host] marks were read
    dev, host = L.EVAL_PROTOTYPES["d4gs_pose_step"][1], L.EVAL_PROTOTYPES["d4gs_pose_step_cpu"][1]
    assert len(dev) == len(host) + 1 and dev[-1] is C.c_void_p  # (the stream)
    for d, h in zip(dev, host):
        if d is C.c_void_p:
            assert hasattr(h, "contents") and h._type_ in (C.c_float, C.c_int32), (d, h)
        else:
            assert d is h
    assert not any(hasattr(t, "contents") and t._type_ in (C.c_float, C.c_int32) for t in L.EVAL_PROTOTYPES["d4gs_pose_bwd"][1])


@pytest.mark.parametrize("old, new, word", [
    ("D4GS_EVAL_API size_t d4gs_pose_bwd_partials_elems(const D4gsDims *dims);",
     "D4GS_EVAL_API size_t d4gs_pose_bwd_partials_elems(const D4gsDims *dims)", "D4GS_EVAL_API prototypes"),       # no semicolon
    ("D4GS_EVAL_API size_t d4gs_pose_bwd_partials_elems(const D4gsDims *dims);",
     "D4GS_EVAL_API size_t d4gs_pose_bwd_partials_elems(const D4gsDimz *dims);", "D4gsDimz"),                      # unknown type
    ("D4GS_EVAL_API size_t d4gs_pose_bwd_partials_elems(const D4gsDims *dims);",
     "D4GS_EVAL_API unsigned d4gs_pose_bwd_partials_elems(const D4gsDims *dims);", "d4gs_pose_bwd_partials_elems"),  # return type
    ("int32_t t_max, double beta1, double beta2, double eps, float *lr_out, float *W,",
     "int32_t t_max, double beta1, long double beta2, double eps, float *lr_out, float *W,", "d4gs_pose_step"),
])
def test_a_damaged_eval_line_raises(old, new, word):
    from deblur4dgs_amd import _lib as L

    text = _header()
    assert text.count(old) == 1, old
    with pytest.raises(ValueError) as e:
        L.parse(text.replace(old, new))
    assert word in str(e.value), str(e.value)


def _dims(L, **kw):
    d = dict(N=100, G=0, K=0, T=0, S=2, D=3, width=64, height=48)
    d.update(kw)
    return L.Dims(**d)


def test_pose_bwd_refuses_bad_arguments_before_any_hip_call(lib):
    from deblur4dgs_amd import _lib as L

    ok_in = dict(means=A, quats=A, scales=A, viewmat=A, Kmat=A, RTs=A)
    ok_out = dict(radii=A, conics=A)
    call = lambda d, pin, pout, *rest: lib.d4gs_pose_bwd(C.byref(d) if d is not None else None, C.byref(pin) if pin is not None else None,
                                                         C.byref(pout) if pout is not None else None, *rest, None)
    good = [A, A, A, A, A, A]  # v_means2d, v_conics, v_depths, v_viewmat, v_RTs, partials
    d = _dims(L)

    def bad(args, *words, dims=d, pin=ok_in, pout=ok_out):
        pin = None if pin is None else L.ProjIn(**pin)
        pout = None if pout is None else L.ProjOut(**pout)
        assert call(dims, pin, pout, *args) == L.EINVAL
        assert all(w in lib.d4gs_last_error() for w in words), lib.d4gs_last_error()

    bad(good, b"dims is NULL", dims=None)
    bad(good, b"NULL", pin=None)
    bad(good, b"NULL", pout=None)
    for k in ("means", "quats", "scales", "viewmat", "Kmat"):
        bad(good, b"d4gs_pose_bwd", b"NULL required", pin={**ok_in, k: None})
    for k in ok_out:
        bad(good, b"d4gs_pose_bwd", b"NULL required", pout={**ok_out, k: None})
    for i in range(4):
        bad(good[:i] + [None] + good[i + 1:], b"d4gs_pose_bwd", b"NULL required")
    bad(good[:5] + [None], b"d4gs_pose_bwd", b"partials")
    bad(good, b"motion dims", dims=_dims(L, G=101, K=2, T=3))  # G > N
    bad(good, b"motion_coefs", dims=_dims(L, G=50, K=2, T=3))  # G > 0 without the bases
    bad(good, b"v_RTs", b"in->RTs", pin={**ok_in, "RTs": None})
    bad(good, b"S=65536", dims=_dims(L, S=65536))


def test_partials_query_is_host_arithmetic(lib):
    from deblur4dgs_amd import _lib as L

    q = lambda **kw: lib.d4gs_pose_bwd_partials_elems(C.byref(_dims(L, **kw)))
    assert q(N=1, S=1) == 24 and q(N=256, S=3) == 3 * 24 and q(N=257, S=3) == 3 * 2 * 24 and q(N=0, S=1) == 24
    assert q(N=1000, G=500, K=9, T=4, S=3) == 3 * 4 * 24 + 3 * 9 * 16  # + room for the blended-bases table
    assert q(N=10, G=11, K=1, T=1) == 0 and q(S=0) == 0 and lib.d4gs_pose_bwd_partials_elems(None) == 0


def test_pose_step_refuses_bad_arguments_before_any_hip_call(lib):
    from deblur4dgs_amd import _lib as L

    ok = [A, A, A, A, A, A, 1e-2, 1e-4, 500, 0.9, 0.999, 1e-8, A, A, None]
    for i, name in ((0, "w2c"), (1, "v_W"), (2, "p"), (3, "m"), (4, "v"), (5, "step"), (13, "W")):
        args = list(ok)
        args[i] = None
        assert lib.d4gs_pose_step(*args) == L.EINVAL and b"d4gs_pose_step:" in lib.d4gs_last_error() and b"NULL" in lib.d4gs_last_error(), name
        args[i] = A + 2
        assert lib.d4gs_pose_step(*args) == L.EINVAL and b"misaligned" in lib.d4gs_last_error(), name
    for t_max in (0, -1):
        args = list(ok)
        args[8] = t_max
        assert lib.d4gs_pose_step(*args) == L.EINVAL and f"t_max={t_max}".encode() in lib.d4gs_last_error()
