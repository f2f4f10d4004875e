"""d4gs_motion_regs_workspace_bytes / d4gs_motion_regs_fwd / d4gs_motion_regs_bwd (csrc/motion_regs.hip) are declared, bound and
exported, and validate their arguments on the host before any launch: fake addresses - nothing is dereferenced; no GPU needed."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_motion_regs_workspace_bytes", "d4gs_motion_regs_fwd", "d4gs_motion_regs_bwd")
A = 0x10000  # a fake, 16-byte aligned device address
G, K, T, B = 100, 5, 8, 2


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def test_new_symbols_are_declared_bound_and_exported_and_the_version_is_305(lib):
    from deblur4dgs_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    assert lib.d4gs_version() == 305 and "#define D4GS_VERSION 305" in header and L.VERSION == 305
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert hasattr(lib, name) and name in L.EXPORTS and f"{name}(" in header, name
        assert getattr(lib, name).argtypes is not None, name
        assert f" T {name}\n" in dyn, name


def test_workspace_query(lib):
    n = lib.d4gs_motion_regs_workspace_bytes(G, K, T, B)
    assert n >= 2 * 4 * 3 * B * G * 3 and n % 16 == 0  # at least the neighbour means and their gradient
    assert lib.d4gs_motion_regs_workspace_bytes(2 * G, K, T, B) > n and lib.d4gs_motion_regs_workspace_bytes(G, K, T, 2 * B) > n
    for bad in ((0, K, T, B), (-1, K, T, B), (G, 0, T, B), (G, 33, T, B), (G, K, 2, B), (G, K, T, 0), (2 ** 30, K, T, 1), (G, K, 2 ** 27, B)):
        assert lib.d4gs_motion_regs_workspace_bytes(*bad) == 0, bad
    assert lib.d4gs_motion_regs_workspace_bytes(G, 32, 3, 1) > 0  # the smallest T and the largest K are legal


def bad(lib, fn, args, word):
    assert getattr(lib, fn)(*args) == -1, (fn, args)  # D4GS_EINVAL
    assert fn.encode() in lib.d4gs_last_error() and word in lib.d4gs_last_error(), lib.d4gs_last_error()


SIZES = ((0, 0, b"size"), (0, -3, b"size"), (1, 0, b"size"), (1, 33, b"size"), (1, -1, b"size"), (2, 2, b"size"), (2, 0, b"size"),
         (3, 0, b"size"), (3, -2, b"size"), (0, 2 ** 30, b"size"), (2, 2 ** 27, b"size"))  # (which of G K T B, value, word)


def test_forward_rejects_bad_arguments_before_any_launch(lib):
    n = lib.d4gs_motion_regs_workspace_bytes(G, K, T, B)
    #     means coefs scales rots transls ts w2cs | G K T B | weights | workspace bytes out stream
    ok = [A] * 7 + [G, K, T, B, 1.0, 2.0, A, n, A, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 13, 15):
        bad(lib, "d4gs_motion_regs_fwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    for i, v, word in SIZES:
        bad(lib, "d4gs_motion_regs_fwd", ok[:7 + i] + [v] + ok[8 + i:], word)
    for i, v in ((14, n - 1), (14, 0), (13, A + 4), (14, lib.d4gs_motion_regs_workspace_bytes(G, K, T, 1))):
        bad(lib, "d4gs_motion_regs_fwd", ok[:i] + [v] + ok[i + 1:], b"workspace")


def test_backward_rejects_bad_arguments_before_any_launch(lib):
    from deblur4dgs_amd import _lib as L

    n = lib.d4gs_motion_regs_workspace_bytes(G, K, T, B)
    full = dict(v_means=A, v_motion_coefs=A, v_scales=A, v_rots=A, v_transls=A)

    def grads(**kw):
        g = L.LeafGrads()
        for k, v in dict(full, **kw).items():
            setattr(g, k, v)
        return C.byref(g)

    #     means coefs scales rots transls | G K T B | weights | workspace bytes v_out grads stream
    ok = [A] * 5 + [G, K, T, B, 1.0, 2.0, A, n, A, grads(), None]
    for i in (0, 1, 2, 3, 4, 11, 13, 14):
        bad(lib, "d4gs_motion_regs_bwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    for k in full:
        bad(lib, "d4gs_motion_regs_bwd", ok[:14] + [grads(**{k: None})] + ok[15:], b"NULL")
    for i, v, word in SIZES:
        bad(lib, "d4gs_motion_regs_bwd", ok[:5 + i] + [v] + ok[6 + i:], word)
    for i, v in ((12, n - 1), (11, A + 8)):
        bad(lib, "d4gs_motion_regs_bwd", ok[:i] + [v] + ok[i + 1:], b"workspace")


def test_python_wrapper_checks_shapes_on_the_host_and_refuses_cpu_tensors():
    from deblur4dgs_amd.losses import motion_regularizers

    def args(G=6, K=3, T=5, B=2, **kw):
        a = dict(means=torch.rand(G, 3), motion_coefs=torch.rand(G, K), rots=torch.rand(K, T, 6), transls=torch.rand(K, T, 3),
                 scales=torch.rand(G, 3), ts=torch.rand(B), w2cs=torch.eye(4).repeat(B, 1, 1))
        a.update(kw)
        return list(a.values())

    with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback, as the other losses
        motion_regularizers(*args())
    for a in (args(G=0), args(T=2), args(motion_coefs=torch.rand(6, 4)), args(transls=torch.rand(3, 6, 3)), args(transls=torch.rand(2, 5, 3)),
              args(w2cs=torch.eye(4).repeat(3, 1, 1)), args(B=0), args(scales=torch.rand(5, 3)), args(means=torch.rand(6, 4)),
              args(w2cs=torch.eye(4)), args(rots=torch.rand(3, 5, 9))):
        with pytest.raises(ValueError):
            motion_regularizers(*a)
