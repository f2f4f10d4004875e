"""d4gs_metrics_blocks / d4gs_masked_metrics (csrc/metrics.hip) are declared, bound and exported, and validate their arguments on
the host before any launch: fake addresses - nothing is dereferenced; no GPU needed."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_metrics_blocks", "d4gs_masked_metrics")
A = 0x10000  # a fake, 16-byte aligned device address
FN = "d4gs_masked_metrics"


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
    assert lib.d4gs_metrics_blocks.restype is C.c_int64


def test_block_counts(lib):
    blocks = lib.d4gs_metrics_blocks
    assert blocks(1, 1, 11, 11) == 1 and blocks(3, 2, 27, 38) == 3 * 2 * 2 * 3 and blocks(1, 1, 16, 17) == 2 and blocks(1, 1, 17, 16) == 2
    assert blocks(3, 1, 288, 512) == 3 * 18 * 32 and blocks(3, 1, 720, 1280) == 3 * 45 * 80 and blocks(1, 1, 1, 1) == 1
    assert blocks(65535, 1, 16, 16) == 65535 and blocks(1, 1, 16 * 65535, 16) == 65535  # the grid's last legal sizes
    for bad in ((0, 1, 11, 11), (1, 0, 11, 11), (1, 1, 0, 11), (1, 1, 11, 0), (-1, 1, 11, 11), (1, 1, -5, 11), (65536, 1, 16, 16),
                (256, 256, 16, 16), (1, 1, 16 * 65535 + 1, 16), (1, 1, 2 ** 31 - 1, 2 ** 31 - 1), (4, 1, 16 * 65535, 16 * 8193)):
        assert blocks(*bad) == 0, bad


def bad(lib, args, *words):
    assert lib.d4gs_masked_metrics(*args) == -1, args  # D4GS_EINVAL
    err = lib.d4gs_last_error()
    assert FN.encode() in err and all(w in err for w in words), err


#     pred target masks | M B H W | want_ssim | partials out stream
OK = [A, A, A, 3, 2, 27, 38, 1, A, A, None]
NAMES = {0: b"pred", 1: b"target", 2: b"masks", 8: b"partials", 9: b"out"}


def put(i, v, base=OK):
    return base[:i] + [v] + base[i + 1:]


def test_null_and_misaligned_pointers_are_refused(lib):
    for i in (0, 1, 8, 9):
        bad(lib, put(i, None), NAMES[i], b"NULL")
    for i in (0, 1, 2):
        for off in (1, 2, 3):
            bad(lib, put(i, A + off), NAMES[i], b"misaligned")
    for i in (8, 9):
        for off in (1, 4, 6):
            bad(lib, put(i, A + off), NAMES[i], b"misaligned")


def test_bad_sizes_are_refused(lib):
    for i, name in ((3, b"M="), (4, b"B="), (5, b"H="), (6, b"W=")):
        for v in (0, -1, -2 ** 31):
            bad(lib, put(i, v), b"bad size", name + str(v).encode())
    bad(lib, put(2, None), b"masks == NULL", b"M must be 1")  # M = 3 without masks
    bad(lib, put(2, None, put(3, 2)), b"masks == NULL", b"M must be 1")
    for h, w in ((10, 38), (27, 10), (1, 1), (10, 10)):
        bad(lib, put(5, h, put(6, w)), b"want_ssim", f"H={h} W={w}".encode())
    for m, b_, h, w in ((65535, 2, 16, 16), (256, 256, 16, 16), (1, 1, 16 * 65535 + 1, 16), (4, 1, 16 * 65535, 16 * 8193), (1, 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        for want in (0, 1):
            bad(lib, put(7, want, [A, A, A, m, b_, h, w, 1, A, A, None]), b"overflows the grid", f"M={m} B={b_} H={h} W={w}".encode())


def test_python_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from deblur4dgs_amd import metrics as M

    p, t = torch.rand(1, 12, 13, 3), torch.rand(1, 12, 13, 3)
    with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback, as the losses
        M.masked_image_metrics(p, t)
    with pytest.raises(RuntimeError, match="ROCm"):
        M.mPSNR().update(p, t, torch.ones(1, 12, 13))
    with pytest.raises(RuntimeError, match="ROCm"):
        M.mSSIM()(p, t)
    with pytest.raises(RuntimeError, match="ROCm"):
        M.compute_psnr(p, t)
    with pytest.raises(RuntimeError, match="ROCm"):
        M.ValidationMetrics(True).update(p, t, torch.ones(1, 12, 13), torch.ones(1, 12, 13))


def test_the_reference_names_import_and_mlpips_says_why_it_does_not():
    from deblur4dgs_amd.metrics import PCK, mPSNR, mSSIM  # noqa: F401  (what replaces `from flow3d.metrics import ...`)

    with pytest.raises(ImportError, match="AlexNet"):
        from deblur4dgs_amd.metrics import mLPIPS  # noqa: F401
    pck = PCK()
    assert float(pck(torch.tensor([[0.0, 0.0], [3.0, 4.0], [1.0, 1.0]]), torch.zeros(3, 2), 2.0)) == pytest.approx(2 / 3)
    pck.update(torch.zeros(2, 2), torch.zeros(2, 2), 0.5)
    assert len(pck) == 2 and float(pck.compute()) == pytest.approx((2 / 3 + 1) / 2)
    pck.reset()
    assert len(pck) == 0
    assert len(mPSNR()) == 0 and len(mSSIM()) == 0
