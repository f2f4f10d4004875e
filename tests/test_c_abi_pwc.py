"""The entry points of csrc/correlation.hip and csrc/warp.hip validate their arguments on the host, before any HIP call: NULL
pointers and bad dimensions are D4GS_EINVAL with a message.  Fake addresses - nothing is dereferenced; no GPU needed."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib, build

    return _lib.bind(C.CDLL(build.build()))


A = 0x10000  # a fake, aligned device address
EINVAL = -1


def rejected(lib, rc, word):
    assert rc == EINVAL
    assert word in lib.d4gs_last_error(), lib.d4gs_last_error()


def test_correlation_rejects_null_and_bad_dimensions(lib):
    for args in ((None, A, 1, 3, 4, 5, 1.0, A), (A, None, 1, 3, 4, 5, 1.0, A), (A, A, 1, 3, 4, 5, 1.0, None)):
        rejected(lib, lib.d4gs_correlation_fwd(*args, None), b"NULL")
    for dims in ((0, 3, 4, 5), (1, 0, 4, 5), (1, 3, 0, 5), (1, 3, 4, -1), (70000, 3, 4, 5)):
        rejected(lib, lib.d4gs_correlation_fwd(A, A, *dims, 0.1, A, None), b"size")
    for args in ((None, A, A, A), (A, None, A, A), (A, A, A, None)):
        rejected(lib, lib.d4gs_correlation_bwd(*args, 1, 3, 4, 5, 0.1, A, A, None), b"NULL")
    rejected(lib, lib.d4gs_correlation_bwd(A, A, None, A, 1, 3, 4, 5, 0.1, A, A, None), b"saved output")  # out is optional at slope 1 only
    rejected(lib, lib.d4gs_correlation_bwd(A, A, A, A, 1, 3, 0, 5, 0.1, A, A, None), b"size")


def test_backwarp_rejects_null_bad_dimensions_and_single_rows(lib):
    for args in ((None, A, 1, 3, 4, 5, A, A), (A, None, 1, 3, 4, 5, A, A), (A, A, 1, 3, 4, 5, None, A), (A, A, 1, 3, 4, 5, A, None)):
        rejected(lib, lib.d4gs_backwarp_fwd(*args, None), b"NULL")
    for dims in ((0, 3, 4, 5), (1, 0, 4, 5), (1, -2, 4, 5)):
        rejected(lib, lib.d4gs_backwarp_fwd(A, A, *dims, A, A, None), b"size")
    for dims in ((1, 3, 1, 5), (1, 3, 4, 1), (1, 3, 0, 5)):  # W / (W - 1)
        rejected(lib, lib.d4gs_backwarp_fwd(A, A, *dims, A, A, None), b">= 2")
        rejected(lib, lib.d4gs_backwarp_bwd(A, A, *dims, A, None), b">= 2")
    for args in ((None, A, 1, 3, 4, 5, A), (A, None, 1, 3, 4, 5, A), (A, A, 1, 3, 4, 5, None)):
        rejected(lib, lib.d4gs_backwarp_bwd(*args, None), b"NULL")


def test_aligned_l1_rejects_null_bad_dimensions_and_misaligned_partials(lib):
    assert lib.d4gs_aligned_l1_blocks(0, 5) == 0 and lib.d4gs_aligned_l1_blocks(4, -1) == 0
    assert lib.d4gs_aligned_l1_blocks(2, 2) == 1 and lib.d4gs_aligned_l1_blocks(16, 17) == 2
    assert lib.d4gs_aligned_l1_blocks(288, 512) == lib.d4gs_aligned_l1_blocks(4096, 4096)  # capped
    ok = [A, A, A, A, 2, 4, 5, A, A]
    for i in (0, 1, 2, 7, 8):  # the mask (3) is optional
        bad = list(ok)
        bad[i] = None
        rejected(lib, lib.d4gs_aligned_l1_fwd(*bad, None), b"NULL")
    rejected(lib, lib.d4gs_aligned_l1_fwd(A, A, A, None, 2, 4, 5, A + 4, A, None), b"8-byte")
    rejected(lib, lib.d4gs_aligned_l1_fwd(A, A, A, None, 0, 4, 5, A, A, None), b"size")
    rejected(lib, lib.d4gs_aligned_l1_fwd(A, A, A, None, 2, 1, 5, A, A, None), b">= 2")
    ok = [A, A, A, A, A, 2, 4, 5, A, A]
    for i in (0, 1, 2, 4, 8):  # the mask (3) and v_target (9) are optional
        bad = list(ok)
        bad[i] = None
        rejected(lib, lib.d4gs_aligned_l1_bwd(*bad, None), b"NULL")
    rejected(lib, lib.d4gs_aligned_l1_bwd(A, A, A, None, A, -1, 4, 5, A, None, None), b"size")
    rejected(lib, lib.d4gs_aligned_l1_bwd(A, A, A, None, A, 2, 4, 1, A, None, None), b">= 2")
