"""d4gs_track_losses_fwd / d4gs_track_losses_bwd (csrc/trimmed.hip) are declared, bound and exported, and validate their arguments
on the host before any HIP call: fake addresses - nothing is dereferenced; no GPU needed."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_track_losses_fwd", "d4gs_track_losses_bwd")
A = 0x10000  # a fake, aligned device address


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def test_new_symbols_are_declared_bound_and_exported_and_the_version_is_305(lib):
    from deblur4dgs_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    assert lib.d4gs_version() == 305 and "#define D4GS_VERSION 305" in header and L.VERSION == 305
    for name in NEW:
        assert hasattr(lib, name) and name in L.EXPORTS and f"{name}(" in header, name
        assert getattr(lib, name).argtypes is not None, name


def bad(lib, fn, args, word):
    assert getattr(lib, fn)(*args) == -1, (fn, args)  # D4GS_EINVAL
    assert fn.encode() in lib.d4gs_last_error() and word in lib.d4gs_last_error(), lib.d4gs_last_error()


def test_forward_rejects_bad_arguments_before_any_gpu_call(lib):
    n = 100
    words = lib.d4gs_trimmed_scratch_words(n, 2)
    assert words > lib.d4gs_trimmed_scratch_words(n, 1)
    #     tracks pix rows vis w t2d td Ks | n_pixels N n_rows n_elements quantile | scratch words out stream
    ok = [A, A, A, A, A, A, A, A, 192, 4, 4, n, 0.98, A, words, A, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 13, 15):
        bad(lib, "d4gs_track_losses_fwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    nan, inf = float("nan"), float("inf")
    for i, v, word in ((9, 0, b"size"), (9, -1, b"size"), (11, 0, b"size"), (11, -5, b"size"), (11, 2 ** 31, b"size"), (8, 0, b"size"),
                       (8, 2 ** 31, b"size"), (10, 0, b"size"), (10, 6, b"size"), (12, 0.0, b"quantile"), (12, nan, b"quantile"),
                       (12, inf, b"quantile"), (14, words - 1, b"scratch"), (14, lib.d4gs_trimmed_scratch_words(n, 1), b"scratch"),
                       (14, -1, b"scratch"), (13, A + 4, b"scratch")):
        bad(lib, "d4gs_track_losses_fwd", ok[:i] + [v] + ok[i + 1:], word)


def test_backward_rejects_bad_arguments_before_any_gpu_call(lib):
    #     tracks pix rows vis w t2d td Ks values out v_losses | n_pixels N n_rows n_elements quantile | v_tracks stream
    ok = [A] * 11 + [192, 4, 8, 100, 0.98, A, None]
    for i in list(range(11)) + [16]:
        bad(lib, "d4gs_track_losses_bwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    for i, v, word in ((12, 0, b"size"), (14, 0, b"size"), (14, -1, b"size"), (11, -1, b"size"), (13, 7, b"size"),
                       (15, float("nan"), b"quantile"), (15, -0.5, b"quantile")):
        bad(lib, "d4gs_track_losses_bwd", ok[:i] + [v] + ok[i + 1:], word)


def test_python_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from deblur4dgs_amd.losses import track_losses

    N, P = 2, 5
    args = [torch.rand(1, 6, 7, N, 3), torch.rand(P, 2), torch.rand(N, 3, 3), torch.rand(N, P, 2), torch.ones(N, P, dtype=torch.bool),
            torch.rand(N * P), torch.rand(N, P)]
    with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback, as the other losses
        track_losses(*args)
    with pytest.raises(ValueError):
        track_losses(torch.rand(1, 6, 7, N * 3), *args[1:])
    with pytest.raises(ValueError):
        track_losses(*args, quantile=0.0)
