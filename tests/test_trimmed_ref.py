"""The trimmed losses without a GPU: the fp64 restatement the GPU tests compare against (tests/trimmed_ref.py) is pinned to values
recorded from the reference's own functions (tests/golden/trimmed_losses.npz, written by tests/golden/gen_trimmed_losses.py), and
the new C entry points validate their arguments before any GPU call."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import trimmed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _cases():
    spec = importlib.util.spec_from_file_location("gen_trimmed_losses", os.path.join(GOLDEN, "gen_trimmed_losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.cases()


CASES = _cases()


def test_fixture_holds_the_cases_the_feature_is_specified_by():
    z = np.load(os.path.join(GOLDEN, "trimmed_losses.npz"))
    assert {k.split("/")[0] for k in z.files} == set(CASES)
    assert {"masked_normalized", "masked_mean", "no_mask", "masked_quantile_1", "gradient_ragged_bool"} <= set(CASES)
    for name, (_, inputs, _) in CASES.items():  # the inputs in the file are the generator's (same seed): nothing drifted
        for k, v in inputs.items():
            assert np.array_equal(z[f"{name}/{k}"], v.numpy()), (name, k)
    assert os.path.getsize(os.path.join(GOLDEN, "trimmed_losses.npz")) < 32 * 1024


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference_fixture(name):
    z = np.load(os.path.join(GOLDEN, "trimmed_losses.npz"))
    fn, inputs, kw = CASES[name]
    t = {k: torch.from_numpy(z[f"{name}/{k}"]) for k in inputs}
    pred = t.pop("pred").clone().requires_grad_()
    loss = getattr(R, fn)(pred, **t, **kw)
    (1.7 * loss).backward()
    want, want_grad = z[f"{name}/loss"], z[f"{name}/pred_grad"]
    assert math.isfinite(float(want)) and np.abs(want_grad).max() > 0
    np.testing.assert_allclose(float(loss.detach()), float(want), rtol=0, atol=1e-12)
    np.testing.assert_allclose(pred.grad.numpy(), want_grad, rtol=0, atol=1e-12)


def test_restatement_corner_cases():
    v = torch.tensor([[3.0], [1.0], [2.0], [2.0], [5.0]], dtype=torch.float64)
    z = torch.zeros_like(v)
    # r = 0.5 * 4 = 2: t = 2, the tie group at 2 goes whole, only 1 is kept
    assert float(R.trimmed_l1_loss(v, z, 0.5)) == 1.0
    assert float(R.masked_l1_loss(v, z, torch.ones(5), True, 0.5)) == pytest.approx(1.0, abs=1e-7)
    assert float(R.masked_l1_loss(v, z, torch.zeros(5), True, 0.5)) == 0.0  # empty weights: 0 / 1e-8
    assert math.isnan(float(R.trimmed_l1_loss(torch.ones(4, 1, dtype=torch.float64), torch.zeros(4, 1, dtype=torch.float64), 0.5)))
    assert float(R.masked_l1_loss(v, z, torch.ones(5), False, 1.0)) == pytest.approx(13.0 / 5)  # quantile >= 1 keeps everything
    board = (torch.arange(5)[:, None] + torch.arange(4)[None]) % 2 == 0
    x = torch.rand(1, 5, 4, dtype=torch.float64)
    assert math.isnan(float(R.compute_gradient_loss(x, x * 0.5, board[None], 0.9)))  # no valid pair (the reference raises)
    with pytest.raises(NotImplementedError):
        R.compute_gradient_loss(torch.rand(1, 4, 4, 3), torch.rand(1, 4, 4, 3), torch.ones(1, 4, 4), 0.9)
    assert R.rank(0.75, 9, torch.float32) == (6, 6, 0.0) and R.rank(0.5, 4) == (1, 2, 0.5)
    assert R.neighbours_apart(torch.tensor([0.0, 1.0, 2.0, 3.0]), 0.5) and not R.neighbours_apart(torch.tensor([0.0, 1.0, 1.0, 3.0]), 0.5)


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


NEW = ("d4gs_trimmed_scratch_words", "d4gs_masked_l1_fwd", "d4gs_masked_l1_bwd", "d4gs_trimmed_l1_fwd", "d4gs_trimmed_l1_bwd",
       "d4gs_gradient_loss_fwd", "d4gs_gradient_loss_bwd")


def test_new_symbols_are_declared_bound_and_exported_and_the_version_is_305(lib):
    from deblur4dgs_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    assert lib.d4gs_version() == 305 and "#define D4GS_VERSION 305" in header
    for name in NEW:
        assert hasattr(lib, name) and name in L.EXPORTS and f"{name}(" in header, name
        assert getattr(lib, name).argtypes is not None, name


def test_scratch_query(lib):
    w = lib.d4gs_trimmed_scratch_words
    assert [w(n, t) for n, t in ((-1, 1), (2 ** 31, 1), (10, 0), (10, 3))] == [0, 0, 0, 0]
    sizes = [w(n, 1) for n in (0, 1, 2, 2048, 2049, 10 ** 6, 2 ** 31 - 1)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and 0 < sizes[0] < sizes[3] < sizes[-1]
    assert w(2 ** 31 - 1, 1) >= 2 ** 31 - 1 and w(1000, 2) >= 2000 + 2 * (w(1000, 1) - 1000)
    assert all(w(n, t) % 2 == 0 for n in (0, 1, 7, 4097) for t in (1, 2))  # whole doubles at the end


def test_bad_arguments_return_einval_before_any_gpu_call(lib):
    """Fake addresses: nothing is dereferenced or launched before the validation (this runs without a GPU)."""
    fake, n = 0x10000, 100
    words = lib.d4gs_trimmed_scratch_words(n, 1)
    nan, inf = float("nan"), float("inf")

    def bad(fn, args, word):
        assert getattr(lib, fn)(*args) == -1, (fn, args)  # D4GS_EINVAL
        assert fn.encode() in lib.d4gs_last_error() and word in lib.d4gs_last_error(), lib.d4gs_last_error()

    ok = [fake, fake, fake, n, 3, 1, 0.98, fake, words, fake, None]  # d4gs_masked_l1_fwd
    for i in (0, 1, 2, 7, 9):
        bad("d4gs_masked_l1_fwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    for i, v, word in ((3, -1, b"size"), (3, 2 ** 31, b"size"), (4, 0, b"size"), (6, 0.0, b"quantile"), (6, -0.5, b"quantile"),
                       (6, nan, b"quantile"), (6, inf, b"quantile"), (8, words - 1, b"scratch"), (8, -5, b"scratch"), (7, fake + 4, b"scratch")):
        bad("d4gs_masked_l1_fwd", ok[:i] + [v] + ok[i + 1:], word)
    ok = [fake, fake, n, 3, 0.9, fake, words, fake, None]  # d4gs_trimmed_l1_fwd
    for i in (0, 1, 5, 7):
        bad("d4gs_trimmed_l1_fwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    for i, v, word in ((2, -1, b"size"), (3, -2, b"size"), (4, 0.0, b"quantile"), (4, nan, b"quantile"), (4, -inf, b"quantile"),
                       (6, words - 1, b"scratch")):
        bad("d4gs_trimmed_l1_fwd", ok[:i] + [v] + ok[i + 1:], word)
    ok = [fake, fake, fake, fake, fake, fake, n, 3, 0.98, fake, None]  # d4gs_masked_l1_bwd
    for i in (0, 1, 2, 3, 4, 5, 9):
        bad("d4gs_masked_l1_bwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    for i, v, word in ((6, -1, b"size"), (7, 0, b"size"), (8, nan, b"quantile"), (8, 0.0, b"quantile")):
        bad("d4gs_masked_l1_bwd", ok[:i] + [v] + ok[i + 1:], word)
    ok = [fake, fake, fake, fake, fake, n, 3, fake, None]  # d4gs_trimmed_l1_bwd
    for i in (0, 1, 2, 3, 4, 7):
        bad("d4gs_trimmed_l1_bwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    bad("d4gs_trimmed_l1_bwd", ok[:5] + [-1] + ok[6:], b"size")
    B, H, W = 2, 5, 10
    words2 = lib.d4gs_trimmed_scratch_words(B * H * W, 2)
    ok = [fake, fake, fake, B, H, W, 0.95, fake, words2, fake, None]  # d4gs_gradient_loss_fwd
    for i in (0, 1, 2, 7, 9):
        bad("d4gs_gradient_loss_fwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    for i, v, word in ((3, -1, b"size"), (4, -1, b"size"), (5, -3, b"size"), (3, 2 ** 31 - 1, b"size"), (6, 0.0, b"quantile"),
                       (6, nan, b"quantile"), (6, inf, b"quantile"), (8, words2 - 1, b"scratch"), (8, words, b"scratch")):
        bad("d4gs_gradient_loss_fwd", ok[:i] + [v] + ok[i + 1:], word)
    ok = [fake, fake, fake, fake, fake, fake, B, H, W, fake, None]  # d4gs_gradient_loss_bwd
    for i in (0, 1, 2, 3, 4, 5, 9):
        bad("d4gs_gradient_loss_bwd", ok[:i] + [None] + ok[i + 1:], b"NULL")
    bad("d4gs_gradient_loss_bwd", ok[:7] + [-1] + ok[8:], b"size")


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from deblur4dgs_amd.losses import compute_gradient_loss, masked_l1_loss, trimmed_l1_loss

    a, b = torch.rand(4, 5, 1), torch.rand(4, 5, 1)
    for call in (lambda: masked_l1_loss(a, b, torch.ones(4, 5), quantile=0.9), lambda: masked_l1_loss(a, b), lambda: trimmed_l1_loss(a, b),
                 lambda: compute_gradient_loss(a[None], b[None], torch.ones(1, 4, 5))):
        with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback, as photometric_loss
            call()
    for q in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            masked_l1_loss(a, b, torch.ones(4, 5), quantile=q)
    with pytest.raises(ValueError):
        trimmed_l1_loss(a, b, 1.5)  # torch.quantile refuses q > 1
    with pytest.raises(ValueError):
        compute_gradient_loss(a[None], b[None], torch.ones(1, 4, 5), quantile=2.0)
