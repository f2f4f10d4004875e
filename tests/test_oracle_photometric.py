"""Oracle self-checks for the photometric term.  pytorch-msssim is absent (parity unpinned, see
oracle/photometric.py); what can be checked here: closed forms, and an independent numpy/scipy evaluation of the same
published definition."""
import numpy as np
import pytest
import torch
from scipy.ndimage import correlate1d

from oracle import photometric as ph
from tests import photometric_cases as pc


def _ssim_numpy(X, Y):
    w = ph.gaussian_window().numpy()

    def filt(a):  # [B,C,H,W] valid separable correlation
        a = correlate1d(a, w, axis=2, mode="constant")[:, :, 5:-5]
        return correlate1d(a, w, axis=3, mode="constant")[:, :, :, 5:-5]

    mu1, mu2 = filt(X), filt(Y)
    s1, s2, s12 = filt(X * X) - mu1 ** 2, filt(Y * Y) - mu2 ** 2, filt(X * Y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = (2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1) * (2 * s12 + C2) / (s1 + s2 + C2)
    return m.reshape(*m.shape[:2], -1).mean(-1).mean()


def test_ssim_closed_forms_and_independent_numpy():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 37, 52, generator=g, dtype=torch.float64)
    y = (x + 0.2 * torch.randn(2, 3, 37, 52, generator=g, dtype=torch.float64)).clamp(0, 1)
    assert abs(float(ph.ssim(x, x)) - 1.0) < 1e-12
    np.testing.assert_allclose(float(ph.ssim(x, y)), _ssim_numpy(x.numpy(), y.numpy()), rtol=1e-10)
    assert abs(float(ph.ssim(x, y)) - float(ph.ssim(y, x))) < 1e-14
    c1, c2 = 0.3, 0.7  # constant images: variances vanish, only the luminance term is left
    want = (2 * c1 * c2 + 1e-4) / (c1 * c1 + c2 * c2 + 1e-4)
    got = float(ph.ssim(torch.full((1, 3, 20, 20), c1, dtype=torch.float64), torch.full((1, 3, 20, 20), c2, dtype=torch.float64)))
    assert abs(got - want) < 1e-12
    assert abs(float(ph.gaussian_window().sum()) - 1.0) < 1e-15


def test_photometric_loss_composition():
    g = torch.Generator().manual_seed(1)
    p, q = torch.rand(1, 30, 33, 3, generator=g, dtype=torch.float64), torch.rand(1, 30, 33, 3, generator=g, dtype=torch.float64)
    m = (torch.rand(1, 30, 33, 1, generator=g) > 0.4).double()
    loss, l1, s = ph.photometric_loss(p, q, m)
    np.testing.assert_allclose(float(l1), float(((p - q) * m).abs().mean()), rtol=1e-14)
    np.testing.assert_allclose(float(loss), 0.8 * float(l1) + 0.2 * (1 - float(s)), rtol=1e-14)


def _misses(got, ref, gmax_ref=None):
    """Does `got` miss the tolerances of tests/test_gpu_photometric.py (SSIM rtol 2e-6 + atol 2e-7, SSIM gradient atol 1e-5 of the
    reference gradient's maximum) against `ref`?  -> (value misses, gradient misses, achieved value error, achieved gradient error / bound)"""
    verr = abs(got["ssim"] - ref["ssim"])
    bound = 1e-5 * (float(ref["g_ssim"].abs().max()) if gmax_ref is None else gmax_ref)
    gerr = float((got["g_ssim"] - ref["g_ssim"]).abs().max())
    return verr > 2e-6 * abs(ref["ssim"]) + 2e-7, gerr > bound, verr, gerr / bound


@pytest.mark.parametrize("masked", [False, True])
def test_gpu_cases_discriminate_the_raw_moment_formula(masked):
    """The GPU test's inputs are worth having only if a kernel with the textbook cancellation fails on them.  The oracle IS the
    textbook formula (sigma^2 = E[x^2] - mu^2 from raw moments), so running it in float32 against itself in float64 stands in for
    such a kernel: it must miss the GPU test's tolerances on every flat / bright / converged case, and meet them on the noise case
    (which is why the older suite could not notice).  The thing measured is the oracle, never the library."""
    neighbour = float(pc.reference("flat_noise_both", masked)["g_ssim"].abs().max())
    mask = pc.soft_mask() if masked else None
    for name in (pc.NOISE,) + pc.FLAT:
        pred, gt = pc.content(name)
        ref, f32 = pc.reference(name, masked), pc.evaluate(pred, gt, mask, torch.float32)
        # pred == gt: the reference gradient is ~0, the bound is 1e-5 of the neighbouring case's maximum, as on the GPU
        v_bad, g_bad, verr, gratio = _misses(f32, ref, neighbour if name == "identical" else None)
        print(f"{name} masked={masked}: fp32 raw-moment SSIM err {verr:.2e}, gradient err / bound {gratio:.2e}")
        if name == pc.NOISE:
            assert not v_bad and not g_bad, (name, verr, gratio)
        else:
            assert v_bad or g_bad, (name, verr, gratio)
            assert g_bad, (name, gratio)  # the gradient under (w_l1, w_ssim) = (0, 1) is the sharper check on every one of them
