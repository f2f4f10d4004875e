"""tests/image_terms_ref.py against torch's own CPU implementation of the ops the reference's trainer calls: F.max_pool2d(., 9, 1, 4),
F.interpolate(scale_factor=1 / factor, mode="area") + F.l1_loss (autograd for the gradient) and F.mse_loss.  Double inputs; values and
gradients agree to 1e-12.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import image_terms_ref as R

SIZES = (4, 5, 7, 8, 9, 11, 16, 17)
UP = 1.7  # upstream factor of every backward


def case(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(B, H, W, C, generator=g, dtype=torch.float64)
    target = torch.rand(B, H, W, C, generator=g, dtype=torch.float64)
    mask = (torch.rand(B, H, W, generator=g) < 0.6).double()
    return pred, target, mask


def area(x, factor):  # channel-last in and out, the reference's wording
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=1.0 / factor, mode="area").permute(0, 2, 3, 1)


@pytest.mark.parametrize("H", SIZES)
def test_dilation_is_max_pool(H):
    for W in SIZES:
        g = torch.Generator().manual_seed(100 * H + W)
        for mask in ((torch.rand(2, H, W, generator=g) < 0.2).double(), torch.rand(2, H, W, generator=g, dtype=torch.float64) - 0.5,
                     -torch.ones(2, H, W, dtype=torch.float64)):
            for r in (0, 1, 4):
                want = F.max_pool2d(mask[:, None], 2 * r + 1, 1, r)[:, 0]
                assert np.array_equal(R.dilate(mask.numpy(), r), want.numpy()), (H, W, r)


def test_dilation_known_answers():
    m = np.zeros((1, 3, 5))
    m[0, 1, 2] = 0.5
    assert np.array_equal(R.dilate(m, 4), np.full((1, 3, 5), 0.5))
    assert np.array_equal(R.dilate(-np.ones((1, 3, 5)), 4), -np.ones((1, 3, 5)))  # the padding is -inf, not 0


@pytest.mark.parametrize("factor", (2, 4))
@pytest.mark.parametrize("H", SIZES)
def test_sharp_keep_is_area_interpolate_and_l1(H, factor):
    for W in SIZES:
        pred, target, mask = case(2, H, W, 3, 1000 * factor + 100 * H + W)
        p = pred.clone().requires_grad_()
        m_ = area(mask[..., None], factor)
        reduced = area(target, factor)
        assert tuple(reduced.shape) == (2, H // factor, W // factor, 3)
        np.testing.assert_allclose(R.area_mean(target.numpy(), factor), reduced.numpy(), rtol=0, atol=1e-12)
        for tgt, t_down in ((target, reduced * m_), (reduced, reduced * m_)):
            p.grad = None
            loss = F.l1_loss(area(p, factor) * m_, t_down.detach())
            (UP * loss).backward()
            got, grad = R.sharp_keep(pred.numpy(), tgt.numpy(), mask.numpy(), factor)
            assert abs(got - float(loss.detach())) <= 1e-12, (H, W, factor, got, float(loss.detach()))
            np.testing.assert_allclose(UP * grad, p.grad.numpy(), rtol=0, atol=1e-12, err_msg=f"{H}x{W} factor {factor}")


def test_sharp_keep_sign_of_zero_is_zero():
    pred, target, mask = case(1, 8, 8, 3, 5)
    mask[:] = 1.0
    target[:, :, :4] = pred[:, :, :4]
    p = pred.clone().requires_grad_()
    F.l1_loss(area(p, 4) * area(mask[..., None], 4), area(target, 4) * area(mask[..., None], 4)).backward()
    _, grad = R.sharp_keep(pred.numpy(), target.numpy(), mask.numpy(), 4)
    assert np.all(grad[:, :, :4] == 0.0) and np.all(grad[:, :, 4:] != 0.0)
    assert np.array_equal(grad == 0.0, p.grad.numpy() == 0.0)


def test_windows_cover_every_pixel_once_or_twice():
    for L in range(4, 24):
        for factor in (1, 2, 4, 8):
            if L < factor:
                continue
            w = R.windows(L, factor)
            cover = np.zeros(L, int)
            for lo, hi in w:
                assert 0 <= lo < hi <= L and hi - lo <= 2 * factor - 1
                cover[lo:hi] += 1
            assert cover.min() >= 1 and cover.max() <= 2 and (L % factor or cover.max() == 1)


@pytest.mark.parametrize("n", (1, 255, 256, 257, 2 * 41 * 70))
def test_mse_is_mse_loss(n):
    g = torch.Generator().manual_seed(n)
    a = torch.rand(n, generator=g, dtype=torch.float64)
    for t in (None, (torch.rand(n, generator=g) < 0.6).double()):
        x = a.clone().requires_grad_()
        loss = F.mse_loss(x, torch.ones_like(x) if t is None else t)
        (UP * loss).backward()
        got, grad = R.mse(a.numpy(), None if t is None else t.numpy())
        assert abs(got - float(loss)) <= 1e-12
        np.testing.assert_allclose(UP * grad, x.grad.numpy(), rtol=0, atol=1e-12)
