"""SURVEY 8f-2 on the GPU: fused L1 + SSIM loss (csrc/photometric.hip through the C ABI) against the fp64 oracle.
Tolerances: value 2e-6 relative (f32 sums of ~1e5 terms, partials added in double; atol 2e-7 on SSIM, and on a loss whose expected
value is 0), gradient 1e-5 of its max norm, per element.  They hold on uniform noise (the first test, the only input this file
had at first) AND on flat, bright and converged images (tests/photometric_cases.py), where SSIM's variances are ~1e-6 beside
means ~1 and a kernel that forms them from raw fp32 moments is off by 1e-4 in the value and by 10-4000 x the gradient bound
(tests/test_oracle_photometric.py shows that on the CPU).  Achieved on an MI355X over every content case, mask and weighting
below: SSIM within 2.9e-8 and the loss within 1.7e-7 relative (even where it is 2e-4), the gradient within 0.57 of its bound on
the worst case (soft-masked smooth bright, at the edge of the zeroed mask tile) and within 0.2 of it elsewhere; with pred == gt,
SSIM = 1, loss = 0 and a gradient of 1e-8 of the bound.  The raw-moment kernel this file used to guard missed them by up to 2.0e-4
in SSIM and 5600 x the gradient bound.
Every check prints achieved / bound before it asserts (pytest -s)."""
import numpy as np
import pytest
import torch

from deblur4dgs_amd.losses import photometric_loss
from oracle import photometric as ph
from tests import photometric_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("B,H,W,masked", [(1, 288, 512, False), (1, 288, 512, True), (2, 45, 77, True), (3, 16, 11, False),
                                          (1, 11, 11, False), (1, 100, 33, True)])
def test_value_and_gradient_match_oracle(B, H, W, masked):
    g = torch.Generator().manual_seed(H * 1000 + W)
    gt = torch.rand(B, H, W, 3, generator=g)
    pred = (gt + 0.15 * torch.randn(B, H, W, 3, generator=g)).clamp(0, 1)
    mask = (torch.rand(B, H, W, 1, generator=g) > 0.3).float() if masked else None
    p64 = pred.double().requires_grad_()
    lo, l1o, so = ph.photometric_loss(p64, gt.double(), None if mask is None else mask.double())
    (3.0 * lo).backward()
    pg = pred.to(DEV).requires_grad_()
    loss, l1, s = photometric_loss(pg, gt.to(DEV), None if mask is None else mask.to(DEV), return_terms=True)
    (3.0 * loss).backward()
    np.testing.assert_allclose(float(loss), float(lo), rtol=2e-6)
    np.testing.assert_allclose(float(l1), float(l1o), rtol=2e-6)
    np.testing.assert_allclose(float(s), float(so), rtol=2e-6, atol=2e-7)
    ref = p64.grad.numpy()
    np.testing.assert_allclose(pg.grad.cpu().numpy(), ref, rtol=0, atol=1e-5 * np.abs(ref).max())


def test_deterministic_and_rejects_bad_shapes():
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(1, 64, 64, 3, generator=g).to(DEV), torch.rand(1, 64, 64, 3, generator=g).to(DEV)
    x = a.clone().requires_grad_()
    l0 = photometric_loss(x, b)
    l0.backward()
    y = a.clone().requires_grad_()
    l1 = photometric_loss(y, b)
    l1.backward()
    assert torch.equal(l0, l1) and torch.equal(x.grad, y.grad)
    with pytest.raises(RuntimeError):
        photometric_loss(torch.rand(1, 8, 64, 3, device=DEV), torch.rand(1, 8, 64, 3, device=DEV))  # H < 11
    with pytest.raises(RuntimeError):
        photometric_loss(torch.rand(1, 32, 32, 4, device=DEV), torch.rand(1, 32, 32, 4, device=DEV))  # C != 3
    with pytest.raises(RuntimeError):
        photometric_loss(torch.rand(1, 32, 32, 3), torch.rand(1, 32, 32, 3))  # CPU tensors: no fallback


def _gpu(pred, gt, mask, w_l1, w_ssim, v):
    """One forward + backward on the device -> (loss, l1, ssim) as floats and the gradient as a CPU fp64 tensor."""
    pg = pred.detach().to(DEV).requires_grad_()
    loss, l1, s = photometric_loss(pg, gt.to(DEV), None if mask is None else mask.to(DEV), w_l1=w_l1, w_ssim=w_ssim,
                                   return_terms=True)
    (v * loss).backward()
    return float(loss), float(l1), float(s), pg.grad.cpu().double()


def _check(tag, got, ref, mask, w_l1, w_ssim, v, zero_loss=False, grad_scale=None):
    """The file's tolerances against an oracle result `ref` (tests.photometric_cases.evaluate).  `grad_scale`: the gradient
    maximum the 1e-5 is relative to, when it is not this case's own."""
    loss, l1, s, grad = got
    want_loss = w_l1 * ref["l1"] + w_ssim * (1.0 - ref["ssim"])
    want_grad = v * (w_l1 * ref["g_l1"] - w_ssim * ref["g_ssim"])
    bound = 1e-5 * (float(want_grad.abs().max()) if grad_scale is None else grad_scale)
    gerr = float((grad - want_grad).abs().max())
    print(f"{tag}: loss {loss:.9g} (want {want_loss:.9g}, rel {abs(loss - want_loss) / max(abs(want_loss), 1e-300):.1e}), "
          f"l1 rel {abs(l1 - ref['l1']) / max(ref['l1'], 1e-300):.1e}, ssim err {abs(s - ref['ssim']):.1e}, "
          f"gradient err / bound {gerr / max(bound, 1e-300):.2e}")
    np.testing.assert_allclose(loss, want_loss, rtol=2e-6, atol=2e-7 if zero_loss else 0.0)
    np.testing.assert_allclose(l1, ref["l1"], rtol=2e-6)
    np.testing.assert_allclose(s, ref["ssim"], rtol=2e-6, atol=2e-7)
    assert gerr <= bound, (tag, gerr, bound)
    if mask is not None:  # a masked-out pixel gets exactly nothing
        dead = (mask.reshape(grad.shape[:3]) == 0).unsqueeze(-1).expand_as(grad)
        assert dead.any() and (grad[dead] == 0).all()


# default weights with a cotangent of 3 (as the first test); SSIM alone and L1 alone with a negative cotangent that is not 1.
# (0, 1) is the sharp one: the gradient tolerance is then relative to the SSIM gradient, not to the L1 sign term beside it.
WEIGHTS = [(0.8, 0.2, 3.0), (0.0, 1.0, -2.5), (1.0, 0.0, -2.5)]


@pytest.mark.parametrize("w_l1,w_ssim,v", WEIGHTS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", pc.CONTENT)
def test_content_cases_match_oracle(name, masked, w_l1, w_ssim, v):
    """Flat, bright, converged, split and constant images (B = 2, different content per item), bare and under a soft alpha
    mask [B,H,W,1] that has fractional values and one exactly zero 16x16 tile."""
    pred, gt = pc.content(name)
    mask = pc.soft_mask() if masked else None
    ref = pc.reference(name, masked)
    got = _gpu(pred, gt, mask, w_l1, w_ssim, v)
    if name == "identical":
        # SSIM = 1 and loss = 0 within the atol; the L1 sign term is exactly 0 (sign(0) = 0); the whole gradient is within 1e-5
        # of the gradient maximum of the neighbouring case pred = gt + 1e-3 noise under the same weights
        nb = pc.reference("flat_noise_both", masked)
        scale = float((v * (w_l1 * nb["g_l1"] - w_ssim * nb["g_ssim"])).abs().max())
        _check(f"{name} masked={masked} w=({w_l1},{w_ssim})", got, ref, mask, w_l1, w_ssim, v, zero_loss=True, grad_scale=scale)
        assert got[1] == 0.0 and abs(got[2] - 1.0) <= 2e-7 and abs(got[0]) <= 2e-7
        if w_ssim == 0.0:
            assert (got[3] == 0).all()
        return
    _check(f"{name} masked={masked} w=({w_l1},{w_ssim})", got, ref, mask, w_l1, w_ssim, v)
    if name.startswith("const") and not masked:  # closed form: the variances vanish, the luminance term is left
        a, b = float(pred[0, 0, 0, 0]), float(gt[0, 0, 0, 0])  # the fp32-quantised levels
        np.testing.assert_allclose(got[2], (2 * a * b + 1e-4) / (a * a + b * b + 1e-4), rtol=2e-6, atol=2e-7)
    if name == "alt_rows" and w_ssim == 0.0:  # pred == gt on the even rows: the L1 gradient vanishes exactly there
        assert (got[3][:, 0::2] == 0).all() and (got[3][:, 1::2] != 0).any()


@pytest.mark.parametrize("H,W", [(11, 43), (43, 11), (26, 27), (27, 26), (17, 32), (33, 12), (12, 33)])
def test_tile_geometry(H, W):
    """The input tile is 16 and the output grid (H-10) x (W-10): its tile count changes at 26/27 and 42/43, and blocks can own
    input pixels but no output pixel.  Noise input, per-element gradients, bare and under a binary [B,H,W] mask."""
    g = torch.Generator().manual_seed(H * 100 + W)
    gt = torch.rand(2, H, W, 3, generator=g)
    pred = (gt + 0.15 * torch.randn(2, H, W, 3, generator=g)).clamp(0, 1)
    mask = (torch.rand(2, H, W, generator=g) > 0.3).float()
    mask[0, 0, 0] = 0.0
    for m in (None, mask):
        ref = pc.evaluate(pred, gt, None if m is None else m.unsqueeze(-1), torch.float64)
        for w_l1, w_ssim, v in WEIGHTS[:2]:
            _check(f"{H}x{W} masked={m is not None} w=({w_l1},{w_ssim})", _gpu(pred, gt, m, w_l1, w_ssim, v), ref, m, w_l1, w_ssim, v)


def test_mask_shapes_give_the_same_bits():
    pred, gt = pc.content("smooth_bright")
    m4 = pc.soft_mask()
    assert ((m4 > 0) & (m4 < 1)).any() and (m4[0, 16:32, 16:32] == 0).all()  # fractional, and a whole 16x16 tile of zeros
    a = _gpu(pred, gt, m4, 0.8, 0.2, 1.0)
    b = _gpu(pred, gt, m4[..., 0].contiguous(), 0.8, 0.2, 1.0)
    assert a[:3] == b[:3] and torch.equal(a[3], b[3])


def test_five_channel_leaf_and_two_live_losses():
    """The trainer passes `pred` as the [..., 0:3] slice of a 5-channel channel-last render (colour, depth, alpha) that requires
    grad, and holds several losses before it runs any backward: the saved maps are per call."""
    cases = [("smooth_bright", 0.8, 0.2, 3.0), ("flat_gt", 0.0, 1.0, -2.5)]
    leaves, losses = [], []
    for name, w_l1, w_ssim, v in cases:
        pred, gt = pc.content(name)
        g = torch.Generator().manual_seed(5)
        leaf = torch.cat([pred, torch.rand(pc.B, pc.H, pc.W, 2, generator=g)], -1).to(DEV).requires_grad_()
        losses.append(v * photometric_loss(leaf[..., 0:3], gt.to(DEV), w_l1=w_l1, w_ssim=w_ssim))
        leaves.append(leaf)
    for loss in losses:  # both forwards are done before the first backward
        loss.backward()
    for (name, w_l1, w_ssim, v), leaf, loss in zip(cases, leaves, losses):
        ref = pc.reference(name, False)
        grad = leaf.grad.cpu().double()
        assert grad.shape[-1] == 5 and (grad[..., 3:] == 0).all()
        got = (float(loss) / v, ref["l1"], ref["ssim"], grad[..., 0:3])  # the terms are checked elsewhere; here loss and gradient
        _check(f"5-channel leaf {name}", got, ref, None, w_l1, w_ssim, v)


def test_deterministic_on_smooth_bright():
    pred, gt = pc.content("smooth_bright")
    for mask in (None, pc.soft_mask()):
        a, b = _gpu(pred, gt, mask, 0.8, 0.2, 1.0), _gpu(pred, gt, mask, 0.8, 0.2, 1.0)
        assert a[:3] == b[:3] and torch.equal(a[3], b[3])
