"""The flow-aligned exposure consistency loss on the GPU (csrc/correlation.hip, csrc/warp.hip through deblur4dgs_amd.pwcnet) against
the fp64 restatement tests/pwc_ref.py, which tests/test_pwc_ref.py pins to the reference, and against the flows recorded from the
reference's own network (tests/golden/pwc.npz).

Inputs are quantised to fp32 first and the restatement gets those same values in fp64, so the two sides differ in arithmetic only.
Cost volume: per element C 2^-23 mean_c(|a| |b|) - the recursive-summation bound for any order, with or without FMA - computed in
fp64 from the inputs; backward 81 2^-23 mean_k(|v| |x|) / C likewise.  Warp and aligned L1: the photometric test's tolerances (value
rtol 2e-6, gradients 1e-5 of their maximum); no mask flip is allowed for - every case first asserts, in fp64, that no sample's
coverage lies within 1e-3 of the 0.999 threshold and that pred != target wherever the mask is 1.

Sizes: the cost volume and the warp at 2x2, 5x8, 7x13 and 20x33 (SPATIAL).  Past the launch caps, where the grid stops growing and
every lane strides: the aligned L1 at 129 x 255 (32 895 px per pair against 128 blocks x 256 lanes: 127 lanes take a second pixel,
and the partials lie 128 per pair), the backward warp at 3 x 593 x 590 (1 049 610 px against 4 096 blocks x 256: the last 1 034 px,
all in batch 2, come in a second turn whose batch index is taken from the strided pixel index; its gradient of 2 planes per image
is zeroed by a strided k_zero_f32)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from deblur4dgs_amd import _lib as L
from deblur4dgs_amd import pwcnet as P
from tests import pwc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
EPS = 2.0 ** -23
UP = 1.7
SPATIAL = [(2, 2), (5, 8), (7, 13), (20, 33)]  # below the 9x9 window; the real level-6 shape; odd; across the 32x8 tile on both axes


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "pwc.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind == "f" else z[k]) for k in z.files}


def pair(C, H, W, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)


# ---- cost volume ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SPATIAL)
@pytest.mark.parametrize("C", [1, 3, 32, 196])
def test_correlation_forward_matches_restatement(C, H, W):
    first, second = pair(C, H, W, 1000 * C + 10 * H + W)
    tol = EPS * C * R.correlation(first.double().abs(), second.double().abs())  # C 2^-23 mean_c(|a| |b|), per element
    for slope in (0.1, 1.0):
        got = P.correlation(first.to(DEV), second.to(DEV), slope).cpu().double()
        want = R.correlation(first.double(), second.double(), slope)
        assert got.shape == (2, 81, H, W)
        err = (got - want).abs()
        print(f"C={C} {H}x{W} slope {slope}: max err {float(err.max()):.3e}, max err / bound {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= tol).all()), (C, H, W, slope, float((err - tol).max()))


def test_correlation_single_pixel_known_answer():
    """Everything zero except one pixel of each input, on a 20x33 image (more than one tile): the one non-zero output sits at the
    pixel of `first`, in the channel of the offset (dy = -2, dx = +3 -> (dy + 4) 9 + dx + 4), and is the mean over the channels;
    an offset beyond the window, or past the border (zero padding), gives nothing."""
    first, second = torch.zeros(2, 3, 20, 33), torch.zeros(2, 3, 20, 33)
    first[0, :, 9, 30] = torch.tensor([2.0, 3.0, 0.5])
    second[0, :, 7, 32] = torch.tensor([5.0, -7.0, 4.0])  # dy = -2, dx = +2 (the window also reaches x = 33, 34: outside)
    first[1, :, 0, 0] = 1.0
    second[1, :, 5, 0] = 1.0  # dy = +5: beyond the window
    out = P.correlation(first.to(DEV), second.to(DEV)).cpu()
    k = (-2 + 4) * 9 + (2 + 4)
    assert float(out[0, k, 9, 30]) == (10.0 - 21.0 + 2.0) / 3 and int((out != 0).sum()) == 1
    leaky = P.correlation(first.to(DEV), second.to(DEV), 0.1).cpu()
    assert float(leaky[0, k, 9, 30]) == pytest.approx(-0.3, rel=3e-7) and int((leaky != 0).sum()) == 1


def test_correlation_two_runs_are_bitwise_equal():
    first, second = pair(32, 20, 33, 77)
    f, s = first.to(DEV).requires_grad_(), second.to(DEV).requires_grad_()
    runs = []
    for _ in range(2):
        out = P.correlation(f, s, 0.1)
        runs.append((out.detach().clone(),) + torch.autograd.grad(out.square().sum(), [f, s]))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("H,W", SPATIAL)
@pytest.mark.parametrize("C", [3, 32])
def test_correlation_backward_matches_autograd_of_restatement(C, H, W):
    first, second = pair(C, H, W, 2000 * C + 10 * H + W)
    v = torch.randn(2, 81, H, W, generator=torch.Generator().manual_seed(H * W + C))
    f64, s64 = first.double().requires_grad_(), second.double().requires_grad_()
    # 81 2^-23 mean_k(|v| |x|) / C per element: the gradient of sum(|v| volume(|.|, |.|)) is (1 / C) sum_k |v_k| |x_k|
    fa, sa = first.double().abs().requires_grad_(), second.double().abs().requires_grad_()
    bound_first, bound_second = [EPS * t for t in torch.autograd.grad((v.double().abs() * R.correlation(fa, sa)).sum(), [fa, sa])]
    for slope in (0.1, 1.0):
        vol = R.correlation(f64, s64, slope)
        # the slope is chosen by the sign of the volume: no element may be so close to zero that fp32 could put it on the other side
        raw = R.correlation(first.double(), second.double())
        margin = EPS * C * R.correlation(first.double().abs(), second.double().abs())
        assert bool(((raw.abs() > margin) | (raw == 0)).all())
        want_first, want_second = torch.autograd.grad((vol * v.double()).sum(), [f64, s64])
        f, s = first.to(DEV).requires_grad_(), second.to(DEV).requires_grad_()
        got_first, got_second = torch.autograd.grad((P.correlation(f, s, slope) * v.to(DEV)).sum(), [f, s])
        for name, got, want, bound in (("v_first", got_first, want_first, bound_first), ("v_second", got_second, want_second, bound_second)):
            err = (got.cpu().double() - want).abs()
            print(f"C={C} {H}x{W} slope {slope} {name}: max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= bound).all()), (name, C, H, W, slope)
        # one side only: the other pointer is NULL
        only_first, = torch.autograd.grad((P.correlation(f, second.to(DEV), slope) * v.to(DEV)).sum(), [f])
        only_second, = torch.autograd.grad((P.correlation(first.to(DEV), s, slope) * v.to(DEV)).sum(), [s])
        assert torch.equal(only_first, got_first) and torch.equal(only_second, got_second)


# ---- warp and aligned L1 -------------------------------------------------------------------------------------------------------
def warp_case(name, fx):
    """-> pred, target, flow, mask (fp32-exact values)"""
    if name == "fixture":
        return [fx[k].float() for k in ("a/pred", "a/target", "a/flow", "a/mask")]
    g = torch.Generator().manual_seed(332)
    P_, H, W = 3, 20, 33
    pred, target = torch.rand(P_, 3, H, W, generator=g), torch.rand(P_, 3, H, W, generator=g)
    flow = 4.0 * (torch.rand(P_, 2, H, W, generator=g) - 0.5)
    flow[0, 0, :, :3] -= 5.0
    flow[1, 1, -3:] += 5.0
    flow[2, :, 5:9, 7:12] = torch.tensor([1.0, -2.0]).view(2, 1, 1)  # whole-pixel displacements
    return pred, target, flow, torch.rand(P_, 1, H, W, generator=g)


def assert_conditions(pred, target, flow):
    """On the inputs, in fp64: no coverage within 1e-3 of the threshold, so fp32 cannot flip a mask.  (A sample with all four taps
    inside has coverage 1 up to fp64 rounding, which is 1e-3 from 0.999 up to that rounding: the margin is taken 1e-9 short.)"""
    cover = R.coverage(flow.double())
    assert bool(((cover - 0.999).abs() > 1e-3 - 1e-9).all()), float((cover - 0.999).abs().min())
    aligned, m = R.get_backwarp(pred.double(), flow.double())
    assert bool(((aligned != target.double()) | (m == 0)).all())
    assert 0 < float(m.mean()) < 1


def check_l1(pred, target, flow, mask, what):
    p64, t64 = pred.double().requires_grad_(), target.double().requires_grad_()
    want = R.aligned_l1(p64, flow.double(), t64, None if mask is None else mask.double())
    wp, wt = torch.autograd.grad((UP * want).sum(), [p64, t64])
    p, t = pred.to(DEV).requires_grad_(), target.to(DEV).requires_grad_()
    got = P.aligned_l1(p, flow.to(DEV), t, None if mask is None else mask.to(DEV))
    gp, gt = torch.autograd.grad((UP * got).sum(), [p, t])
    print(what, "losses", got.tolist(), "restatement", want.tolist(), "max |grad|", float(wp.abs().max()), float(wt.abs().max()),
          "max grad diff", float((gp.cpu().double() - wp).abs().max()), float((gt.cpu().double() - wt).abs().max()))
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=2e-6, atol=0, err_msg=what)
    np.testing.assert_allclose(gp.cpu().numpy(), wp.numpy(), rtol=0, atol=1e-5 * float(wp.abs().max()), err_msg=what)
    np.testing.assert_allclose(gt.cpu().numpy(), wt.numpy(), rtol=0, atol=1e-5 * float(wt.abs().max()), err_msg=what)
    only_pred, = torch.autograd.grad((UP * P.aligned_l1(p, flow.to(DEV), target.to(DEV), None if mask is None else mask.to(DEV))).sum(), [p])
    np.testing.assert_allclose(only_pred.cpu().numpy(), wp.numpy(), rtol=0, atol=1e-5 * float(wp.abs().max()), err_msg=what + " (no v_target)")


@pytest.mark.parametrize("name", ["fixture", "random"])
def test_backwarp_matches_restatement(name, fx):
    pred, target, flow, _ = warp_case(name, fx)
    assert_conditions(pred, target, flow)
    want, want_mask = R.get_backwarp(pred.double(), flow.double())
    x = pred.to(DEV).requires_grad_()
    got, mask = P.backwarp(x, flow.to(DEV))
    assert torch.equal(mask.cpu().double(), want_mask) and not mask.requires_grad
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.numpy(), rtol=0, atol=2e-6 * float(want.abs().max()))
    v = torch.randn(pred.shape, generator=torch.Generator().manual_seed(5))
    x64 = pred.double().requires_grad_()
    want_grad, = torch.autograd.grad((R.get_backwarp(x64, flow.double())[0] * v.double()).sum(), [x64])
    got_grad, = torch.autograd.grad((got * v.to(DEV)).sum(), [x])
    np.testing.assert_allclose(got_grad.cpu().numpy(), want_grad.numpy(), rtol=0, atol=1e-5 * float(want_grad.abs().max()))
    if name == "fixture":  # and the reference's own output, recorded
        np.testing.assert_allclose(got.detach().cpu().numpy(), fx["a/warped"].numpy(), rtol=0, atol=2e-6)
    with pytest.raises(RuntimeError, match="flow carries a gradient"):
        P.backwarp(x, flow.to(DEV).requires_grad_())
    with pytest.raises(ValueError):
        P.backwarp(torch.rand(1, 3, 1, 8, device=DEV), torch.zeros(1, 2, 1, 8, device=DEV))


@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("name", ["fixture", "random"])
def test_aligned_l1_matches_restatement(name, with_mask, fx):
    pred, target, flow, mask = warp_case(name, fx)
    assert_conditions(pred, target, flow)
    check_l1(pred, target, flow, mask if with_mask else None, f"{name} mask={with_mask}")
    if name == "fixture":  # the reference's own loss: the mean over the pairs
        got = P.aligned_l1(pred.to(DEV), flow.to(DEV), target.to(DEV), mask.to(DEV) if with_mask else None).mean()
        np.testing.assert_allclose(float(got), float(fx["a/masked/loss" if with_mask else "a/plain/loss"]), rtol=2e-6)


def test_aligned_l1_known_answers():
    """A flow that pushes every sample outside the image: loss 0 and zero gradients.  The identity flow: mean |pred - target| mask."""
    pred, target, _, mask = warp_case("random", None)
    H, W = pred.shape[-2:]
    p, t = pred.to(DEV).requires_grad_(), target.to(DEV).requires_grad_()
    away = torch.zeros(3, 2, H, W)
    away[0, 0], away[1, 1], away[2, 0] = W + 1.0, -(H + 1.0), -1e30
    loss = P.aligned_l1(p, away.to(DEV), t, mask.to(DEV))
    gp, gt = torch.autograd.grad(loss.sum(), [p, t])
    assert not loss.any() and not gp.any() and not gt.any()
    loss = P.aligned_l1(p, torch.zeros(3, 2, H, W, device=DEV), t, mask.to(DEV))
    want = ((pred.double() - target.double()).abs() * mask.double()).mean(dim=(1, 2, 3))
    np.testing.assert_allclose(loss.detach().cpu().numpy(), want.numpy(), rtol=2e-6)
    gp, gt = torch.autograd.grad(loss.sum(), [p, t])
    want_grad = torch.sign(pred.double() - target.double()) * mask.double() / (3 * H * W)
    np.testing.assert_allclose(gp.cpu().numpy(), want_grad.numpy(), rtol=0, atol=1e-5 * float(want_grad.abs().max()))
    assert torch.equal(gt, -gp)
    eq = pred.clone()
    eq[:, :, ::2] = target[:, :, ::2]  # sign(0) = 0
    g, = torch.autograd.grad(P.aligned_l1(eq.to(DEV).requires_grad_(), torch.zeros(3, 2, H, W, device=DEV), t).sum(), [t])
    assert not g[:, :, ::2].any() and g[:, :, 1::2].all()


# ---- past the launch caps: the grid stops growing and every lane strides ---------------------------------------------------------------
WB = 256                # warp.hip: constexpr int WB = REDUCE_NT (reduce.h: REDUCE_NT = 256)
WARP_MAX_BLOCKS = 4096  # warp.hip: constexpr int WARP_MAX_BLOCKS = 4096
AL1_CAPPED = (129, 255)       # 32 895 px per pair > 128 x 256: lanes 0..126 of block 0 take a second pixel
WARP_CAPPED = (3, 2, 593, 590)  # 1 049 610 px > 4096 x 256: the last 1 034 take a second turn, all of them in batch 2


def settled_flow(B, H, W, g, amp=4.0):
    """Random flows of a few pixels.  Among so many samples some land within 1e-3 of the 0.999 coverage threshold at the border;
    those are moved by a hundredth of a pixel, in fp64 on the CPU, until none is left (assert_conditions checks the result)."""
    flow = amp * (torch.rand(B, 2, H, W, generator=g) - 0.5)
    for _ in range(8):
        cover = R.coverage(flow.double())  # exactly inside: 1 up to fp64 rounding, which the margin allows for
        close = ((cover > 0.997) & (cover < 1 - 1e-8))[:, None].expand(B, 2, H, W)
        if not bool(close.any()):
            break
        flow = torch.where(close, flow + 0.01, flow)
    return flow


def capped_l1_case():
    H, W = AL1_CAPPED
    assert L.lib().d4gs_aligned_l1_blocks(H, W) == 128 and H * W > 128 * WB  # the cap is reached and a second turn exists
    g = torch.Generator().manual_seed(129255)
    pred, target = torch.rand(2, 3, H, W, generator=g), torch.rand(2, 3, H, W, generator=g)
    return pred, target, settled_flow(2, H, W, g), torch.rand(2, 1, H, W, generator=g)


@pytest.mark.parametrize("with_mask", [True, False])
def test_aligned_l1_past_the_block_cap_matches_restatement(with_mask):
    """129 x 255: k_al1_fwd and k_al1_bwd run 128 blocks per pair and stride; the partials are laid out 128 per pair."""
    pred, target, flow, mask = capped_l1_case()
    assert_conditions(pred, target, flow)
    check_l1(pred, target, flow, mask if with_mask else None, f"129x255 mask={with_mask}")


def test_aligned_l1_past_the_block_cap_known_answer():
    """pred == target but for one value per pair, at a pixel that only a second turn reaches (index >= 128 x 256), under a zero flow:
    the loss is that |d| / (3 H W), the gradient sits on that value alone and v_target = -v_pred."""
    H, W = AL1_CAPPED
    assert L.lib().d4gs_aligned_l1_blocks(H, W) == 128 and H * W > 128 * WB
    target = torch.randint(0, 16, (2, 3, H, W), generator=torch.Generator().manual_seed(4)).float() / 64  # a grid: d is exact
    pred = target.clone()
    spots = ((0, 1, 128, 200), (1, 2, H - 1, W - 1))  # (pair, channel, y, x)
    for (p_, c, y, x), d in zip(spots, (0.5, -0.25)):
        assert y * W + x >= 128 * WB
        pred[p_, c, y, x] = target[p_, c, y, x] + d
        assert float(pred[p_, c, y, x] - target[p_, c, y, x]) == d
    p, t = pred.to(DEV).requires_grad_(), target.to(DEV).requires_grad_()
    loss = P.aligned_l1(p, torch.zeros(2, 2, H, W, device=DEV), t)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), np.array([0.5, 0.25]) / (3 * H * W), rtol=2e-6, atol=0)
    gp, gt = torch.autograd.grad(loss.sum(), [p, t])
    want = torch.zeros(2, 3, H, W)
    for (p_, c, y, x), d in zip(spots, (0.5, -0.25)):
        want[p_, c, y, x] = math.copysign(float(np.float32(1.0 / (3.0 * H * W))), d)
    assert torch.equal(gp.cpu(), want) and torch.equal(gt, -gp)


def test_backwarp_past_the_block_cap():
    """3 x 593 x 590: k_backwarp_fwd / _bwd run 4096 blocks and the lanes of the first five take a second pixel, whose batch
    b = p / plane is 2; k_zero_f32 strides over the C = 2 planes of the gradient.  Values and mask against the restatement and the
    backward against its autograd, at test_backwarp_matches_restatement's bounds; batch 2 bit for bit against a call on it alone."""
    B, C, H, W = WARP_CAPPED
    n_pix, first_turn = B * H * W, WARP_MAX_BLOCKS * WB
    assert first_turn < n_pix <= first_turn + H * W and n_pix - first_turn == 1034 and first_turn > 2 * H * W  # the tail lies in batch 2
    assert n_pix * C > first_turn  # and the zeroing strides too
    g = torch.Generator().manual_seed(593590)
    pred = torch.rand(B, C, H, W, generator=g)
    flow = settled_flow(B, H, W, g, amp=6.0)
    cover = R.coverage(flow.double())
    assert bool(((cover - 0.999).abs() > 1e-3 - 1e-9).all()), float((cover - 0.999).abs().min())
    want, want_mask = R.get_backwarp(pred.double(), flow.double())
    tail = want_mask.reshape(-1)[first_turn:]
    assert 0 < float(tail.mean()) < 1 and 0 < float(want_mask.mean()) < 1  # the second turn holds both kinds of sample
    x = pred.to(DEV).requires_grad_()
    got, mask = P.backwarp(x, flow.to(DEV))
    assert torch.equal(mask.cpu().double(), want_mask) and not mask.requires_grad
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.numpy(), rtol=0, atol=2e-6 * float(want.abs().max()))
    v = torch.randn(pred.shape, generator=torch.Generator().manual_seed(5))
    x64 = pred.double().requires_grad_()
    want_grad, = torch.autograd.grad((R.get_backwarp(x64, flow.double())[0] * v.double()).sum(), [x64])
    got_grad, = torch.autograd.grad((got * v.to(DEV)).sum(), [x])
    err = float((got_grad.cpu().double() - want_grad).abs().max())
    print(f"backwarp {B}x{C}x{H}x{W}: max |grad| {float(want_grad.abs().max()):.3e}, max grad err {err:.3e}, "
          f"bound {1e-5 * float(want_grad.abs().max()):.3e}")
    np.testing.assert_allclose(got_grad.cpu().numpy(), want_grad.numpy(), rtol=0, atol=1e-5 * float(want_grad.abs().max()))
    alone, alone_mask = P.backwarp(pred[2:3].to(DEV), flow[2:3].to(DEV))  # 349 870 px: below the cap, b = 0 throughout
    assert H * W <= first_turn
    assert torch.equal(got.detach()[2:3].view(torch.int32), alone.view(torch.int32)) and torch.equal(mask[2:3], alone_mask)


# ---- the network ---------------------------------------------------------------------------------------------------------------
def seeded_pwcnet(fx):
    names = [str(n) for n in fx["b/names"]]
    shapes = [tuple(int(x) for x in row if x) for row in fx["b/shapes"]]
    state = R.seeded_state(list(zip(names, shapes)))
    np.testing.assert_allclose(R.checksum(state), fx["c/checksum"], rtol=1e-13)
    net = P.PWCNet(load_pretrained=False)
    net.net.load_state_dict({k: v.float() for k, v in state.items()})
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def alignnet(fx):
    return seeded_pwcnet(fx)


def test_network_matches_the_reference_flows(fx, alignnet):
    """Tolerance: 8 x the error of the reference's own network run in fp32 on the CPU (recorded beside the flows), relative to
    max |flow| - the factor allows for MIOpen's convolution algorithms rounding differently from the CPU's direct ones."""
    with torch.no_grad():
        flow = alignnet.net(fx["c/first"].float().to(DEV), fx["c/second"].float().to(DEV)).cpu().double()
        wflow = alignnet(fx["c/source"].float().to(DEV), fx["c/target"].float().to(DEV)).cpu().double()
    for name, got, want, ref_err in (("network", flow, fx["c/flow"], float(fx["d/flow_fp32_err"])),
                                     ("wrapper", wflow, fx["c/wrapper_flow"], float(fx["d/wrapper_flow_fp32_err"]))):
        err = float((got - want).abs().max() / want.abs().max())
        print(f"{name}: rel err {err:.3e}, reference fp32 on the CPU {ref_err:.3e}, bound {8 * ref_err:.3e}")
        assert got.shape == want.shape
        assert err <= 8 * ref_err, (name, err, ref_err)


def exposure_stack(seed, S=3, H=64, W=64):
    """[S,1,H,W,5]: smooth images that drift by a pixel or two per sub-sample, an alpha in (0.2, 1), one more channel"""
    g = torch.Generator().manual_seed(seed)
    base, _ = R.network_inputs(seed, 1, H + 8, W + 8)
    rgb = torch.stack([base[0, :, 4 + e:4 + e + H, 4 + 2 * e:4 + 2 * e + W] for e in range(S)]) + 0.02 * torch.rand(S, 3, H, W, generator=g, dtype=F64)
    alpha = 0.2 + 0.8 * torch.rand(S, 1, H, W, generator=g, dtype=F64)
    extra = torch.rand(S, 1, H, W, generator=g, dtype=F64)
    return torch.cat([rgb, alpha, extra], 1).permute(0, 2, 3, 1)[:, None].float().contiguous()


def reference_loop(all_imgs, alignloss):
    """flow3d/trainer.py:599-618, pair by pair in its order"""
    total = 0.0
    n = all_imgs.shape[0]
    chw = lambda t: t.permute(0, 3, 1, 2)
    for e in range(n - 1):
        total = total + alignloss(chw(all_imgs[e:e + 1, 0, :, :, 0:3]), chw(all_imgs[e + 1:e + 2, 0, :, :, 0:3]),
                                  mask=chw(all_imgs[e + 1:e + 2, 0, :, :, 3:4].detach()))
    for e in range(1, n):
        total = total + alignloss(chw(all_imgs[e:e + 1, 0, :, :, 0:3]), chw(all_imgs[0:1, 0, :, :, 0:3]).detach(),
                                  mask=chw(all_imgs[0:1, 0, :, :, 3:4].detach()))
    return total / (n - 1)


class RecordedFlows(torch.nn.Module):
    """Stands where the flow network stands.  Given a network: calls it and keeps the flows; given flows: hands them out pair by
    pair, in the order of the calls."""

    def __init__(self, net=None, flows=None):
        super().__init__()
        self.net, self.flows, self.at = net, flows, 0

    def forward(self, source, target):
        if self.net is not None:
            self.flows = self.net(source, target)
            return self.flows
        n = source.shape[0]
        self.at += n
        return self.flows[self.at - n:self.at]


def test_batched_loss_equals_the_reference_ordered_loop(alignnet):
    x = exposure_stack(9).to(DEV).requires_grad_()
    recorder = RecordedFlows(net=alignnet)
    loss = P.exposure_consistency_loss(x, recorder)
    grad, = torch.autograd.grad(UP * loss, [x])
    y = x.detach().clone().requires_grad_()
    want = reference_loop(y, P.AlignedLoss(alignnet))  # 2 (S - 1) network passes at batch 1
    want_grad, = torch.autograd.grad(UP * want, [y])
    print("batched", float(loss), "loop", float(want), "rel diff", abs(float(loss) - float(want)) / float(want),
          "max |grad|", float(want_grad.abs().max()), "max grad diff", float((grad - want_grad).abs().max()))
    assert float(want) > 0
    np.testing.assert_allclose(float(loss), float(want), rtol=1e-6)
    assert grad[..., :3].any() and not grad[..., 3:].any()  # RGB only: the alpha is a detached mask
    # Which pair feeds which sub-sample, and that sub-sample 0 receives nothing as a target: the same loop, which detaches that
    # target explicitly, over the flows of the batched pass (a pass at batch 1 gives flows that differ in the last fp32 digits,
    # which is the network's arithmetic and not the pairing).  Gradients at the loss kernels' tolerance.
    z = x.detach().clone().requires_grad_()
    same = reference_loop(z, P.AlignedLoss(RecordedFlows(flows=recorder.flows)))
    same_grad, = torch.autograd.grad(UP * same, [z])
    print("loop over the batched flows", float(same), "max |grad|", float(same_grad.abs().max()), "max grad diff", float((grad - same_grad).abs().max()))
    np.testing.assert_allclose(float(loss), float(same), rtol=1e-6)
    np.testing.assert_allclose(grad.cpu().numpy(), same_grad.cpu().numpy(), rtol=0, atol=1e-5 * float(same_grad.abs().max()))
    # and directly: with S = 2 sub-sample 0 is the prediction of pair 0 and the detached target of pair 1 - its gradient is pair 0's alone
    two = x.detach()[:2].clone().requires_grad_()
    rec2 = RecordedFlows(net=alignnet)
    g_two, = torch.autograd.grad(P.exposure_consistency_loss(two, rec2), [two])
    img = two.detach()[:, 0, :, :, :3].permute(0, 3, 1, 2)
    p0 = img[:1].clone().requires_grad_()
    g_p0, = torch.autograd.grad(P.aligned_l1(p0, rec2.flows[:1], img[1:2], two.detach()[1:2, 0, :, :, 3]).sum(), [p0])
    np.testing.assert_allclose(g_two[0, 0, :, :, :3].permute(2, 0, 1).cpu().numpy(), g_p0[0].cpu().numpy(), rtol=0,
                               atol=1e-5 * float(g_p0.abs().max()))


def test_graph_capture_and_replay(alignnet):
    """The whole call - one batched network pass, the loss, its backward - in one captured graph (capture aborts on any host wait),
    at the default hardware-queue count.  Both replays give the eager loss (to the batched test's 1e-6).  The warm-up runs on the
    stream the capture then uses, as torch asks of every capture: MIOpen and rocBLAS keep per-stream state that they set up on
    first use, which must not happen inside the capture."""
    static = exposure_stack(10).to(DEV).requires_grad_()

    def run():
        loss = P.exposure_consistency_loss(static, alignnet)
        return loss, torch.autograd.grad(loss, [static])[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager_loss, eager_grad = [t.clone() for t in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = run()
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        print("replay", i, float(out[0]), "eager", float(eager_loss), "max grad diff", float((out[1] - eager_grad).abs().max()))
        np.testing.assert_allclose(float(out[0]), float(eager_loss), rtol=1e-6)
        np.testing.assert_allclose(out[1].cpu().numpy(), eager_grad.cpu().numpy(), rtol=0, atol=1e-5 * float(eager_grad.abs().max()))


def test_example_runs_with_the_consistency_loss():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_dynamic_step.py"), "--consistency-loss", "--steps", "2"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    losses = [float(v) for v in re.findall(r"loss\s+(\S+)", r.stdout)]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout
