"""The image terms on the GPU (csrc/image_terms.hip through deblur4dgs_amd.losses): the dilation bit for bit against torch's CPU
max_pool2d of the same fp32 tensor, the sharp-keep and coverage losses against the fp64 statement tests/image_terms_ref.py, which
tests/test_image_terms_ref.py pins to torch's CPU ops.

Inputs are fp32 and the statement sees the same numbers in fp64, so the two sides differ in arithmetic only.  Bounds are those of
tests/test_gpu_trimmed_losses.py: the value at rtol 2e-6, the gradient within 1e-5 of its maximum.  No sign flip is allowed for:
every random sharp-keep case first asserts, from the fp64 statement alone, that every non-zero |pbar mbar - tbar mbar| is at least
1e-5 (the device forms it in double from exact window sums: its error is ~1e-16), and the tie case is exact in fp32.

The coverage loss runs at n = 1, 255, 256, 257 (around one block), 5 740 (23 blocks) and 1 049 610 = 3 x 593 x 590, which is past
the cap of 4 096 blocks x 256: 1 034 elements are summed in a second turn of the stride and 4 096 partials, 16 per thread, are
totalled."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from deblur4dgs_amd import _lib as L
from deblur4dgs_amd.losses import coverage_loss, dilate_mask, photometric_loss, sharp_keep_loss
from tests import image_terms_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UP = 1.7  # upstream factor of every backward


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- dilation

def dilate_contents(H, W):
    """name -> [2,H,W] fp32, the two images different so that a batch bleed shows."""
    g = torch.Generator().manual_seed(1000 * H + W)
    second = (torch.rand(H, W, generator=g) < 0.1).float()
    out = {}
    for name, (y, x) in {"top-left": (0, 0), "top-right": (0, W - 1), "bottom-left": (H - 1, 0), "bottom-right": (H - 1, W - 1),
                         "centre": (H // 2, W // 2)}.items():
        hot = torch.zeros(H, W)
        hot[y, x] = 0.5
        out[name] = torch.stack([hot, second])
    out["zeros"] = torch.stack([torch.zeros(H, W), second])
    out["minus one"] = torch.stack([-torch.ones(H, W), second - 1.0])
    out["non-binary"] = torch.rand(2, H, W, generator=g) * 4.0 - 2.0
    return out


@pytest.mark.parametrize("H,W", ((1, 1), (3, 5), (9, 9), (10, 70), (41, 70)))
def test_dilation_is_bitwise_max_pool(H, W):
    for name, mask in dilate_contents(H, W).items():
        for r in (0, 1, 4):
            want = F.max_pool2d(mask[:, None], 2 * r + 1, 1, r)[:, 0]
            got, comp = dilate_mask(mask.to(DEV), 2 * r + 1, return_complement=True)
            assert got.dtype == torch.float32 and tuple(got.shape) == (2, H, W)
            assert torch.equal(bits(got), bits(want)), (name, r, H, W)
            assert torch.equal(bits(comp), bits(1.0 - want)), (name, r, H, W)
            assert torch.equal(bits(dilate_mask(mask.to(DEV), 2 * r + 1)), bits(want))  # without the complement


def test_dilation_known_answers_and_the_trailing_axis():
    one = torch.zeros(1, 3, 5)
    one[0, 1, 2] = 0.5
    assert torch.equal(dilate_mask(one.to(DEV)).cpu(), torch.full((1, 3, 5), 0.5))  # the image is smaller than the window
    assert torch.equal(dilate_mask(-torch.ones(2, 3, 5, device=DEV)).cpu(), -torch.ones(2, 3, 5))  # the identity is -inf, not 0
    m = (torch.rand(2, 10, 70, generator=torch.Generator().manual_seed(3)) < 0.05).float()
    got = dilate_mask(m[..., None].to(DEV))
    assert tuple(got.shape) == (2, 10, 70, 1) and not got.requires_grad
    assert torch.equal(got[..., 0].cpu(), F.max_pool2d(m[:, None], 9, 1, 4)[:, 0])
    assert torch.equal(dilate_mask((m > 0.5).to(DEV)).cpu(), F.max_pool2d(m[:, None], 9, 1, 4)[:, 0])  # a bool mask, as the data loader's


@pytest.mark.parametrize("r", (16, 17, 100))
def test_dilation_at_the_radius_where_the_kernel_changes(r):
    """r <= 16 runs from an LDS patch, larger radii walk the window in global memory; r = 100 is beyond the 41 x 70 image."""
    mask = dilate_contents(41, 70)["non-binary"]
    got, comp = dilate_mask(mask.to(DEV), 2 * r + 1, return_complement=True)
    want = F.max_pool2d(mask[:, None], 2 * r + 1, 1, r)[:, 0]
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(comp), bits(1.0 - want))


# -------------------------------------------------------------------------------------------------------------- sharp-keep

def keep_case(B, H, W, C, seed):
    """Uniform images and a 60 % mask."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, H, W, C, generator=g), torch.rand(B, H, W, C, generator=g), (torch.rand(B, H, W, generator=g) < 0.6).float()


def separated(pred, target, mask, factor):
    d = np.abs(R.keep_elements(pred.numpy(), target.numpy(), mask.numpy(), factor)[0])
    return d[d != 0].size == 0 or d[d != 0].min() >= 1e-5


def keep_on_gpu(pred, target, mask, factor):
    p = pred.to(DEV).requires_grad_()
    loss = sharp_keep_loss(p, target.to(DEV), mask.to(DEV), factor)
    (UP * loss).backward()
    return loss.detach().cpu(), p.grad.cpu()


def check(got, want, what):
    (gl, gg), (wl, wg) = got, want
    gmax = float(np.abs(wg).max())
    print(what, "loss", float(gl), "statement", wl, "rel", abs(float(gl) - wl) / max(abs(wl), 1e-300), "max |grad|", UP * gmax,
          "max grad diff / max", float(np.abs(gg.double().numpy() - UP * wg).max()) / max(UP * gmax, 1e-300))
    np.testing.assert_allclose(float(gl), wl, rtol=2e-6, atol=0, err_msg=what)
    np.testing.assert_allclose(gg.numpy(), UP * wg, rtol=0, atol=1e-5 * UP * gmax, err_msg=what)


# (H, W, factor) -> seed: chosen on the CPU so that the separation holds; it is asserted again in the test
KEEP_CASES = {(4, 4, 4): 0, (7, 7, 4): 0, (9, 11, 4): 0, (9, 11, 2): 0, (16, 16, 4): 0, (41, 70, 4): 0}


@pytest.mark.parametrize("H,W,factor", sorted(KEEP_CASES))
def test_sharp_keep_matches_the_statement(H, W, factor):
    """4x4: one window; 7x7: one 7x7 window; 9x11: overlapping windows on both axes; 41x70: 1020 outputs, several blocks."""
    pred, target, mask = keep_case(2, H, W, 3, KEEP_CASES[(H, W, factor)])
    reduced = torch.from_numpy(R.area_mean(target.numpy(), factor)).float()  # fp32: its own numbers, seen in fp64 by the statement
    for name, tgt in (("full target", target), ("reduced target", reduced)):
        assert separated(pred, tgt, mask, factor), (H, W, factor, name)  # a wrong seed, not a skip
        want = R.sharp_keep(pred.numpy(), tgt.numpy(), mask.numpy(), factor)
        check(keep_on_gpu(pred, tgt, mask, factor), want, f"sharp-keep {H}x{W} factor {factor} {name}")
    got = keep_on_gpu(pred, target, mask[..., None], factor)  # the mask with a trailing axis
    assert torch.equal(got[0], keep_on_gpu(pred, target, mask, factor)[0])


def test_sharp_keep_factor_one_uses_the_target_as_it_is():
    pred, target, mask = keep_case(2, 5, 6, 3, 11)
    assert separated(pred, target, mask, 1)
    check(keep_on_gpu(pred, target, mask, 1), R.sharp_keep(pred.numpy(), target.numpy(), mask.numpy(), 1), "sharp-keep factor 1")


def test_sharp_keep_exact_ties_get_exactly_zero():
    """Images and mask on a grid of 1/64, H and W multiples of 4: every window mean is exact in fp32, so d == 0 exactly on the left half
    where pred == target.  sign(0) = 0: the gradient there is exactly 0.0, and it is not elsewhere."""
    g = torch.Generator().manual_seed(7)
    B, H, W = 2, 8, 16
    pred = torch.randint(0, 48, (B, H, W, 3), generator=g).float() / 64
    target = pred.clone()
    target[:, :, W // 2:] += 1.0 / 64  # every window mean of the right half differs by 1/64
    mask = torch.randint(1, 65, (B, H, W), generator=g).float() / 64  # no empty window
    loss, grad = keep_on_gpu(pred, target, mask, 4)
    assert torch.all(grad[:, :, :W // 2] == 0.0) and torch.all(grad[:, :, W // 2:] != 0.0)
    want = R.sharp_keep(pred.numpy(), target.numpy(), mask.numpy(), 4)
    check((loss, grad), want, "sharp-keep ties")
    assert np.array_equal(want[1] == 0.0, grad.numpy() == 0.0)


def test_mask_and_target_get_no_gradient():
    pred, target, mask = keep_case(2, 9, 11, 3, KEEP_CASES[(9, 11, 4)])
    plain = keep_on_gpu(pred, target, mask, 4)[1]
    p, t, m = pred.to(DEV).requires_grad_(), target.to(DEV).requires_grad_(), mask.to(DEV).requires_grad_()
    (UP * sharp_keep_loss(p, t, m, 4)).backward()
    assert torch.equal(p.grad.cpu(), plain) and t.grad is None and m.grad is None
    reduced = torch.from_numpy(R.area_mean(target.numpy(), 4)).float().to(DEV)
    with torch.no_grad():  # forward only
        loss = sharp_keep_loss(pred.to(DEV), reduced, mask.to(DEV), 4)
    assert not loss.requires_grad and torch.equal(loss.cpu(), keep_on_gpu(pred, reduced.cpu(), mask, 4)[0])


# ---------------------------------------------------------------------------------------------------------------- coverage

MSE_SHAPES = {1: (1, 1, 1, 1), 255: (1, 15, 17, 1), 256: (1, 16, 16, 1), 257: (1, 1, 257, 1), 2 * 41 * 70: (2, 41, 70, 1),
              3 * 593 * 590: (3, 593, 590, 1)}  # the last: past the block cap, 1 034 elements in a second turn
MSE_MAX_BLOCKS = 4096  # image_terms.hip: constexpr int MSE_MAX_BLOCKS = 4096, blocks of 256


def mse_on_gpu(acc, target):
    a = acc.to(DEV).requires_grad_()
    loss = coverage_loss(a, None if target is None else target.to(DEV))
    (UP * loss).backward()
    return loss.detach().cpu(), a.grad.cpu()


@pytest.mark.parametrize("n", sorted(MSE_SHAPES))
def test_coverage_matches_the_statement(n):
    g = torch.Generator().manual_seed(n)
    acc = torch.rand(MSE_SHAPES[n], generator=g)
    assert acc.numel() == n
    if n > 2 * 41 * 70:  # k_mse_fwd strides and k_image_terms_finish totals 4096 partials, 16 per thread
        assert L.lib().d4gs_mse_blocks(n) == MSE_MAX_BLOCKS and n > MSE_MAX_BLOCKS * 256
    target = (torch.rand(MSE_SHAPES[n], generator=g) < 0.6).float()
    same = torch.rand(MSE_SHAPES[n], generator=g) < (0.25 if n > 1 else 0.0)
    hit = torch.where(same, torch.ones_like(acc), acc)  # acc == 1 on a quarter: opaque pixels under the all-ones target
    got = mse_on_gpu(hit, None)
    check(got, R.mse(hit.numpy()), f"coverage n={n} target None")
    assert torch.all(got[1][same] == 0.0) and torch.all(got[1][~same] != 0.0)
    hit = torch.where(same, target, acc)
    got = mse_on_gpu(hit, target)
    check(got, R.mse(hit.numpy(), target.numpy()), f"coverage n={n} tensor target")
    assert torch.all(got[1][same] == 0.0) and torch.all(got[1][~same] != 0.0)
    got3 = mse_on_gpu(hit[..., 0], target)  # acc without the trailing axis
    assert torch.equal(got3[0], got[0]) and torch.equal(got3[1], got[1][..., 0])


def test_coverage_of_one_element_in_the_strided_tail():
    """acc == target but for one element that only the second turn of k_mse_fwd's stride reaches: the loss is d^2 / n and the
    gradient 2 d / n there and 0.0 everywhere else, both exact up to the one rounding of the quotient."""
    shape = MSE_SHAPES[3 * 593 * 590]
    n = 3 * 593 * 590
    assert L.lib().d4gs_mse_blocks(n) == MSE_MAX_BLOCKS and n > MSE_MAX_BLOCKS * 256
    at = MSE_MAX_BLOCKS * 256 + 777  # thread 9 of block 3, second turn
    assert MSE_MAX_BLOCKS * 256 <= at < n
    for target in (None, (torch.rand(shape, generator=torch.Generator().manual_seed(8)) < 0.6).float()):
        acc = torch.ones(shape) if target is None else target.clone()
        acc.view(-1)[at] -= 0.5  # 0.5 or -0.5: exact
        loss, grad = mse_on_gpu(acc, target)
        check((loss, grad), R.mse(acc.numpy(), None if target is None else target.numpy()), f"coverage one-hot target {target is not None}")
        np.testing.assert_allclose(float(loss), 0.25 / n, rtol=2e-6, atol=0)
        want = torch.zeros(n)
        want[at] = -0.5
        assert torch.equal(grad.view(-1) != 0, want != 0)
        np.testing.assert_allclose(float(grad.view(-1)[at]), UP * 2 * -0.5 / n, rtol=2e-6, atol=0)


# ------------------------------------------------------------------------------------------- reproducibility, capture, errors

def _step_inputs(seed, H=41, W=70):
    g = torch.Generator().manual_seed(seed)
    pred, gt, mask = keep_case(1, H, W, 3, seed)
    return [x.to(DEV) for x in (pred, gt, mask, torch.rand(1, H, W, 1, generator=g))]


def _step(pred, gt, mask, acc):
    """What --image-losses adds to the example's step, on one stream."""
    dilated = dilate_mask(mask)
    loss = photometric_loss(pred, gt, mask=dilated) + sharp_keep_loss(pred, gt, mask) + coverage_loss(acc)
    loss.backward()
    return loss.detach()


def _eager(seed):
    pred, gt, mask, acc = _step_inputs(seed)
    pred.requires_grad_(), acc.requires_grad_()
    return _step(pred, gt, mask, acc), pred.grad, acc.grad


def test_two_runs_are_bitwise_equal():
    pred, target, mask = keep_case(2, 41, 70, 3, 5)
    acc = torch.rand(2, 41, 70, 1, generator=torch.Generator().manual_seed(6))
    for a, b in zip(keep_on_gpu(pred, target, mask, 4) + mse_on_gpu(acc, mask) + mse_on_gpu(acc, None) + _eager(9),
                    keep_on_gpu(pred, target, mask, 4) + mse_on_gpu(acc, mask) + mse_on_gpu(acc, None) + _eager(9)):
        assert torch.equal(bits(a), bits(b)) and torch.isfinite(a).all() and a.any()


def test_graph_capture_and_replay_on_one_stream():
    """dilate_mask -> photometric_loss(mask=...) + sharp_keep_loss + coverage_loss -> backward in ONE captured graph on one stream,
    after two eager warm-up runs (capture aborts on any host wait: this is the test that the path has none).  Two replays with new
    input contents equal the eager results bit for bit."""
    static = _step_inputs(20)
    static[0].requires_grad_(), static[3].requires_grad_()
    for _ in range(2):
        _step(*static)
        static[0].grad = static[3].grad = None
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = _step(*static)
    for seed in (21, 22):
        with torch.no_grad():
            for s, f in zip(static, _step_inputs(seed)):
                s.copy_(f)
        g.replay()
        torch.cuda.synchronize()
        e_loss, e_pred, e_acc = _eager(seed)
        assert torch.equal(bits(loss), bits(e_loss)), (seed, float(loss), float(e_loss))
        assert torch.equal(bits(static[0].grad), bits(e_pred)) and torch.equal(bits(static[3].grad), bits(e_acc)), seed
        assert torch.isfinite(e_loss) and e_pred.any() and e_acc.any()


def test_errors():
    pred, target, mask = keep_case(1, 8, 12, 3, 0)
    with pytest.raises(RuntimeError, match="ROCm"):
        dilate_mask(mask)
    with pytest.raises(RuntimeError, match="ROCm"):
        sharp_keep_loss(pred.to(DEV), target, mask.to(DEV))
    with pytest.raises(RuntimeError, match="ROCm"):
        coverage_loss(mask.to(DEV), mask)
    p, t, m = pred.to(DEV), target.to(DEV), mask.to(DEV)
    with pytest.raises(ValueError, match="below factor"):
        sharp_keep_loss(p[:, :3], t[:, :3], m[:, :3], 4)  # torch: an empty tensor and a NaN loss
    with pytest.raises(ValueError, match="below factor"):
        sharp_keep_loss(p[:, :, :7], t[:, :, :7], m[:, :, :7], 8)
    with pytest.raises(ValueError, match="kernel_size"):
        dilate_mask(m, kernel_size=8)
    for bad_t in (t[:, :4], t[..., :2], t[:, :2, :2]):
        with pytest.raises(ValueError, match="target"):
            sharp_keep_loss(p, bad_t, m)
    with pytest.raises(ValueError, match="masks"):
        sharp_keep_loss(p, t, m[:, :4])
    with pytest.raises(ValueError, match="target"):
        coverage_loss(m, m[:, :4])


def test_example_trains_with_image_losses_inside_the_graph():
    """examples/train_dynamic_step.py with image_losses=True on a small scene: the whole step (three renders, the photometric terms
    under the dilated mask and its complement, sharp-keep and coverage losses, backward, one-launch Adam) captures after two eager
    steps and replays.  Step 0 runs eagerly in both modes from the same parameters, so its loss is the same number; the losses are
    finite, fall in both modes, and the replayed steps follow the eager ones within a quarter of the eager run's descent.  That
    bound is not a parity bound (the losses' replays are compared bit for bit in test_graph_capture_and_replay_on_one_stream): two
    eager runs of this example on one seed already differ by ~3e-3 at step 5 (1.1502 and 1.1531 were seen; the example's renders
    are not bitwise reproducible from step to step), a replay that lost or froze one of the added terms would be off by the size
    of that term - together they are half of the loss - and the descent over the six steps is 0.13."""
    import importlib.util
    import math
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_dynamic_step_image", os.path.join(root, "examples", "train_dynamic_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kw = dict(steps=6, W=128, H=96, n_fg=3000, n_bg=5000, K=6, verbose=False, hip_adam=True, image_losses=True)
    eager = mod.train(**kw)[0]
    graph = mod.train(graph=True, **kw)[0]
    plain = mod.train(**{**kw, "image_losses": False, "steps": 1})[0]
    descent = eager[0] - eager[-1]
    print("eager", eager, "| graph", graph, "| descent", descent, "| without the image losses", plain[0])
    assert all(math.isfinite(l) for l in graph + eager)
    assert math.isclose(graph[0], eager[0], rel_tol=1e-6)
    assert descent > 0 and graph[-1] < graph[0]
    assert all(abs(a - b) <= 0.25 * descent for a, b in zip(graph, eager)), (graph, eager, descent)
    assert eager[0] > plain[0]  # the four terms are in the loss
