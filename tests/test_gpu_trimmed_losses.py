"""The quantile-trimmed losses on the GPU (csrc/trimmed.hip through deblur4dgs_amd.losses) against the fp64 restatement
tests/trimmed_ref.py, which tests/test_trimmed_ref.py pins to the reference.

Inputs are quantised to fp32 first and the restatement gets those same values in fp64 (and forms the rank in fp32, as torch.quantile
does for fp32 input), so the two sides differ in arithmetic only.  Tolerances are those of tests/test_gpu_photometric.py: the value
at rtol 2e-6 (both sides add the same fp32-representable inputs; the device forms each element in fp32 - a few ulps of 6e-8 with
random signs - and adds them in double), the gradient at 1e-5 of its maximum.  No kept-set flips are allowed for: every random case
first asserts, from the fp64 values alone, that the order statistics around the threshold are at least 1e-5 of the value range
apart (trimmed_ref.neighbours_apart), and the structured cases have elements that are exact in fp32."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from deblur4dgs_amd.losses import compute_gradient_loss, masked_l1_loss, trimmed_l1_loss
from tests import trimmed_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
UP = 1.7  # upstream factor of every backward
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 70_001)  # below / at / above a wave, a block, one round of partials


def pick_q(n, candidates=(0.9, 0.98, 0.95, 0.8, 0.85, 0.77, 0.66, 0.97531)):
    """A quantile whose rank q (n - 1) has its fractional part in [0.05, 0.95] in fp64 (n <= 2 cannot: r = 0, or r = q)."""
    for q in candidates:
        if n < 2 or 0.05 <= math.modf(q * (n - 1))[0] <= 0.95:
            return q
    raise AssertionError(n)


def l1_case(n, D, seed, noise=0.2):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(n, D, generator=g)
    pred = gt + noise * torch.randn(n, D, generator=g)
    mask = (torch.rand(n, 1, generator=g) < 0.7).float()
    return pred, gt, mask


def grad_case(B, H, W, seed, kind):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, H, W, 1, generator=g)
    pred = gt + 0.3 * torch.randn(B, H, W, 1, generator=g)
    if kind == "true":
        mask = torch.ones(B, H, W, dtype=torch.bool)
    elif kind == "false":
        mask = torch.zeros(B, H, W, dtype=torch.bool)
    elif kind == "board":
        mask = ((torch.arange(H)[:, None] + torch.arange(W)[None]) % 2 == 0)[None].expand(B, H, W).clone()
    else:
        mask = torch.rand(B, H, W, generator=g) < 0.7
    return pred, gt, mask


def grad_elements(pred, gt, mask):
    """fp64 elements of the two terms (for the separation condition)."""
    p, t, m = pred.double()[..., 0], gt.double()[..., 0], mask.reshape(pred.shape[:3]) != 0
    dx = ((p[:, :, 1:] - p[:, :, :-1]) - (t[:, :, 1:] - t[:, :, :-1])).abs()[m[:, :, 1:] & m[:, :, :-1]]
    dy = ((p[:, 1:] - p[:, :-1]) - (t[:, 1:] - t[:, :-1])).abs()[m[:, 1:] & m[:, :-1]]
    return dx, dy


def on_gpu(fn, pred, *args, **kw):
    p = pred.to(DEV).requires_grad_()
    loss = fn(p, *[a.to(DEV) if torch.is_tensor(a) else a for a in args], **kw)
    (UP * loss).backward()
    return loss.detach().cpu(), p.grad.cpu()


def on_ref(fn, pred, *args, **kw):
    p = pred.double().requires_grad_()
    loss = fn(p, *[(a.double() if a.is_floating_point() else a) if torch.is_tensor(a) else a for a in args], rank_dtype=F32, **kw)
    (UP * loss).backward()
    return loss.detach(), p.grad


def check(got, want, what):
    (gl, gg), (wl, wg) = got, want
    print(what, "loss", float(gl), "restatement", float(wl), "max |grad| ", float(wg.abs().max()), "max grad diff", float((gg.double() - wg).abs().max()))
    np.testing.assert_allclose(float(gl), float(wl), rtol=2e-6, atol=0, err_msg=what)  # (NaN == NaN here: the empty kept sets)
    np.testing.assert_allclose(gg.numpy(), wg.numpy(), rtol=0, atol=1e-5 * float(wg.abs().max()), err_msg=what)


def both(name, *args, what="", **kw):
    ours = {"masked": masked_l1_loss, "trimmed": trimmed_l1_loss, "gradient": compute_gradient_loss}[name]
    ref = {"masked": R.masked_l1_loss, "trimmed": R.trimmed_l1_loss, "gradient": R.compute_gradient_loss}[name]
    check(on_gpu(ours, *args, **kw), on_ref(ref, *args, **kw), f"{name} {what} {kw}")


# Seeds: a formula per case, replaced here where the separation condition did not hold for it (found and checked on the CPU; the
# condition is asserted again in every test, so a wrong entry fails there and not in the comparison).
SEEDS = {("l1", 70001, 1): 78920, ("int", 0.5, 4097): 36599, ("row", 0.5, 4097): 36600, ("int", 0.5, 70001): 775092,
         ("row", 0.5, 70001): 545442, ("row", 0.75, 4097): 36600, ("int", 0.75, 70001): 656307, ("row", 0.75, 70001): 545442,
         ("train",): 549839}


def seed_for(*key, default):
    return SEEDS.get(key, default)


def l1_seed(n, D):
    return seed_for("l1", n, D, default=1000 * D + n)


@pytest.mark.parametrize("n", SIZES)
def test_l1_forms_match_restatement_at_every_size(n):
    q = pick_q(n)
    for D in (1, 2, 3):
        pred, gt, mask = l1_case(n, D, l1_seed(n, D))
        assert R.neighbours_apart(R.elements(pred.double(), gt.double()), q), (n, D)
        both("masked", pred, gt, mask, what=f"n={n} D={D}", normalize=True, quantile=q)
        both("masked", pred, gt, mask[:, 0] > 0, what=f"n={n} D={D} bool mask", normalize=False, quantile=q)
        both("masked", pred, gt, what=f"n={n} D={D} no mask", quantile=q)
        both("trimmed", pred, gt, what=f"n={n} D={D}", quantile=q)
    pred, gt, mask = l1_case(n, 3, l1_seed(n, 3))
    both("masked", pred, gt, mask, what=f"n={n} quantile 1", quantile=1.0)  # nothing selected, everything kept
    both("masked", pred, gt, torch.rand(n, generator=torch.Generator().manual_seed(n)), what=f"n={n} float weights", quantile=q)


INT_RANKS = [(0.5, n) for n in SIZES if n % 2 == 1 and n > 1] + [(0.75, n) for n in SIZES if (n - 1) % 4 == 0 and n > 1]


@pytest.mark.parametrize("q,n", INT_RANKS)
def test_integer_ranks(q, n):
    """q (n - 1) is an integer on which fp32 and fp64 agree: the threshold IS an element, and strictly-below drops it."""
    assert R.rank(q, n, F32) == R.rank(q, n, torch.float64) and R.rank(q, n)[2] == 0.0
    pred, gt, mask = l1_case(n, 1, seed_for("int", q, n, default=7 * n + 1))
    assert R.neighbours_apart(R.elements(pred.double(), gt.double()), q)
    both("masked", pred, gt, mask, what=f"n={n}", quantile=q)
    both("trimmed", pred, gt, what=f"n={n}", quantile=q)
    img = l1_case(n, 1, seed_for("row", q, n, default=7 * n + 2))
    pred, gt = img[0].reshape(1, 1, n, 1), img[1].reshape(1, 1, n, 1)  # one row: n - 1 horizontal pairs, no vertical one
    q = pick_q(n - 1)  # n - 1 pairs
    assert R.neighbours_apart(grad_elements(pred, gt, torch.ones(1, 1, n))[0], q)
    both("gradient", pred, gt, torch.ones(1, 1, n, dtype=torch.bool), what=f"row of {n}", quantile=q)  # NaN: the y term is empty


GRAD_SHAPES = [(1, 1, 2), (1, 2, 1), (1, 3, 3), (1, 17, 31), (1, 64, 65), (2, 40, 33)]


def grad_q(B, H, W, kind, pred, gt, mask):
    dx, dy = grad_elements(pred, gt, mask)
    for q in (0.95, 0.9, 0.8, 0.85, 0.77, 0.66, 0.6):
        ok = all(d.numel() < 3 or 0.05 <= math.modf(q * (d.numel() - 1))[0] <= 0.95 for d in (dx, dy))
        if ok:
            return q, dx, dy
    raise AssertionError((B, H, W, kind))


@pytest.mark.parametrize("B,H,W", GRAD_SHAPES)
@pytest.mark.parametrize("kind", ["true", "false", "board", "random"])
def test_gradient_loss_matches_restatement(B, H, W, kind):
    pred, gt, mask = grad_case(B, H, W, seed_for("grad", B, H, W, kind, default=100 * H + W), kind)
    q, dx, dy = grad_q(B, H, W, kind, pred, gt, mask)
    if kind in ("false", "board"):
        assert dx.numel() == dy.numel() == 0  # no valid pair: NaN (the reference raises)
    for d in (dx, dy):
        assert R.neighbours_apart(d, q), (B, H, W, kind)
    both("gradient", pred, gt, mask, what=f"{B}x{H}x{W} {kind}", quantile=q)
    both("gradient", pred[..., 0], gt[..., 0], mask[..., None].float(), what=f"{B}x{H}x{W} {kind} 3-D, float mask", quantile=q)


def exact_case(name):
    """-> v (fp32-exact elements, shuffled), q.  gt = 0 and pred = +-v, so both sides see the same elements bit for bit."""
    g = torch.Generator().manual_seed(5)
    if name == "shared_high_digits":  # 1 + i 2^-20: the first two digits of every key are equal, the third nearly
        v, q = 1.0 + torch.arange(4096, dtype=torch.float64) * 2.0 ** -20, 0.9
    elif name == "sixty_decades":  # every digit spreads
        v, q = 10.0 ** (torch.rand(3002, generator=g, dtype=torch.float64) * 60 - 30), 0.9
    elif name == "ties_at_zero":  # pred == gt on 60 %: the threshold is inside the tie group at 0 and nothing is below it
        v, q = torch.cat([torch.zeros(600, dtype=torch.float64), 0.5 + torch.rand(400, generator=g, dtype=torch.float64)]), 0.5
    elif name == "ties_at_three_eighths":  # groups of 100 at k / 8; ranks 359 and 360 are both in group 3, which goes whole
        v, q = (torch.arange(800) // 100).double() / 8, 0.45
    v = v.float()
    return v[torch.randperm(v.numel(), generator=g)], q


@pytest.mark.parametrize("name", ["shared_high_digits", "sixty_decades", "ties_at_zero", "ties_at_three_eighths"])
def test_every_radix_pass_and_tie_groups(name):
    v, q = exact_case(name)
    n = v.numel()
    s = torch.sort(v.double()).values
    lo, hi, frac = R.rank(q, n, F32)
    assert (lo, hi) == R.rank(q, n)[:2]
    if name.startswith("ties"):
        assert s[lo] == s[hi] and (s == s[lo]).sum() >= 100  # the threshold is the tie group's value, exactly, on both sides
        n_kept = int((s < s[lo]).sum())
        assert n_kept == {"ties_at_zero": 0, "ties_at_three_eighths": 300}[name]
    else:  # the threshold, formed in fp32 from these fp32-exact elements, is strictly inside the gap between the two
        t32 = s[lo].float() + (s[hi].float() - s[lo].float()) * torch.tensor(frac, dtype=F32)
        assert 0.05 <= frac <= 0.95 and s[lo] < t32.double() < s[hi]
    sign = torch.where(torch.arange(n) % 3 == 0, -1.0, 1.0)
    pred, gt = (v * sign)[:, None], torch.zeros(n, 1)
    mask = (torch.arange(n) % 4 != 1).float()
    both("masked", pred, gt, mask, what=name, normalize=True, quantile=q)
    both("masked", pred, gt, mask, what=name, normalize=False, quantile=q)
    both("trimmed", pred, gt, what=name, quantile=q)
    if name == "ties_at_three_eighths":
        grad = on_gpu(trimmed_l1_loss, pred, gt, quantile=q)[1][:, 0]
        assert int((grad != 0).sum()) == 200 and not grad[v >= 0.375].any()  # groups 1, 2 (sign(0) = 0 in group 0); group 3 dropped
    # the same elements as horizontal pairs of one image row: pred = running sum of +-v
    row = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.float64), (v * sign).double()]), 0).float()
    d = (row[1:].double() - row[:-1].double()).abs()
    if name != "sixty_decades" and torch.equal(d.float().double(), d) and torch.equal(torch.sort(d).values, s):  # (the sum must stay exact)
        both("gradient", row.reshape(1, 1, -1, 1), torch.zeros(1, 1, n + 1, 1), torch.ones(1, 1, n + 1), what=name + " as a row", quantile=q)


def test_empty_kept_set():
    """n = 1 (the threshold is the element) and a constant input (one tie group): 0 for the normalised masked form, NaN for the means."""
    for pred, gt in ((torch.tensor([[0.3, 0.9]]), torch.tensor([[0.1, 0.2]])), (torch.full((300, 1), 0.25), torch.zeros(300, 1))):
        n = pred.shape[0]
        m = torch.ones(n, device=DEV)
        p = pred.to(DEV).requires_grad_()
        a = masked_l1_loss(p, gt.to(DEV), m, quantile=0.9)
        b = trimmed_l1_loss(p, gt.to(DEV), quantile=0.9)
        c = masked_l1_loss(p, gt.to(DEV), m, normalize=False, quantile=0.9)
        (a + torch.nan_to_num(b) + torch.nan_to_num(c)).backward()
        assert float(a) == 0.0 and math.isnan(float(b)) and math.isnan(float(c))
        assert not p.grad.any()
        both("masked", pred, gt, m.cpu(), what=f"empty n={n}", quantile=0.9)
        both("trimmed", pred, gt, what=f"empty n={n}", quantile=0.9)


def test_rejects_what_the_reference_rejects():
    x = torch.rand(1, 4, 4, 3, device=DEV)
    with pytest.raises(NotImplementedError):
        compute_gradient_loss(x, x, torch.ones(1, 4, 4, device=DEV))
    with pytest.raises(ValueError):
        masked_l1_loss(x, x, torch.ones(1, 4, 3, device=DEV), quantile=0.9)


def _three(pred3, gt3, mask3, predd, gtd, maskd, maskb):
    """forward and backward of the three functions -> (losses, gradients)"""
    la = masked_l1_loss(pred3, gt3, mask3, quantile=0.98)
    lb = trimmed_l1_loss(pred3, gt3, quantile=0.9)
    lc = compute_gradient_loss(predd, gtd, maskb, quantile=0.95)
    ld = masked_l1_loss(predd, gtd, maskd, normalize=False, quantile=0.98)
    total = la + 2.0 * lb + 3.0 * lc + 4.0 * ld
    g3, gd = torch.autograd.grad(total, [pred3, predd])
    return torch.stack([la, lb, lc, ld]).detach(), g3, gd


def _three_inputs(seed, keep=0.7, B=2, H=40, W=33):
    g = torch.Generator().manual_seed(seed)
    n = 70_001
    gt3 = torch.rand(n, 3, generator=g)
    pred3 = gt3 + 0.2 * torch.randn(n, 3, generator=g)
    mask3 = (torch.rand(n, generator=g) < 0.7).float()
    gtd = torch.rand(B, H, W, 1, generator=g)
    predd = gtd + 0.3 * torch.randn(B, H, W, 1, generator=g)
    maskb = torch.rand(B, H, W, generator=g) < keep
    return [t.to(DEV) for t in (pred3, gt3, mask3, predd, gtd, maskb.float()[..., None], maskb)]


def test_two_runs_are_bitwise_equal():
    t = _three_inputs(3)
    runs = []
    for _ in range(2):
        a = [x.clone() for x in t]
        a[0].requires_grad_(), a[3].requires_grad_()
        runs.append(_three(*a))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert torch.isfinite(runs[0][0]).all() and runs[0][1].any() and runs[0][2].any()


def test_graph_capture_and_replay_with_a_different_pair_count():
    """Forward and backward of all three functions in ONE captured graph (capture aborts on any host wait: this is the test that the
    path has none).  Replays with new data in the static inputs - the new mask has a different number of valid pairs, which only
    the device learns - equal eager calls on the same data bit for bit."""
    static = _three_inputs(11)
    static[0].requires_grad_(), static[3].requires_grad_()
    _three(*static)  # warm-up: code objects loaded, nothing lazy left inside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _three(*static)
    pairs = set()
    for seed, keep in ((11, 0.7), (12, 0.4), (13, 0.95)):
        fresh = _three_inputs(seed, keep)
        pairs.add(int((fresh[6][:, :, 1:] & fresh[6][:, :, :-1]).sum()))
        with torch.no_grad():
            for s, f in zip(static, fresh):
                s.copy_(f)
        g.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in out]
        fresh[0].requires_grad_(), fresh[3].requires_grad_()
        eager = _three(*fresh)
        for name, x, y in zip(("losses", "grad 3-wide", "grad depth"), replayed, eager):
            assert torch.equal(x, y), (seed, name, x.flatten()[:4], y.flatten()[:4])
        assert torch.isfinite(eager[0]).all()
    assert len(pairs) == 3


def test_training_shape_once():
    """[1,288,512,1] with the reference's quantiles (trainer.py:402-415): disparity-like values in a narrow range, so the first
    radix digits are shared by every key."""
    g = torch.Generator().manual_seed(seed_for("train", default=288512))
    gt = 1.0 / (2.0 + 3.0 * torch.rand(1, 288, 512, 1, generator=g))
    pred = gt * (1.0 + 0.1 * torch.randn(1, 288, 512, 1, generator=g))
    mask = (torch.rand(1, 288, 512, 1, generator=g) < 0.8).float()
    assert R.neighbours_apart(R.elements(pred.double(), gt.double()), 0.98)
    for d in grad_elements(pred, gt, mask[..., 0] > 0.5):
        assert R.neighbours_apart(d, 0.95)
    both("masked", pred, gt, mask, what="training shape", quantile=0.98)
    both("gradient", pred, gt, mask > 0.5, what="training shape", quantile=0.95)


def test_example_trains_with_depth_losses_inside_the_graph():
    """examples/train_dynamic_step.py with depth_losses=True on a small scene: the whole step (three renders, photometric and
    trimmed losses, backward, one-launch Adam) captures after two eager steps and replays; the losses are finite and the final one
    equals the eager run's of the same seed to the tolerance the example's graph mode already gets in tests/test_gpu_adam.py: the
    spread the eager run shows between two seeds of the synthetic scene (here asked of every step, not only the last)."""
    spec = importlib.util.spec_from_file_location("train_dynamic_step_depth", os.path.join(ROOT, "examples", "train_dynamic_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kw = dict(steps=6, W=128, H=96, n_fg=3000, n_bg=5000, K=6, verbose=False, hip_adam=True, depth_losses=True)
    eager = mod.train(**kw)[0]
    eager_seed2 = mod.train(seed=2, **kw)[0]
    graph = mod.train(graph=True, **kw)[0]
    plain = mod.train(**{**kw, "depth_losses": False})[0]
    spread = abs(eager[-1] - eager_seed2[-1])
    print("eager", eager, "| graph", graph, "| eager seed 2", eager_seed2[-1], "| spread", spread, "| without the depth losses", plain[0])
    assert all(math.isfinite(l) for l in graph + eager)
    assert all(abs(a - b) <= spread for a, b in zip(graph, eager)), (graph, eager, spread)
    assert eager[0] > plain[0]  # the three terms are in the loss
