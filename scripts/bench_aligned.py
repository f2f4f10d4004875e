"""The flow-aligned exposure consistency loss (csrc/correlation.hip, csrc/warp.hip, deblur4dgs_amd/pwcnet.py) against the same
quantities from the fp32 torch restatement tests/pwc_ref.py on the same GPU, at the training shape: a 288x512 frame (padded to
320x512 inside the network), S = 11 sub-samples, 2 (S - 1) = 20 pairs.

  * the cost volume at each pyramid level (B = 20, leaky ReLU 0.1 included on both sides), microseconds per call;
  * the whole batched loss, forward + backward: HIP ops against the same network with corr_fn / warp_fn and the loss restated;
  * the batched pass against a loop of 20 single-pair passes (both HIP).

Device events around windows of `--iters` calls, the two sides alternating, `--rounds` windows each; median and spread of the windows.
The parent commit cannot run this loss at all, so the restatement is the only comparison there is.

    python scripts/bench_aligned.py [--out profiles/aligned_loss.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import pwcnet as P  # noqa: E402
from tests import pwc_ref as R  # noqa: E402  (measurement script only: the torch baseline)

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_aligned.py measures on the GPU; none found")
dev = "cuda:0"
S, H, W = 11, 288, 512
PAIRS = 2 * (S - 1)
LEVELS = {6: (196, 5, 8), 5: (128, 10, 16), 4: (96, 20, 32), 3: (64, 40, 64), 2: (32, 80, 128)}


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n  # microseconds per call


def versus(f_a, f_b, iters, warm=3):
    for _ in range(warm):
        f_a(), f_b()
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(window(f_a, iters))
        tb.append(window(f_b, iters))
    stat = lambda t: {"median": statistics.median(t), "min": min(t), "max": max(t)}
    return stat(ta), stat(tb)


result = {"frame": [H, W], "S": S, "pairs": PAIRS, "iters": a.iters, "rounds": a.rounds, "unit": "us per call", "correlation": {}}
g = torch.Generator().manual_seed(0)
for level, (C, h, w) in LEVELS.items():
    first, second = torch.randn(PAIRS, C, h, w, generator=g).to(dev), torch.randn(PAIRS, C, h, w, generator=g).to(dev)
    hip, ref = versus(lambda: P.correlation(first, second, 0.1), lambda: R.correlation(first, second, 0.1), a.iters)
    rec = {"shape": [PAIRS, C, h, w], "hip_us": hip, "torch_restatement_us": ref,
           "max_abs_diff": float((P.correlation(first, second, 0.1) - R.correlation(first, second, 0.1)).abs().max())}
    result["correlation"][f"level {level}"] = rec
    print("correlation level", level, json.dumps(rec))

torch.manual_seed(0)
net_hip = P.PWCNet(load_pretrained=False).to(dev).eval().requires_grad_(False)
net_ref = P.PWCNet(load_pretrained=False, corr_fn=R.correlation, warp_fn=R.get_backwarp).to(dev).eval().requires_grad_(False)
net_ref.load_state_dict(net_hip.state_dict())
base, _ = R.network_inputs(3, 1, H + 2 * S, W + 2 * S)
rgb = torch.stack([base[0, :, e:e + H, 2 * e:2 * e + W] for e in range(S)])
alpha = 0.2 + 0.8 * torch.rand(S, 1, H, W, generator=g, dtype=torch.float64)
stack = torch.cat([rgb, alpha], 1).permute(0, 2, 3, 1)[:, None].float().contiguous().to(dev)


def restated_loss(x):
    img = x[:, 0, :, :, 0:3].permute(0, 3, 1, 2)
    al = x[:, 0, :, :, 3].detach()
    pred = torch.cat([img[:-1], img[1:]], 0)
    target = torch.cat([img[1:], img[:1].detach().expand(S - 1, -1, -1, -1)], 0)
    mask = torch.cat([al[1:], al[:1].expand(S - 1, -1, -1)], 0)
    with torch.no_grad():
        flow = net_ref(pred, target)
    return R.aligned_l1(pred, flow, target, mask[:, None]).sum() / (S - 1)


def looped_loss(x):
    loss_fn = P.AlignedLoss(net_hip)
    chw = lambda t: t.permute(0, 3, 1, 2)
    total = 0.0
    for e in range(S - 1):
        total = total + loss_fn(chw(x[e:e + 1, 0, :, :, 0:3]), chw(x[e + 1:e + 2, 0, :, :, 0:3]), mask=chw(x[e + 1:e + 2, 0, :, :, 3:4].detach()))
    for e in range(1, S):
        total = total + loss_fn(chw(x[e:e + 1, 0, :, :, 0:3]), chw(x[0:1, 0, :, :, 0:3]).detach(), mask=chw(x[0:1, 0, :, :, 3:4].detach()))
    return total / (S - 1)


def fwd_bwd(fn):
    x = stack.clone().requires_grad_()
    loss = fn(x)
    loss.backward()
    return loss.detach()


batched = lambda: fwd_bwd(lambda x: P.exposure_consistency_loss(x, net_hip))
n = max(2, a.iters // 4)
hip, ref = versus(batched, lambda: fwd_bwd(restated_loss), n)
result["batched_loss_fwd_bwd"] = {"hip_us": hip, "torch_restatement_us": ref, "loss_hip": float(batched()), "loss_restatement": float(fwd_bwd(restated_loss))}
print("batched loss", json.dumps(result["batched_loss_fwd_bwd"]))
hip, loop = versus(batched, lambda: fwd_bwd(looped_loss), n)
result["batched_vs_loop_of_20"] = {"batched_us": hip, "loop_us": loop, "loss_loop": float(fwd_bwd(looped_loss))}
print("batched vs loop", json.dumps(result["batched_vs_loop_of_20"]))
if a.out:
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
