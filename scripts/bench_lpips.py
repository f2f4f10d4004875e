"""LPIPS (csrc/lpips.hip, deblur4dgs_amd/lpips.py) at 1x288x512: one ValidationMetrics(lpips=net).update with the validator's three
masks, and one `distance`, each split into the trunk (MIOpen's five convolutions, deterministic algorithms, one call per side and
mask as the product runs it; beside it the same images as one batch) and the head (everything else); and the head against the same arithmetic composed of torch operations on the device - the formulation of tests/lpips_ref.py
in fp32, mask by mask as three mLPIPS objects would run it - in the same run.  Device events around windows of `--iters` evaluations,
the sides alternating, `--rounds` windows each, after a warm-up; median and spread of the windows.  Launch counts: kernels seen by
torch.profiler in one evaluation.  The trunk's weights are the seeded ones of the tests (timing does not depend on their values).

    python scripts/bench_lpips.py [--out profiles/lpips_times.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd import lpips as hip  # noqa: E402
from deblur4dgs_amd.metrics import ValidationMetrics  # noqa: E402
from tests import lpips_ref as ref  # noqa: E402  (measurement script only: weights and the eager formulation)

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_lpips.py measures on the GPU; none found")
dev = "cuda:0"
H, W = 288, 512


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n  # microseconds per evaluation


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return len([e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()])
    except Exception as e:  # the count is a by-product: report why it is missing
        return f"not measured ({type(e).__name__})"


def line(name, times, n):
    return f"{name:<68s} median {statistics.median(times):9.1f} us   min {min(times):9.1f}   max {max(times):9.1f}   launches {n}"


fx = ref.load_fixture()
net = hip.LPIPS(ref.seeded_trunk(), ref.lins_state(fx)).to(dev)
lins = [getattr(net, f"lin{k}").model[1].weight.reshape(1, -1, 1, 1) for k in range(5)]
shift, scale = (torch.tensor(v, device=dev).view(1, 3, 1, 1) for v in (ref.SHIFT, ref.SCALE))
g = torch.Generator().manual_seed(H)
target = torch.rand(1, H, W, 3, generator=g)
pred = (target + 0.1 * torch.randn(1, H, W, 3, generator=g)).clamp(0, 1).to(dev)
target = target.to(dev)
valid = (torch.rand(1, H, W, generator=g) < 0.9).float()
fg = torch.zeros(1, H, W)
fg[:, H // 4:3 * H // 4, W // 3:2 * W // 3] = 1
valid, fg = valid.to(dev), fg.to(dev)
masks = torch.stack((valid, fg * valid, (1 - fg) * valid))


def trunk(x, calls=1):
    """the five features of x [n,3,H,W], the trunk run in `calls` equal parts (the product: one call per side and mask)"""
    with hip.deterministic_convolutions():
        parts = [net.net(c) for c in x.chunk(calls)]
    return parts[0] if calls == 1 else [torch.cat([p[k] for p in parts]) for k in range(5)]


def hip_prepare(m, normalize):
    return hip.prepare(pred, target, m, normalize)


def hip_tail(feats, m, spatial):
    n = feats[0].shape[0] // 2
    maps = [hip.layer_distance(f[:n], f[n:], w) for f, w in zip(feats, lins)]
    return hip.score(maps, H, W, m)[:2] if spatial else hip.mean_score(maps)


def eager_prepare(m, normalize):
    """the trunk's input as torch composes it, one mask after the other"""
    out = []
    for img in (pred, target):
        for k in range(1 if m is None else m.shape[0]):
            x = img if m is None else img * m[k][..., None]
            x = (2 * x - 1 if normalize else x).permute(0, 3, 1, 2)
            out.append((x - shift) / scale)
    return torch.cat(out)


def eager_tail(feats, m, spatial):
    """normalize_tensor, squared difference, 1x1 convolution, upsample or mean, layer sum, masked sum: fp32 torch operations"""
    n = feats[0].shape[0] // 2
    res = []
    for f, w in zip(feats, lins):
        f0, f1 = f[:n], f[n:]
        g0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
        g1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
        d = F.conv2d((g0 - g1) ** 2, w)
        res.append(F.interpolate(d, scale_factor=(1. * H / d.shape[2], 1. * W / d.shape[3]), mode="bilinear", align_corners=False)
                   if spatial else d.mean([2, 3], keepdim=True))
    val = res[0]
    for r in res[1:]:
        val = val + r
    if not spatial:
        return val.reshape(-1)
    if m is None:
        return val.sum(), torch.tensor(float(H * W), device=dev)
    return [((val[k] * m[k]).sum(), m[k].sum().to(torch.int64)) for k in range(m.shape[0])]


lines = [f"LPIPS at 1x{H}x{W} (fp32), iters {a.iters} per window, {a.rounds} windows; microseconds per evaluation", ""]
with torch.no_grad():
    vm = ValidationMetrics(lpips=net)
    f_update = lambda: (vm.reset(), vm.update(pred, target, valid, fg))
    f_six = lambda: ValidationMetrics().update(pred, target, valid, fg)
    f_dist = lambda: net.distance(pred, target, normalize=True)
    cases = {}
    for name, m, spatial in (("update (three masks, spatial)", masks, True), ("distance (no mask, mean)", None, False)):
        x = hip_prepare(m, True)
        x = x.reshape(-1, 3, H, W)
        feats = [f.contiguous() for f in trunk(x, x.shape[0])]
        cases[name] = (m, spatial, x, feats)
    for _ in range(5):  # warm-up: MIOpen's choices, the allocator
        f_update(), f_six(), f_dist()
        for m, spatial, x, feats in cases.values():
            trunk(x, x.shape[0]), trunk(x), hip_prepare(m, True), hip_tail(feats, m, spatial), eager_prepare(m, True), eager_tail(feats, m, spatial)
    torch.cuda.synchronize()
    # the two heads agree
    m, spatial, x, feats = cases["update (three masks, spatial)"]
    hs, es = hip_tail(feats, m, True), eager_tail(feats, m, True)
    gap = max(abs(float(hs[0][k, 0]) - float(es[k][0])) / float(hs[0][k, 0]) for k in range(3))
    lines.append(f"largest relative difference of the three masked sums, HIP head against the torch composition: {gap:.2e}")
    lines.append(f"trunk input identical: {torch.equal(hip_prepare(m, True).reshape(-1, 3, H, W), eager_prepare(m, True))}")
    lines.append("")
    rows = {"ValidationMetrics(lpips=net).update, three masks": f_update, "ValidationMetrics().update (the six old numbers)": f_six,
            "LPIPS.distance": f_dist}
    for name, (m, spatial, x, feats) in cases.items():
        rows[f"{name}: trunk, one call per side and mask"] = lambda x=x: trunk(x, x.shape[0])
        rows[f"{name}: trunk, all images one batch (not used)"] = lambda x=x: trunk(x)
        rows[f"{name}: head, HIP"] = lambda m=m, s=spatial, f=feats: (hip_prepare(m, True), hip_tail(f, m, s))
        rows[f"{name}: head, torch composition"] = lambda m=m, s=spatial, f=feats: (eager_prepare(m, True), eager_tail(f, m, s))
    times = {k: [] for k in rows}
    for _ in range(a.rounds):
        for k, fn in rows.items():
            times[k].append(window(fn, a.iters))
    for k, fn in rows.items():
        lines.append(line(k, times[k], launches(fn)))
    lines.append("")
    for name in cases:
        h, e = statistics.median(times[f"{name}: head, HIP"]), statistics.median(times[f"{name}: head, torch composition"])
        lines.append(f"{name}: torch composition / HIP head = {e / h:.2f}")
text = "\n".join(lines) + "\n"
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text)
