"""Fixture of the LPIPS metric: small images and masks, and what the REFERENCE's own PNetLin(pnet_type='alex', version='0.1')
(models/networks_basic.py) and mLPIPS (flow3d/metrics.py) return for them on the CPU in float64.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_lpips.py   ->  tests/golden/lpips.npz

The reference's `models` package is imported from the checkout under stubs that carry no LPIPS arithmetic: `skimage`, `skimage.color`,
`skimage.measure` and `skimage.transform` are empty modules, `tqdm` is stubbed if absent, and `torchvision.models.alexnet` returns an
object whose `features` is a plain nn.Sequential of the thirteen standard layers.  PNetLin is built with pnet_rand=True, use_dropout=True
and .eval(); the reference's `models/weights/v0.1/alex.pth` (the five head weights) is loaded with strict=False, and the trunk is
tests/lpips_ref.py::seeded_trunk() - a trained AlexNet is about 10 MB and no part of this repository.  flow3d/metrics.py is loaded as
tests/golden/gen_metrics.py loads it; its `_NoTrainLpips` (torchmetrics', not installed) is replaced by an adaptor that holds the
reference's PNetLin(spatial=True) and applies `2 x - 1` for normalize=True, so that mLPIPS.update itself produces every entry.

Shapes (B,H,W): (1,31,31) the deep maps are 1x1; (1,35,35); (2,47,64); (1,64,99).  Images, fp32 in [0, 1]: `uniform` (pred uniform,
target = pred + 0.1 normal noise, clamped: no cancellation magnifies the trunk's rounding) and `same` (target == pred).  Masks: `none`,
`ones`, `zero`, `bernoulli` (0.7), `dyadic` (0, 0.5, 1), and the validator's three on (2,47,64) (flow3d/validator.py:460-475).

Recorded, all float64 from the reference run in double: per shape and image kind `map` [B,H,W] (spatial=True) and `mean` [B]
(spatial=False) of the images scaled to [-1, 1], and the five layer maps `layer{k}` [B,h,w] (PNetLin returns them only upsampled or
averaged, so they are put together from its own parts: scaling_layer, net, models.normalize_tensor and lin{k}.model); per
mask `sum` and `total` of one mLPIPS update; `sequence/*`: three updates of one mLPIPS, their entries and the mean of the ratios.
`lin{k}`: the head weights.  `trunk_checksum`.  `ref_gap_map`, `ref_gap_mean`: the largest gap, relative to the largest recorded value
of the case, between the reference's float32 run and its float64 run.  Only arrays travel.  Fixed zip timestamps: the same generator
gives the same bytes."""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_metrics import import_reference_metrics  # noqa: E402
from gen_motion_regs import write_npz  # noqa: E402


def import_reference_models(ref_root):
    for name in ("skimage", "skimage.color", "skimage.measure", "skimage.transform"):
        sys.modules.setdefault(name, types.ModuleType(name))
    for sub in ("color", "measure", "transform"):
        setattr(sys.modules["skimage"], sub, sys.modules[f"skimage.{sub}"])
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.ModuleType("tqdm")
        sys.modules["tqdm"].tqdm = lambda it, *a, **k: it

    def alexnet(pretrained=False, **kwargs):
        net = types.SimpleNamespace()
        net.features = nn.Sequential(
            nn.Conv2d(3, 64, 11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
            nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
            nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2))
        return net

    tv, tvm = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    tvm.alexnet, tv.models = alexnet, tvm
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tvm
    sys.path.insert(0, ref_root)
    from models import networks_basic

    return networks_basic


def reference_net(nb, ref_root, trunk, spatial, dtype):
    net = nb.PNetLin(pnet_type="alex", pnet_rand=True, spatial=spatial, use_dropout=True, version="0.1").eval()
    heads = torch.load(os.path.join(ref_root, "models", "weights", "v0.1", "alex.pth"), map_location="cpu")
    missing = net.load_state_dict(heads, strict=False)
    assert not missing.unexpected_keys and all(k.startswith(("net.", "scaling_layer.")) for k in missing.missing_keys), missing
    slices = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}
    own = {f"net.slice{slices[int(k.split('.')[1])]}.{k.split('.', 1)[1]}": v for k, v in trunk.items()}
    rest = net.load_state_dict(own, strict=False)
    assert not rest.unexpected_keys and all(k.startswith(("lin", "scaling_layer.")) for k in rest.missing_keys), rest
    return net.to(dtype)


if __name__ == "__main__":
    from tests import lpips_ref as R

    ref_root = os.environ["D4GS_REFERENCE"]
    nb = import_reference_models(ref_root)
    trunk = R.seeded_trunk()
    nets = {(sp, dt): reference_net(nb, ref_root, trunk, sp, dt) for sp in (True, False) for dt in (torch.float32, torch.float64)}
    arrays = {"trunk_checksum": np.array(R.checksum(trunk))}
    for k in range(5):
        w = getattr(nets[True, torch.float64], f"lin{k}").model[1].weight
        arrays[f"lin{k}"] = w.detach().float().reshape(-1).numpy()
        assert float(w.min()) >= 0
    print("head weight maxima:", [float(arrays[f"lin{k}"].max()) for k in range(5)], file=sys.stderr)

    class Adaptor(nn.Module):  # stands where torchmetrics' _NoTrainLpips stood: the reference's own network, spatial
        dtype = torch.float64

        def __init__(self, net="alex", spatial=True):
            super().__init__()
            assert net == "alex" and spatial

        def forward(self, in0, in1, normalize=False):
            if normalize:
                in0, in1 = 2 * in0 - 1, 2 * in1 - 1
            return nets[True, self.dtype](in0, in1)

    metrics = import_reference_metrics(ref_root)
    metrics._NoTrainLpips, metrics._TORCHVISION_AVAILABLE = Adaptor, True

    def update(metric, pred, target, mask, dtype):
        Adaptor.dtype = dtype
        metric.update(pred.to(dtype), target.to(dtype), None if mask is None else mask.to(dtype))

    gap = {"map": 0.0, "mean": 0.0}

    def note(kind, lo, hi):
        if float(hi.abs().max()) > 0:
            gap[kind] = max(gap[kind], float((lo.double() - hi).abs().max() / hi.abs().max()))
        else:
            assert float(lo.abs().max()) == 0

    with torch.no_grad():
        for si, shape in enumerate(R.SHAPES):
            B, H, W = shape
            sname = R.shape_name(shape)
            g = torch.Generator().manual_seed(4000 + si)
            pred = torch.rand(B, H, W, 3, generator=g, dtype=torch.float32)
            target = (pred + 0.1 * torch.randn(B, H, W, 3, generator=g, dtype=torch.float32)).clamp(0, 1)
            arrays[f"{sname}/pred"], arrays[f"{sname}/target"] = pred.numpy(), target.numpy()
            arrays[f"{sname}/mask/bernoulli"] = (torch.rand(B, H, W, generator=g) < 0.7).float().numpy()
            arrays[f"{sname}/mask/dyadic"] = (torch.randint(0, 3, (B, H, W), generator=g).float() / 2).numpy()
            for kind in R.IMAGES:
                p, t = R.images_of(arrays, sname, kind)
                out = {}
                for dt in (torch.float32, torch.float64):
                    x0, x1 = (2 * v.to(dt).permute(0, 3, 1, 2) - 1 for v in (p, t))
                    smap = nets[True, dt](x0, x1)[:, 0]
                    mean, layers = nets[False, dt](x0, x1, retPerLayer=True)
                    # the per-layer maps, from the network's own parts.  (retPerLayer's entry 0 is overwritten by the total: `val += `)
                    per_layer = nets[True, dt].net.forward(nets[True, dt].scaling_layer(x0)), nets[True, dt].net.forward(nets[True, dt].scaling_layer(x1))
                    maps = [getattr(nets[True, dt], f"lin{k}").model(
                        (sys.modules["models"].normalize_tensor(a) - sys.modules["models"].normalize_tensor(b)) ** 2)[:, 0]
                        for k, (a, b) in enumerate(zip(*per_layer))]
                    for k, lm in list(enumerate(maps))[1:]:
                        assert torch.equal(lm.mean((1, 2)), layers[k].reshape(-1)) or torch.allclose(lm.mean((1, 2)), layers[k].reshape(-1), rtol=1e-6, atol=0)
                    out[dt] = (smap, mean.reshape(-1), maps)
                smap, mean, maps = out[torch.float64]
                assert [tuple(m.shape[1:]) for m in maps] == list(R.alex_sizes(H, W))
                note("map", out[torch.float32][0], smap)
                note("mean", out[torch.float32][1], mean)
                arrays[f"{sname}/{kind}/map"], arrays[f"{sname}/{kind}/mean"] = smap.numpy(), mean.numpy()
                for k, lm in enumerate(maps):
                    arrays[f"{sname}/{kind}/layer{k}"] = lm.numpy()
                if kind == "same":
                    assert float(smap.abs().max()) == 0 and float(mean.abs().max()) == 0 and float(out[torch.float32][0].abs().max()) == 0
                for mk in R.MASKS:
                    mask = R.mask_of(arrays, sname, mk)
                    vals = {}
                    for dt in (torch.float32, torch.float64):
                        one = metrics.mLPIPS()
                        update(one, p, t, mask, dt)
                        vals[dt] = (one.sum_scores[0], one.total[0])
                    assert vals[torch.float64][1].dtype == torch.int64 and int(vals[torch.float32][1]) == int(vals[torch.float64][1])
                    note("map", vals[torch.float32][0], vals[torch.float64][0])
                    arrays[f"{sname}/{kind}/{mk}/sum"], arrays[f"{sname}/{kind}/{mk}/total"] = vals[torch.float64][0].numpy(), vals[torch.float64][1].numpy()
                    if kind == "same" or mk == "zero":
                        assert float(vals[torch.float64][0]) == 0 and float(vals[torch.float32][0]) == 0

        # the validator's three masks on (2,47,64)
        B, H, W = R.VALIDATOR_SHAPE
        sname = R.shape_name(R.VALIDATOR_SHAPE)
        g = torch.Generator().manual_seed(5000)
        valid = (torch.rand(B, H, W, generator=g) < 0.9).float()
        valid[:, :3] = 0
        fg = torch.zeros(B, H, W)
        fg[:, 14:36, 9:40] = 1
        arrays["validator/valid_mask"], arrays["validator/fg_mask"] = valid.numpy(), fg.numpy()
        p, t = R.images_of(arrays, sname, "uniform")
        for key, m in R.validator_masks(arrays)[2].items():
            one = metrics.mLPIPS()
            update(one, p, t, m, torch.float64)
            arrays[f"validator/{key}/sum"], arrays[f"validator/{key}/total"] = one.sum_scores[0].numpy(), one.total[0].numpy()

        # three updates of one metric, then compute()
        steps = ((R.shape_name(R.SHAPES[2]), "uniform", "bernoulli"), (R.shape_name(R.SHAPES[1]), "uniform", "none"),
                 (R.shape_name(R.SHAPES[3]), "uniform", "dyadic"))
        arrays["sequence/steps"] = np.array(["/".join(s) for s in steps])
        seq = {dt: metrics.mLPIPS() for dt in (torch.float32, torch.float64)}
        for dt, one in seq.items():
            one.device = "cpu"
            for sname, kind, mk in steps:
                update(one, *R.images_of(arrays, sname, kind), R.mask_of(arrays, sname, mk), dt)
            assert len(one) == 3
        hi = seq[torch.float64]
        arrays["sequence/sums"], arrays["sequence/totals"] = torch.stack(hi.sum_scores).numpy(), torch.stack(hi.total).numpy()
        arrays["sequence/compute"] = (torch.stack(hi.sum_scores) / torch.stack(hi.total)).mean().numpy()
        # the reference's own compute() builds float32 tensors from the entries: the same number to float32
        for one in seq.values():
            assert abs(float(one.compute()) - float(arrays["sequence/compute"])) <= 4e-6 * float(arrays["sequence/compute"])
    arrays["ref_gap_map"], arrays["ref_gap_mean"] = np.float64(gap["map"]), np.float64(gap["mean"])
    dst = os.path.join(HERE, "lpips.npz")
    write_npz(dst, arrays)
    print(f"{len(arrays)} arrays -> {dst} ({os.path.getsize(dst)} bytes); float32 reference against its float64 run: {gap}", file=sys.stderr)
