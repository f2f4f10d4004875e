"""Fixture of the validator's masked PSNR and SSIM: small images and masks, and what the REFERENCE's own mPSNR and mSSIM
(flow3d/metrics.py) return for them in float32 on the CPU.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_metrics.py   ->  tests/golden/metrics.npz

flow3d/metrics.py is loaded from its file under stubs of `torchmetrics`, which is not installed here.  The stubs carry no arithmetic:
the base class `Metric` with `add_state` and `reset`, `PeakSignalNoiseRatio`, and `StructuralSimilarityIndexMeasure` with
torchmetrics' defaults kernel_size=11, sigma=1.5, k1=0.01, k2=0.03 and its list state `similarity`; `dim_zero_cat`, and the two names
the LPIPS class imports.  Every number recorded comes out of the reference's own `update` and `compute`.  Only arrays travel.

Shapes (B,H,W): (1,11,11) one output pixel; (1,26,26) 16 output columns exactly; (2,27,38) 17 output rows, a partial second tile,
two images; (1,43,27); (1,64,48).  Images, fp32: `uniform` (pred and target independent uniform), `flat` (target 0.9 + 0.002 u,
pred 0.9 + 0.002 u' + 0.05 (u'' - 0.5): variances ~1e-6 and ~2e-4 beside means ~0.9), `same` (pred == target == the uniform pred).
Masks: `none`, `ones`, `zero`, `blob` (ones on the image less a 2-pixel border and less a centred hole 13 wide where the image
allows - whole windows are empty inside it), `rows` (every third row zero: its horizontal windows are empty, the vertical ones
over them are not; on wide images the last 12 columns of the even rows are zero too), `bernoulli` (0.7), `dyadic` (0, 0.5, 1).
`validator`: three masks valid, fg * valid, (1 - fg) * valid on the largest shape (flow3d/validator.py:460-475).  `sequence`: three
updates of one mPSNR and one mSSIM, and their compute().

The archive also holds the largest gap between the reference's fp32 results and tests/metrics_ref.py in fp64 over these cases
(`ref_gap_ssim` absolute, `ref_gap_sse_rel` relative, and each per image kind as `ref_gap_ssim/<kind>`: the flat images set the
largest, fp32's cancellation in E[x^2] - mu^2 divided by c2): tests/test_metrics_ref.py allows ten times the gap of the case's kind.  Fixed zip timestamps:
the same generator gives the same bytes."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_motion_regs import write_npz  # noqa: E402

SHAPES = ((1, 11, 11), (1, 26, 26), (2, 27, 38), (1, 43, 27), (1, 64, 48))
IMAGES = ("uniform", "flat", "same")
MASKS = ("none", "ones", "zero", "blob", "rows", "bernoulli", "dyadic")


def shape_name(s):
    return "x".join(str(v) for v in s)


def import_reference_metrics(ref_root):
    class Metric:
        def __init__(self, **kwargs):
            self._defaults = {}

        def add_state(self, name, default, dist_reduce_fx=None):
            self._defaults[name] = default
            setattr(self, name, list(default) if isinstance(default, list) else default.clone())

        def reset(self):
            for name, default in self._defaults.items():
                setattr(self, name, list(default) if isinstance(default, list) else default.clone())

    class PeakSignalNoiseRatio(Metric):
        def __init__(self, data_range=None, base=10.0, reduction="elementwise_mean", dim=None, **kwargs):
            super().__init__(**kwargs)
            self.data_range, self.base, self.reduction, self.dim = data_range, base, reduction, dim

    class StructuralSimilarityIndexMeasure(Metric):
        def __init__(self, gaussian_kernel=True, sigma=1.5, kernel_size=11, reduction="elementwise_mean", data_range=None, k1=0.01,
                     k2=0.03, return_full_image=False, **kwargs):
            super().__init__(**kwargs)
            self.sigma, self.kernel_size, self.reduction, self.data_range, self.k1, self.k2 = sigma, kernel_size, reduction, data_range, k1, k2
            self.add_state("similarity", default=[], dist_reduce_fx="cat")

    def dim_zero_cat(x):
        return torch.cat([v[None] if v.dim() == 0 else v for v in x], 0)

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    module("torchmetrics")
    module("torchmetrics.functional")
    module("torchmetrics.functional.image")
    module("torchmetrics.functional.image.lpips", _NoTrainLpips=None)
    module("torchmetrics.image", PeakSignalNoiseRatio=PeakSignalNoiseRatio, StructuralSimilarityIndexMeasure=StructuralSimilarityIndexMeasure)
    module("torchmetrics.metric", Metric=Metric)
    module("torchmetrics.utilities", dim_zero_cat=dim_zero_cat)
    module("torchmetrics.utilities.imports", _TORCHVISION_AVAILABLE=False)
    spec = importlib.util.spec_from_file_location("reference_flow3d_metrics", os.path.join(ref_root, "flow3d", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda: torch.rand(*shape, 3, generator=g, dtype=torch.float32)
    out = {"uniform/pred": u(), "uniform/target": u()}
    out["flat/target"] = 0.9 + 0.002 * u()
    out["flat/pred"] = 0.9 + 0.002 * u() + 0.05 * (u() - 0.5)
    return out


def make_masks(shape, seed):
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    out = {"ones": torch.ones(B, H, W), "zero": torch.zeros(B, H, W)}
    blob = torch.zeros(B, H, W)
    blob[:, 2:H - 2, 2:W - 2] = 1
    hh, hw = min(13, H - 8), min(13, W - 8)
    y0, x0 = (H - hh) // 2, (W - hw) // 2
    blob[:, y0:y0 + hh, x0:x0 + hw] = 0
    out["blob"] = blob
    rows = torch.ones(B, H, W)
    rows[:, 1::3] = 0
    if W >= 24:
        rows[:, 0::2, W - 12:] = 0
    out["rows"] = rows
    out["bernoulli"] = (torch.rand(B, H, W, generator=g) < 0.7).float()
    out["dyadic"] = torch.randint(0, 3, (B, H, W), generator=g).float() / 2
    return out


def images_of(arrays, sname, kind):
    if kind == "same":
        return arrays[f"{sname}/uniform/pred"], arrays[f"{sname}/uniform/pred"]
    return arrays[f"{sname}/{kind}/pred"], arrays[f"{sname}/{kind}/target"]


def validator_masks(g):
    B, H, W = SHAPES[-1]
    valid = (torch.rand(B, H, W, generator=g) < 0.9).float()
    valid[:, :3] = 0
    fg = torch.zeros(B, H, W)
    fg[:, 20:47, 9:31] = 1
    return valid, fg


def reference_values(ref, pred, target, mask):
    """-> (sse, total, psnr, ssim per image) from the reference's own classes, one update"""
    ps, ss = ref.mPSNR(), ref.mSSIM()
    ps.update(pred, target, mask)
    ss.update(pred, target, mask)
    return ps.sum_squared_error[0], ps.total[0], ps.compute(), ss.similarity[0]


if __name__ == "__main__":
    from tests import metrics_ref as R

    ref = import_reference_metrics(os.environ["D4GS_REFERENCE"])
    arrays, gap_ssim, gap_sse = {}, {k: 0.0 for k in IMAGES}, {k: 0.0 for k in IMAGES}

    def record(name, kind, pred, target, mask):
        with torch.no_grad():
            sse, total, psnr, ssim = reference_values(ref, pred, target, mask)
            r_sse, r_msum, r_ssim = R.masked_image_metrics(pred, target, mask)
        arrays[f"{name}/sse"], arrays[f"{name}/total"] = sse.numpy(), total.numpy()
        arrays[f"{name}/psnr"], arrays[f"{name}/ssim"] = psnr.numpy(), ssim.numpy()
        assert sse.dtype == torch.float32 and ssim.dtype == torch.float32 and total.dtype == torch.int64
        gap_ssim[kind] = max(gap_ssim[kind], float((ssim.double() - r_ssim[0]).abs().max()))
        if float(r_sse.sum()) > 0:
            gap_sse[kind] = max(gap_sse[kind], abs(float(sse) - float(r_sse.sum())) / float(r_sse.sum()))
        else:
            assert float(sse) == 0.0
        assert int(total) == int(torch.trunc(r_msum.sum())) * 3
        return sse, total, psnr, ssim

    for si, shape in enumerate(SHAPES):
        sname = shape_name(shape)
        for k, v in make_images(shape, 1000 + si).items():
            arrays[f"{sname}/{k}"] = v.numpy()
        for k, v in make_masks(shape, 2000 + si).items():
            arrays[f"{sname}/mask/{k}"] = v.numpy()
        for kind in IMAGES:
            pred, target = (torch.from_numpy(a) for a in images_of(arrays, sname, kind))
            for mk in MASKS:
                mask = None if mk == "none" else torch.from_numpy(arrays[f"{sname}/mask/{mk}"])
                sse, total, psnr, ssim = record(f"{sname}/{kind}/{mk}", kind, pred, target, mask)
                if kind == "same" or mk == "zero":  # exact: SSIM 1 and SSE 0 (and no pixel counted under the zero mask)
                    assert bool((ssim == 1).all()) and float(sse) == 0.0 and (mk != "zero" or int(total) == 0), (sname, kind, mk)

    # the validator's three masks on the largest shape
    sname = shape_name(SHAPES[-1])
    g = torch.Generator().manual_seed(3000)
    valid, fg = validator_masks(g)
    arrays["validator/valid_mask"], arrays["validator/fg_mask"] = valid.numpy(), fg.numpy()
    pred, target = (torch.from_numpy(a) for a in images_of(arrays, sname, "uniform"))
    for key, m in (("main", valid), ("fg", fg * valid), ("bg", (1 - fg) * valid)):
        record(f"validator/{key}", "uniform", pred, target, m)

    # three updates of one metric each, then compute(): shapes 27x38 (two images), 43x27, 64x48
    ps, ss = ref.mPSNR(), ref.mSSIM()
    steps = ((shape_name(SHAPES[2]), "uniform", "bernoulli"), (shape_name(SHAPES[3]), "flat", "none"), (shape_name(SHAPES[4]), "uniform", "blob"))
    arrays["sequence/steps"] = np.array(["/".join(s) for s in steps])
    with torch.no_grad():
        for sname, kind, mk in steps:
            pred, target = (torch.from_numpy(a) for a in images_of(arrays, sname, kind))
            mask = None if mk == "none" else torch.from_numpy(arrays[f"{sname}/mask/{mk}"])
            ps.update(pred, target, mask)
            ss.update(pred, target, mask)
        assert len(ps) == 3 and len(ss) == 4
        arrays["sequence/psnr"], arrays["sequence/ssim"] = ps.compute().numpy(), ss.compute().numpy()
    assert gap_ssim["same"] == 0.0 and gap_sse["same"] == 0.0
    arrays["ref_gap_ssim"], arrays["ref_gap_sse_rel"] = np.float64(max(gap_ssim.values())), np.float64(max(gap_sse.values()))
    for k in IMAGES:  # per image kind: the flat images set the largest gap (fp32 cancellation in E[x^2] - mu^2, divided by c2)
        arrays[f"ref_gap_ssim/{k}"], arrays[f"ref_gap_sse_rel/{k}"] = np.float64(gap_ssim[k]), np.float64(gap_sse[k])
    dst = os.path.join(HERE, "metrics.npz")
    write_npz(dst, arrays)
    print(f"{len(arrays)} arrays -> {dst} ({os.path.getsize(dst)} bytes); fp32 reference against the fp64 restatement: SSIM {gap_ssim} "
          f"absolute, SSE {gap_sse} relative", file=sys.stderr)
