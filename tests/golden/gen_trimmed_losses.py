"""Fixture of the quantile-trimmed losses: small inputs, and the losses and `pred` gradients that the REFERENCE's own
masked_l1_loss / trimmed_l1_loss / compute_gradient_loss (flow3d/loss_utils.py) give for them in float64 on the CPU.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_trimmed_losses.py   ->  tests/golden/trimmed_losses.npz

Only data travels: the arrays below.  flow3d/loss_utils.py imports PWC-Net (cupy) further down, so the functions are taken from
the part of the file above that import; scikit-learn (used by an unrelated helper there) is stubbed when it is not installed."""
import os
import sys
import types

import numpy as np
import torch


def load_reference():
    src = open(os.path.join(os.environ["D4GS_REFERENCE"], "flow3d", "loss_utils.py")).read()
    head = src[:src.index("from flow3d.models.pwcnet")]
    try:
        import sklearn.neighbors  # noqa: F401
    except ImportError:
        stub = types.ModuleType("sklearn.neighbors")
        stub.NearestNeighbors = None
        sys.modules.setdefault("sklearn", types.ModuleType("sklearn"))
        sys.modules["sklearn.neighbors"] = stub
    ns = {}
    exec(compile(head, "loss_utils_head", "exec"), ns)
    return ns


def cases():
    """name -> (function name, inputs, keyword arguments).  Continuous random values: no ties at the threshold."""
    g = torch.Generator().manual_seed(20240)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    out = {}
    gt, pred = r(5, 6, 3), r(5, 6, 3)
    mask = (r(5, 6, 1) > 0.3).double()
    weights = r(5, 6, 1)
    out["masked_normalized"] = ("masked_l1_loss", dict(pred=pred, gt=gt, mask=mask), dict(normalize=True, quantile=0.98))
    out["masked_weights_normalized"] = ("masked_l1_loss", dict(pred=pred, gt=gt, mask=weights), dict(normalize=True, quantile=0.9))
    out["masked_mean"] = ("masked_l1_loss", dict(pred=pred, gt=gt, mask=mask), dict(normalize=False, quantile=0.8))
    out["no_mask"] = ("masked_l1_loss", dict(pred=pred, gt=gt), dict(quantile=0.75))
    out["trimmed_default"] = ("trimmed_l1_loss", dict(pred=r(23, 2), gt=r(23, 2)), dict())
    out["masked_quantile_1"] = ("masked_l1_loss", dict(pred=pred, gt=gt, mask=mask), dict(quantile=1.0))
    out["no_mask_quantile_1"] = ("masked_l1_loss", dict(pred=pred, gt=gt), dict(quantile=1.0))
    B, H, W = 2, 5, 6
    ragged = r(B, H, W) > 0.35
    ragged[0, 2, :] = False  # a whole row out, and a corner
    ragged[1, :2, :2] = False
    out["gradient_ragged_bool"] = ("compute_gradient_loss", dict(pred=r(B, H, W, 1), gt=r(B, H, W, 1), mask=ragged), dict(quantile=0.95))
    out["gradient_ragged_3d"] = ("compute_gradient_loss", dict(pred=r(B, H, W), gt=r(B, H, W), mask=ragged), dict(quantile=0.6))
    return out


if __name__ == "__main__":
    ref = load_reference()
    arrays = {}
    for name, (fn, inputs, kw) in cases().items():
        pred = inputs["pred"].clone().requires_grad_()
        args = {k: v for k, v in inputs.items() if k != "pred"}
        loss = ref[fn](pred, **args, **kw)
        (1.7 * loss).backward()  # an upstream factor: the gradient is not just the loss's own
        for k, v in inputs.items():
            arrays[f"{name}/{k}"] = v.numpy()
        arrays[f"{name}/loss"] = loss.detach().numpy()
        arrays[f"{name}/pred_grad"] = pred.grad.numpy()
        print(name, float(loss.detach()), file=sys.stderr)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trimmed_losses.npz")
    np.savez_compressed(dst, **arrays)
    print(f"{len(arrays)} arrays -> {dst} ({os.path.getsize(dst)} bytes)", file=sys.stderr)
