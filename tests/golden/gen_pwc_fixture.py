"""Fixture of the flow-aligned loss: what the REFERENCE's own get_backwarp, AlignedLoss.forward arithmetic, Network and PWCNet wrapper
(flow3d/models/pwcnet.py, flow3d/loss_utils.py) give for small inputs on the CPU.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_pwc_fixture.py   ->  tests/golden/pwc.npz

Only data travels: the arrays below.  The reference's cost volume is CUDA C compiled through cupy and has no CPU path, so its
module is stubbed with the restatement tests/pwc_ref.correlation (81 shifted products); everything else - the architecture, the
warp, the wrapper's resizing, the loss arithmetic - is the reference's code, executed.  AlignedLoss.__init__ loads a pretrained blob
that is not part of the checkout, so the class body is taken from loss_utils.py and an instance is made without running __init__.

Records: (a) get_backwarp and the loss with gradients for explicit flows; (b) names and shapes of Network().state_dict();
(c) Network and wrapper flows in fp64 under the seeded weights of tests/pwc_ref.seeded_state; (d) the relative error of the same
reference network run in fp32 on this CPU against its fp64 run."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import pwc_ref as R  # noqa: E402

UP = 1.7  # upstream factor of the recorded gradients


def load_reference():
    root = os.environ["D4GS_REFERENCE"]
    stub = types.ModuleType("flow3d.models.external.pwcnet.correlation")
    stub.correlation = types.SimpleNamespace(FunctionCorrelation=lambda tenFirst, tenSecond: R.correlation(tenFirst, tenSecond))
    for name in ("flow3d", "flow3d.models", "flow3d.models.external", "flow3d.models.external.pwcnet"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["flow3d.models.external.pwcnet.correlation"] = stub
    pwc = {"__name__": "reference_pwcnet"}
    exec(compile(open(os.path.join(root, "flow3d", "models", "pwcnet.py")).read(), "reference_pwcnet", "exec"), pwc)
    src = open(os.path.join(root, "flow3d", "loss_utils.py")).read()
    body = src[src.index("class AlignedLoss"):src.index("def normalize_batch")]
    ns = {"torch": torch, "nn": torch.nn, "PWCNet": pwc["PWCNet"], "get_backwarp": pwc["get_backwarp"], "__name__": "reference_loss"}
    exec(compile(body, "reference_aligned_loss", "exec"), ns)
    return pwc, ns["AlignedLoss"]


def aligned_loss_with(AlignedLoss, alignnet):
    obj = AlignedLoss.__new__(AlignedLoss)
    torch.nn.Module.__init__(obj)
    obj.lrec = torch.nn.L1Loss()
    obj.alignnet = alignnet
    return obj


def warp_cases():
    """[2,3,6,9]; flows that leave the image on every side (and stay inside elsewhere)"""
    g = torch.Generator().manual_seed(611)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    B, H, W = 2, 6, 9
    pred, target = r(B, 3, H, W), r(B, 3, H, W)
    flow = 3.0 * (r(B, 2, H, W) - 0.5)
    flow[0, 0, :, :2] -= 4.0   # out on the left
    flow[0, 0, :, -2:] += 4.0  # on the right
    flow[1, 1, :2] -= 4.0      # at the top
    flow[1, 1, -2:] += 4.0     # at the bottom
    flow[1, :, 2, 3] = 0.0     # one exact identity sample
    mask = r(B, 1, H, W)
    return pred, target, flow, mask


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    pwc, AlignedLoss = load_reference()
    arrays = {}
    # the reference builds its sampling grid with torch.linspace in the DEFAULT dtype and caches it by shape: fp64 runs need the
    # default to be fp64, and the cache emptied before the fp32 runs
    torch.set_default_dtype(torch.float64)
    # (a)
    pred, target, flow, mask = warp_cases()
    warped, fmask = pwc["get_backwarp"](pred.clone(), flow.clone())
    arrays.update({"a/pred": pred, "a/target": target, "a/flow": flow, "a/mask": mask, "a/warped": warped, "a/flow_mask": fmask})
    assert 0 < float(fmask.mean()) < 1
    for tag, m in (("masked", mask), ("plain", None)):
        p, t = pred.clone().requires_grad_(), target.clone().requires_grad_()
        loss = aligned_loss_with(AlignedLoss, lambda a, b: flow.clone())(p, t, mask=m)
        (UP * loss).backward()
        arrays.update({f"a/{tag}/loss": loss.detach(), f"a/{tag}/pred_grad": p.grad, f"a/{tag}/target_grad": t.grad})
    # (b), (c), (d)
    torch.manual_seed(0)
    net = pwc["Network"]().double()
    names_shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    arrays["b/names"] = np.array([k for k, _ in names_shapes])
    arrays["b/shapes"] = np.array([list(s) + [0] * (4 - len(s)) for _, s in names_shapes], dtype=np.int64)
    state = R.seeded_state(names_shapes)
    arrays["c/checksum"] = np.array(R.checksum(state))
    net.load_state_dict(state)
    net.eval()
    wrapper = pwc["PWCNet"](load_pretrained=False).double()
    wrapper.net.load_state_dict(state)
    wrapper.eval()
    first, second = R.network_inputs(1, 2, 64, 64)
    src, tgt = R.network_inputs(2, 1, 48, 80)
    with torch.no_grad():
        flow64 = net(first, second)
        wflow64 = wrapper(src, tgt)
        torch.set_default_dtype(torch.float32)
        pwc["backwarp_tenGrid"].clear(), pwc["backwarp_tenPartial"].clear()
        flow32 = net.float()(first.float(), second.float()).double()
        wflow32 = wrapper.float()(src.float(), tgt.float()).double()
    for name, f in (("network", flow64), ("wrapper", wflow64)):
        top = float(f.abs().max())
        print(f"{name} flow: max |f| {top:.4g}, shape {tuple(f.shape)}", file=sys.stderr)
        assert 1e-2 <= top <= 1e2, (name, top)
    arrays.update({"c/first": first, "c/second": second, "c/flow": flow64, "c/source": src, "c/target": tgt, "c/wrapper_flow": wflow64})
    arrays["d/flow_fp32_err"] = np.array(float((flow32 - flow64).abs().max() / flow64.abs().max()))
    arrays["d/wrapper_flow_fp32_err"] = np.array(float((wflow32 - wflow64).abs().max() / wflow64.abs().max()))
    print("fp32 errors:", float(arrays["d/flow_fp32_err"]), float(arrays["d/wrapper_flow_fp32_err"]), file=sys.stderr)
    out = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in arrays.items()}
    dst = os.path.join(HERE, "pwc.npz")
    np.savez_compressed(dst, **out)
    print(f"{len(out)} arrays -> {dst} ({os.path.getsize(dst)} bytes)", file=sys.stderr)
