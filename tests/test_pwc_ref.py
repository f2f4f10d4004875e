"""tests/pwc_ref.py (the yardstick of tests/test_gpu_pwc.py) and the product's Network / PWCNet topology against values recorded
from the reference's own code (tests/golden/pwc.npz, written by tests/golden/gen_pwc_fixture.py).  No GPU: the product network runs
on the CPU with corr_fn / warp_fn set to the restatements, which is what those arguments are for."""
import os

import numpy as np
import pytest
import torch

from tests import pwc_ref as R

UP = 1.7
F64 = torch.float64


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "pwc.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind == "f" else z[k]) for k in z.files}


def close(got, want, tol, what):
    err = float((got - want).abs().max())
    print(what, "max abs err", err, "max |want|", float(want.abs().max()))
    assert err <= tol * max(1.0, float(want.abs().max())), (what, err)


def test_backwarp_restatement_matches_the_reference(fx):
    warped, mask = R.get_backwarp(fx["a/pred"], fx["a/flow"])
    assert torch.equal(mask, fx["a/flow_mask"])
    assert 0 < float(mask.mean()) < 1  # some samples leave the image, some stay
    close(warped, fx["a/warped"], 1e-12, "warped")


@pytest.mark.parametrize("tag", ["masked", "plain"])
def test_aligned_l1_restatement_matches_the_reference(fx, tag):
    pred, target = fx["a/pred"].clone().requires_grad_(), fx["a/target"].clone().requires_grad_()
    loss = R.aligned_l1(pred, fx["a/flow"], target, fx["a/mask"] if tag == "masked" else None).mean()  # L1Loss: the mean over the batch too
    (UP * loss).backward()
    close(loss.detach(), fx[f"a/{tag}/loss"], 1e-12, "loss")
    close(pred.grad, fx[f"a/{tag}/pred_grad"], 1e-12, "pred grad")
    close(target.grad, fx[f"a/{tag}/target_grad"], 1e-12, "target grad")
    assert fx[f"a/{tag}/pred_grad"].abs().max() > 0 and fx[f"a/{tag}/target_grad"].abs().max() > 0


def test_correlation_restatement_known_answer():
    """One non-zero pixel in each input: the volume is non-zero at that pixel of `first` only, in the channel of the offset."""
    first, second = torch.zeros(1, 2, 7, 9, dtype=F64), torch.zeros(1, 2, 7, 9, dtype=F64)
    first[0, :, 3, 4] = torch.tensor([2.0, 3.0])
    second[0, :, 1, 7] = torch.tensor([5.0, -7.0])  # dy = -2, dx = +3
    out = R.correlation(first, second)
    k = (-2 + 4) * 9 + (3 + 4)
    assert float(out[0, k, 3, 4]) == (2.0 * 5.0 - 3.0 * 7.0) / 2 and int((out != 0).sum()) == 1
    assert float(R.correlation(first, second, 0.1)[0, k, 3, 4]) == pytest.approx(-0.55, rel=1e-15)


def product_net(fx, wrapper):
    from deblur4dgs_amd.pwcnet import Network, PWCNet

    kw = dict(corr_fn=R.correlation, warp_fn=R.get_backwarp)
    net = PWCNet(load_pretrained=False, **kw) if wrapper else Network(**kw)
    names = [str(n) for n in fx["b/names"]]
    shapes = [tuple(int(x) for x in row if x) for row in fx["b/shapes"]]
    return net.double().eval(), names, shapes


def test_state_dict_keys_and_shapes_are_the_references(fx):
    net, names, shapes = product_net(fx, wrapper=False)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got == list(zip(names, shapes))  # the same names, shapes and order


def test_network_and_wrapper_match_the_reference_in_fp64(fx):
    net, names, shapes = product_net(fx, wrapper=False)
    state = R.seeded_state(list(zip(names, shapes)))
    np.testing.assert_allclose(R.checksum(state), fx["c/checksum"], rtol=1e-13)  # the generator drew the same weights
    net.load_state_dict(state)
    with torch.no_grad():
        close(net(fx["c/first"], fx["c/second"]), fx["c/flow"], 1e-10, "network flow")
    wrapper = product_net(fx, wrapper=True)[0]
    wrapper.load_reference_state({k.replace("net", "module"): v for k, v in state.items()})  # the published blob's naming
    with torch.no_grad():
        close(wrapper(fx["c/source"], fx["c/target"]), fx["c/wrapper_flow"], 1e-10, "wrapper flow")
    assert 1e-2 <= float(fx["c/flow"].abs().max()) <= 1e2 and 1e-2 <= float(fx["c/wrapper_flow"].abs().max()) <= 1e2


def test_pretrained_loader_reads_a_file_with_the_references_keys(fx, tmp_path):
    from deblur4dgs_amd.pwcnet import PWCNet

    _, names, shapes = product_net(fx, wrapper=False)
    state = R.seeded_state(list(zip(names, shapes)))
    path = str(tmp_path / "synthetic-network-default.pth")
    torch.save({k.replace("net", "module"): v.float() for k, v in state.items()}, path)
    model = PWCNet(load_pretrained=True, weights_path=path, corr_fn=R.correlation, warp_fn=R.get_backwarp)
    for k, v in model.net.state_dict().items():
        assert torch.equal(v, state[k].float()), k
    with pytest.raises(ValueError):
        PWCNet(load_pretrained=True)


def test_device_seams_reject_cpu_tensors_and_flow_gradients():
    from deblur4dgs_amd import pwcnet as P

    x = torch.rand(1, 3, 4, 5)
    with pytest.raises(RuntimeError, match="ROCm"):
        P.correlation(x, x)
    with pytest.raises(RuntimeError, match="ROCm"):
        P.backwarp(x, torch.zeros(1, 2, 4, 5))
    with pytest.raises(RuntimeError, match="ROCm"):
        P.aligned_l1(x, torch.zeros(1, 2, 4, 5), x)
    with pytest.raises(RuntimeError, match="flow carries a gradient"):
        P.backwarp(x, torch.zeros(1, 2, 4, 5, requires_grad=True))
