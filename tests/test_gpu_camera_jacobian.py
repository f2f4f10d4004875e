"""The camera-path Jacobian of csrc/camera.hip, block by block, over the whole range the zero-initialised heads cross.

`k_camera_path` evaluates the path in dual numbers and writes `jac [S,12,12]` beside `RTs`; every gradient the two `MoveModel` heads and
the trunk receive is a contraction with it.  For small head rotations its four blocks (rotation rows | translation rows) x (d tau | d phi)
differ by orders of magnitude - the rotation rows depend on phi only through tau, |block| ~ |tau1 - tau0| / 8 beside blocks of size 1 - so
a norm over the whole tensor, or a dense cotangent, hides the small block completely.  Here every block is judged against its own maximum
(tests/camera_path_cases.py states the cases, the reference and the tolerance):

  forward    RTs within 3e-6; each block of jac within 1e-4 of the block's maximum + 8 * 2^-23 * max|J_ref|
  backward   CameraPathFn's v_delta0 / v_delta1 against J_ref^T v for a dense, a rotation-only and a translation-only cotangent, the tau and
             the phi half of each separately: 1e-4 of the half's maximum + 8 * 2^-23 * max|J_ref| * sum|v|
  MoveModel  head outputs scaled to 1e-5 .. 1e-2: the last head layers' weight gradient per output row, their bias gradient per tau / phi
             half, everything else per tensor - against fp64 autograd of oracle.camera.forward_start_end_mid
  pose       d4gs_pose_encode_bwd at the identity rotation and at rotation angles 1e-2 and 2.5 about a general axis

Before the series of left_jacobian / left_jacobian_inv were extended to theta^2 <= 1e-2 the rotation-rows / d phi block was 25 % - 350 %
wrong for head rotations of 2e-6 .. 1e-3 ("The small-angle coefficients of the camera path", has the measured figures)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from deblur4dgs_amd import _lib as L
from deblur4dgs_amd import move_model as mm
from oracle import camera
from tests import camera_path_cases as cc
from tests.test_gpu_camera_path import _model, _pose
from tests.util import check, check_columns, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, INDEX, T = 8, 2, 2.0  # time_params [1,8], an interior frame: the exposure window moves, as on the render path


def _fwd(d0, d1, S):
    """d4gs_camera_path_fwd with its jac buffer, as CameraPathFn.forward calls it -> RTs [S,3,4], jac [S,12,12], (dtimes, dT) on the GPU."""
    d0, d1 = d0.to(DEV).contiguous(), d1.to(DEV).contiguous()
    tp = torch.full((1, P), 0.5, device=DEV)
    buf = torch.full((S * 12 + S * 144 + 2 * S + 2,), float("nan"), device=DEV)
    RTs, jac, times, dtimes, dT = buf.split([S * 12, S * 144, S, S, 2])
    L.check(L.lib().d4gs_camera_path_fwd(mm._p(d0), mm._p(d1), S, mm._p(tp), P, INDEX, T, mm._p(RTs), mm._p(jac), mm._p(times),
                                         mm._p(dtimes), mm._p(dT), mm._stream(d0)), "camera_path_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf).all()), "an output was left unwritten, or is not finite"
    return RTs.view(S, 3, 4), jac.view(S, 12, 12), dtimes, dT


@pytest.mark.parametrize("key", cc.KEYS, ids=cc.IDS)
def test_forward_jacobian_block_by_block(key):
    r = cc.reference(*key)
    RTs, jac, _, _ = _fwd(r["d0"], r["d1"], r["S"])
    case = f"a12 jac {cc.case_id(key)}"
    np.testing.assert_allclose(RTs.cpu().numpy(), r["RTs"].numpy(), rtol=0, atol=3e-6, err_msg=case)
    jmax = float(r["jac"].abs().max())
    bad = []
    for name in cc.BLOCKS:
        got, ref = cc.block(jac, name), cc.block(r["jac"], name)
        record(case, name, got, ref)
        err, tol = float(np.abs(got - ref).max()), cc.block_tol(r["jac"], name)
        line = (f"{name}: max err {err:.2e} (= {err / (cc.EPS32 * jmax):.1f} x 2^-23 max|J|), max|block| {np.abs(ref).max():.2e}, "
                f"tol {tol:.2e}")
        print(case, line)
        if not err <= tol:
            bad.append(line)
    assert not bad, f"{case}: " + "; ".join(bad)


def _cotangents(S):
    g = torch.Generator().manual_seed(100 + S)
    dense = torch.randn(S, 3, 4, generator=g)
    rot, trans = dense.clone(), dense.clone()
    rot[:, :, 3] = 0
    trans[:, :, :3] = 0
    return {"dense": dense, "rotation only": rot, "translation only": trans}


@pytest.mark.parametrize("key", cc.KEYS, ids=cc.IDS)
def test_backward_contraction_per_half(key):
    """CameraPathFn forward + backward: v_delta = J^T v.  The kernel sums 12 S products in fp32, which is what the floor's sum|v| is for."""
    r = cc.reference(*key)
    S = r["S"]
    d0, d1 = r["d0"][None].to(DEV).requires_grad_(), r["d1"][None].to(DEV).requires_grad_()
    tp = torch.full((1, P), 0.5, device=DEV, requires_grad=True)
    RTs, times, dT = mm.CameraPathFn.apply(d0, d1, tp, S, INDEX, T, True)
    jmax = float(r["jac"].abs().max())
    bad = []
    for cname, v in _cotangents(S).items():
        g0, g1, gt = torch.autograd.grad(RTs, (d0, d1, tp), v.to(DEV), retain_graph=True)
        assert g0.shape == g1.shape == (1, 6) and float(gt.abs().max()) == 0.0
        got = torch.cat([g0[0], g1[0]]).double().cpu().numpy()
        want = torch.einsum("sij,si->j", r["jac"], v.double().reshape(S, 12)).numpy()
        floor = cc.FLOOR * jmax * float(v.abs().sum())
        for lo, what in ((0, "v_delta0 tau"), (3, "v_delta0 phi"), (6, "v_delta1 tau"), (9, "v_delta1 phi")):
            err = float(np.abs(got[lo:lo + 3] - want[lo:lo + 3]).max())
            tol = 1e-4 * float(np.abs(want[lo:lo + 3]).max()) + floor
            if not err <= tol:
                bad.append(f"{cname} / {what}: max err {err:.2e}, max|ref| {np.abs(want[lo:lo + 3]).max():.2e}, tol {tol:.2e}")
    assert not bad, f"a12 bwd {cc.case_id(key)}: " + "; ".join(bad)


@pytest.mark.parametrize("key", [("b", 1e-3, 2), ("b", 1e-3, 11), ("a", 1e-3, 16)], ids=cc.case_id)
def test_times_only_cotangent_gives_exact_zero_deltas(key):
    """No cotangent on RTs: through autograd (which hands the kernel a zero v_RTs) and through the C ABI with v_RTs = NULL, both deltas
    are exact zeros - written, not left over - and time_params gets the exposure-window gradient."""
    r = cc.reference(*key)
    S = r["S"]
    d0, d1 = r["d0"][None].to(DEV).requires_grad_(), r["d1"][None].to(DEV).requires_grad_()
    tp = torch.full((1, P), 0.5, device=DEV, requires_grad=True)
    RTs, times, dT = mm.CameraPathFn.apply(d0, d1, tp, S, INDEX, T, True)
    v_times = torch.linspace(-1.0, 2.0, S, device=DEV).view(1, S)
    g0, g1, gt = torch.autograd.grad(times, (d0, d1, tp), v_times)
    want_tp = float((v_times.cpu().double()[0] * (2 * torch.arange(S, dtype=torch.float64) / (S - 1) - 1)).sum())  # d = p on (0.1, 0.9)
    for g in (g0, g1):
        assert torch.equal(g.cpu(), torch.zeros(1, 6))
    np.testing.assert_allclose(gt.cpu().numpy()[0], np.eye(P)[INDEX] * want_tp, rtol=0, atol=1e-5 * max(1.0, abs(want_tp)))

    _, jac, dtimes, dTbuf = _fwd(r["d0"], r["d1"], S)
    out = torch.full((12 + P,), float("nan"), device=DEV)
    z = C.c_void_p(0)
    L.check(L.lib().d4gs_camera_path_bwd(mm._p(jac), mm._p(dtimes), mm._p(dTbuf), z, mm._p(v_times.contiguous()), z, S, INDEX, P,
                                         mm._p(out[:6]), mm._p(out[6:12]), mm._p(out[12:]), mm._stream(out)), "camera_path_bwd")
    torch.cuda.synchronize()
    assert torch.equal(out[:12].cpu(), torch.zeros(12))
    np.testing.assert_array_equal(out[12:].cpu().numpy(), gt.cpu().numpy()[0])


W2C = [0.2, -0.1, 0.3, 0.5, -0.4, 0.1]  # the pose of test_gpu_camera_path's gradient test


def _scaled_model(target):
    """test_gpu_camera_path._model(seed=3) with the last layer of both heads scaled so that the largest head output is `target`."""
    m = _model(seed=3)
    w2c = _pose(W2C)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    d0, d1, _, _ = camera.move_model_forward(sd, w2c[:3, :3].double(), w2c[:3, 3:4].double(), T)
    f = target / max(float(d0.abs().max()), float(d1.abs().max()))
    with torch.no_grad():
        for head in (m.RT_head0, m.RT_head1):
            head[-1].weight.mul_(f)
            head[-1].bias.mul_(f)
    return m, w2c


def _zero(case, tensor, got, ref, floor):
    """A piece that is zero by construction: the reference holds its own rounding only (a tenth of the floor at most), the kernel's stays
    within the floor."""
    g, r = float(got.abs().max()), float(ref.abs().max())
    print(f"{case} / {tensor}: structurally zero, max|got| {g:.2e}, max|ref| {r:.2e}, floor {floor:.2e}")
    assert r <= 0.1 * floor and g <= floor, f"{case} / {tensor}: max|got| {g:.2e}, max|ref| {r:.2e}, floor {floor:.2e}"


@pytest.mark.parametrize("target,S", [(1e-5, 2), (1e-5, 11), (1e-4, 2), (1e-4, 11), (1e-3, 2), (1e-3, 11), (1e-2, 2), (1e-2, 11), (1e-3, 16)])
@pytest.mark.parametrize("cot", ["dense", "rotation only"])
def test_move_model_gradients_per_head_row(cot, target, S):
    m, w2c = _scaled_model(target)
    wR = _cotangents(S)[cot]
    g = torch.Generator().manual_seed(1)
    wt, wd = torch.randn(1, S, generator=g), 0.7

    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in m.state_dict().items()}
    Ro = w2c[:3, :3].double().clone().requires_grad_()
    To = w2c[:3, 3:4].double().clone().requires_grad_()
    with torch.no_grad():
        h0, h1, _, _ = camera.move_model_forward(sd, Ro, To, T)
    print(f"head outputs (target {target:g}): d0 = {h0[0].tolist()}  d1 = {h1[0].tolist()}")
    assert 0.999 * target <= max(float(h0.abs().max()), float(h1.abs().max())) <= 1.001 * target
    # With S = 2 the rotation rows do not depend on phi at all (camera_path_cases.py, WHAT IS ZERO BY CONSTRUCTION), so under the
    # rotation-only cotangent the phi half of both head gradients is zero in the reference up to its rounding: a ratio to max|ref| says
    # nothing there.  Those rows get the backward test's absolute floor instead, 8 * 2^-23 * max|J| * sum|v| on v_delta's phi half, times
    # the largest input activation of the layer for its weight rows; every other row and tensor is judged as everywhere else.
    zero_phi = S == 2 and cot == "rotation only"
    if zero_phi:
        with torch.no_grad():
            jmax = float(torch.autograd.functional.jacobian(lambda d: cc.path(d, S), torch.cat([h0[0], h1[0]]), vectorize=True).abs().max())
            x = camera._mlp(camera.posenc(camera.SE3_to_se3(torch.cat([Ro, To], -1))[None]), sd, "RT_main", 5)
            act = {h: float(F.leaky_relu(F.linear(x, sd[f"RT_head{h}.0.weight"], sd[f"RT_head{h}.0.bias"]), 0.01).abs().max()) for h in (0, 1)}
        floor = cc.FLOOR * jmax * float(wR.abs().sum())
    oR, ot, od = camera.forward_start_end_mid(sd, Ro, To, T, S, "second")
    ((oR * wR.double()).sum() + (ot * wt.double()).sum() + wd * od.sum()).backward()

    Rg = w2c[:3, :3].to(DEV).clone().requires_grad_()
    Tg = w2c[:3, 3:4].to(DEV).clone().requires_grad_()
    m.zero_grad(set_to_none=True)
    RTs, times, dT = m.forward_start_end_mid({"R": Rg, "T": Tg, "timestep": T}, num_cameras=S)
    ((RTs * wR.to(DEV)).sum() + (times * wt.to(DEV)).sum() + wd * dT.sum()).backward()
    torch.cuda.synchronize()
    got = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).cpu() for n, p in m.named_parameters()}
    got["input.R"], got["input.T"] = Rg.grad.cpu(), Tg.grad.cpu()
    want = {n: (sd[n].grad if sd[n].grad is not None else torch.zeros_like(sd[n])) for n in sd}
    want["input.R"], want["input.T"] = Ro.grad, To.grad
    case = f"a12 heads ~{target:g} S={S} {cot}"
    np.testing.assert_allclose(RTs.detach().cpu().numpy(), oR.detach().numpy(), rtol=0, atol=3e-6)
    failed = []
    for n in got:
        try:
            if n in ("RT_head0.2.weight", "RT_head1.2.weight"):  # [6,64]: one column per output row after the transpose
                if zero_phi:
                    check_columns(case, n + "[:3].T", got[n][:3].T, want[n][:3].T)
                    _zero(case, n + "[3:]", got[n][3:], want[n][3:], floor * act[int(n[7])])
                else:
                    check_columns(case, n + ".T", got[n].T, want[n].T)
            elif n in ("RT_head0.2.bias", "RT_head1.2.bias"):
                check(case, n + "[tau]", got[n][:3], want[n][:3])
                if zero_phi:
                    _zero(case, n + "[phi]", got[n][3:], want[n][3:], floor)
                else:
                    check(case, n + "[phi]", got[n][3:], want[n][3:])
            else:  # 1e-4 of the tensor's maximum (no absolute floor: with the heads scaled down the trunk's gradients are ~ 1e-6)
                check(case, n, got[n], want[n])
        except AssertionError as e:  # report every tensor that is off, not just the first
            failed.append(str(e).strip().splitlines()[0])
    assert not failed, f"{case}:\n" + "\n".join(failed)


AXIS = (0.36, -0.48, 0.8)
CLAMP = 1 - 1e-7  # SO3_to_so3 clamps (trace - 1) / 2 to [-CLAMP, CLAMP]


def _rotation(angle):
    a = torch.tensor(AXIS, dtype=torch.float64)
    K = camera.skew_symmetric(a / a.norm())
    return (torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)).float()


@pytest.mark.parametrize("angle", [0.0, 1e-2, 2.5], ids=["identity", "angle1e-2", "angle2.5"])
def test_pose_encode_input_gradient_at_unvisited_poses(angle):
    """d4gs_pose_encode_bwd alone, with a random adjoint of the 66 encoding channels, against fp64 autograd of the oracle's
    posenc(SE3_to_se3(.)): the identity rotation with T != 0 (the first camera of many datasets: acos sits on its clamp, w = 0, the norm on
    its sub-gradient), a small and a large rotation about a general axis.  Tolerance: the suite's 1e-4 of the tensor maximum."""
    R, Tv = _rotation(angle), torch.tensor([[0.4], [-0.7], [1.3]])
    if angle == 0.0:
        assert torch.equal(R, torch.eye(3))
    # the clamp cannot fall the other way in fp32: c is either beyond the bound or at least 1e-5 inside it
    c = float((R.double().trace() - 1) / 2)
    assert abs(c) >= CLAMP or abs(c) <= CLAMP - 1e-5, c
    v = torch.randn(66, generator=torch.Generator().manual_seed(5))

    Ro, To = R.double().requires_grad_(), Tv.double().requires_grad_()
    enc = camera.posenc(camera.SE3_to_se3(torch.cat([Ro, To], -1)).unsqueeze(0))
    (enc[0] * v.double()).sum().backward()

    Rg, Tg, vg = R.to(DEV), Tv.to(DEV).reshape(3), v.to(DEV)
    got_enc = mm.pose_encode(Rg, Tg.view(3, 1))
    out = torch.full((12,), float("nan"), device=DEV)
    L.check(L.lib().d4gs_pose_encode_bwd(mm._p(Rg), Rg.stride(0), mm._p(Tg), Tg.stride(0), mm._p(vg), mm._p(out[:9]), mm._p(out[9:]),
                                         mm._stream(Rg)), "pose_encode_bwd")
    torch.cuda.synchronize()
    np.testing.assert_allclose(got_enc.cpu().numpy(), enc.detach().numpy(), rtol=0, atol=3e-5)
    case = f"a12 pose grad {'identity' if angle == 0.0 else f'angle {angle:g}'}"
    check(case, "input.R", out[:9].view(3, 3).cpu(), Ro.grad)
    check(case, "input.T", out[9:].view(3, 1).cpu(), To.grad)
