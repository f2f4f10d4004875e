"""d4gs_pose_step_cpu (csrc/pose_refine.hip) - the CPU twin of the fused step that ends an iteration of test-time pose refinement -
against torch.optim.Adam + CosineAnnealingLR called in the reference's order (flow3d/validator.py:432-452: scheduler.step() BEFORE
optimizer.step()).  500 steps on a seeded gradient sequence with a generic, non-orthonormal base rotation.  No GPU needed."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

ITERS, LR0, ETA_MIN, BETAS, EPS = 500, 1e-2, 1e-4, (0.9, 0.999), 1e-8


def _inputs():
    g = torch.Generator().manual_seed(20)
    w2c = torch.eye(4, dtype=torch.float64)
    w2c[:3, :3] = torch.eye(3, dtype=torch.float64) + 0.4 * torch.randn(3, 3, generator=g, dtype=torch.float64)  # generic: not a rotation
    w2c[:3, 3] = torch.randn(3, generator=g, dtype=torch.float64)
    # gradients of the composed matrix: a drifting mean plus noise, scales from 1e-3 to 1 across the entries (row 3 is never read)
    scale = 10.0 ** torch.linspace(-3, 0, 16, dtype=torch.float64).reshape(4, 4)
    v_W = (torch.randn(ITERS, 4, 4, generator=g, dtype=torch.float64) + 0.5 * torch.randn(1, 4, 4, generator=g, dtype=torch.float64)) * scale
    return w2c.float(), v_W.float()  # what every run reads: fp32 values


def torch_run(dtype, w2c, v_W, scheduler_first=True):
    """The reference's loop on the given gradients of w2c_trans -> (p [ITERS,12], m, v, lrs [ITERS]) after every update."""
    w2c, v_W = w2c.to(dtype), v_W.to(dtype)
    transR = torch.nn.Parameter(torch.eye(3, dtype=dtype))
    transT = torch.nn.Parameter(torch.zeros(3, 1, dtype=dtype))
    opt = torch.optim.Adam([{"params": [transR, transT], "lr": LR0}], betas=BETAS, eps=EPS)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=ITERS, eta_min=ETA_MIN)
    out = [[], [], [], []]
    flat = lambda a, b: torch.cat([a.detach().reshape(-1), b.detach().reshape(-1)]).double().clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "lr_scheduler.step() before optimizer.step()": the reference's order, on purpose
        for i in range(ITERS):
            transR.grad = v_W[i, :3, :3] @ w2c[:3, :3].T  # autograd of transR @ R0
            transT.grad = v_W[i, :3, 3:].clone()
            if scheduler_first:
                sched.step()
            out[3].append(opt.param_groups[0]["lr"])
            opt.step()
            if not scheduler_first:
                sched.step()
            st = opt.state
            out[0].append(flat(transR, transT))
            out[1].append(flat(st[transR]["exp_avg"], st[transT]["exp_avg"]))
            out[2].append(flat(st[transR]["exp_avg_sq"], st[transT]["exp_avg_sq"]))
    return [torch.stack(x) for x in out[:3]] + [np.asarray(out[3], np.float64)]


def twin_run(w2c, v_W):
    from deblur4dgs_amd import _lib as L

    lib = L.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    base = np.ascontiguousarray(w2c.numpy())
    p = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)])
    m, v = np.zeros(12, np.float32), np.zeros(12, np.float32)
    step, lr, W = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(16, np.float32)
    out = [[], [], [], []]
    for i in range(ITERS):
        g = np.ascontiguousarray(v_W[i].numpy())
        rc = lib.d4gs_pose_step_cpu(fp(base), fp(g), fp(p), fp(m), fp(v), step.ctypes.data_as(C.POINTER(C.c_int32)), LR0, ETA_MIN, ITERS,
                                    BETAS[0], BETAS[1], EPS, fp(lr), fp(W))
        assert rc == 0 and step[0] == i + 1
        # the composed matrix is [transR R0 | transT + t0; 0 0 0 1] of the NEW parameters
        want = np.eye(4)
        want[:3, :3] = p[:9].reshape(3, 3).astype(np.float64) @ base[:3, :3].astype(np.float64)
        want[:3, 3] = p[9:].astype(np.float64) + base[:3, 3]
        assert np.abs(W.reshape(4, 4) - want).max() <= 4e-7 * np.abs(want).max(), i
        assert (W[12:] == (0, 0, 0, 1)).all()
        for k, a in enumerate((p, m, v)):
            out[k].append(torch.from_numpy(a.astype(np.float64)))
        out[3].append(float(lr[0]))
    return [torch.stack(x) for x in out[:3]] + [np.asarray(out[3], np.float64)]


@pytest.fixture(scope="module")
def runs():
    w2c, v_W = _inputs()
    return dict(truth=torch_run(torch.float64, w2c, v_W), yard=torch_run(torch.float32, w2c, v_W), twin=twin_run(w2c, v_W),
                swapped=torch_run(torch.float64, w2c, v_W, scheduler_first=False))


def _errors(run, truth):
    return [float((a - b).abs().max()) for a, b in zip(run[:3], truth[:3])]


def test_twin_matches_torch_adam_and_cosine_schedule_in_the_reference_order(runs):
    """Bound, as tests/test_gpu_adam.py states it: the max-abs error of the parameters and of both moments, over all 500 steps,
    against the torch run in fp64 is <= 2 x that of the torch run in fp32."""
    yard, ours = _errors(runs["yard"], runs["truth"]), _errors(runs["twin"], runs["truth"])
    print("yardstick (torch fp32 vs fp64) p, m, v:", yard, " twin:", ours)
    assert all(y > 0 for y in yard)
    for name, y, o in zip(("p", "exp_avg", "exp_avg_sq"), yard, ours):
        assert o <= 2 * y, (name, o, y)
    # the parameters moved: the comparison is not one of two untouched identities
    assert float((runs["truth"][0][-1] - runs["truth"][0][0]).abs().min()) > 1e-3


def test_lr_sequence_is_the_schedulers_and_ends_at_eta_min(runs):
    ours, sched = runs["twin"][3], runs["truth"][3]
    assert (np.abs(ours - sched) <= 2.0 ** -24 * 1.001 * sched).all()  # the fp32 rounding of the scheduler's double
    assert ours[-1] == np.float64(np.float32(ETA_MIN))  # update 499 runs at lr(500) = eta_min
    assert ours[0] < LR0 and (np.diff(ours) < 0).all()  # update 0 runs at lr(1), not at lr(0) = lr0


def test_mutation_lr_of_the_previous_epoch_is_told_apart(runs):
    """Adam.step() before scheduler.step() - update i at lr(i) instead of lr(i + 1) - is a different trajectory: measured against
    THAT truth the twin misses the bound of the first test, so the bound does tell the two orders apart."""
    yard = _errors(runs["yard"], runs["truth"])
    against_swapped = _errors(runs["twin"], runs["swapped"])
    assert against_swapped[0] > 2 * yard[0], (against_swapped, yard)
    assert runs["swapped"][3][0] == LR0 and runs["swapped"][3][-1] > ETA_MIN


def test_arguments_are_validated():
    from deblur4dgs_amd import _lib as L

    lib = L.lib()
    a = np.zeros(16, np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    st = np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    ok = [fp(a), fp(a.copy()), fp(a.copy()), fp(a.copy()), fp(a.copy()), st, LR0, ETA_MIN, ITERS, 0.9, 0.999, EPS, None, fp(a.copy())]
    assert lib.d4gs_pose_step_cpu(*ok) == 0  # lr_out is optional
    for i in (0, 1, 2, 3, 4, 5, 13):
        bad = list(ok)
        bad[i] = None
        assert lib.d4gs_pose_step_cpu(*bad) == L.EINVAL and b"d4gs_pose_step_cpu" in lib.d4gs_last_error() and b"NULL" in lib.d4gs_last_error()
    bad = list(ok)
    bad[8] = 0
    assert lib.d4gs_pose_step_cpu(*bad) == L.EINVAL and b"t_max=0" in lib.d4gs_last_error()
