"""Multi-tensor Adam without a GPU: the numerics of the kernel's per-element function through its CPU twin
(d4gs_adam_step_cpu runs the same `__host__ __device__` code as k_adam), the torch.optim.Optimizer contract of the per-tensor
handles, and the argument validation of the C entry points."""
import copy
import ctypes as C
import os

import pytest
import torch

from tests import adam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twin(params):
    from deblur4dgs_amd.optim import AdamGroup, adam_step_cpu

    group = AdamGroup()
    hs = [group.adam(p, R.LRS[i], eps=R.EPSS[i]) for i, p in enumerate(params)]
    return (lambda: adam_step_cpu(group)), (lambda i: hs[i].state.get(params[i], {}))


def test_twin_numerics_against_fp64_torch_adam():
    """50 steps on the mixed table (tests/adam_ref.py).  Truth: torch.optim.Adam in fp64; yardstick: the same optimizer in fp32
    on the CPU.  Per tensor, the twin's max-abs error in the parameter and in both moments is <= 2 x the yardstick's: the
    margin covers one differently ordered but equally valid fp32 evaluation of the same formula, nothing more.  (As measured
    here both moments are bit-identical to torch's fp32 path, so their two columns are equal; the parameter differs in a few
    last bits where torch's vectorised CPU sqrt is not the correctly rounded one.)  Both columns go to profiles/adam_parity.md."""
    truth = R.run(R.torch_adam, torch.float64)
    yard = R.errors(R.run(R.torch_adam, torch.float32), truth)
    skipped = []

    def on_step(s, params, state_of, step_fn):
        p = params[R.SKIPPED]
        before = None if p.grad is not None else (p.detach().clone(), {k: v.clone() for k, v in state_of(R.SKIPPED).items()})
        step_fn()
        if before is not None:
            assert torch.equal(p.detach(), before[0])
            for k, v in before[1].items():  # step, exp_avg, exp_avg_sq: bit-identical, the step did not advance
                assert torch.equal(state_of(R.SKIPPED)[k], v), k
            skipped.append(s)

    ours_raw = R.run(_twin, torch.float32, on_step=on_step)
    ours = R.errors(ours_raw, truth)
    assert skipped == sorted(R.SKIP_STEPS)
    for i, r in enumerate(ours_raw):  # every tensor counted its own steps
        assert r[3] == R.STEPS - (len(R.SKIP_STEPS) if i == R.SKIPPED else 0) == truth[i][3]
    with open(os.path.join(ROOT, "profiles", "adam_parity.md"), "w") as f:
        f.write(R.table(yard, ours, "Adam parity: CPU twin of k_adam (d4gs_adam_step_cpu)"))
    for i, (y, o) in enumerate(zip(yard, ours)):
        print(R.SHAPES[i], "yardstick", y, "twin", o)
    for i, (y, o) in enumerate(zip(yard, ours)):
        for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
            assert o[k] <= 2 * y[k], (R.SHAPES[i], name, o[k], y[k])


def _cpu_handle(n=10, lr=1e-2, seed=0):
    from deblur4dgs_amd.optim import AdamGroup, adam_step_cpu

    torch.manual_seed(seed)
    p = torch.nn.Parameter(torch.randn(n, 3))
    group = AdamGroup()
    h = group.adam(p, lr)
    return group, h, p, adam_step_cpu


def test_handle_is_a_torch_optimizer_and_refuses_cpu_steps():
    group, h, p, step_cpu = _cpu_handle()
    assert isinstance(h, torch.optim.Adam) and isinstance(h, torch.optim.Optimizer)
    assert len(h.param_groups) == 1 and h.param_groups[0]["params"] == [p]
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h.step()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        group.step()
    assert len(h.state) == 0  # nothing happened
    step_cpu(group)
    assert set(h.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and float(h.state[p]["step"]) == 1.0


def test_state_dict_round_trip_with_torch_adam():
    """A handle's checkpoint loads into torch.optim.Adam and continues identically there, and the other way round."""
    group, h, p, step_cpu = _cpu_handle()
    grads = [torch.randn(10, 3, generator=torch.Generator().manual_seed(s)) for s in range(6)]
    for g in grads[:3]:
        p.grad = g.clone()
        step_cpu(group)
    # handle -> torch
    q = torch.nn.Parameter(p.detach().clone())
    ref = torch.optim.Adam([q], lr=123.0, foreach=False, fused=False)
    ref.load_state_dict(copy.deepcopy(h.state_dict()))  # (as through torch.save / torch.load: load_state_dict shares tensors with its argument)
    assert ref.param_groups[0]["lr"] == 1e-2 and float(ref.state[q]["step"]) == 3.0
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(ref.state[q][k], h.state[p][k])
    # torch -> a fresh handle; all three continue with the same gradients
    from deblur4dgs_amd.optim import AdamGroup

    group2 = AdamGroup()
    r = torch.nn.Parameter(p.detach().clone())
    h2 = group2.adam(r, 5.0)
    h2.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert h2.param_groups[0]["lr"] == 1e-2 and float(h2.state[r]["step"]) == 3.0
    for g in grads[3:]:
        p.grad, q.grad, r.grad = g.clone(), g.clone(), g.clone()
        step_cpu(group), ref.step(), step_cpu(group2)
    assert torch.equal(p, r)  # the reloaded handle is the original, bit for bit
    assert float(h2.state[r]["step"]) == 6.0 == float(ref.state[q]["step"])
    assert torch.equal(h.state[p]["exp_avg"], ref.state[q]["exp_avg"]) and torch.equal(h.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])
    assert (p - q).abs().max().item() <= 1e-6  # (last bits: torch's CPU sqrt)


def test_lambda_lr_drives_a_handle():
    group, h, p, step_cpu = _cpu_handle(lr=1e-2)
    q = torch.nn.Parameter(p.detach().clone())
    ref = torch.optim.Adam([q], lr=1e-2, foreach=False, fused=False)
    sched = torch.optim.lr_scheduler.LambdaLR(h, lambda e: 0.5 ** e)
    sched_ref = torch.optim.lr_scheduler.LambdaLR(ref, lambda e: 0.5 ** e)
    for s in range(4):
        g = torch.randn(10, 3, generator=torch.Generator().manual_seed(s))
        p.grad, q.grad = g.clone(), g.clone()
        step_cpu(group), ref.step()
        sched.step(), sched_ref.step()
        assert h.param_groups[0]["lr"] == pytest.approx(1e-2 * 0.5 ** (s + 1))
    assert (p - q).abs().max().item() <= 1e-6  # the scheduled lr is the one the update used (an unscheduled run ends ~1e-2 away)


def test_control_surgery_on_a_handle():
    """dup_in_optim / remove_from_optim / reset_in_optim re-key a handle like any single-parameter Adam, and the group's next
    table is built from the new tensors."""
    from deblur4dgs_amd import optim
    from deblur4dgs_amd.control import dup_in_optim, remove_from_optim, reset_in_optim
    from deblur4dgs_amd.rows import RowPlan

    group, h, p, step_cpu = _cpu_handle(n=6)
    p.grad = torch.ones_like(p)
    step_cpu(group)
    m_old = h.state[p]["exp_avg"].clone()
    dup = torch.tensor([True, False, False, True, False, False])
    plan = RowPlan(torch.zeros(6, dtype=torch.bool), dup)
    p2 = torch.nn.Parameter(plan.gather(p.detach()))
    dup_in_optim(h, [p2], plan)
    assert h.param_groups[0]["params"] == [p2] and p not in h.state
    m2 = h.state[p2]["exp_avg"]
    assert m2.shape == (8, 3) and torch.equal(m2[:6], m_old) and not m2[6:].any()  # new rows start at zero
    rec = optim._record(h, create=False)
    assert rec[0] is p2 and rec[2]["exp_avg"] is m2 and rec[2]["exp_avg"].data_ptr() == m2.data_ptr()  # what the table is filled from
    p2.grad = torch.ones_like(p2)
    step_cpu(group)
    assert float(h.state[p2]["step"]) == 2.0 and m2[6:].abs().min() > 0  # the new rows are being updated
    cull = torch.tensor([False, True] * 4)
    plan = RowPlan(cull)
    p3 = torch.nn.Parameter(plan.gather(p2.detach()))
    remove_from_optim(h, [p3], plan)
    assert h.state[p3]["exp_avg"].shape == (4, 3) and torch.equal(h.state[p3]["exp_avg"], m2[~cull])
    p3.grad = torch.ones_like(p3)
    step_cpu(group)
    assert float(h.state[p3]["step"]) == 3.0
    p4 = torch.nn.Parameter(p3.detach().clone())
    reset_in_optim(h, [p4])
    assert float(h.state[p4]["step"]) == 0.0 and not h.state[p4]["exp_avg"].any() and not h.state[p4]["exp_avg_sq"].any()
    p4.grad = torch.ones_like(p4)
    step_cpu(group)
    assert float(h.state[p4]["step"]) == 1.0 and optim._record(h, create=False)[0] is p4


def test_bad_arguments_return_einval_and_version_is_305():
    from deblur4dgs_amd import _lib as L

    lib = L.lib()
    assert lib.d4gs_version() == 305
    assert "#define D4GS_VERSION 305" in open(os.path.join(ROOT, "include", "d4gs.h")).read()
    fake = 0x10000
    for args in ((None, 1, fake, 1, fake, None), (fake, 1, None, 1, fake, None), (fake, 1, fake, 1, None, None),
                 (fake + 4, 1, fake, 1, fake, None), (fake, 1, fake + 2, 1, fake, None), (fake, -1, fake, 1, fake, None),
                 (fake, 2, fake, 1, fake, None)):
        assert lib.d4gs_adam_step(*args) == -1, args  # D4GS_EINVAL before any HIP call
        assert b"d4gs_adam_step" in lib.d4gs_last_error()
    assert lib.d4gs_adam_step(None, 0, None, 0, None, None) == 0  # an empty table launches nothing
    assert lib.d4gs_adam_set_grads(None, 1, None, None) == -1
    assert lib.d4gs_adam_step_cpu(None, 1) == -1
    x = torch.zeros(8)
    step = torch.zeros(())
    ok = dict(param=x.data_ptr(), grad=x.data_ptr(), exp_avg=x.data_ptr(), exp_avg_sq=x.data_ptr(), step=step.data_ptr(), n=8,
              lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    for bad in (dict(param=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(step=None), dict(n=-1),
                dict(param=x.data_ptr() + 2), dict(grad=x.data_ptr() + 1)):
        rec = (L.AdamRec * 1)(L.AdamRec(**{**ok, **bad}))
        assert lib.d4gs_adam_step_cpu(rec, 1) == -1, bad
        assert b"record 0" in lib.d4gs_last_error()
    assert not x.any() and float(step) == 0.0  # nothing was written
    assert [lib.d4gs_adam_blocks(n) for n in (0, 1, 2048, 2049, 4096)] == [1, 1, 1, 2, 2]
    assert C.sizeof(L.AdamRec) == 80
