"""Multi-tensor Adam on the device (csrc/adam.hip through deblur4dgs_amd.optim.AdamGroup): numerics against the fp64 truth,
run-to-run and group-versus-handle bit equality, capture in a HIP graph, the control steps, and the example's --hip-adam.

The table of tests/adam_ref.py has 8 records and one record of several chunks (800 000 elements, n % 4 = 0).  The sizes past that:
130 records (three launches of the 64-pointer gradient patch, the NULL pointers first in the second and third), and records of
2 049, 4 099 and 6 146 elements (2, 3 and 4 chunks of 2 048 with an n % 4 tail of 1, 3 and 2 in the last chunk), each on the
16-byte and on the dword path."""
import importlib.util
import os

import pytest
import torch

from tests import adam_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _example():
    spec = importlib.util.spec_from_file_location("train_dynamic_step_adam", os.path.join(ROOT, "examples", "train_dynamic_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _group(params):
    from deblur4dgs_amd.optim import AdamGroup

    group = AdamGroup()
    hs = [group.adam(p, R.LRS[i], eps=R.EPSS[i]) for i, p in enumerate(params)]
    return group.step, (lambda i: hs[i].state.get(params[i], {}))


def test_device_table_numerics_and_run_to_run_bits():
    """The mixed table of tests/adam_ref.py, 50 steps of `group.step()` on the device.  Per tensor, the max-abs error of the
    parameter and of both moments against torch.optim.Adam in fp64 is <= 2 x that of torch.optim.Adam in fp32 on the CPU (the
    yardstick of tests/test_adam_cpu.py, same margin, same reason); a tensor without a gradient is left bit-identical with its
    step count; two runs from the same start are bitwise equal (no atomics, no cross-workgroup traffic)."""
    truth = R.run(R.torch_adam, torch.float64)
    yard = R.errors(R.run(R.torch_adam, torch.float32), truth)
    skipped = []

    def on_step(s, params, state_of, step_fn):
        p = params[R.SKIPPED]
        before = None if p.grad is not None else (p.detach().clone(), {k: v.clone() for k, v in state_of(R.SKIPPED).items()})
        step_fn()
        if before is not None:
            assert torch.equal(p.detach(), before[0])
            for k, v in before[1].items():
                assert torch.equal(state_of(R.SKIPPED)[k], v), k
            skipped.append(s)

    run1 = R.run(_group, torch.float32, DEV, on_step=on_step)
    run2 = R.run(_group, torch.float32, DEV)
    assert skipped == sorted(R.SKIP_STEPS)
    ours = R.errors(run1, truth)
    with open(os.path.join(ROOT, "profiles", "adam_parity_gpu.md"), "w") as f:
        f.write(R.table(yard, ours, "Adam parity: k_adam on the device (AdamGroup.step)"))
    for i, (y, o) in enumerate(zip(yard, ours)):
        print(R.SHAPES[i], "yardstick", y, "device", o)
    for i, (a, b) in enumerate(zip(run1, run2)):
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] == truth[i][3], R.SHAPES[i]
    for i, (y, o) in enumerate(zip(yard, ours)):
        for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
            assert o[k] <= 2 * y[k], (R.SHAPES[i], name, o[k], y[k])


def test_group_step_equals_stepping_each_handle_and_dword_path_equals_vector_path():
    """One launch over the table, one launch per handle, and a copy whose parameters sit 4 bytes off a 16-byte boundary (the
    dword path of the kernel): the same per-element code, so the same bits."""
    from deblur4dgs_amd.optim import AdamGroup

    def make(offset):
        params = []
        for p0 in R.initial_params():
            buf = torch.zeros(p0.numel() + offset, device=DEV)
            p = buf[offset:].view(p0.shape).detach()
            p.copy_(p0)
            params.append(p.requires_grad_())
        group = AdamGroup()
        return params, group, [group.adam(p, R.LRS[i], eps=R.EPSS[i]) for i, p in enumerate(params)]

    (pa, ga, ha), (pb, gb, hb), (pc, gc, hc) = make(0), make(0), make(1)
    assert all(p.data_ptr() % 16 == 0 for p in pa) and all(p.data_ptr() % 16 == 4 for p in pc)
    for s in range(6):
        for i in range(len(pa)):
            g = R.gradient(s, i)
            for params in (pa, pb, pc):
                params[i].grad = None if g is None else g.to(DEV)
        ga.step()
        for h in hb:
            h.step()
        gc.step()
    torch.cuda.synchronize()
    for i in range(len(pa)):
        for params, hs in ((pb, hb), (pc, hc)):
            assert torch.equal(pa[i], params[i]), i
            for k in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(ha[i].state[pa[i]][k], hs[i].state[params[i]][k]), (i, k)
    assert float(ha[R.SKIPPED].state[pa[R.SKIPPED]]["step"]) == 6 - len([s for s in R.SKIP_STEPS if s < 6])


ADAM_PATCH = 64  # adam.hip: constexpr int ADAM_PATCH = 64, the gradient pointers of one k_adam_set_grads launch
MANY = 130
MANY_SIZES = [(1, 3, 5, 64, 2049, 4099, 6146)[i % 7] for i in range(MANY)]
MANY_WITHOUT = (64, 128)  # no gradient after the first step: the first pointer of the second and of the third patch is NULL


def _many_gradient(step, i):
    g = torch.Generator().manual_seed(9000 + 131 * step + i)
    return (torch.randn(MANY_SIZES[i], generator=g) + 0.3) * (0.1 if i % 2 else 3e-3)


def _many(device):
    """130 tensors, every third 4 bytes off a 16-byte line (the dword path), lr and eps distinct over neighbours"""
    from deblur4dgs_amd.optim import AdamGroup

    g = torch.Generator().manual_seed(21)
    params, group = [], AdamGroup()
    for i, n in enumerate(MANY_SIZES):
        off = 1 if i % 3 == 0 else 0
        buf = torch.zeros(n + 4, device=device)
        p = buf[off:off + n].detach()
        p.copy_(torch.randn(n, generator=g))
        assert device == "cpu" or p.data_ptr() % 16 == 4 * off
        params.append(p.requires_grad_())
    return params, group, [group.adam(p, 1e-3 * (1 + i % 5), eps=(1e-8, 1e-6, 1e-10)[i % 3]) for i, p in enumerate(params)]


def test_a_group_of_130_tensors_in_three_pointer_patches_with_every_chunk_tail():
    """130 records: d4gs_adam_set_grads patches their gradient pointers in launches of 64, 64 and 2, and k_adam finds each block's
    record among 130; the sizes 2 049, 4 099 and 6 146 are records of 2, 3 and 4 chunks whose last chunk ends in an n % 4 tail of
    1, 3 and 2 elements, on the 16-byte path and, every third tensor, on the dword path.  Six steps, the first eager with every
    gradient (it creates the state), the other five replayed from ONE captured `group.step()` - the only path on which the pointers
    are patched by the kernel (an eager step uploads the table) - with no sync() in between, so the replays see the gradient
    pointers the patch launches wrote and no others.  Bitwise equal to the same steps run eagerly in one launch, to stepping each
    handle alone, and to the CPU twin on copies; tensors 64 and 128 get no gradient after the first step and stay untouched."""
    from deblur4dgs_amd import _lib as L
    from deblur4dgs_amd.optim import adam_step_cpu

    assert -(-MANY // ADAM_PATCH) == 3 and all(i % ADAM_PATCH == 0 for i in MANY_WITHOUT)
    assert {n % 4 for n in MANY_SIZES if n > L.ADAM_CHUNK} == {1, 2, 3} and {L.lib().d4gs_adam_blocks(n) for n in MANY_SIZES} == {1, 2, 3, 4}
    steps = 6
    grad = lambda s, i: None if (s > 0 and i in MANY_WITHOUT) else _many_gradient(s, i)
    (pg, gg, hg), (pe, ge, he), (ph, gh, hh), (pc, gc, hc) = _many(DEV), _many(DEV), _many(DEV), _many("cpu")
    # eager in one launch; each handle alone; the CPU twin
    for s in range(steps):
        for i in range(MANY):
            g = grad(s, i)
            for params, dev in ((pe, DEV), (ph, DEV), (pc, "cpu")):
                params[i].grad = None if g is None else g.to(dev)
        ge.step()
        for h in hh:
            h.step()
        adam_step_cpu(gc)
    # graph: step 0 eagerly, then one capture whose gradients are new tensors, replayed for steps 1 .. 5
    first = [grad(0, i).to(DEV) for i in range(MANY)]  # kept alive: the table's pointers of before the patch stay readable
    for p, g in zip(pg, first):
        p.grad = g
    gg.step()
    static = [None if i in MANY_WITHOUT else torch.zeros(n, device=DEV) for i, n in enumerate(MANY_SIZES)]
    for p, g in zip(pg, static):
        p.grad = g
    untouched = {i: (pg[i].detach().clone(), {k: v.clone() for k, v in hg[i].state[pg[i]].items()}) for i in MANY_WITHOUT}
    torch.cuda.synchronize()
    generation = gg.generation
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gg.step()
    for s in range(1, steps):
        for i in range(MANY):
            if static[i] is not None:
                static[i].copy_(grad(s, i))
        graph.replay()
    torch.cuda.synchronize()
    assert gg.generation == generation
    for i in range(MANY):
        for name, params, hs in (("one eager launch", pe, he), ("each handle alone", ph, hh), ("CPU twin", pc, hc)):
            assert torch.equal(pg[i].detach().cpu(), params[i].detach().cpu()), (name, i, MANY_SIZES[i])
            for k in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(hg[i].state[pg[i]][k].cpu(), hs[i].state[params[i]][k].cpu()), (name, i, MANY_SIZES[i], k)
        assert float(hg[i].state[pg[i]]["step"]) == (1.0 if i in MANY_WITHOUT else float(steps))
    for i, (p0, st0) in untouched.items():
        assert torch.equal(pg[i].detach(), p0) and all(torch.equal(hg[i].state[pg[i]][k], v) for k, v in st0.items()), i
    assert not torch.equal(pg[4].detach()[-1:].cpu(), _many("cpu")[0][4].detach()[-1:])  # the tail element of a 2 049 record moved


NAMES = ("means", "quats", "scales", "opacities", "colors", "motion_coefs", "rots", "transls")


def _render_step(L, sc, K, W, H, w):
    from deblur4dgs_amd.exposure import render_exposure

    res = render_exposure(L["means"], L["quats"], L["scales"], L["opacities"], L["colors"], 3, L["motion_coefs"], L["rots"],
                          L["transls"], sc["times"], sc["RTs"], sc["viewmat"], K, W, H, background=torch.ones(3, device=K.device),
                          return_depth=True, deferred_size_check=True)
    (res["blended"] * w).sum().backward()


def test_backward_and_group_step_replay_from_a_hip_graph():
    """Backward + `group.step()` of a small render captured in ONE graph (after one eager step created the Adam state), replayed
    5 times with one lr changed between replays (`group.sync()` pushes it into the device table; the captured launch reads it
    there).  The parameters equal, bitwise, the same 5 steps run eagerly with the HIP Adam."""
    from deblur4dgs_amd import engine
    from deblur4dgs_amd.optim import AdamGroup
    from deblur4dgs_amd.synth import make_scene

    N, G, K_, S, W, H = 6000, 4000, 4, 3, 160, 96
    sc = {k: v.to(DEV) for k, v in make_scene(N, G, K_, S, W, H, seed=8).items() if torch.is_tensor(v)}
    K = sc["K"]
    w = torch.randn(H, W, 4, generator=torch.Generator().manual_seed(0)).to(DEV)

    def setup():
        L = {k: sc[k].clone().requires_grad_() for k in NAMES}
        group = AdamGroup()
        return L, group, {k: group.adam(L[k], 1e-3) for k in NAMES}

    def set_lr(hs, it):
        if it >= 2:
            hs["means"].param_groups[0]["lr"] = 3e-3  # what a scheduler does

    engine.check_deferred()
    # eager: 1 + 5 steps
    Le, ge, he = setup()
    for it in range(-1, 5):
        set_lr(he, it)
        for v in Le.values():
            v.grad = None
        _render_step(Le, sc, K, W, H, w)
        ge.step()
        engine.check_deferred()
    # graph: the same first step eagerly, then capture once and replay 5 times
    Lg, gg, hg = setup()
    _render_step(Lg, sc, K, W, H, w)
    gg.step()
    engine.check_deferred()
    for v in Lg.values():
        v.grad = None
    generation = gg.generation
    graph, watch = torch.cuda.CUDAGraph(), engine.GraphWatch()
    with watch.capturing(), torch.cuda.graph(graph):
        _render_step(Lg, sc, K, W, H, w)
        gg.step()
    for it in range(5):
        set_lr(hg, it)
        gg.sync()
        graph.replay()
        watch.replayed()
        watch.check()
    torch.cuda.synchronize()
    watch.check()
    assert gg.generation == generation  # the table the graph captured is still the group's table
    for k in NAMES:
        assert torch.equal(Lg[k], Le[k]), k
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(hg[k].state[Lg[k]][key], he[k].state[Le[k]][key]), (k, key)
        assert float(hg[k].state[Lg[k]]["step"]) == 6.0
    assert not torch.equal(Lg["means"], sc["means"])


def test_control_steps_rebuild_the_table_and_new_rows_start_from_zero_moments():
    """densify_step / cull_step on a small SceneModel whose optimizers are handles of one group: the next `group.step()` runs on
    the new tensors (the table was rebuilt), the moment rows of new Gaussians start at zero, kept rows carry theirs over."""
    from deblur4dgs_amd.control import ControlCfg, cull_step, densify_step, new_running_stats
    from deblur4dgs_amd.optim import AdamGroup

    mod = _example()
    model, _ = mod.build(n_fg=300, n_bg=500, K=4, W=64, H=48, dev=DEV)
    group = AdamGroup()
    optimizers = {f"{part}.params.{n}": group.adam(p, 1e-2) for part in ("fg", "bg") for n, p in getattr(model, part).params.items()}

    def step_with_unit_grads():
        for o in optimizers.values():
            p = o.param_groups[0]["params"][0]
            p.grad = torch.ones_like(p)
        group.step()

    step_with_unit_grads()
    n0, gen0 = model.num_gaussians, group.generation
    h = optimizers["fg.params.means"]
    m_before = h.state[h.param_groups[0]["params"][0]]["exp_avg"].clone()
    assert torch.equal(m_before, torch.full_like(m_before, m_before.flatten()[0].item())) and m_before.flatten()[0] > 0
    stats = new_running_stats(n0, DEV)
    stats["vis_count"] += 1
    stats["xys_grad_norm_acc"][::3] = 1.0  # every third Gaussian is over the densification threshold
    n_split, n_dup = densify_step(model, stats, optimizers, ControlCfg(), global_step=1)
    assert n_split + n_dup > 0 and model.num_gaussians > n0
    p_new = h.param_groups[0]["params"][0]
    assert p_new is model.fg.params["means"] and p_new.shape[0] > 300
    m_new = h.state[p_new]["exp_avg"]
    n_zero = int((m_new == 0).all(-1).sum())
    assert n_zero > 0 and int((m_new == m_before.flatten()[0]).all(-1).sum()) == p_new.shape[0] - n_zero  # new rows: zero moments
    fresh = (m_new == 0).all(-1)
    before = p_new.detach().clone()
    step_with_unit_grads()
    torch.cuda.synchronize()
    assert group.generation > gen0 and float(h.state[p_new]["step"]) == 2.0
    assert (p_new.detach() != before).all()  # every row, the new ones included, was updated
    m_after = h.state[p_new]["exp_avg"]
    one = torch.ones((), device=DEV)
    assert torch.equal(m_after[fresh], torch.lerp(torch.zeros_like(m_after[fresh]), one, 1 - 0.9))  # started at zero
    assert (m_after[~fresh] > m_after[fresh].flatten()[0]).all()                                     # carried over
    gen1 = group.generation
    with torch.no_grad():
        model.fg.params["opacities"][::2] = -10.0  # sigmoid -> far below the cull threshold
    n_cull = cull_step(model, stats, optimizers, ControlCfg(), global_step=2)
    assert n_cull > 0
    step_with_unit_grads()
    torch.cuda.synchronize()
    p_c = h.param_groups[0]["params"][0]
    assert group.generation > gen1 and p_c.shape[0] < p_new.shape[0] and float(h.state[p_c]["step"]) == 3.0
    assert h.state[p_c]["exp_avg"].shape == p_c.shape and torch.isfinite(p_c).all()


def test_example_trains_with_hip_adam_inside_the_graph():
    """examples/train_dynamic_step.py, 12 steps at the size of the existing example test: `graph=True, hip_adam=True` (the whole
    step, optimizers included, replayed from one graph) reduces the loss like `graph=True` alone does.  Reference for the final
    loss: the eager run with torch's fused Adam (what the example did before this option existed).  Allowed difference to it:
    the spread that eager run itself shows between two seeds of the synthetic scene (seed 0 and seed 2; computed here, every
    figure is printed before the assertions).  NOT YET RECORDED: no GPU run of this test could be made when it was written, so
    the spread's value is not stated here - record the printed figures in this docstring and in DESIGN.md section 13 from the
    first GPU run."""
    mod = _example()
    kw = dict(steps=12, W=128, H=96, n_fg=3000, n_bg=5000, K=6, verbose=False)
    parent = mod.train(**kw)[0]
    parent_seed2 = mod.train(seed=2, **kw)[0]
    graph_torch = mod.train(graph=True, **kw)[0]
    graph_hip = mod.train(graph=True, hip_adam=True, **kw)[0]
    eager_hip = mod.train(hip_adam=True, **kw)[0]
    spread = abs(parent[-1] - parent_seed2[-1])
    print("final losses: eager fused", parent[-1], "| eager fused, seed 2", parent_seed2[-1], "| graph + torch Adam", graph_torch[-1],
          "| graph + HIP Adam", graph_hip[-1], "| eager + HIP Adam", eager_hip[-1], "| seed spread", spread)
    for losses in (graph_hip, eager_hip, graph_torch):
        assert all(l == l and l < 1e3 for l in losses)
        assert losses[-1] < 0.9 * losses[0], losses
    assert abs(graph_hip[-1] - parent[-1]) <= spread
    assert abs(graph_torch[-1] - parent[-1]) <= spread
    assert abs(eager_hip[-1] - parent[-1]) <= spread
