"""N>1 path on CPU: world_size-2 (and 3) `gloo` processes run the exposure-sharded blend + flat gradient
all-reduce and must reproduce the single-process blend of the reference (oracle/scene.py:blend_exposure,
which restates flow3d/scene_model.py:386-397 literally) - forward and backward."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _by_value(items):
    """Tensors cross the queue as numpy arrays (pickled by value).  A torch tensor is passed as a file descriptor the
    receiver has to fetch from the SENDER - which has usually exited by then (ConnectionResetError / FileNotFoundError)."""
    return tuple(x.numpy() if torch.is_tensor(x) else x for x in items)


def _tensors(items):
    import numpy as np

    return tuple(torch.from_numpy(x) if isinstance(x, np.ndarray) else x for x in items)


def _worker(rank, world, port, S, C, seed, q, dtype=torch.float64):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deblur4dgs_amd.exposure import reference_policy
    from deblur4dgs_amd.parallel import FlatGradAllReduce, ShardedBlendFn, owned_subsamples

    g = torch.Generator().manual_seed(seed)
    H, W = 6, 5
    renders = torch.rand(S, H, W, C, generator=g, dtype=dtype)
    renders[:, 0, 0, 3] = 0.0  # exact ties on the max-policy channel (e.g. mask == 0 everywhere)
    renders[S - 1, 1, 1, 3] = 5.0  # the LAST sub-sample holds the max: the reference takes max{raw_0..S-2, mean}
    alphas = torch.rand(S, H, W, generator=g, dtype=dtype)
    wb = torch.randn(H, W, C, generator=g, dtype=dtype)
    wa = torch.randn(H, W, generator=g, dtype=dtype)
    scale = torch.ones(S, dtype=dtype, requires_grad=True)  # a "leaf" every sub-sample depends on
    own = owned_subsamples(S, world, rank)
    loc = (renders[own] * scale[own].view(-1, 1, 1, 1)).requires_grad_() if False else renders[own] * scale[own].view(-1, 1, 1, 1)
    loc.retain_grad()
    la = alphas[own].clone().requires_grad_()
    out, acc = ShardedBlendFn.apply(loc, la, own, S, reference_policy(C), None)
    ((out * wb).sum() + (acc * wa).sum()).backward()
    leaves = {"scale": scale}
    FlatGradAllReduce(leaves).reduce(leaves)
    q.put(_by_value((rank, own, out.detach(), acc.detach(), loc.grad.clone(), la.grad.clone(), scale.grad.clone())))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,S,C", [(2, 8, 17), (2, 5, 5), (3, 7, 4), (2, 1, 5), (2, 2, 17)])
def test_sharded_blend_matches_reference_blend(world, S, C):
    from oracle import scene as oscene

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, S, C, 11, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [_tensors(q.get(timeout=120)) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    g = torch.Generator().manual_seed(11)
    H, W = 6, 5
    renders = torch.rand(S, H, W, C, generator=g, dtype=torch.float64)
    renders[:, 0, 0, 3] = 0.0
    renders[S - 1, 1, 1, 3] = 5.0
    alphas = torch.rand(S, H, W, generator=g, dtype=torch.float64)
    wb = torch.randn(H, W, C, generator=g, dtype=torch.float64)
    wa = torch.randn(H, W, generator=g, dtype=torch.float64)
    scale = torch.ones(S, dtype=torch.float64, requires_grad=True)
    r = (renders * scale.view(-1, 1, 1, 1))
    r.retain_grad()
    a = alphas.clone().requires_grad_()
    blended, acc, _ = oscene.blend_exposure([r[s][None] for s in range(S)], [a[s][None] for s in range(S)], single=(S == 1))
    ((blended[0] * wb).sum() + (acc[0] * wa).sum()).backward()
    # fp64; the sharded sum adds the sub-samples in a different (and, for world > 2, run-dependent) order than the
    # stacked reference: a few ulps of values up to ~10, hence 1e-12 rather than bitwise
    for rank, own, out, acc_r, gr, ga, gscale in res:
        torch.testing.assert_close(out, blended[0].detach(), rtol=0, atol=1e-12)
        torch.testing.assert_close(acc_r, acc[0].detach(), rtol=0, atol=1e-12)
        torch.testing.assert_close(gr, r.grad[own], rtol=0, atol=1e-12)
        torch.testing.assert_close(ga, a.grad[own], rtol=0, atol=1e-12)
        torch.testing.assert_close(gscale, scale.grad, rtol=0, atol=1e-11)  # all-reduced leaf gradient


@pytest.mark.parametrize("world,S,C", [(2, 8, 5), (3, 6, 17)])
def test_reduce_blend_in_fp32_equals_the_single_process_blend_within_summation_order(world, S, C):
    """The DEFAULT forward collective of exposure sharding: SUM all-reduce of [H,W,D'+1] + MAX all-reduce of the
    policy channels, in the path's own precision (fp32).  It adds the sub-samples in a different order than the stacked
    single-process blend (rank-local partial sums first), so equality is up to fp32 summation order: the stated
    tolerance is 2e-6 * max|value| (S <= 16 terms of magnitude <= max: a few ulps) for the image, the accumulation and
    every local gradient; the gathered-stack path below keeps the bitwise claim."""
    from oracle import scene as oscene

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, S, C, 17, q, torch.float32)) for r in range(world)]
    for p in procs:
        p.start()
    res = [_tensors(q.get(timeout=120)) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g = torch.Generator().manual_seed(17)
    H, W = 6, 5
    renders = torch.rand(S, H, W, C, generator=g, dtype=torch.float32)
    renders[:, 0, 0, 3] = 0.0
    renders[S - 1, 1, 1, 3] = 5.0
    alphas = torch.rand(S, H, W, generator=g, dtype=torch.float32)
    wb = torch.randn(H, W, C, generator=g, dtype=torch.float32)
    wa = torch.randn(H, W, generator=g, dtype=torch.float32)
    r = renders.double().requires_grad_()
    a = alphas.double().requires_grad_()
    blended, acc, _ = oscene.blend_exposure([r[s][None] for s in range(S)], [a[s][None] for s in range(S)], single=(S == 1))
    ((blended[0] * wb.double()).sum() + (acc[0] * wa.double()).sum()).backward()
    TOL = 2e-6
    for rank, own, out, acc_r, gr, ga, _gscale in res:
        assert out.dtype == torch.float32
        for got, want in ((out, blended[0]), (acc_r, acc[0]), (gr, r.grad[own]), (ga, a.grad[own])):
            want = want.detach()
            assert float((got.double() - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))


def _oracle_blend(renders, alphas, policy):
    """(stack [S,H,W,C], alphas [S,H,W], policy) -> (out [H,W,C], acc [H,W]) through oracle/scene.py's literal
    restatement of scene_model.py:386-397 (the policy IS the reference's: channel 3 max, 16 min)."""
    from oracle import scene as oscene

    S = renders.shape[0]
    blended, acc, _ = oscene.blend_exposure([renders[s][None] for s in range(S)], [alphas[s][None] for s in range(S)],
                                            single=(S == 1))
    return blended[0], acc[0]


def _gather_worker(rank, world, port, S, C, seed, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deblur4dgs_amd.exposure import reference_policy
    from deblur4dgs_amd.parallel import FlatGradAllReduce, GatherBlendFn, owned_subsamples

    g = torch.Generator().manual_seed(seed)
    H, W = 6, 5
    renders = torch.rand(S, H, W, C, generator=g, dtype=torch.float64)
    renders[:, 0, 0, 3] = 0.0
    renders[S - 1, 1, 1, 3] = 5.0
    alphas = torch.rand(S, H, W, generator=g, dtype=torch.float64)
    wb = torch.randn(H, W, C, generator=g, dtype=torch.float64)
    wa = torch.randn(H, W, generator=g, dtype=torch.float64)
    ws = torch.randn(S, H, W, C + 1, generator=g, dtype=torch.float64)  # a loss on the per-sub-sample stack too
    scale = torch.ones(S, dtype=torch.float64, requires_grad=True)
    means = torch.ones(3, dtype=torch.float64, requires_grad=True)      # a "per-Gaussian" leaf: early async all-reduce
    own = owned_subsamples(S, world, rank)
    loc = renders[own] * scale[own].view(-1, 1, 1, 1) * means.sum() / 3.0
    loc.retain_grad()
    la = alphas[own].clone().requires_grad_()
    out, acc, stack_r, stack_a = GatherBlendFn.apply(loc, la, S, reference_policy(C), None, _oracle_blend)
    stack = torch.cat([stack_r, stack_a[..., None]], -1)
    leaves = {"scale": scale, "means": means}
    red = FlatGradAllReduce(leaves)
    red.arm(leaves)
    ((out * wb).sum() + (acc * wa).sum() + (stack * ws).sum()).backward()
    armed = red._work is not None
    red.reduce(leaves)
    q.put(_by_value((rank, own, out.detach(), acc.detach(), stack.detach(), loc.grad.clone(), la.grad.clone(),
                     scale.grad.clone(), means.grad.clone(), armed)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,S,C", [(2, 8, 17), (2, 2, 5), (3, 6, 4), (2, 4, 20)])
def test_gather_blend_equals_the_single_process_blend_bitwise(world, S, C):
    """The default exposure-sharded blend: one all-gather, then the single-process blend on the full stack - outputs
    and local gradients are BITWISE those of the single-process run (same summation order), and the flat gradient
    reducer's early asynchronous piece fires from autograd's hooks."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, S, C, 13, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [_tensors(q.get(timeout=120)) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    g = torch.Generator().manual_seed(13)
    H, W = 6, 5
    renders = torch.rand(S, H, W, C, generator=g, dtype=torch.float64)
    renders[:, 0, 0, 3] = 0.0
    renders[S - 1, 1, 1, 3] = 5.0
    alphas = torch.rand(S, H, W, generator=g, dtype=torch.float64)
    wb = torch.randn(H, W, C, generator=g, dtype=torch.float64)
    wa = torch.randn(H, W, generator=g, dtype=torch.float64)
    ws = torch.randn(S, H, W, C + 1, generator=g, dtype=torch.float64)
    scale = torch.ones(S, dtype=torch.float64, requires_grad=True)
    means = torch.ones(3, dtype=torch.float64, requires_grad=True)
    r = renders * scale.view(-1, 1, 1, 1) * means.sum() / 3.0
    r.retain_grad()
    a = alphas.clone().requires_grad_()
    blended, acc = _oracle_blend(r, a, None)
    stack = torch.cat([r, a[..., None]], -1)
    ((blended * wb).sum() + (acc * wa).sum() + (stack * ws).sum()).backward()
    for rank, own, out, acc_r, st, gr, ga, gscale, gmeans, armed in res:
        assert own == list(range(rank, S, world)) and armed
        assert torch.equal(out, blended.detach()) and torch.equal(acc_r, acc.detach()) and torch.equal(st, stack.detach())
        assert torch.equal(gr, r.grad[own]) and torch.equal(ga, a.grad[own])
        # replicated loss, every rank differentiates its own sub-samples: the all-reduced leaf gradients are the totals
        torch.testing.assert_close(gscale, scale.grad, rtol=0, atol=1e-12)
        torch.testing.assert_close(gmeans, means.grad, rtol=1e-12, atol=1e-9)


def _toy_render(means, quats, scales, opacities, colors, n_sig, motion_coefs, rots, transls, times, RTs, viewmat, Kmat, Wd, Hd,
                background=None, blend=True, **_kw):
    """A differentiable stand-in for render_exposure on CPU tensors (the N > 1 logic is what is under test, not the kernels):
    [S_loc,H,W,4] images that depend non-linearly on every leaf and differently on every sub-sample, so that the max-policy
    channel (3) has a different winner per pixel and every collective of the sharded step carries real data."""
    import types

    from oracle import scene as oscene

    g = torch.Generator().manual_seed(23)
    base = torch.rand(Hd, Wd, 4, generator=g, dtype=means.dtype)
    phase = torch.rand(Hd, Wd, 4, generator=g, dtype=means.dtype) * 6.0
    per_g = sum((t * t).mean() for t in (means, quats, scales, opacities, colors, motion_coefs))
    shared = rots.mean() + transls.square().mean() + viewmat.mean()
    gain = times * 1.7 + RTs.reshape(RTs.shape[0], -1).sum(-1)  # [S_loc]
    renders = base[None] * torch.sin(phase[None] + gain.view(-1, 1, 1, 1)) + 0.3 * (per_g + shared) * torch.cos(gain).view(-1, 1, 1, 1)
    alphas = torch.sigmoid(base[None, ..., :1] + gain.view(-1, 1, 1, 1) * per_g)
    st = types.SimpleNamespace(n_isect=0)
    out = dict(renders=renders, alphas=alphas, state=st, blended=None, acc=None)
    if blend:
        S = renders.shape[0]
        b, a, _ = oscene.blend_exposure([renders[s][None] for s in range(S)], [alphas[s, ..., 0][None] for s in range(S)], single=(S == 1))
        out["blended"], out["acc"] = b[0], a[0]
    return out


def _toy_leaves(S, dtype=torch.float64):
    g = torch.Generator().manual_seed(5)
    shp = dict(means=(7, 3), quats=(7, 4), scales=(7, 3), opacities=(7,), colors=(7, 3), motion_coefs=(7, 2), rots=(2, 3, 6),
               transls=(2, 3, 3), times=(S,), RTs=(S, 3, 4), viewmat=(4, 4))
    return {k: torch.randn(*v, generator=g, dtype=dtype).requires_grad_() for k, v in shp.items()}


def _toy_targets(v, H, W, dtype=torch.float64):
    g = torch.Generator().manual_seed(100 + v)
    return torch.randn(H, W, 4, generator=g, dtype=dtype), torch.randn(H, W, generator=g, dtype=dtype)


def _mesh_worker(rank, world, port, V, E, S, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deblur4dgs_amd.parallel import ShardedExposure, mesh_coords

    H, W = 6, 5
    leaves = _toy_leaves(S)
    v, e = mesh_coords(world, rank, V, E)
    wimg, wacc = _toy_targets(v, H, W)
    sh = ShardedExposure(world, rank, mode="mesh", mesh=(V, E))
    sh.render = _toy_render
    for _ in range(2):  # twice: the second step starts from .grad tensors that alias the flat all-reduce buffer
        sh.step(leaves, None, W, H, None, wimg, wacc)
    q.put(_by_value((rank, v, e, *[leaves[k].grad.clone() for k in sorted(leaves)])))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("V,E,S", [(2, 2, 8), (2, 1, 3), (1, 2, 5)])
def test_views_x_exposure_mesh_equals_the_single_process_gradients(V, E, S):
    """VERDICT r4 #1b: a V x E mesh - V camera views, each view's S exposure sub-samples split E ways.  The blend collectives
    (SUM / MAX forward, MIN backward) run inside the view's exposure sub-group (dist.new_group), the flat gradient all-reduce
    over the world, 1 / V on the loss.  Every rank must end with the gradient of mean_v loss_v(full S-sample blend of view v),
    computed here in ONE process with the literal restatement of the reference blend (oracle/scene.py)."""
    world = V * E
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mesh_worker, args=(r, world, port, V, E, S, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [_tensors(q.get(timeout=180)) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    H, W = 6, 5
    leaves = _toy_leaves(S)
    total = 0.0
    for v in range(V):
        wimg, wacc = _toy_targets(v, H, W)
        r = _toy_render(*[leaves[k] for k in ("means", "quats", "scales", "opacities", "colors")], 3,
                        *[leaves[k] for k in ("motion_coefs", "rots", "transls", "times", "RTs", "viewmat")], None, W, H, blend=True)
        total = total + ((r["blended"] * wimg).sum() + (r["acc"] * wacc).sum()) / V
    total.backward()
    seen = set()
    for rank, v, e, *grads in res:
        seen.add((v, e))
        for k, g in zip(sorted(leaves), grads):
            want = leaves[k].grad
            assert float((g - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max())), (rank, k)
    assert seen == {(v, e) for v in range(V) for e in range(E)}


def test_owned_subsamples_partition():
    from deblur4dgs_amd.parallel import owned_subsamples

    for S in (1, 8, 11, 16):
        for world in (1, 2, 4, 8):
            allv = sorted(s for r in range(world) for s in owned_subsamples(S, world, r))
            assert allv == list(range(S))


def _run_bench_dry(n, flags, env=None, timeout=600):
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "1",
           "--dry-run", *flags]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=root, env={**os.environ, **(env or {})})
    assert r.returncode == 0, r.stderr[-3000:]
    # gloo prints its own connection banner on stdout, and the ranks' banners may interleave inside a line
    # (seen once under load: a banner glued to the front of the JSON line - so the line is taken from its first brace)
    lines = [ln[ln.index("{"):] for ln in r.stdout.splitlines() if '"metric"' in ln and "{" in ln]
    assert len(lines) == 1, r.stdout  # the contract: ONE JSON line, from rank 0
    d = json.loads(lines[0][:lines[0].rindex("}") + 1])
    assert d["n_gpus"] == n and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["data"].startswith("dry-run")
    return d, r.stderr


@pytest.mark.parametrize("flags,expect_launch", [(["--no-graph"], "eager step (--no-graph)"), ([], "graph capture failed")])
def test_bench_n_gt_1_control_flow_runs_on_gloo(flags, expect_launch):
    """the first multi-GPU SCALE run must not also be the first run of bench.py's N > 1 code.  `--dry-run` drives
    exactly that code on CPU tensors over gloo, launched the way the driver launches it (torch.distributed.run, one process per
    "GPU"): process group, the exposure-sharded step with its blend collectives and the armed gradient all-reduce, the eager
    measurement FIRST, then (default path) the graph attempt in which rank 0 fails to capture and the cross-rank MIN agreement must
    send BOTH ranks to the eager step, max-over-ranks timing, the secondary view-sharded measurement - and ONE JSON line on stdout."""
    d, _ = _run_bench_dry(2, ["--full", *flags])
    assert d["scaling"] == "strong" and "cfg4" in d["config"]["parallelism"] and d["config"]["frames_per_step"] == 1
    assert d["views_weak_scaling"]["value"] > 0 and d["views_weak_scaling"]["scaling"] == "weak"
    assert "exposure_strong_scaling" not in d  # (it IS the primary at N = 2)
    assert expect_launch in d["config"]["launch"]  # default: rank 0 could not capture -> every rank timed the eager step


def test_bench_default_at_4_ranks_is_the_strict_cfg4_with_the_mesh_as_a_secondary_object():
    """`--shard auto` (ADVICE r5 / VERDICT r5 #9): the primary line is BASELINE cfg4 in the strict sense at every N - ONE frame, its
    sub-samples over all ranks, strong scaling, value = N / t - so that it means the same thing at N = 2 and N = 8; the (N/2) x 2
    views x exposure mesh (exposure sub-groups from dist.new_group, world gradient all-reduce) and the views-only number ride on
    the same line as secondary objects."""
    d, _ = _run_bench_dry(4, ["--full"])
    tiny_n = d["config"]["gaussians"]
    assert d["scaling"] == "strong" and d["config"]["frames_per_step"] == 1 and "cfg4" in d["config"]["parallelism"]
    assert abs(d["value"] - tiny_n / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert "exposure_strong_scaling" not in d  # (it IS the primary)
    me, vw = d["views_x_exposure_mesh"], d["views_weak_scaling"]
    assert me["scaling"] == "weak" and me["frames_per_step"] == 2 and "mesh 2x2" in me["parallelism"] and "NOT BASELINE cfg4" in me["note"]
    assert abs(me["value"] - 2 * tiny_n / (me["ms_per_step"] * 1e-3)) <= 1e-6 * me["value"]  # whole job: 2 frames per step
    assert vw["scaling"] == "weak" and vw["frames_per_step"] == 4


def test_bench_mesh_as_the_primary_line_when_asked_for():
    d, _ = _run_bench_dry(4, ["--full", "--shard", "mesh", "--mesh", "2x2"])
    assert d["scaling"] == "weak" and d["config"]["frames_per_step"] == 2 and "mesh 2x2" in d["config"]["parallelism"]
    ex = d["exposure_strong_scaling"]
    assert ex["scaling"] == "strong" and ex["frames_per_step"] == 1 and "views_x_exposure_mesh" not in d


def test_bench_plain_run_times_the_primary_only_and_dumps_its_outputs(tmp_path):
    """Without --full the line carries the primary measurement alone (no secondary shardings), and --dump-outputs writes the last
    timed step's leaf gradients (rank 0) as float32 .npy files."""
    import numpy as np

    d, _ = _run_bench_dry(2, ["--dump-outputs", str(tmp_path)])
    assert d["scaling"] == "strong" and "cfg4" in d["config"]["parallelism"]
    assert not {"views_weak_scaling", "views_x_exposure_mesh", "exposure_strong_scaling", "cpu_baseline", "roofline"} & set(d)
    files = sorted(p.name for p in tmp_path.iterdir())
    assert "grad_means.npy" in files and "grad_viewmat.npy" in files, files
    g = np.load(tmp_path / "grad_means.npy")
    assert g.dtype == np.float32 and g.shape == (d["config"]["gaussians"], 3) and np.isfinite(g).all() and np.abs(g).sum() > 0


def test_bench_dump_sample_is_fixed_and_within_the_limit(tmp_path, monkeypatch):
    """--dump-outputs above its size limit: every large array keeps the same seeded sample of its elements, small ones stay whole."""
    import importlib.util

    import numpy as np

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("d4gs_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(3)
    arrays = {"big": torch.randn(300_000, 3, generator=g), "img": torch.randn(64, 96, 4, generator=g).double(),
              "small": torch.randn(11, generator=g)}
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), arrays)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    assert sum(a.nbytes for a in got.values()) <= 1 << 20
    assert got["big"].dtype == np.float32 and got["img"].dtype == np.float64 and 0 < got["big"].size < arrays["big"].numel()
    assert np.array_equal(got["small"], arrays["small"].numpy())
    for k in arrays:
        assert np.array_equal(got[k], np.load(tmp_path / "b" / f"{k}.npy"))
    assert np.isin(got["big"], arrays["big"].numpy().reshape(-1)).all()  # a sample of the array's own elements


def test_bench_prints_the_eager_line_when_the_graph_phase_hangs():
    """a rank that never returns from its capture (D4GS_BENCH_INJECT_HANG=graph: the last rank sleeps
    forever, rank 0 blocks in the agreement all-reduce).  The eager step was measured first; the watchdog must print THAT line - one
    JSON line, `config.launch` saying why - and every rank must leave with exit code 0 long before any collective time-out."""
    import time

    t0 = time.time()
    d, err = _run_bench_dry(2, ["--full", "--graph-timeout", "6"], env={"D4GS_BENCH_INJECT_HANG": "graph"}, timeout=240)
    assert time.time() - t0 < 120
    assert "WATCHDOG" in d["config"]["launch"] and "HIP-graph capture" in d["watchdog_fired_in"]
    assert d["scaling"] == "strong" and "views_weak_scaling" not in d  # nothing after the hung phase ran
    assert "watchdog" in err


def test_bench_leaves_with_exit_code_3_when_the_first_collective_hangs():
    """Nothing has been measured when the EAGER step hangs (communicator bring-up, the first collective): no line can be printed, but
    every rank must still leave on its own - exit code 3, the phase named on stderr - instead of sitting in the collective until the
    backend's own time-out (600 s for RCCL) or the driver's clock."""
    import subprocess
    import sys
    import time

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--dry-run", "--graph-timeout", "4"]
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root, env={**os.environ, "D4GS_BENCH_INJECT_HANG": "eager"})
    assert time.time() - t0 < 120
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")], r.stdout  # no half-measured line
    assert "NO line" in r.stderr and "eager primary step" in r.stderr
