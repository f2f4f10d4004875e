"""deblur4dgs_amd.losses.motion_regularizers on the GPU (csrc/motion_regs.hip on the pose kernels) against the values recorded from
the reference's own functions (tests/golden/motion_regs.npz) and, beyond them, against the fp64 restatement tests/motion_ref.py,
which tests/test_motion_ref.py pins to the same fixture.

Bound: tests.util.check, 1e-4 * max|ref| per tensor with no flip allowance - nothing discrete sits on this path.  Inputs are made in
fp32 and the fp64 side gets those same values, so the two differ in arithmetic only.  Random cases are drawn like the fixture's and
held to the fixture's conditioning (tests/golden/gen_motion_regs.py: every track and basis acceleration >= 0.05, every Gaussian >= 0.5
from every camera centre, |means| <= 4; the seed advances until they hold, judged on the fp64 values alone), so that a unit vector
a / |a| is as well determined in fp32 as it is in fp64."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from deblur4dgs_amd import engine
from deblur4dgs_amd.losses import motion_regularizers, scene_motion_regularizers
from tests import motion_ref as M
from tests.util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAVES = ("means", "motion_coefs", "rots", "transls", "scales")
ARGS = LEAVES + ("ts", "w2cs")
TERMS = ("smooth_bases", "smooth_tracks", "z_accel", "scale_var")
MIX = (1.3, 0.7, 2.1, 0.9)
CASES = ("default_small", "block_edges", "one", "many_times", "static_bases", "linear_rows")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "motion_regs.npz"))


def mixed(terms):
    return sum(w * t for w, t in zip(MIX, terms))


def on_gpu(case, dtype=torch.float32, **kw):
    """case: dict of CPU tensors -> ([four values], [five gradients of the mix]) on the CPU"""
    c = {k: case[k].detach().to(DEV, dtype) for k in ARGS}
    for k in LEAVES:
        c[k].requires_grad_()
    terms = motion_regularizers(*[c[k] for k in ARGS], **kw)
    grads = torch.autograd.grad(mixed(terms), [c[k] for k in LEAVES])
    return [t.detach().cpu() for t in terms], [g.cpu() for g in grads]


def on_ref(case, **kw):
    c = {k: case[k].detach().double() for k in ARGS}
    for k in LEAVES:
        c[k].requires_grad_()
    terms = M.motion_regularizers(*[c[k] for k in ARGS], **kw)
    grads = torch.autograd.grad(mixed(terms), [c[k] for k in LEAVES])
    return [t.detach() for t in terms], list(grads)


def compare(name, got, want):
    for t_name, a, b in zip(TERMS, got[0], want[0]):
        assert a.dim() == 0 and a.dtype == torch.float32
        check(name, t_name, a, b)
    for k, a, b in zip(LEAVES, got[1], want[1]):
        assert a.shape == b.shape and torch.isfinite(a).all()
        check(name, f"grad {k}", a, b)


def random_case(G, K, T, ts, seed):
    """fp32 inputs drawn like the fixture's (module docstring); the seed advances until the fp64 values are well conditioned"""
    for attempt in range(200):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        rn = lambda *s: torch.randn(*s, generator=g)
        B = len(ts)
        w2cs = torch.eye(4).repeat(B, 1, 1)
        for b in range(B):
            q, r = torch.linalg.qr(rn(3, 3))
            w2cs[b, :3, :3] = q * torch.sign(torch.diagonal(r)) + (0.1 * rn(3, 3) if b % 2 else 0.0)  # every other one off orthonormal
            w2cs[b, :3, 3] = torch.tensor([0.0, 0.0, 7.0]) + 0.5 * rn(3)
        c = dict(means=2.0 * torch.rand(G, 3, generator=g) - 1.0, motion_coefs=rn(G, K), scales=-3.0 + 0.7 * rn(G, 3),
                 rots=torch.tensor([1.0, 0, 0, 0, 1, 0]) + 0.3 * rn(K, T, 6), transls=0.8 * rn(K, T, 3),
                 ts=torch.tensor(ts, dtype=torch.float32), w2cs=w2cs)
        d = {k: v.double() for k, v in c.items()}
        m0, m1, m2 = M.neighbour_means(d["means"], d["motion_coefs"], d["rots"], d["transls"], d["ts"])
        ok = (2 * m1 - m0 - m2).norm(dim=-1).min() >= 0.05 and M.accel_norms(d["rots"]).min() >= 0.05 and \
            M.accel_norms(d["transls"]).min() >= 0.05 and (m1 - M.camera_centres(d["w2cs"])).norm(dim=-1).min() >= 0.5 and \
            max(m0.abs().max(), m1.abs().max(), m2.abs().max()) <= 4.0
        if ok:
            return c
    raise AssertionError((G, K, T, ts, seed))


# ---- 1. fixture parity --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_matches_the_values_recorded_from_the_reference(golden, name):
    case = {k: torch.tensor(golden[f"{name}/{k}"]) for k in ARGS}
    got = on_gpu(case)
    want = ([torch.tensor(golden[f"{name}/{t}"]) for t in TERMS], [torch.tensor(golden[f"{name}/grad/{k}"]) for k in LEAVES])
    compare(f"motion_regs {name}", got, want)
    zero = torch.zeros(())
    if name == "static_bases":  # exact zeros, not small numbers: m0, m1, m2 are the same bits and a zero norm has a zero gradient
        for t_name, t in zip(TERMS[:3], got[0]):
            assert torch.equal(t, zero), t_name
        for k, g in zip(LEAVES, got[1]):
            assert torch.equal(g, torch.zeros_like(g)) != (k == "scales"), k
    if name == "linear_rows":  # the two straight rows have norm exactly 0 in fp32 as well; their neighbours' gradients stay finite
        r, t = case["rots"], case["transls"]
        assert torch.equal(M.accel_norms(r)[1, 2], zero) and torch.equal(M.accel_norms(t)[0, 1], zero)
        assert float(got[0][0]) > 1.0 and torch.isfinite(got[1][2]).all() and torch.isfinite(got[1][3]).all()


def test_each_term_sends_its_own_gradient(golden):
    """block_edges: the upstream gradient of one term at a time (the others get an explicit zero cotangent)"""
    name = "block_edges"
    c = {k: torch.tensor(golden[f"{name}/{k}"]).to(DEV) for k in ARGS}
    for k in LEAVES:
        c[k].requires_grad_()
    terms = motion_regularizers(*[c[k] for k in ARGS])
    for i, t_name in enumerate(TERMS):
        grads = torch.autograd.grad(terms[i], [c[k] for k in LEAVES], retain_graph=True)
        for k, g in zip(LEAVES, grads):
            ref = torch.tensor(golden[f"{name}/grad_{t_name}/{k}"])
            if ref.any():
                check(f"motion_regs {name} {t_name} alone", f"grad {k}", g.cpu(), ref)
            else:
                assert torch.equal(g.cpu(), torch.zeros_like(ref)), (t_name, k)


# ---- 2. beyond the fixture ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8, 9, 20])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 257])
def test_block_edges_and_basis_counts_against_the_restatement(G, K):
    case = random_case(G, K, 5, [1.0, 2.6], 7 * G + K)
    compare(f"motion_regs G={G} K={K}", on_gpu(case), on_ref(case))


def test_three_frames_every_time_clamps_to_the_middle():
    case = random_case(100, 4, 3, [0.0, 1.0, 2.0, 5.5], 11)
    got = on_gpu(case)
    compare("motion_regs T=3", got, on_ref(case))
    same = on_gpu(dict(case, ts=torch.ones(4)))
    for a, b in zip(got[0] + got[1], same[0] + same[1]):
        assert torch.equal(a, b)


def test_weights_of_the_two_halves():
    case = random_case(40, 3, 6, [2.0], 5)
    compare("motion_regs weights 0.3, 5", on_gpu(case, weight_rot=0.3, weight_transl=5.0), on_ref(case, weight_rot=0.3, weight_transl=5.0))


# ---- 3. the eager-torch formulation on the pose API ---------------------------------------------------------
def _example():
    spec = importlib.util.spec_from_file_location("train_dynamic_step_motion", os.path.join(ROOT, "examples", "train_dynamic_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model(case, n_bg=0):
    from deblur4dgs_amd.scene_model import GaussianParams, MotionBases, SceneModel

    G = case["means"].shape[0]
    g = torch.Generator().manual_seed(G)
    rest = lambda n: (torch.randn(n, 4, generator=g), torch.randn(n, 3, generator=g), torch.randn(n, generator=g))
    q, col, op = rest(G)
    fg = GaussianParams(case["means"].clone(), q, case["scales"].clone(), col, op, motion_coefs=case["motion_coefs"].clone())
    bg = None
    if n_bg:
        q, col, op = rest(n_bg)
        bg = GaussianParams(torch.randn(n_bg, 3, generator=g), q, torch.randn(n_bg, 3, generator=g), col, op)
    Ks = torch.tensor([[64.0, 0, 32], [0, 64.0, 24], [0, 0, 1]])[None]
    return SceneModel(Ks, torch.eye(4)[None], fg, MotionBases(case["rots"].clone(), case["transls"].clone()), bg).to(DEV)


@pytest.mark.parametrize("G,K,T,ts", [(300, 6, 10, [2.0, 5.0]), (130, 20, 12, [0.0, 4.37, 11.0])])
def test_agrees_with_the_eager_torch_formulation_on_the_pose_api(G, K, T, ts):
    """compute_transforms(cat(ts - 1, ts, ts + 1)) + einsum + norms + torch.linalg.inv, as a trainer writes it today
    (tests/test_gpu_poses.py::test_trainer_style_use_of_the_pose_api; examples/train_dynamic_step.py's comparator)"""
    case = random_case(G, K, T, ts, 300 + G)
    model = _model(case, n_bg=50)
    tsd, w2cs = case["ts"].to(DEV), case["w2cs"].to(DEV)
    leaves = [model.fg.params["means"], model.fg.params["motion_coefs"], model.motion_bases.params["rots"],
              model.motion_bases.params["transls"], model.fg.params["scales"]]
    got = scene_motion_regularizers(model, tsd, w2cs)
    want = _example().torch_motion_regularizers(model, tsd, w2cs)
    g_got = torch.autograd.grad(mixed(got), leaves)
    g_want = torch.autograd.grad(mixed(want), leaves)
    name = f"motion_regs vs eager torch G={G} K={K}"
    compare(name, ([t.detach().cpu() for t in got], [g.cpu() for g in g_got]), ([t.detach().cpu() for t in want], [g.cpu() for g in g_want]))


# ---- 4. reproducibility -------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal():
    case = random_case(1500, 20, 9, [1.0, 3.3, 7.0], 77)
    a, b = on_gpu(case), on_gpu(case)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(x, y)
    assert all(g.any() for g in a[1])


# ---- 5. autograd plumbing -----------------------------------------------------------------------------------
def test_only_the_leaves_that_ask_get_a_gradient():
    case = random_case(70, 9, 6, [2.0, 3.0], 21)
    full = on_gpu(case)
    c = {k: case[k].to(DEV) for k in ARGS}
    c["rots"].requires_grad_()
    terms = motion_regularizers(*[c[k] for k in ARGS])
    mixed(terms).backward()
    assert torch.equal(c["rots"].grad.cpu(), full[1][2])
    assert all(c[k].grad is None for k in ARGS if k != "rots")
    # ts and w2cs are data: no gradient even when they ask
    for k in ARGS:
        c[k] = c[k].detach().requires_grad_()
    grads = torch.autograd.grad(mixed(motion_regularizers(*[c[k] for k in ARGS])), [c[k] for k in ARGS], allow_unused=True)
    assert grads[5] is None and grads[6] is None and all(g is not None for g in grads[:5])
    # without any gradient the outputs are plain tensors
    with torch.no_grad():
        plain = motion_regularizers(*[c[k] for k in ARGS])
    assert not any(t.requires_grad for t in plain) and all(torch.equal(t.cpu(), f) for t, f in zip(plain, full[0]))


def test_a_leaf_changed_in_place_before_the_backward_is_detected():
    case = random_case(70, 9, 6, [2.0, 3.0], 21)
    c = {k: case[k].to(DEV) for k in ARGS}
    for k in LEAVES:
        c[k].requires_grad_()
    terms = motion_regularizers(*[c[k] for k in ARGS])
    with torch.no_grad():
        c["rots"].mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        mixed(terms).backward()


def test_non_contiguous_float64_and_integer_inputs():
    case = random_case(70, 9, 6, [2.0, 3.0], 21)
    full = on_gpu(case)
    c = {}
    for k in ARGS:  # every second column of a wider float64 tensor
        wide = torch.zeros(*case[k].shape[:-1], 2 * case[k].shape[-1], dtype=torch.float64, device=DEV)
        wide[..., ::2] = case[k].to(DEV)
        c[k] = wide[..., ::2]
        assert not c[k].is_contiguous() or c[k].shape[-1] == 1
    c["ts"] = torch.tensor([2, 3], dtype=torch.int64, device=DEV)  # frame indices as the reference's batches hold them
    for k in LEAVES:
        c[k].requires_grad_()
    terms = motion_regularizers(*[c[k] for k in ARGS])
    grads = torch.autograd.grad(mixed(terms), [c[k] for k in LEAVES])
    for t, f in zip(terms, full[0]):
        assert torch.equal(t.detach().cpu(), f)
    for k, g, f in zip(LEAVES, grads, full[1]):
        assert g.dtype == torch.float64 and g.shape == c[k].shape and torch.equal(g.float().cpu(), f), k


def test_value_errors_and_cpu_tensors():
    case = random_case(6, 3, 5, [1.0, 2.0], 3)
    dev = {k: case[k].to(DEV) for k in ARGS}
    call = lambda **kw: motion_regularizers(*[{**dev, **kw}[k] for k in ARGS])
    for kw in (dict(means=dev["means"][:0], motion_coefs=dev["motion_coefs"][:0], scales=dev["scales"][:0]),  # G == 0
               dict(rots=dev["rots"][:, :2], transls=dev["transls"][:, :2]),  # T < 3
               dict(motion_coefs=dev["motion_coefs"][:, :2]), dict(transls=dev["transls"][:, :4]), dict(transls=dev["transls"][:2]),
               dict(w2cs=dev["w2cs"][:1]), dict(ts=dev["ts"][:1]), dict(scales=dev["scales"][:5])):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(RuntimeError, match="ROCm"):
        call(w2cs=case["w2cs"])
    assert all(math.isfinite(float(t)) for t in call())


# ---- 6. graph capture ---------------------------------------------------------------------------------------
def _fwd_bwd(c):
    terms = motion_regularizers(*[c[k] for k in ARGS])
    grads = torch.autograd.grad(mixed(terms), [c[k] for k in LEAVES])
    return [t.detach() for t in terms] + list(grads)


def test_graph_capture_and_replay_after_an_in_place_update():
    """Forward and backward in ONE captured graph (capture aborts on any host wait: this is the test that the path has none).  A
    replay after `means` and `rots` changed in place equals the eager call on the new values bit for bit."""
    case = random_case(700, 12, 8, [1.0, 4.5], 41)
    fresh = random_case(700, 12, 8, [1.0, 4.5], 42)
    static = {k: case[k].to(DEV) for k in ARGS}
    for k in LEAVES:
        static[k].requires_grad_()
    _fwd_bwd(static)  # warm-up: code objects loaded, nothing lazy left inside the capture
    torch.cuda.synchronize()
    g, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with engine.GraphWatch().capturing(), torch.cuda.graph(g, stream=stream):
        out = _fwd_bwd(static)
    g.replay()
    torch.cuda.synchronize()
    first = [o.clone() for o in out]
    with torch.no_grad():
        static["means"].copy_(fresh["means"])
        static["rots"].copy_(fresh["rots"])
    g.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in out]
    for values, old in ((dict(case, means=fresh["means"], rots=fresh["rots"]), False), (case, True)):
        c = {k: values[k].to(DEV) for k in ARGS}
        for k in LEAVES:
            c[k].requires_grad_()
        eager = _fwd_bwd(c)
        for i, (x, y) in enumerate(zip(first if old else replayed, eager)):
            assert torch.equal(x, y), (old, i, x.flatten()[:4], y.flatten()[:4])
    assert not torch.equal(first[1], replayed[1]) and all(torch.isfinite(o).all() for o in replayed)


# ---- 7. the example -----------------------------------------------------------------------------------------
def _train_keeping_the_model(mod, **kw):
    """mod.train(**kw) -> (losses, [the models it built]): train() builds the model it trains first, then the one that renders its
    targets"""
    models, build = [], mod.build

    def keeping_build(*a, **k):
        out = build(*a, **k)
        models.append(out[0])
        return out

    mod.build = keeping_build
    try:
        return mod.train(**kw)[0], models
    finally:
        mod.build = build


def test_example_trains_with_the_motion_regularizers_inside_the_graph():
    """examples/train_dynamic_step.py with motion_regs=True on a small scene: the whole step captures after two eager steps and
    replays; the losses are finite and go down, the motion bases receive a gradient, and the first (eager) step's loss equals the one
    with the eager-torch formulation of the four terms within the bound of this file."""
    mod = _example()
    kw = dict(steps=6, W=128, H=96, n_fg=3000, n_bg=5000, K=6, verbose=False, hip_adam=True)
    graph, models = _train_keeping_the_model(mod, graph=True, motion_regs=True, **kw)
    torch_form = mod.train(steps=1, motion_regs="torch", **{k: v for k, v in kw.items() if k != "steps"})[0]
    plain = mod.train(steps=1, **{k: v for k, v in kw.items() if k != "steps"})[0]
    print("graph", graph, "| eager torch form, step 0", torch_form[0], "| without the regularizers, step 0", plain[0])
    assert all(math.isfinite(l) for l in graph) and graph[-1] < graph[0]
    for p in models[0].motion_bases.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    assert abs(graph[0] - torch_form[0]) <= 1e-4 * abs(torch_form[0])
    assert graph[0] > plain[0]  # four non-negative terms were added
    with pytest.raises(AssertionError, match="cannot be captured"):
        mod.train(graph=True, motion_regs="torch", **kw)
