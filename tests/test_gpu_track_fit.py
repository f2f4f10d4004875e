"""deblur4dgs_amd.losses.track_fit_losses and deblur4dgs_amd.scene_init.run_initial_optim on the GPU (csrc/track_fit.hip on the pose
kernels, trimmed.hip's selection, adam.hip's step) against what the reference's own code gave (tests/golden/track_fit.npz) and,
beyond the fixture, against the fp64 restatement tests/track_fit_ref.py, which tests/test_track_fit_ref.py pins to the same fixture.

Bound of the values and gradients: tests.util.check, 1e-4 * max|ref| per tensor with no flip allowance.  Inputs are made in fp32 and
the fp64 side gets those same values, so the two differ in arithmetic only; every case is held to track_fit_ref.gaps_ok on the fp64
values first (the seed advances until it holds), so that no kept-set flip and no sign of an |x| can separate fp32 from fp64.

Bound of the trajectories (fixture (b)): fp32 Adam amplifies the rounding of a gradient element by the inverse of its relative size,
and no bound follows from the formats alone.  TRAJ_BOUND is 4 x the largest deviation measured on an MI355X over the five cases and
four tensors, each relative to that tensor's largest parameter change (TRAJ_MEASURED; DESIGN.md section 27 has the table); the margin
covers the spread of the amplification from case to case.  As a condition, not a measurement: no element may deviate by more than
half of what its param group can travel at all, 0.5 * sum_i lr_r(i)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deblur4dgs_amd import losses
from deblur4dgs_amd import scene_init as S
from deblur4dgs_amd.optim import AdamGroup
from deblur4dgs_amd.scene_model import GaussianParams, MotionBases
from tests import track_fit_ref as R
from tests.util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("default", "general_cam", "one", "t4", "k9", "static_bases", "behind", "blind")
TRAJECTORIES = ("traj_one", "traj_small", "traj_general", "traj_ramp", "traj_ramp_k2")
CHUNK = 4  # frames per block of the second grid dimension (csrc/track_fit.hip, FIT_CHUNK)
# largest |fp32 GPU - fp64 reference| / largest parameter change, per tensor (means, motion_coefs, rots, transls), measured on an MI355X
TRAJ_MEASURED = dict(traj_one=(2.51e-5, 0.0, 3.88e-6, 4.92e-7), traj_small=(2.12e-5, 1.59e-5, 4.31e-6, 1.78e-6),
                     traj_general=(3.77e-5, 4.96e-5, 7.58e-6, 2.20e-6), traj_ramp=(8.52e-6, 0.0, 1.37e-6, 4.64e-7),
                     traj_ramp_k2=(4.17e-6, 1.76e-5, 2.49e-6, 1.02e-6))
TRAJ_BOUND = 4 * max(max(v) for v in TRAJ_MEASURED.values())  # 1.98e-4


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "track_fit.npz"))


def load_case(golden, name):
    return {k: torch.tensor(golden[f"{name}/{k}"]) for k in R.LEAVES + R.DATA}


def targets_of(case):
    tracks = S.TrackObservations(case["xyz"].to(DEV), case["visibles"].to(DEV), case["invisibles"].to(DEV), case["confidences"].to(DEV),
                                 torch.zeros(case["xyz"].shape[0], 3, device=DEV))
    return S.track_fit_targets(tracks, case["Ks"].to(DEV), case["w2cs"].to(DEV)), tracks


def on_gpu(case, mix, quantile=0.95, targets=None):
    """-> (terms [6], the four gradients of (mix * terms).sum()) on the CPU"""
    targets = targets_of(case)[0] if targets is None else targets
    lv = [case[k].to(DEV).requires_grad_() for k in R.LEAVES]
    terms = losses.track_fit_losses(*lv, targets, quantile=quantile)
    assert terms.shape == (6,) and terms.dtype == torch.float32
    grads = torch.autograd.grad((terms * torch.as_tensor(mix, dtype=torch.float32, device=DEV)).sum(), lv)
    return terms.detach().cpu(), [g.cpu() for g in grads]


def compare(name, got, want):
    for i, t_name in enumerate(R.TERMS):
        check(name, t_name, got[0][i], want[0][i])
    for k, a, b in zip(R.LEAVES, got[1], want[1]):
        assert a.shape == b.shape and torch.isfinite(a).all()
        check(name, f"grad {k}", a, b)


# ---- 1. fixture (a) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_matches_the_values_recorded_from_the_reference(golden, name):
    case = load_case(golden, name)
    got = on_gpu(case, golden["mix"])
    want = (torch.tensor(golden[f"{name}/terms"]), [torch.tensor(golden[f"{name}/grad/{k}"]) for k in R.LEAVES])
    compare(f"track_fit {name}", got, want)
    if name == "static_bases":  # exact zeros, not small numbers: the frames of a static basis set are the same bits
        assert torch.equal(got[0][3:], torch.zeros(3))
        _, g = on_gpu(case, (0.0, 0.0, 0.0, 0.9, 1.1, 0.6))  # the three smoothness terms alone: a zero norm has a zero gradient
        for k, x in zip(R.LEAVES, g):
            assert torch.equal(x, torch.zeros_like(x)), k
    if name == "one":  # softmax of one coefficient is 1
        assert float(got[0][2]) == 0.0 and torch.equal(got[1][1], torch.zeros(1, 1))
    if name == "blind":  # a Gaussian without any weight: the two track terms send it nothing
        _, g = on_gpu(case, (1.3, 0.7, 0.0, 0.0, 0.0, 0.0))
        assert torch.equal(g[0][0], torch.zeros(3)) and torch.equal(g[1][0], torch.zeros_like(g[1][0])) and bool(g[0][1:].abs().sum() > 0)


def test_the_depth_clamp_passes_no_gradient_below_its_bound():
    """quantile = 1 keeps every element, the one behind its camera included: its error is huge (v.xy / 1e-5), and its gradient must
    not reach v.z.  Against fp64 at the same bound."""
    case, detail = R.conditioned_case(5, 2, 4, 7, quantile=1.0, behind=True)
    assert float(detail["vz"][1, 0]) < 1e-5 and float(detail["w2k"][1, 0]) > 0
    mix = (0.0, 1.0, 0.0, 0.0, 0.0, 0.0)
    compare("track_fit clamp", on_gpu(case, mix, quantile=1.0), R.on_ref(case, mix, quantile=1.0))


# ---- 2. shape sweep ------------------------------------------------------------------------------------------
SWEEP = [(G, K, T) for G in (1, 63, 64, 65, 257) for K in (1, 8, 9, 20) for T in (3, 4, 7)]
# every frame-chunk edge: one chunk (CHUNK - 1, CHUNK, CHUNK + 1 frames) and two (2 CHUNK - 1, 2 CHUNK, 2 CHUNK + 1)
EDGES = [(G, K, T) for G, K in ((65, 9), (257, 8)) for T in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1)]


@pytest.mark.parametrize("G,K,T", SWEEP + [e for e in EDGES if e not in SWEEP])
def test_shape_sweep_against_fp64(G, K, T):
    case, _ = R.conditioned_case(G, K, T, seed=G * 100 + K * 10 + T, general_cam=(G + K + T) % 2 == 0)  # gaps_ok asserted inside
    mix = (1.3, 0.7, 2.1, 0.9, 1.1, 0.6)
    compare(f"track_fit sweep G{G} K{K} T{T}", on_gpu(case, mix), R.on_ref(case, mix))


# ---- 3. composition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general_cam", "k9", "t4"])
def test_agrees_with_a_composition_of_the_older_losses(golden, name):
    case = load_case(golden, name)
    targets, tracks = targets_of(case)
    lv = [case[k].to(DEV) for k in R.LEAVES]
    terms = losses.track_fit_losses(*lv, targets)
    w3, w2 = tracks.visibles.float() * tracks.confidences, tracks.invisibles.float() * tracks.confidences
    composed = R.compose_terms(*lv, tracks.xyz, w3, w2, case["Ks"].to(DEV), case["w2cs"].to(DEV))
    want = torch.tensor(golden[f"{name}/terms"])
    for i, t_name in enumerate(R.TERMS):
        check(f"track_fit composed {name}", t_name, composed[i].cpu(), want[i])      # the composition is the same mathematics ...
        check(f"track_fit vs composed {name}", t_name, terms[i].cpu(), composed[i].double().cpu())  # ... and the kernel agrees with it


# ---- 4. reproducibility and plumbing -------------------------------------------------------------------------
def test_bitwise_reproducible_and_graph_replay_equals_eager(golden):
    case = load_case(golden, "default")
    targets, _ = targets_of(case)
    mix = torch.tensor(golden["mix"], dtype=torch.float32, device=DEV)
    lv = [case[k].to(DEV).requires_grad_() for k in R.LEAVES]

    def run():
        terms = losses.track_fit_losses(*lv, targets)
        return [terms.detach().clone()] + [g.clone() for g in torch.autograd.grad((terms * mix).sum(), lv)]

    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        held = run()
    for _ in range(2):
        for x in held:
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(a, held))
    # another object of the same observations gives the same bits: the preparation is reproducible too
    assert torch.equal(targets.buf, targets_of(case)[0].buf)


def test_a_leaf_changed_in_place_before_backward_raises(golden):
    case = load_case(golden, "t4")
    targets, _ = targets_of(case)
    for k in range(4):
        lv = [case[n].to(DEV).requires_grad_() for n in R.LEAVES]
        used = [x * 1.0 for x in lv]  # non-leaf inputs, so that an in-place change is allowed at all
        terms = losses.track_fit_losses(*used, targets)
        with torch.no_grad():
            used[k].add_(1.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            terms.sum().backward()


# ---- 5. the loop: graph, eager, by hand ----------------------------------------------------------------------
def fresh(case):
    G = case["means"].shape[0]
    fg = GaussianParams(case["means"].clone(), torch.ones(G, 4), torch.zeros(G, 3), torch.zeros(G, 3), torch.zeros(G),
                        motion_coefs=case["motion_coefs"].clone()).to(DEV)
    return fg, MotionBases(case["rots"].clone(), case["transls"].clone()).to(DEV)


def params_of(fg, bases):
    return [fg.params["means"], fg.params["motion_coefs"], bases.params["rots"], bases.params["transls"]]


def by_hand(case, tracks, n):
    """the loop written out: track_fit_losses + the schedule step + AdamGroup.step(), eagerly, through autograd"""
    fg, bases = fresh(case)
    means, coefs, rots, transls = params_of(fg, bases)
    targets = S.track_fit_targets(tracks, case["Ks"].to(DEV), case["w2cs"].to(DEV))
    order = [rots, transls, coefs, means]
    group = AdamGroup()
    handles = [group.adam(p, lr) for p, lr in zip(order, S.FIT_LR0)]
    for p in order:
        p.grad = torch.zeros_like(p)
    it, weights = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(6, device=DEV)
    lrs, terms_hist = torch.zeros(n, 4, device=DEV), torch.zeros(n, 6, device=DEV)
    for i in range(n):
        S.track_fit_schedule(group, it, n, weights, lrs)
        terms = losses.track_fit_losses(means, coefs, rots, transls, targets)
        terms_hist[i] = terms.detach()
        for p, g in zip(order, torch.autograd.grad((terms * weights).sum(), order)):
            p.grad.copy_(g)  # in place: a new gradient tensor would make the group upload its table, host-side rates included
        group.step()
    return params_of(fg, bases), terms_hist, lrs, handles


def test_graph_eager_and_hand_written_loops_give_the_same_bits(golden):
    case, n = load_case(golden, "general_cam"), 12
    _, tracks = targets_of(case)
    runs = []
    for graph in (True, False):
        fg, bases = fresh(case)
        hist = S.run_initial_optim(fg, bases, tracks, case["Ks"].to(DEV), case["w2cs"].to(DEV), num_iters=n, graph=graph)
        assert hist["losses"].shape == (n, 7) and hist["lrs"].shape == (n, 4) and hist["losses"].is_cuda
        runs.append((params_of(fg, bases), hist))
    hand, hand_terms, hand_lrs, handles = by_hand(case, tracks, n)
    for k, a, b, c, start in zip(R.LEAVES, runs[0][0], runs[1][0], hand, (case[k] for k in R.LEAVES)):
        assert torch.equal(a, b) and torch.equal(a, c), k
        assert not torch.equal(a.detach().cpu(), start) or k == "motion_coefs" and start.shape[1] == 1, k  # it moved
    assert torch.equal(runs[0][1]["losses"], runs[1][1]["losses"]) and torch.equal(runs[0][1]["lrs"], runs[1][1]["lrs"])
    assert torch.equal(runs[0][1]["losses"][:, 1:], hand_terms) and torch.equal(runs[0][1]["lrs"], hand_lrs)
    losses_, lrs = runs[0][1]["losses"].cpu(), runs[0][1]["lrs"].cpu()
    assert torch.isfinite(losses_).all() and bool((losses_[:, 0] > 0).all())
    for i in (0, n - 1):  # the total is the weighted sum of the six terms with the schedule's weights
        want = sum(w * float(t) for w, t in zip(R.weights(i, n), losses_[i, 1:]))
        assert abs(float(losses_[i, 0]) - want) <= 1e-6 * abs(want)
    want_lrs = torch.tensor([[lr0 * 0.1 ** (i / n) for lr0 in R.LR0] for i in range(n)], dtype=torch.float64)
    assert float(((lrs.double() - want_lrs).abs() / want_lrs).max()) <= 2.0 ** -23  # within an fp32 rounding of the closed form


def test_the_handles_are_left_at_the_last_rate(golden):
    case, n = load_case(golden, "t4"), 5
    _, tracks = targets_of(case)
    fg, bases = fresh(case)
    seen = []
    orig = AdamGroup.adam

    def spy(self, param, lr, *a, **k):
        h = orig(self, param, lr, *a, **k)
        seen.append(h)
        return h

    AdamGroup.adam = spy
    try:
        hist = S.run_initial_optim(fg, bases, tracks, case["Ks"].to(DEV), case["w2cs"].to(DEV), num_iters=n)
    finally:
        AdamGroup.adam = orig
    last = hist["lrs"][-1].cpu()
    assert len(seen) == 4
    for h, lr0, got in zip(seen, R.LR0, last):
        lr = h.param_groups[0]["lr"]
        assert lr == lr0 * 0.1 ** ((n - 1) / n) and abs(np.float32(lr) - np.float32(got)) <= np.spacing(np.float32(lr)) and float(h.state[h.param_groups[0]["params"][0]]["step"]) == n


# ---- 6. fixture (b): the reference's own trajectory ----------------------------------------------------------
def trajectory_deviation(golden, name):
    case, n = load_case(golden, name), int(golden[f"{name}/num_iters"])
    _, tracks = targets_of(case)
    fg, bases = fresh(case)
    S.run_initial_optim(fg, bases, tracks, case["Ks"].to(DEV), case["w2cs"].to(DEV), num_iters=n)
    out = {}
    for k, p in zip(R.LEAVES, params_of(fg, bases)):
        want = torch.tensor(golden[f"{name}/after/{k}"])
        moved = float((want - case[k].double()).abs().max())
        out[k] = (float((p.detach().cpu().double() - want).abs().max()), moved)
    return out, n


@pytest.mark.parametrize("name", TRAJECTORIES)
def test_lands_where_the_references_own_run_initial_optim_landed(golden, name):
    dev, n = trajectory_deviation(golden, name)
    travel = {k: 0.5 * sum(lr0 * 0.1 ** (i / n) for i in range(n)) for k, lr0 in zip(("rots", "transls", "motion_coefs", "means"), R.LR0)}
    for k, (err, moved) in dev.items():
        rel = err / moved if moved > 0 else 0.0
        print(f"trajectory {name} {k}: max deviation {err:.3e}, largest change {moved:.3e}, relative {rel:.3e}")
        assert err <= travel[k], (k, err, travel[k])  # the condition: never more than half of the group's possible travel
        if moved == 0:
            assert err == 0.0, k  # (one basis: softmax of one coefficient has no gradient and the coefficient never moves)
        else:
            assert rel <= TRAJ_BOUND, (k, rel, TRAJ_BOUND)


# ---- 7. convergence ------------------------------------------------------------------------------------------
def convergence_case():
    """The scene-initialisation fixture's largest case - tracks synthesised from known rigid motions plus noise - with the Procrustes
    initialisation the REFERENCE's own init_motion_params_with_procrustes gave for it (tests/golden/scene_init.npz), and fixed cameras."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "scene_init.npz"))
    n = "default_small"
    valid, cano_t = torch.tensor(g[f"{n}/valid"]), int(g[f"{n}/cano_t"])
    xyz, vis, conf = (torch.tensor(g[f"{n}/{k}"])[valid] for k in ("xyz", "visibles", "confidences"))
    T = xyz.shape[1]
    w2cs = torch.eye(4).repeat(T, 1, 1)
    w2cs[:, 2, 3] = 7.0
    w2cs[:, 0, 3] = 0.05 * torch.arange(T)
    Ks = torch.tensor([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]]).repeat(T, 1, 1)
    return dict(means=xyz[:, cano_t].clone(), motion_coefs=torch.tensor(g[f"{n}/motion_coefs"]).float(), rots=torch.tensor(g[f"{n}/rots"]).float(),
                transls=torch.tensor(g[f"{n}/transls"]).float(), xyz=xyz, visibles=vis, invisibles=~vis, confidences=conf, Ks=Ks, w2cs=w2cs)


def test_a_procrustes_initialisation_gets_closer_to_its_tracks():
    case = convergence_case()
    targets, tracks = targets_of(case)
    fg, bases = fresh(case)
    hist = S.run_initial_optim(fg, bases, tracks, case["Ks"].to(DEV), case["w2cs"].to(DEV), num_iters=100)
    with torch.no_grad():
        after = losses.track_fit_losses(*params_of(fg, bases), targets)
    first, last = float(hist["losses"][0, 1]), float(after[0])
    print(f"convergence: track_3d {first:.6f} -> {last:.6f} after 100 iterations, ratio {last / first:.4f}")
    assert last < first


# ---- 8. the example ------------------------------------------------------------------------------------------
def test_example_runs_with_a_warm_up():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "init_scene.py"), "--tracks", "300", "--frames", "6", "--bases", "2",
                          "--points", "500", "--warmup", "20"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "warm-up first" in out.stdout and "warm-up last" in out.stdout and "render" in out.stdout
