"""Fixture of the warm-up fit (deblur4dgs_amd.losses.track_fit_losses, deblur4dgs_amd.scene_init.run_initial_optim): small synthetic
fits, and what the REFERENCE's own code gives for them in float64 on the CPU.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_track_fit.py   ->  tests/golden/track_fit.npz

Executed from the reference (imported by gen_scene_init.import_reference, which stubs the libraries that are not installed):
  (a) the six terms of one iteration of run_initial_optim's loop (flow3d/init_utils.py:321-388), through the reference's own
      functions - GaussianParams.get_coefs, MotionBases.compute_transforms, masked_l1_loss, compute_se3_smoothness_loss,
      compute_accel_loss, compute_z_acc_loss - and the leaf gradients of the fixed mix MIX of them.  What connects those calls is
      stated in `reference_flow` below in this file's own words (the frame times, [R | t] applied to the means, the weight planes).
  (b) `init_utils.run_initial_optim(num_iters=n)` ITSELF: the four parameters after n iterations.
Two names of init_utils are rebound first: `project_2d_tracks` (stubbed to None by import_reference: flow3d/vis/utils.py pulls in viser;
stated here in this file's own words - two einsums and a clamp) and `tqdm` (a plain iterator with a `set_description` that does
nothing).  torch's default dtype is float64 while the reference runs.  Only data travels: the arrays below.

Every input is rounded to fp32 before use, so the GPU sees the same numbers.  So that fp32 cannot take another discrete decision than
fp64, a case's seed is advanced until tests/track_fit_ref.gaps_ok holds (the order statistics of e on both sides of the threshold at
least 1e-5 max e apart, every acceleration norm outside the designed zeros >= 0.05, every point >= 0.5 from every centre, no weighted
|x| argument within rounding of its kink) - for a trajectory case at EVERY iteration, where also every gradient element must be exactly
zero or at least 1e-3 of its tensor's maximum (TRAJECTORIES says which cases are held to that, and what became of the one that cannot be).
The archive is written with fixed zip timestamps: the same generator gives the same bytes."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_motion_regs import write_npz  # noqa: E402
from gen_scene_init import import_reference  # noqa: E402
from tests import track_fit_ref as R  # noqa: E402

MIX = (1.3, 0.7, 2.1, 0.9, 1.1, 0.6)
#        name            G    K   T  seed  flags
CASES = (("default", 333, 20, 24, 100, {}),
         ("general_cam", 65, 5, 8, 200, dict(general_cam=True)),
         ("one", 1, 1, 3, 300, {}),
         ("t4", 70, 3, 4, 400, {}),
         ("k9", 130, 9, 6, 500, {}),
         ("static_bases", 65, 4, 6, 600, dict(static=True)),
         ("behind", 5, 2, 4, 700, dict(behind=True)),  # G T = 20: the point behind its camera is the one element beyond the 0.95 quantile
         ("blind", 40, 3, 5, 800, dict(blind=True)))
#               name          G  K  T  seed  iterations  every gradient element >= 1e-3 of its tensor's maximum at every iteration
TRAJECTORIES = (("traj_one", 1, 1, 3, 900, 6, True),
                ("traj_small", 5, 2, 4, 1000, 5, True),
                ("traj_general", 65, 5, 8, 1100, 4, False),  # 880 gradient elements: some are always small; gaps_ok holds throughout
                ("traj_ramp", 1, 1, 3, 1200, 404, False),    # past iteration 400: w ramps.  Gradient elements cross zero on the way
                                                             # down; gaps_ok holds throughout
                ("traj_ramp_k2", 3, 2, 3, 1300, 404, False))  # the same with two bases: the coefficients move past iteration 400 too


def project_2d_tracks(tracks_3d_w, Ks, T_cw, return_depth=False):
    """(T,N,3) world points -> (T,N,2) pixels [and the depth]: camera = T_cw [x; 1], image = Ks camera, pixel = xy / max(z, 1e-5)"""
    cam = torch.einsum("tij,tnj->tni", T_cw[:, :3, :3], tracks_3d_w) + T_cw[:, None, :3, 3]
    img = torch.einsum("tij,tnj->tni", Ks, cam)
    uv = img[..., :2] / img[..., 2:].clamp_min(1e-5)
    return (uv, img[..., 2]) if return_depth else uv


class plain_iterator:
    def __init__(self, it):
        self.it = it

    def __iter__(self):
        return iter(self.it)

    def set_description(self, *a, **k):
        pass


def reference_objects(TrackObservations, case):
    from flow3d.params import GaussianParams, MotionBases

    c = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in case.items()}
    G = c["means"].shape[0]
    quats = torch.tensor([1.0, 0, 0, 0]).repeat(G, 1)
    fg = GaussianParams(c["means"].clone(), quats, torch.zeros(G, 3), torch.zeros(G, 3), torch.zeros(G), motion_coefs=c["motion_coefs"].clone())
    bases = MotionBases(c["rots"].clone(), c["transls"].clone())
    tracks = TrackObservations(c["xyz"], c["visibles"], c["invisibles"], c["confidences"], torch.zeros(G, 3))
    return fg, bases, tracks, c["Ks"], c["w2cs"]


def reference_flow(L, fg, bases, tracks, Ks, w2cs):
    """-> the six terms of one iteration.  Six functions of the reference are called - GaussianParams.get_coefs,
    MotionBases.compute_transforms, masked_l1_loss, compute_se3_smoothness_loss, compute_accel_loss, compute_z_acc_loss; what
    connects them (the frame times, applying [R | t] to the means, the two weight planes, the projection) is written here."""
    T = bases.num_frames
    frames = torch.arange(T)
    offsets = torch.tensor([-1, 0, 1])
    nb_times = (offsets[:, None] + frames.clamp(1, T - 2)[None, :]).reshape(-1)  # the T times before, the T times at, the T times after
    weights = fg.get_coefs()
    mu = fg.params["means"]

    def deform(times):
        tf = bases.compute_transforms(times, weights)  # [G, len(times), 3, 4] = [R | t]
        return (tf[..., :3] @ mu[:, None, :, None]).squeeze(-1) + tf[..., 3]

    at_frames = deform(frames)  # [G, T, 3]
    conf = tracks.confidences
    seen, hidden = tracks.visibles.to(conf.dtype) * conf, tracks.invisibles.to(conf.dtype) * conf
    pixels = lambda x: project_2d_tracks(x.transpose(0, 1), Ks, w2cs).transpose(0, 1)  # [G, T, 3] -> [G, T, 2]
    track_3d = L.masked_l1_loss(at_frames, tracks.xyz, seen.unsqueeze(-1))
    track_2d = L.masked_l1_loss(pixels(at_frames), pixels(tracks.xyz), hidden.unsqueeze(-1), quantile=0.95) / Ks[0, 0, 0]
    coef_sparse = 1 - weights.square().sum(-1).mean()
    smooth_bases = L.compute_se3_smoothness_loss(bases.params["rots"], bases.params["transls"])
    smooth_tracks = L.compute_accel_loss(at_frames)
    z_accel = L.compute_z_acc_loss(deform(nb_times).unflatten(1, (3, T)), w2cs)  # [G, 3, T, 3], the layout it takes
    return torch.stack([track_3d, track_2d, coef_sparse, smooth_bases, smooth_tracks, z_accel])


def f64(run):
    torch.set_default_dtype(torch.float64)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return run()
    finally:
        torch.set_default_dtype(torch.float32)


def inputs(name, case):
    return {f"{name}/{k}": (v.numpy().astype(np.float32) if v.is_floating_point() else v.numpy()) for k, v in case.items()}


if __name__ == "__main__":
    init_utils, TrackObservations = import_reference()
    L = sys.modules["flow3d.loss_utils"]
    init_utils.project_2d_tracks = project_2d_tracks
    init_utils.tqdm = plain_iterator
    arrays = {"mix": np.asarray(MIX)}
    for name, G, K, T, seed, flags in CASES:
        case, detail = R.conditioned_case(G, K, T, seed, **flags)

        def run():
            fg, bases, tracks, Ks, w2cs = reference_objects(TrackObservations, case)
            terms = reference_flow(L, fg, bases, tracks, Ks, w2cs)
            leaves = [fg.params["means"], fg.params["motion_coefs"], bases.params["rots"], bases.params["transls"]]
            return terms.detach(), torch.autograd.grad((terms * torch.tensor(MIX)).sum(), leaves)

        terms, grads = f64(run)
        mine, my_grads = R.on_ref(case, MIX)
        assert terms.dtype == torch.float64 and torch.allclose(terms, mine, rtol=1e-12, atol=1e-14), (name, terms, mine)
        if name == "static_bases":
            assert torch.equal(terms[3:], torch.zeros(3, dtype=torch.float64)), terms
        if name == "behind":
            assert float(detail["vz"][1, 0]) < 1e-5 and float(case["invisibles"][0, 1] * case["confidences"][0, 1]) > 0
            assert int((detail["e"] >= detail["thr"]).sum()) == 1 and not bool(detail["e"][1, 0] < detail["thr"])
        if name == "blind":
            assert not bool(case["visibles"][0].any() | case["invisibles"][0].any())
        arrays.update(inputs(name, case))
        arrays[f"{name}/terms"] = terms.numpy()
        arrays[f"{name}/thr"] = np.float64(detail["thr"])
        for k, g in zip(R.LEAVES, grads):
            arrays[f"{name}/grad/{k}"] = g.numpy()
        print(name, f"G={G} K={K} T={T}", "terms", [f"{x:.5g}" for x in terms.tolist()], file=sys.stderr)
    for name, G, K, T, seed, n, strict in TRAJECTORIES:
        for attempt in range(400):
            case = R.make_case(G, K, T, seed + 1000 * attempt, general_cam=(name == "traj_general"))
            bad, small = [], []

            def on_step(i, t, grads, detail):
                if not R.gaps_ok(detail):
                    bad.append(i)
                for g in grads:
                    a = g.abs()
                    if not bool(((a == 0) | (a >= 1e-3 * a.max())).all()):
                        small.append(i)

            mine = R.simulate(case, n, on_step=on_step)
            if not bad and not (strict and small):
                break
        else:
            raise SystemExit(f"{name}: no well-conditioned seed")

        def run():
            fg, bases, tracks, Ks, w2cs = reference_objects(TrackObservations, case)
            init_utils.run_initial_optim(fg, bases, tracks, Ks, w2cs, num_iters=n)
            return [x.detach() for x in (fg.params["means"], fg.params["motion_coefs"], bases.params["rots"], bases.params["transls"])]

        after = f64(run)
        for k, a, b in zip(R.LEAVES, after, mine):  # this project's statement of the loop lands where the reference's own loop lands
            assert a.dtype == torch.float64 and torch.allclose(a, b, rtol=1e-10, atol=1e-12), (name, k, float((a - b).abs().max()))
        arrays.update(inputs(name, case))
        arrays[f"{name}/num_iters"] = np.int32(n)
        arrays[f"{name}/small_gradient_iterations"] = np.int32(len(set(small)))
        for k, a in zip(R.LEAVES, after):
            arrays[f"{name}/after/{k}"] = a.numpy()
        print(name, f"G={G} K={K} T={T} n={n} seed {seed + 1000 * attempt}", f"iterations with a small gradient element: {len(set(small))}",
              file=sys.stderr)
    dst = os.path.join(HERE, "track_fit.npz")
    write_npz(dst, arrays)
    print(f"{len(arrays)} arrays -> {dst} ({os.path.getsize(dst)} bytes)", file=sys.stderr)
