#!/usr/bin/env python3
"""A stage-2 style training step on the drop-in scene model, on synthetic data.

Mirrors the SHAPE of the reference's `Trainer.train_step` (flow3d/trainer.py:203-274) - three render groups per step
(static `bg_only` blurry frame, dynamic full blurry frame with mask / track / depth channels, static `mid` frame),
the reference's photometric loss (0.8 L1 + 0.2 (1 - SSIM), fused), one Adam optimizer per parameter tensor, the
densification statistics of `_prepare_control_step` and (with --control-every) the densify / cull control steps -
without the reference's data pipeline (out of scope).  With --depth-losses the step
also carries the reference's quantile-trimmed losses (deblur4dgs_amd.losses): the disparity loss and the
depth-gradient loss on the `mid` render (trainer.py:399-416) and the L1 term of the mask loss on the dynamic render (:626-630).
With --consistency-loss the dynamic group's loss gains the reference's flow-aligned exposure consistency term (trainer.py:599-618,
weight 2; deblur4dgs_amd.pwcnet) under a seeded random-weight PWC-Net - the pretrained blob is not shipped.
With --track-losses the 2-D track loss and the mapped-depth loss (trainer.py:633-667,681-689; deblur4dgs_amd.losses.track_losses,
DESIGN.md section 17) on synthetic query tracks replace the stand-in that otherwise gives the twelve track channels a gradient;
`--track-losses torch` evaluates the same two terms the way the reference writes them, in eager torch (a timing comparator: it
waits for the device and cannot be captured).
With --motion-regs the step also carries the four regularizers of the trainer that look at no image (trainer.py:691-728: smooth
motion bases, smooth foreground tracks, small acceleration along the viewing ray, the variance of the raw scales;
deblur4dgs_amd.losses.scene_motion_regularizers); `--motion-regs torch` evaluates them the way the reference
writes them, in eager torch on the pose API (a timing comparator: torch.linalg.inv waits for the device, so it cannot be captured).
With --image-losses the step carries the remaining image-sized passes of the trainer (deblur4dgs_amd.losses):
the foreground mask dilated by a 9 x 9 max-pool (trainer.py:120) masks a second photometric term of the dynamic render and, as its
complement, one of the static render (:388-392,575-580) - and, with --depth-losses, the static depth losses (:397,413); the
sharp-keep loss ties the middle sub-sample to the blurry target at quarter resolution (:736-747); the coverage term pulls the
accumulated alpha to one (:624-626).
It exists to show the seam in a real autograd + optimizer loop:

    python examples/train_dynamic_step.py --steps 20
    python examples/train_dynamic_step.py --graph --hip-adam --depth-losses
    python examples/train_dynamic_step.py --graph --hip-adam --consistency-loss
    python examples/train_dynamic_step.py --graph --hip-adam --track-losses
    python examples/train_dynamic_step.py --graph --hip-adam --motion-regs
    python examples/train_dynamic_step.py --graph --hip-adam --image-losses
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deblur4dgs_amd import engine  # noqa: E402
from deblur4dgs_amd.control import ControlCfg, accumulate_from_model, cull_step, densify_step, spatial_order_step  # noqa: E402
from deblur4dgs_amd.losses import (compute_gradient_loss, coverage_loss, dilate_mask, masked_l1_loss, photometric_loss,  # noqa: E402
                                   scene_motion_regularizers, sharp_keep_loss, track_losses as hip_track_losses)
from deblur4dgs_amd.pwcnet import PWCNet, exposure_consistency_loss  # noqa: E402
from deblur4dgs_amd.scene_model import GaussianParams, MotionBases, SceneModel  # noqa: E402
from deblur4dgs_amd.synth import make_scene  # noqa: E402


def build(n_fg=40_000, n_bg=100_000, K=20, W=512, H=288, dev="cuda:0", seed=0):
    """The reference's default scene size (run_training_dynamic.py:118-120): 40 k fg + 100 k bg, 20 bases."""
    sc = make_scene(n_fg + n_bg, n_fg, K, 1, W, H, seed=seed)
    keys = ("means", "quats", "scales", "colors", "opacities")
    fg = GaussianParams(*[sc[k][:n_fg].clone() for k in keys], motion_coefs=sc["motion_coefs"].clone())
    bg = GaussianParams(*[sc[k][n_fg:].clone() for k in keys])
    model = SceneModel(sc["K"][None].clone(), sc["viewmat"][None].clone(), fg, MotionBases(sc["rots"], sc["transls"]), bg)
    return model.to(dev), sc


def make_tracks(tgt_tracks_3d, target_Ks, target_ts, t, n_tracks, seed):
    """Synthetic track supervision for the dynamic frame, in the reference's batch layout: `n_tracks` distinct query pixels in raster
    order, and per target frame the 2-D position and depth the target scene's own track points project to (plus a pixel of noise),
    a visibility and a confidence from the seed.  -> the arguments of track_losses after tracks_3d."""
    _, H, W, N, _ = tgt_tracks_3d.shape
    dev = tgt_tracks_3d.device
    g = torch.Generator().manual_seed(seed)
    idx = torch.sort(torch.randperm(H * W, generator=g)[:n_tracks]).values.to(dev)
    query = torch.stack([idx % W, idx // W], -1).float()
    P = query.shape[0]
    proj = torch.einsum("nij,pnj->npi", target_Ks, tgt_tracks_3d[0].reshape(H * W, N, 3)[idx])
    depth = proj[..., 2].clamp(min=1e-6)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    target_2d = proj[..., :2] / depth[..., None] + 2.0 * (r(N, P, 2) - 0.5)
    visibles = (r(N, P) < 0.7) & (proj[..., 2] > 0.01)  # (a hole of the synthetic target has no point to track)
    confidences = r(N * P)
    num_frames = 7  # the example's clip: the frame at t = 3 and targets around it
    w_interval = torch.exp(-2.0 * (t - target_ts).abs() / num_frames)
    return query, target_Ks, target_2d, visibles, confidences[:, None] * w_interval, depth * (1.0 + 0.1 * (r(N, P) - 0.5))


def torch_track_losses(tracks_3d, query, target_Ks, target_2d, visibles, weights, target_depths, quantile=0.98):
    """The same two terms in eager torch over the whole image, the reference's way: project every pixel of every target image, pick
    the query pixels with a boolean image mask and the visible ones with a second (each a `nonzero`: the host waits for the device)
    and take the threshold with torch.quantile (a full sort).  A timing comparator for track_losses; it cannot be captured."""
    _, H, W, N, _ = tracks_3d.shape
    proj = torch.einsum("nij,npj->npi", target_Ks, tracks_3d[0].permute(2, 0, 1, 3).reshape(N, H * W, 3))
    depth = proj[..., 2:].clamp(min=1e-6)
    xy = proj[..., :2] / depth
    image_mask = torch.zeros(H, W, device=tracks_3d.device)
    qi = query.to(torch.int64)
    image_mask[qi[:, 1], qi[:, 0]] = 1.0
    at_queries = image_mask.reshape(1, H * W).expand(N, H * W) > 0.5
    vis = visibles.reshape(-1)
    w = weights[vis].sum(-1)

    def normalised(v, keep):
        return (v * w)[keep].sum() / (w[keep].sum() + 1e-8)

    v2d = (xy[at_queries][vis] - target_2d.reshape(-1, 2)[vis]).abs().mean(-1)
    vdepth = (1 / (depth[at_queries][vis] + 1e-5) - 1 / (target_depths.reshape(-1)[vis, None] + 1e-5)).abs()[:, 0]
    return normalised(v2d, v2d < torch.quantile(v2d, quantile)), normalised(vdepth, torch.ones_like(vis[vis]))


def torch_motion_regularizers(model, ts, w2cs):
    """The four regularizers in eager torch on the pose API, the reference's way (trainer.py:691-728): the (G, 3n, 3, 4) transforms of
    the three neighbour times, a pad and an einsum for the means, norms, torch.linalg.inv for the camera centres (its error check
    waits for the device) and torch.var.  A timing comparator for scene_motion_regularizers; it cannot be captured."""
    bases, fg = model.motion_bases.params, model.fg.params
    accel = lambda x: torch.linalg.vector_norm(x[:, 1:-1] * 2 - (x[:, :-2] + x[:, 2:]), dim=-1).mean()
    smooth_bases = accel(bases["rots"]) + 2.0 * accel(bases["transls"])
    tc = ts.clamp(1, model.num_frames - 2)
    tfs = model.compute_transforms(torch.cat((tc - 1, tc, tc + 1)))
    nbs = torch.einsum("gnij,gj->gni", tfs, torch.nn.functional.pad(fg["means"], (0, 1), value=1.0)).reshape(tfs.shape[0], 3, -1, 3)
    before, at, after = nbs.unbind(1)
    smooth_tracks = torch.linalg.vector_norm(at * 2 - (before + after), dim=-1).mean() / 2
    ray = torch.nn.functional.normalize(at - torch.linalg.inv(w2cs)[:, :3, 3], dim=-1)
    z_accel = ((at - before) * ray).sum(-1).square().mean() + ((after - at) * ray).sum(-1).square().mean()
    return smooth_bases, smooth_tracks, z_accel, torch.var(fg["scales"], dim=-1).mean()


def train(steps=20, dev="cuda:0", W=512, H=288, verbose=True, control_every=0, fused_stats=True, deferred=True,
          graph=False, hip_adam=False, seed=0, step_events=None, depth_losses=False, consistency_loss=False, track_losses=False,
          n_tracks=4096, motion_regs=False, image_losses=False, **kw):
    """fused_stats: the densification statistics come out of the rasterizer's backward (attach_control_stats) instead
    of a pass over `_current_xys[i].grad`; deferred: no render waits for its intersection count on the host
    (`deferred_size_check`), the counts are verified once per step; graph: the three renders, the loss and the whole
    backward of a step are captured ONCE in a HIP graph (after two eager warm-up steps) and replayed - the step is then
    one hipGraphLaunch plus the optimizers (re-captured whenever a control step changes N); hip_adam: the per-tensor optimizers
    are handles of one `deblur4dgs_amd.optim.AdamGroup` - one HIP launch steps them all, and with graph=True that launch is
    captured behind the backward, so the whole step, optimizers included, is the one hipGraphLaunch.  seed: the synthetic
    scene (its targets: seed + 1); step_events: a list that receives one timing event per step, recorded where the step
    begins (per-step times without a host sync: scripts/bench_adam.py); depth_losses: add the reference's disparity, depth-gradient
    and mask-L1 losses with its default weights (configs.py: w_depth_reg 0.5, w_depth_grad 1, w_mask 1) - they wait for nothing on
    the host, so the step still captures; consistency_loss: add 2 x exposure_consistency_loss of the dynamic render's sub-samples
    (one batched PWC-Net pass of 2 (S - 1) pairs under no_grad, one loss kernel; no host wait either); track_losses: the 2-D track
    loss and the mapped-depth loss on `n_tracks` synthetic query tracks (make_tracks) with the reference's weights (configs.py:
    w_track 2 after its division by max(H, W), w_depth_const 0.1) in place of the stand-in on the track channels - True: the HIP
    path, which captures; "torch": the reference's formulation in eager torch, which waits for the device and does not;
    motion_regs: add the reference's smooth-bases, smooth-tracks, z-acceleration and scale-variance regularizers with its weights
    (configs.py: 0.1, 2, 1, 0.01) for the step's frame and camera - True: one HIP call each way, which captures; "torch": the
    reference's wording in eager torch (torch_motion_regularizers), which does not; image_losses: add the dilated-mask photometric
    terms of the dynamic and the static render (w_rgb 1), the sharp-keep loss (weight 1) and the coverage term (w_mask 1), and hand
    the depth losses the complement of the dilated mask - the mask is dilated inside the step, as the reference does, and the
    step still captures."""
    assert not graph or (fused_stats and deferred), "graph capture needs the sync-free step"
    assert track_losses in (False, True, "torch") and not (graph and track_losses == "torch"), "the torch form cannot be captured"
    assert motion_regs in (False, True, "torch") and not (graph and motion_regs == "torch"), "the torch form cannot be captured"
    model, sc = build(W=W, H=H, dev=dev, seed=seed, **kw)
    model.deferred_size_check = bool(deferred)
    w2c, K = sc["viewmat"][None].to(dev), sc["K"][None].to(dev)
    # targets: renders of a perturbed copy of the scene (so the loss has something to fit)
    with torch.no_grad():
        tgt_model, _ = build(W=W, H=H, dev=dev, seed=seed + 1, **kw)
        tgt_dyn = tgt_model.render(3, w2c, K, (W, H), mode="blury")["img"]
        tgt_sta = tgt_model.render(3, w2c, K, (W, H), bg_only=True, mode="blury")["img"]
        if depth_losses:  # the perturbed scene also supplies the depth of the `mid` frame
            tgt_mid = tgt_model.render(3, w2c, K, (W, H), bg_only=True, return_depth=True, mode="mid")
            tgt_disp = 1.0 / (tgt_mid["depth"] + 1e-5)
        if depth_losses or image_losses:  # and the foreground mask
            tgt_mask = (tgt_model.render(3, w2c, K, (W, H), return_mask=True, mode="blury")["mask"] > 0.5).float()
        if depth_losses:
            # outside the foreground mask (with image_losses: outside the dilated one, inside the step) and, the scene being synthetic,
            # only where the target's background covers the pixel: a hole has depth 0, a disparity of 1e5
            depth_covered = (tgt_mid["acc"] > 0.5).float()
            depth_masks = (1.0 - tgt_mask) * depth_covered
            depth_valid = depth_masks > 0.5
        if track_losses:  # supervision from the perturbed scene's own track points
            tgt_ts = torch.tensor([1.0, 2.0, 4.0, 5.0], device=dev)
            tgt_tracks = tgt_model.render(3, w2c, K, (W, H), target_ts=tgt_ts, target_w2cs=w2c.expand(4, 4, 4).contiguous(),
                                          mode="blury")["tracks_3d"]
            tracks = make_tracks(tgt_tracks, K.expand(4, 3, 3).contiguous(), tgt_ts, 3.0, min(n_tracks, W * H), seed)
    alignnet = None
    if consistency_loss:  # a seeded random-weight flow network, frozen: the loss differentiates the images, not the network
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            alignnet = PWCNet(load_pretrained=False).to(dev).eval().requires_grad_(False)
    # (torch's fused Adam faults the GPU when its gradients live in a CUDA-graph memory pool - scripts/graph_bisect.py;
    # the graph mode therefore uses the plain implementation)
    adam = lambda p, lr: torch.optim.Adam([p], lr=lr, fused=p.is_cuda and not graph)
    group = None
    if hip_adam:  # the same optimizers (one torch.optim.Adam subclass per tensor, same keys), stepped together by one kernel
        from deblur4dgs_amd.optim import AdamGroup

        group = AdamGroup()
        adam = group.adam
    lrs = {"means": 1.6e-4, "colors": 1e-2, "opacities": 1e-2, "scales": 5e-3, "quats": 5e-3, "motion_coefs": 5e-3}
    # one Adam per tensor, keyed like the reference's Trainer.optimizers (trainer.py:1168-1196): the control steps
    # re-key them when rows are added / removed
    optimizers = {f"{part}.params.{n}": adam(p, lrs[n]) for part in ("fg", "bg") for n, p in getattr(model, part).params.items()}
    others = [adam(p, 1.6e-4) for p in model.motion_bases.parameters()] + [adam(p, 5e-4) for p in model.move_model.parameters()]
    opts = lambda: list(optimizers.values()) + others
    cfg = ControlCfg()
    N = model.num_gaussians
    stats = {"xys_grad_norm_acc": torch.zeros(N, device=dev), "vis_count": torch.zeros(N, dtype=torch.int64, device=dev),
             "max_radii": torch.zeros(N, device=dev)}
    target_ts = torch.tensor([1.0, 2.0, 4.0, 5.0], device=dev)
    target_w2cs = w2c.expand(4, 4, 4).contiguous()
    reg_ts = torch.tensor([3.0], device=dev)  # the frame every render of the step looks at
    losses = []
    warm = min(5, steps // 2)  # lazy initialisation (Adam state, code objects) stays out of the timing
    def fwd_bwd():
        out1 = model.render(3, w2c, K, (W, H), bg_only=True, return_depth=True, return_mask=True, mode="blury")
        if fused_stats:  # statistics of the dynamic render, accumulated by its own backward (trainer.py:953-990)
            model.attach_control_stats(stats, batch_size=1)
        out2 = model.render(3, w2c, K, (W, H), target_ts=target_ts, target_w2cs=target_w2cs, return_depth=True,
                            return_mask=True, mode="blury")  # 17 channels
        model.detach_control_stats()
        side = (model._current_xys, model._current_radii, model._current_img_wh)
        out3 = model.render(3, w2c, K, (W, H), bg_only=True, return_depth=True, mode="mid")
        # the reference's photometric term, 0.8 L1 + 0.2 (1 - SSIM) (trainer.py:388-392,575-586), fused
        loss = photometric_loss(out1["img"], tgt_sta) + photometric_loss(out2["img"], tgt_dyn) + \
            0.1 * photometric_loss(out3["img"], tgt_sta)
        if track_losses:
            l2d, ldepth = (torch_track_losses if track_losses == "torch" else hip_track_losses)(out2["tracks_3d"], *tracks)
            loss = loss + 2.0 * l2d / max(H, W) + 0.1 * ldepth
        else:  # a stand-in that gives the track channels a gradient
            loss = loss + 1e-3 * out2["tracks_3d"].square().mean()
        d_masks, d_valid = (depth_masks, depth_valid) if depth_losses else (None, None)
        if image_losses:
            dilated, outside = dilate_mask(tgt_mask, return_complement=True)  # trainer.py:388,575: MaxPool2d(9, 1, 4), and 1 - it
            loss = loss + photometric_loss(out2["img"], tgt_dyn, mask=dilated) + photometric_loss(out1["img"], tgt_sta, mask=outside) + \
                sharp_keep_loss(out2["pred_sharp_img"], tgt_dyn, tgt_mask) + 1.0 * coverage_loss(out2["acc"])
            if depth_losses:  # trainer.py:397,413
                d_masks = outside * depth_covered
                d_valid = d_masks > 0.5
        if depth_losses:
            pred_disp = 1.0 / (out3["depth"] + 1e-5)
            loss = loss + 0.5 * masked_l1_loss(pred_disp, tgt_disp, mask=d_masks, quantile=0.98) + \
                1.0 * compute_gradient_loss(pred_disp, tgt_disp, mask=d_valid, quantile=0.95) + \
                1.0 * masked_l1_loss(out2["mask"], tgt_mask, quantile=0.98)
        if consistency_loss:
            loss = loss + 2.0 * exposure_consistency_loss(out2["exposure_imgs"], alignnet)
        if motion_regs:
            sb, st, za, sv = (torch_motion_regularizers if motion_regs == "torch" else scene_motion_regularizers)(model, reg_ts, w2c)
            loss = loss + 0.1 * sb + 2.0 * st + 1.0 * za + 0.01 * sv
        loss.backward()
        return loss.detach(), side

    params = [p for o in opts() for g in o.param_groups for p in g["params"]]
    captured = None  # (graph, static loss, engine.GraphWatch)
    eager_since_capture = 0
    for it in range(steps):
        if it == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if step_events is not None:
            step_events.append(torch.cuda.Event(enable_timing=True))
            step_events[-1].record()
        if captured is not None:
            # a replayed graph keeps the list capacities of its capture: the counts of the PREVIOUS replay (copied to pinned
            # memory by nodes of the graph itself) are looked at before the next one - an overflowed replay rendered nothing,
            # so its step is void; go back to eager steps, which size the lists from the new counts, and capture again
            try:
                captured[2].check()
            except RuntimeError as e:
                if verbose:
                    print(f"step {it:3d}  {e}")
                captured, eager_since_capture = None, 0
        if graph and captured is None and eager_since_capture >= 2:
            for p_ in params:
                p_.grad = None
            g_, watch = torch.cuda.CUDAGraph(), engine.GraphWatch()
            cap_stream = torch.cuda.Stream()
            if alignnet is not None:  # MIOpen / rocBLAS set up per-stream state on first use: not inside the capture
                cap_stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(cap_stream), torch.no_grad():
                    probe = torch.zeros(2 * 10, 3, H, W, device=dev)
                    alignnet(probe, probe)
                torch.cuda.synchronize()
            with watch.capturing(), torch.cuda.graph(g_, stream=cap_stream):
                loss_static, _ = fwd_bwd()
                if group is not None:
                    group.step()  # reads lr and step counts from its device table: valid at every replay
            captured = (g_, loss_static, watch)
        if captured is not None:
            if group is not None:
                group.sync()  # an lr a scheduler moved since the last step reaches the device table (no-op otherwise)
            captured[0].replay()  # gradients land in the same .grad tensors every step
            captured[2].replayed()
            loss, side = captured[1], None
        else:
            for o in opts():
                o.zero_grad(set_to_none=True)
            loss, side = fwd_bwd()
            eager_since_capture += 1
        xys2, radii2, wh2 = side if side is not None else (None, None, None)
        if group is None:
            for o in opts():
                o.step()
        elif captured is None:  # (a replayed graph has stepped them already)
            group.step()
        if not fused_stats:
            model._current_xys, model._current_radii, model._current_img_wh = xys2, radii2, wh2
            accumulate_from_model(stats, model, batch_size=1)
        if deferred:
            engine.check_deferred()  # raises if a render of this step overflowed its intersection lists
        losses.append(loss.detach().clone())  # no host sync inside the loop
        if control_every and it > 0 and it % control_every == 0:  # adaptive control: N changes between steps
            n_split, n_dup = densify_step(model, stats, optimizers, cfg, global_step=it)
            n_cull = cull_step(model, stats, optimizers, cfg, global_step=it)
            spatial_order_step(model, stats, optimizers)  # the control step rewrites every row anyway: leave them in Morton order of
            #                                                the first camera's image plane (binning / gather locality)
            for v in stats.values():
                v.zero_()
            params = [p for o in opts() for g in o.param_groups for p in g["params"]]
            captured, eager_since_capture = None, 0  # N changed: new shapes, new parameters -> capture again
            if verbose:
                print(f"step {it:3d}  control: split {n_split}, dup {n_dup}, cull {n_cull} -> {model.num_gaussians} Gaussians")
        if verbose and (it % 10 == 0 or it == steps - 1):
            print(f"step {it:3d}  loss {float(losses[-1]):.5f}")
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / (steps - warm)
    losses = [float(l) for l in losses]
    if verbose:
        print(f"{1e3 * dt:.2f} ms / step  (3 render groups: 11 + 11 + 1 sub-samples, {model.num_gaussians} Gaussians, fwd + bwd + Adam)")
        if os.environ.get("D4GS_EXAMPLE_STATS"):  # what the engine measured per render shape: live-row fraction, list capacity
            for key, f in engine._LIVE_FRAC.items():
                print("  shape", key, "live fraction %.3f" % f, "capacity (rectangles / exact tiles)",
                      [(engine._guess_get(key + (xt,)) or (None,))[0] for xt in (False, True)])
        print(f"visible-instance count accumulated: {int(stats['vis_count'].sum())}")
    return losses, stats, dt


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--control-every", type=int, default=0, help="densify + cull every N steps (0: never)")
    ap.add_argument("--round1", action="store_true", help="statistics as a separate pass, host waits for every list size")
    ap.add_argument("--graph", action="store_true", help="replay the step's renders + loss + backward from a HIP graph")
    ap.add_argument("--hip-adam", action="store_true", help="step every optimizer with one HIP launch (inside the graph with --graph)")
    ap.add_argument("--depth-losses", action="store_true",
                    help="add the reference's disparity, depth-gradient and mask-L1 losses (quantile-trimmed, HIP, graph-capturable)")
    ap.add_argument("--consistency-loss", action="store_true",
                    help="add the reference's flow-aligned exposure consistency loss (HIP cost volume and warp, graph-capturable)")
    ap.add_argument("--track-losses", nargs="?", const="hip", default=None, choices=("hip", "torch"),
                    help="the reference's 2-D track and mapped-depth losses on synthetic query tracks: HIP and graph-capturable, or "
                         "`torch`: the reference's eager formulation (full-image projection, boolean selection, torch.quantile)")
    ap.add_argument("--tracks", type=int, default=4096, help="query tracks of --track-losses")
    ap.add_argument("--motion-regs", nargs="?", const="hip", default=None, choices=("hip", "torch"),
                    help="the reference's smooth-bases, smooth-tracks, z-acceleration and scale-variance regularizers: HIP and "
                         "graph-capturable, or `torch`: the reference's eager formulation on the pose API (torch.linalg.inv)")
    ap.add_argument("--image-losses", action="store_true",
                    help="add the dilated-mask photometric terms, the sharp-keep loss and the coverage term (HIP, graph-capturable)")
    a = ap.parse_args()
    train(a.steps, control_every=a.control_every, fused_stats=not a.round1, deferred=not a.round1, graph=a.graph, hip_adam=a.hip_adam,
          depth_losses=a.depth_losses, consistency_loss=a.consistency_loss,
          track_losses={None: False, "hip": True, "torch": "torch"}[a.track_losses], n_tracks=a.tracks,
          motion_regs={None: False, "hip": True, "torch": "torch"}[a.motion_regs], image_losses=a.image_losses)
