#!/usr/bin/env python3
"""The training step of examples/train_dynamic_step.py fed from a device-resident clip (deblur4dgs_amd.feed).

A synthetic clip at the reference's shape - 24 frames of 288 x 512, 2-D tracks between every pair of frames - is rendered once from a
perturbed copy of the scene and kept on the GPU as a `DeviceClip`.  Every dynamic frame gets ONE captured HIP graph that begins with

    clip.draw(seed)                  # four new target frames, from a device counter
    batch = clip.batch(q, out=buffers)

and goes on with the three render groups of the reference's step (static blurry, dynamic blurry with mask / track / depth channels,
static mid), the photometric loss, `track_losses_from_tables(out["tracks_3d"], batch["track_tables"])`, the backward and one HIP Adam
launch.  A replay therefore trains on targets no earlier replay of that graph has seen, without a host read or a fresh allocation.
One graph per frame because `SceneModel.render` takes the frame's time as a host number (move_model.py calls int(time) and
float(time)); the host picks the frame order.

    python examples/train_clip.py --steps 200
    python examples/train_clip.py --frames 4 --tracks 4096
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deblur4dgs_amd import engine  # noqa: E402
from deblur4dgs_amd.feed import DeviceClip  # noqa: E402
from deblur4dgs_amd.losses import photometric_loss, track_losses_from_tables  # noqa: E402
from deblur4dgs_amd.optim import AdamGroup  # noqa: E402
from train_dynamic_step import build  # noqa: E402


def make_clip(tgt_model, w2c, K, W, H, F, start, end, n_tracks, seed, num_targets=4) -> DeviceClip:
    """The clip a dataset would hold, from the target scene itself: per frame its blurry render, depth and foreground mask; per pair
    (query frame q, target frame t) the pixels the target scene's track points of q's query pixels project to at t, with logits from
    the seed.  The queries sit on the pixel grid, distinct and in raster order, as the reference's do."""
    dev = w2c.device
    g = torch.Generator().manual_seed(seed)
    imgs, depths, masks, tracks = [], [], [], []
    with torch.no_grad():
        for t in range(F):
            o = tgt_model.render(t, w2c, K, (W, H), return_depth=True, return_mask=True, mode="blury")
            imgs.append(o["img"][0]), depths.append(o["depth"][0, ..., 0]), masks.append((o["mask"][0, ..., 0] > 0.5).float())
        w2c4 = w2c.expand(4, 4, 4).contiguous()
        for q in range(F):
            idx = torch.sort(torch.randperm(H * W, generator=g)[:n_tracks]).values.to(dev)
            rows = torch.empty(F, idx.numel(), 4, device=dev)
            for t0 in range(0, F, 4):
                ts = torch.arange(t0, t0 + 4, device=dev).clamp(max=F - 1).float()
                pts = tgt_model.render(q, w2c, K, (W, H), target_ts=ts, target_w2cs=w2c4, mode="mid")["tracks_3d"][0].reshape(H * W, 4, 3)[idx]
                proj = torch.einsum("ij,pnj->npi", K[0], pts)
                n = min(4, F - t0)
                rows[t0:t0 + n, :, :2] = (proj[..., :2] / proj[..., 2:].clamp(min=1e-6))[:n]
            rows[q, :, 0], rows[q, :, 1] = (idx % W).float(), (idx // W).float()
            rows[..., 2:] = (torch.randn(F, idx.numel(), 2, generator=g) * 2.0 - 2.0).to(dev)  # mostly visible, mostly confident
            tracks.append(rows)
    imgs, depths, masks = torch.stack(imgs), torch.stack(depths), torch.stack(masks)
    return DeviceClip(imgs, depths, masks, torch.ones_like(masks), K.expand(F, 3, 3).contiguous(), w2c.expand(F, 4, 4).contiguous(),
                      torch.arange(F, device=dev), tracks, start, end, num_targets)


def train(steps=100, dev="cuda:0", W=512, H=288, F=24, start=1, end=23, frames=0, n_tracks=8192, seed=0, verbose=True, **kw):
    """frames: how many of the dynamic frames start .. end-1 are trained on (0: all of them); every one costs two eager steps and a
    capture before the timed replays begin.  -> (losses, seconds per replayed step, the clip)"""
    model, sc = build(W=W, H=H, dev=dev, seed=seed, **kw)
    model.deferred_size_check = True
    w2c, K = sc["viewmat"][None].to(dev), sc["K"][None].to(dev)
    tgt_model, _ = build(W=W, H=H, dev=dev, seed=seed + 1, **kw)
    clip = make_clip(tgt_model, w2c, K, W, H, F, start, end, min(n_tracks, W * H), seed)
    del tgt_model
    out = clip.buffers()
    group = AdamGroup()
    lrs = {"means": 1.6e-4, "colors": 1e-2, "opacities": 1e-2, "scales": 5e-3, "quats": 5e-3, "motion_coefs": 5e-3}
    for part in ("fg", "bg"):
        for n, p in getattr(model, part).params.items():
            group.adam(p, lrs[n])
    for p in model.motion_bases.parameters():
        group.adam(p, 1.6e-4)
    for p in model.move_model.parameters():
        group.adam(p, 5e-4)
    params = [p for h in group.handles for grp in h.param_groups for p in grp["params"]]

    def step(q):
        """one training step on query frame q: what a graph of this example holds"""
        live = [p.grad for p in params if p.grad is not None]
        if live:  # every graph accumulates into the SAME gradient tensors, zeroed here: the optimizer's device table never moves
            torch._foreach_zero_(live)
        clip.draw(seed)
        b = clip.batch(q, out=out)
        cam, intr, img = b["w2cs"], b["Ks"], b["imgs"]
        out1 = model.render(q, cam, intr, (W, H), bg_only=True, return_depth=True, return_mask=True, mode="blury")
        out2 = model.render(q, cam, intr, (W, H), target_ts=b["target_ts"][0], target_w2cs=b["target_w2cs"][0], return_depth=True,
                            return_mask=True, mode="blury")  # 17 channels
        out3 = model.render(q, cam, intr, (W, H), bg_only=True, return_depth=True, mode="mid")
        outside = 1.0 - b["masks"][..., None]
        loss = photometric_loss(out1["img"], img, mask=outside) + photometric_loss(out2["img"], img) + \
            0.1 * photometric_loss(out3["img"], img, mask=outside)
        l2d, ldepth = track_losses_from_tables(out2["tracks_3d"], b["track_tables"])
        loss = loss + 2.0 * l2d / max(H, W) + 0.1 * ldepth  # configs.py: w_track 2 after the division by max(H, W), w_depth_const 0.1
        loss.backward()
        group.step()
        return loss.detach()

    order = list(range(start, end))[:frames or None]
    graphs = {}  # frame -> (graph, static loss, engine.GraphWatch)
    pool = torch.cuda.graph_pool_handle()  # the graphs replay one after the other: they share their intermediates' memory

    def capture(q):
        done = tries = 0
        while done < 2:  # eager: the optimizer's state and the list capacities of this frame exist before the capture
            step(q)
            try:
                engine.check_deferred()
                done += 1
            except RuntimeError:  # a new frame overflowed the lists sized for the last one: the step was void, the guess has moved
                tries += 1
                if tries > 4:
                    raise
        g_, watch, cap_stream = torch.cuda.CUDAGraph(), engine.GraphWatch(), torch.cuda.Stream()
        cap_stream.wait_stream(torch.cuda.current_stream())
        with watch.capturing(), torch.cuda.graph(g_, stream=cap_stream, pool=pool):
            loss_static = step(q)
        graphs[q] = (g_, loss_static, watch)

    t0 = time.perf_counter()
    for q in order:
        capture(q)
    torch.cuda.synchronize()
    if verbose:
        print(f"{len(order)} graphs captured in {time.perf_counter() - t0:.1f} s ({clip.P_max} queries per frame, {clip.num_targets} targets)")
    picks = torch.randint(len(order), (steps,), generator=torch.Generator().manual_seed(seed)).tolist()  # the host picks the frame order
    losses, voided = [], 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it, k in enumerate(picks):
        q = order[k]
        try:  # a replay keeps the list capacities of its capture: the counts of its previous replay are looked at before the next
            graphs[q][2].check()
        except RuntimeError as e:
            if verbose:
                print(f"step {it:3d}  frame {q}: {e}")
            voided += 1
            capture(q)
        g_, loss_static, watch = graphs[q]
        g_.replay()
        watch.replayed()
        losses.append(loss_static.clone())  # no host sync inside the loop
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / max(steps, 1)
    clip.check(out)  # the one host read of the feed: no selection was ever out of range
    losses = [float(x) for x in losses]
    if verbose:
        for it in range(0, steps, max(steps // 10, 1)):
            print(f"step {it:3d}  frame {order[picks[it]]:2d}  loss {losses[it]:.5f}")
        print(f"{1e3 * dt:.2f} ms / step  ({steps} replays over {len(order)} frames, draw + batch + 3 render groups + losses + backward + Adam in "
              f"one graph launch; {voided} re-captured; {int(clip.counter)} draws)")
    return losses, dt, clip


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="timed graph replays, the frame of each picked by the host")
    ap.add_argument("--frames", type=int, default=0, help="train on the first N dynamic frames only (0: all 22)")
    ap.add_argument("--tracks", type=int, default=8192, help="query tracks per frame")
    a = ap.parse_args()
    train(a.steps, frames=a.frames, n_tracks=a.tracks)
