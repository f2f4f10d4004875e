#!/usr/bin/env python3
"""Times of one training batch at the reference's shape (288 x 512, 24 frames, 4 targets, --tracks queries per frame; profiles/feed_times.txt):

  hip     clip.draw + clip.batch(q, out=buffers): two launches, replayed from a HIP graph and run eagerly
  torch   the same batch composed from torch ops on the device (indexing, sigmoid, two grid_samples, the trainer's cat / expand / where)
  host    the reference's path, file loading excluded: parse_tapir_track_info and two grid_samples on the CPU (the dataset's tensors live
          there), an upload of every batch tensor, then the trainer's shaping on the device

    python scripts/bench_feed.py [--tracks 8192] [--reps 200]
    rocprofv3 --kernel-trace --stats -- python scripts/bench_feed.py --only hip     # the kernels' own times
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deblur4dgs_amd.feed import DeviceClip  # noqa: E402

DEV = "cuda:0"


def normalize_coords(coords, h, w):
    return coords / torch.tensor([w - 1.0, h - 1.0], device=coords.device) * 2 - 1.0


def torch_batch(c, q, target_inds, num_frames):
    """__getitem__'s training branch and the trainer's shaping, on whatever device `c` lives on"""
    H, W = c["depths"].shape[1:]
    tt = c["tracks"][q][target_inds]  # [N,P,4]
    N, P = tt.shape[:2]
    vis, conf = 1 - torch.sigmoid(tt[..., 2]), 1 - torch.sigmoid(tt[..., 3])
    visible, invisible = vis * conf > 0.5, (1 - vis) * conf > 0.5
    conf = conf * (visible | invisible).float()
    grid = normalize_coords(tt[..., None, :2], H, W)
    depth = F.grid_sample(c["depths"][target_inds, None], grid, align_corners=True, padding_mode="border")[:, 0, :, 0]
    img = F.grid_sample(c["imgs"][target_inds].permute(0, 3, 1, 2), grid, align_corners=True, padding_mode="border").squeeze(-1)
    target_ts = c["time_ids"][target_inds]
    return dict(ts=c["time_ids"][q:q + 1], w2cs=c["w2cs"][q:q + 1], Ks=c["Ks"][q:q + 1], imgs=c["imgs"][q:q + 1], depths=c["depths"][q:q + 1],
                masks=c["masks"][q:q + 1], valid_masks=c["valid_masks"][q:q + 1], query_tracks_2d=c["tracks"][q][q][:, :2], target_ts=target_ts,
                target_w2cs=c["w2cs"][target_ts], target_Ks=c["Ks"][target_ts], target_tracks_2d=tt[..., :2], target_visibles=visible,
                target_invisibles=invisible, target_confidences=conf, target_track_depths=depth, target_track_imgs=img)


def shape_tables(b, H, W, num_frames):
    """trainer.py:549-565, 646-659 and the tables of losses.track_losses, on the device"""
    N, P = b["target_visibles"].shape
    w_interval = torch.exp(-2 * (b["ts"].repeat_interleave(N) - b["target_ts"]).abs() / num_frames)
    weights = (b["target_confidences"].reshape(-1)[:, None] * w_interval).sum(-1)
    xy = b["query_tracks_2d"].to(torch.int64)
    pix = (xy[:, 1] * W + xy[:, 0]).to(torch.int32)[None].expand(N, P).reshape(-1)
    rows = torch.arange(N, device=pix.device, dtype=torch.int32)[:, None].expand(N, P).reshape(-1)
    return pix.contiguous(), rows.contiguous(), b["target_visibles"].reshape(-1).to(torch.uint8), weights, b["target_tracks_2d"].reshape(-1, 2), \
        b["target_track_depths"].reshape(-1), b["target_Ks"].reshape(-1, 9)


def timed(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", choices=("hip",), default=None)
    a = ap.parse_args()
    Fr, H, W, N, P, start, end = 24, 288, 512, 4, a.tracks, 1, 23
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)
    host = dict(imgs=r(Fr, H, W, 3), depths=r(Fr, H, W) + 1, masks=(r(Fr, H, W) < 0.5).float(), valid_masks=torch.ones(Fr, H, W),
                Ks=r(Fr, 3, 3), w2cs=r(Fr, 4, 4), time_ids=torch.arange(Fr),
                tracks=[torch.cat([r(Fr, P, 1) * (W - 1), r(Fr, P, 1) * (H - 1), torch.randn(Fr, P, 2, generator=g) * 2], -1) for _ in range(Fr)])
    for q in range(Fr):
        idx = torch.sort(torch.randperm(H * W, generator=g)[:P]).values
        host["tracks"][q][q, :, 0], host["tracks"][q][q, :, 1] = (idx % W).float(), (idx // W).float()
    dev = {k: [t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV) for k, v in host.items()}
    clip = DeviceClip(dev["imgs"], dev["depths"], dev["masks"], dev["valid_masks"], dev["Ks"], dev["w2cs"], dev["time_ids"], dev["tracks"],
                      start, end, N)
    out = clip.buffers()
    q = 7

    def hip():
        clip.draw(1)
        clip.batch(q, out=out)

    hip()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip()
    print(f"288 x 512, 24 frames, N = {N} targets, P = {P} queries per frame, {a.reps} repetitions, wall time per batch")
    print(f"hip    draw + batch(out=), graph replay   {timed(graph.replay, a.reps):9.1f} us")
    print(f"hip    draw + batch(out=), eager          {timed(hip, a.reps):9.1f} us")
    clip.check(out)
    if a.only is None:
        targets = [3, 9, 12, 20]
        ti_dev, ti_host = torch.tensor(targets, device=DEV), torch.tensor(targets)

        def on_device():
            shape_tables(torch_batch(dev, q, ti_dev, end - start), H, W, end - start)

        def on_host():
            b = torch_batch(host, q, ti_host, end - start)
            shape_tables({k: v.to(DEV, non_blocking=True) for k, v in b.items()}, H, W, end - start)

        print(f"torch  the same batch from torch ops, device  {timed(on_device, a.reps):7.1f} us")
        print(f"host   CPU parse + 2 grid_samples + upload    {timed(on_host, max(a.reps // 10, 5), warm=2):7.1f} us   ({torch.get_num_threads()} CPU threads)")
