"""Fixture of the batch feed (deblur4dgs_amd/feed.py): two small synthetic clips, and what the REFERENCE's own functions make of them on
the CPU in float64.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_feed.py   ->  tests/golden/feed.npz

Executed from the reference: flow3d/data/utils.py, loaded from its path (it needs torch and numpy only) - `parse_tapir_track_info` and
`normalize_coords` - and `F.grid_sample` with the exact arguments of flow3d/data/stereo_low_dataset.py:645-665, all under torch's default
dtype float64.  The weights are trainer.py:549,646-647 with the trailing axis summed, as `losses.track_losses` documents:
confidence[n,p] sum_n' exp(-2 |ts - target_ts[n']| / num_frames), in float64.  Only arrays travel.

Every input is rounded to fp32 before use, so the GPU sees the same numbers.  A sample whose `vis * conf` or `(1 - vis) * conf` lies
within 1e-3 of 0.5 is drawn again; at most 2 % of the samples may be (the share is printed and stored as `redrawn`).

The clips: H x W = 24 x 32 and 13 x 17, F = 6 frames, start, end = 1, 5, P_q = 65, 1, 63, 64, 65, 257 queries for the query frames
0 .. 5, so P_max > P_q for all but one.  The queries of frame q - the rows of its own target frame q - sit on the pixel grid, distinct
and in raster order (the 257 queries of the 13 x 17 clip cannot be distinct among 221 pixels: they walk the raster and start again).
A fifth of all other samples lies outside the image, on every side; a tenth has exact integer coordinates.  time_ids is a permutation
of 0 .. 5 that is not the identity: the reference takes target_w2cs and target_Ks at the TIME id.  Rows of the track table that no
case reads are zero (they compress; the table keeps its full shape).  The images hold multiples of 1 / 256, as decoded 8-bit frames
nearly do.  The archive is written with fixed zip timestamps: the same generator gives the same bytes."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_motion_regs import write_npz  # noqa: E402

FRAMES, START, END = 6, 1, 5
P_Q = (65, 1, 63, 64, 65, 257)
TIME_IDS = (0, 2, 1, 3, 5, 4)
CLIPS = (("24x32", 24, 32, 1), ("13x17", 13, 17, 2))
#         name      query  targets
CASES = (("q0_n4", 0, (1, 4, 2, 3)),
         ("q1_n1", 1, (3,)),            # P_q = 1
         ("q2_n4", 2, (4, 1, 3, 2)),    # 63
         ("q3_n1", 3, (3,)),            # 64; the target is the query frame: the queries' own integer coordinates are sampled
         ("q4_n4", 4, (2, 4, 1, 3)),    # 65
         ("q5_n1", 5, (0,)))            # 257: two blocks of lanes; a target outside the dynamic frames


def f32(a):
    return np.asarray(a, np.float32)


def load_utils():
    spec = importlib.util.spec_from_file_location("reference_data_utils", os.path.join(os.environ["D4GS_REFERENCE"], "flow3d", "data", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw_rows(n, H, W, r):
    """[n,4] fresh samples: x, y, occlusion logit, expected-distance logit"""
    x, y = r.uniform(0, W - 1, n), r.uniform(0, H - 1, n)
    out, side = r.uniform(size=n) < 0.2, r.integers(0, 4, n)
    x = np.where(out & (side == 0), r.uniform(-6, -0.1, n), np.where(out & (side == 1), r.uniform(W - 0.9, W + 6, n), x))
    y = np.where(out & (side == 2), r.uniform(-6, -0.1, n), np.where(out & (side == 3), r.uniform(H - 0.9, H + 6, n), y))
    whole = r.uniform(size=n) < 0.1
    x, y = np.where(whole, np.round(x), x), np.where(whole, np.round(y), y)
    return f32(np.stack([x, y, r.normal(0, 2, n), r.normal(0, 2, n)], -1))


def at_edge(rows):
    t = rows.astype(np.float64)
    vis, conf = 1 - 1 / (1 + np.exp(-t[..., 2])), 1 - 1 / (1 + np.exp(-t[..., 3]))
    return (np.abs(vis * conf - 0.5) < 1e-3) | (np.abs((1 - vis) * conf - 0.5) < 1e-3)


def make_clip(H, W, seed):
    r = np.random.default_rng(seed)
    gy, gx = np.mgrid[0:H, 0:W]
    clip = dict(imgs=f32(r.integers(0, 257, (FRAMES, H, W, 3)) / 256.0),
                depths=f32(2.0 + 0.05 * gx + 0.03 * gy + r.uniform(0, 0.5, (FRAMES, H, W))),
                masks=(r.uniform(size=(FRAMES, H, W)) < 0.4).astype(np.uint8), valid_masks=(r.uniform(size=(FRAMES, H, W)) < 0.9).astype(np.uint8),
                Ks=f32([[[30.0 + t, 0.3, 15.5 + 0.2 * t], [0.0, 28.0 - 0.5 * t, 11.0], [0.0, 0.0, 1.0]] for t in range(FRAMES)]),
                w2cs=f32(np.concatenate([r.normal(size=(FRAMES, 3, 4)), np.tile([[[0.0, 0.0, 0.0, 1.0]]], (FRAMES, 1, 1))], 1)),
                time_ids=np.asarray(TIME_IDS, np.int64))
    used = {q: {q} for q in range(FRAMES)}
    for _, q, targets in CASES:
        used[q] |= set(targets)
    samples = redrawn = 0
    for q, P in enumerate(P_Q):
        tr = np.zeros((FRAMES, P, 4), np.float32)
        for t in sorted(used[q]):
            rows = draw_rows(P, H, W, r)
            if t == q:  # the queries: on the grid, distinct (while the image has pixels left) and in raster order
                pixels = np.sort(r.choice(H * W, P, replace=False)) if P <= H * W else np.arange(P) % (H * W)
                rows[:, 0], rows[:, 1] = pixels % W, pixels // W
            for _ in range(100):
                bad = at_edge(rows)
                if not bad.any():
                    break
                redrawn += int(bad.sum())
                rows[bad, 2:] = draw_rows(int(bad.sum()), H, W, r)[:, 2:]
            else:
                raise SystemExit("samples stay at an edge")
            tr[t] = rows
            samples += P
        clip[f"tracks_{q}"] = tr
    assert redrawn <= 0.02 * samples, (redrawn, samples)
    print(f"{H} x {W}: re-drawn {redrawn} of {samples} samples ({100 * redrawn / samples:.2f} %)", file=sys.stderr)
    clip["redrawn"] = np.int32(redrawn)
    return clip


def reference_batch(utils, clip, q, targets):
    """__getitem__'s training branch (stereo_low_dataset.py:603-665) for query frame q and the given target_inds, in float64"""
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    H, W = clip["depths"].shape[1:]
    target_inds = torch.tensor(targets)
    time_ids = torch.from_numpy(clip["time_ids"])
    depths, imgs = t64(clip["depths"]), t64(clip["imgs"])
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            target_tracks_2d = torch.stack([t64(clip[f"tracks_{q}"][t]) for t in targets], dim=0)
            target_ts = time_ids[target_inds]
            visibles, invisibles, confidences = utils.parse_tapir_track_info(target_tracks_2d[..., 2], target_tracks_2d[..., 3])
            track_depths = F.grid_sample(depths[target_inds, None], utils.normalize_coords(target_tracks_2d[..., None, :2], H, W),
                                         align_corners=True, padding_mode="border")[:, 0, :, 0]
            track_imgs = F.grid_sample(imgs[target_inds].permute(0, 3, 1, 2), utils.normalize_coords(target_tracks_2d[..., None, :2], H, W),
                                       align_corners=True, padding_mode="border").squeeze(-1)
            # trainer.py:549,646-647 for B = 1, the [P_all, N] product summed over its trailing axis
            frame_intervals = (time_ids[q].repeat_interleave(len(targets)) - target_ts).abs()
            w_interval = torch.exp(-2 * frame_intervals / (END - START))
            weights = (confidences.reshape(-1)[..., None] * w_interval).sum(-1).reshape(confidences.shape)
    finally:
        torch.set_default_dtype(torch.float32)
    assert track_depths.dtype == torch.float64 and track_imgs.shape == (len(targets), 3, target_tracks_2d.shape[1])
    query = clip[f"tracks_{q}"][q][:, :2].astype(np.int64)
    return dict(query=np.int32(q), targets=np.asarray(targets, np.int32), target_ts=target_ts.numpy(), visibles=visibles.numpy(),
                invisibles=invisibles.numpy(), confidences=confidences.numpy(), track_depths=track_depths.numpy(),
                track_imgs=track_imgs.numpy(), weights=weights.numpy(), pix=(query[:, 1] * W + query[:, 0]).astype(np.int32))


if __name__ == "__main__":
    utils = load_utils()
    arrays = {}
    for name, H, W, seed in CLIPS:
        clip = make_clip(H, W, seed)
        arrays.update({f"{name}/{k}": v for k, v in clip.items()})
        for case, q, targets in CASES:
            arrays.update({f"{name}/{case}/{k}": v for k, v in reference_batch(utils, clip, q, targets).items()})
    dst = os.path.join(HERE, "feed.npz")
    write_npz(dst, arrays)
    print(f"{len(arrays)} arrays -> {dst} ({os.path.getsize(dst)} bytes)", file=sys.stderr)
    assert os.path.getsize(dst) < 256 * 1024
