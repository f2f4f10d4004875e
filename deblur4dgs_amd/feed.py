"""One training batch per step from a clip that lives in device memory.

The reference makes a batch in `StereoLowDataset.__getitem__` (flow3d/data/stereo_low_dataset.py:574-666) and `train_collate_fn`
(flow3d/data/base_dataset.py:59-77): four `np.load`s, `parse_tapir_track_info`, two CPU `grid_sample`s, an upload, and then in the
trainer (trainer.py:549-565, 646-659) a round of `torch.cat`, `repeat_interleave` and a mask scatter that shape the track supervision.
`DeviceClip` holds the clip on the GPU and does all of it in ONE launch (`csrc/feed.hip`, the "Feed" block of include/d4gs.h), into
buffers of fixed address, reading nothing on the host - so a captured step sees new data on every replay:

    clip = DeviceClip(imgs, depths, masks, valid_masks, Ks, w2cs, time_ids, tracks_2d, start, end)
    out = clip.buffers()
    with torch.cuda.graph(g):
        clip.draw(seed)                     # num_targets_per_frame distinct dynamic frames; a device counter moves on
        batch = clip.batch(q, out=out)      # the reference's batch for query frame q and those targets, plus `track_tables`
        ... losses.track_losses_from_tables(tracks_3d, batch["track_tables"]) ...
    clip.check(out)                         # the one host read, when the caller wants it

What differs from the reference, on purpose:
  * file loading stays with the caller, as in `observations`: `tracks_2d[q]` is the stack over t of the rows of `{q}_{t}.npy`;
  * the draw is a counter-based integer hash of (seed, step), not numpy's global stream (`observations.bkgd_points` already takes
    that position); `draw_cpu` is its exact host twin;
  * with `out=` the per-query tensors are padded to P_max = max_q P_q (padding rows: coordinates, depth, image sample, confidence
    and weight 0, flags false, pix -1, the query (-1, -1); `n_queries` holds P_q);
  * an index or target that is out of range on the device yields an all-padding batch and a bit in `status` instead of a fault.
`target_w2cs` and `target_Ks` are taken at the targets' TIME ids, as the reference takes them (`self.w2cs[target_ts]`).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib as L
from ._lib import check, need_gpu, stream_of, vp

__all__ = ["DeviceClip", "BatchBuffers", "draw_cpu", "STATUS_BITS"]

WHO = "deblur4dgs_amd.feed"
MAX_TARGETS = 64
STATUS_BITS = {1: "the index is outside 0 .. F-1", 2: "a target is outside 0 .. F-1", 4: "a target's time id is outside 0 .. F-1",
               8: "the query frame's offsets into the track table are inconsistent"}


def draw_cpu(seed: int, step: int, start: int, end: int, n: int) -> list[int]:
    """The targets `DeviceClip.draw(seed)` writes when its counter stands at `step`: d4gs_feed_draw_cpu, the kernel's own functions
    compiled for the host."""
    counter, targets = C.c_int64(int(step)), (C.c_int32 * max(int(n), 1))()
    check(L.lib().d4gs_feed_draw_cpu(C.byref(counter), int(seed) & (2 ** 64 - 1), int(start), int(end), int(n), targets),
          "d4gs_feed_draw_cpu")
    return list(targets)[:int(n)]


@dataclass
class BatchBuffers:
    """One fixed allocation per batch tensor, the per-query ones padded to P_max.  `n_queries` (P_q) and `status` are int32 device
    scalars."""
    ts: torch.Tensor
    w2cs: torch.Tensor
    Ks: torch.Tensor
    imgs: torch.Tensor
    valid_masks: torch.Tensor
    masks: torch.Tensor
    depths: torch.Tensor
    query_tracks_2d: torch.Tensor
    target_ts: torch.Tensor
    target_w2cs: torch.Tensor
    target_Ks: torch.Tensor
    target_tracks_2d: torch.Tensor
    target_visibles: torch.Tensor
    target_invisibles: torch.Tensor
    target_confidences: torch.Tensor
    target_track_depths: torch.Tensor
    target_track_imgs: torch.Tensor
    pix: torch.Tensor
    rows: torch.Tensor
    vis: torch.Tensor
    weights: torch.Tensor
    n_queries: torch.Tensor
    status: torch.Tensor


class DeviceClip:
    """imgs [F,H,W,3], depths, masks, valid_masks [F,H,W], Ks [F,3,3], w2cs [F,4,4] fp32 and time_ids [F] (int) on the GPU;
    tracks_2d: a list of F tensors, entry q [F,P_q,4] = for query frame q and every target frame t the rows (x, y, occlusion logit,
    expected-distance logit) of the reference's `{q}_{t}.npy`.  The dynamic frames are start .. end-1."""

    def __init__(self, imgs, depths, masks, valid_masks, Ks, w2cs, time_ids, tracks_2d, start: int, end: int,
                 num_targets_per_frame: int = 4):
        for t in (imgs, depths, masks, valid_masks, Ks, w2cs, time_ids, *tracks_2d):
            need_gpu(t, WHO)
        if imgs.dim() != 4 or imgs.shape[-1] != 3:
            raise ValueError(f"imgs must be [F,H,W,3], got {tuple(imgs.shape)}")
        F, H, W, _ = imgs.shape
        for name, x, want in (("depths", depths, (F, H, W)), ("masks", masks, (F, H, W)), ("valid_masks", valid_masks, (F, H, W)),
                              ("Ks", Ks, (F, 3, 3)), ("w2cs", w2cs, (F, 4, 4)), ("time_ids", time_ids, (F,))):
            if tuple(x.shape) != want:
                raise ValueError(f"{name} must be {want}, got {tuple(x.shape)}")
        if F < 1 or H < 1 or W < 1 or F * H * W * 3 > 2 ** 31 - 1:
            raise ValueError(f"a clip of {F} frames of {H} x {W}: each size >= 1, F H W 3 <= 2^31 - 1")
        if time_ids.is_floating_point() or time_ids.dtype == torch.bool:
            raise ValueError(f"time_ids must be an integer tensor, got {time_ids.dtype}")
        if len(tracks_2d) != F:
            raise ValueError(f"{len(tracks_2d)} track tensors for {F} frames")
        for q, t in enumerate(tracks_2d):
            if t.dim() != 3 or t.shape[0] != F or t.shape[2] != 4 or t.shape[1] < 1:
                raise ValueError(f"tracks_2d[{q}] must be [{F},P,4] with P >= 1, got {tuple(t.shape)}")
        if not 0 <= start < end <= F:
            raise ValueError(f"start={start}, end={end}: 0 <= start < end <= {F}")
        N = int(num_targets_per_frame)
        if not 1 <= N <= min(end - start, MAX_TARGETS):
            raise ValueError(f"num_targets_per_frame={N}: 1 <= it <= min(end - start, {MAX_TARGETS}) = {min(end - start, MAX_TARGETS)}")
        dev = imgs.device
        f32 = lambda x: x.detach().to(dev, torch.float32).contiguous()
        self.imgs, self.depths, self.masks, self.valid_masks = f32(imgs), f32(depths), f32(masks), f32(valid_masks)
        self.Ks, self.w2cs = f32(Ks), f32(w2cs)
        self.time_ids = time_ids.detach().to(dev, torch.int64).contiguous()
        self.F, self.H, self.W, self.start, self.end, self.num_targets = F, H, W, int(start), int(end), N
        self.P = [int(t.shape[1]) for t in tracks_2d]
        self.P_max = max(self.P)
        if N * self.P_max * 3 > 2 ** 31 - 1:
            raise ValueError(f"{N} targets of {self.P_max} queries: N P_max 3 <= 2^31 - 1")
        # one [sum_q F P_q, 4] table, query frame q's rows at offsets[q] .. offsets[q+1], target-frame-major
        self.tracks = torch.cat([f32(t).reshape(-1, 4) for t in tracks_2d]).contiguous()
        offsets = [0]
        for p in self.P:
            offsets.append(offsets[-1] + F * p)
        self.offsets = torch.tensor(offsets, dtype=torch.int64, device=dev)
        self.device = dev
        self._frames = torch.arange(F, dtype=torch.int32, device=dev)  # index q as a device tensor: the view [q:q+1], no copy
        self._start = torch.full((1,), int(start), dtype=torch.int64, device=dev)
        self.targets = torch.arange(start, start + N, dtype=torch.int32, device=dev)  # what draw() writes
        self.counter = torch.zeros((), dtype=torch.int64, device=dev)                 # the step counter draw() moves on
        self.status = torch.zeros((), dtype=torch.int32, device=dev)                  # of the calls without `out`

    def get_dyn_image_ids(self):
        return list(range(self.start, self.end))

    def _alloc(self, N, P, planes) -> BatchBuffers:
        dev, H, W = self.device, self.H, self.W
        e = lambda *s, dtype=torch.float32: torch.empty(*s, device=dev, dtype=dtype)
        return BatchBuffers(
            ts=e(1, dtype=torch.int64), w2cs=e(1, 4, 4), Ks=e(1, 3, 3), imgs=e(1, H, W, 3) if planes else None,
            valid_masks=e(1, H, W) if planes else None, masks=e(1, H, W) if planes else None, depths=e(1, H, W) if planes else None,
            query_tracks_2d=e(P, 2), target_ts=e(N, dtype=torch.int64), target_w2cs=e(N, 4, 4), target_Ks=e(N, 3, 3),
            target_tracks_2d=e(N, P, 2), target_visibles=e(N, P, dtype=torch.uint8), target_invisibles=e(N, P, dtype=torch.uint8),
            target_confidences=e(N, P), target_track_depths=e(N, P), target_track_imgs=e(N, 3, P), pix=e(N * P, dtype=torch.int32),
            rows=e(N * P, dtype=torch.int32), vis=e(N * P, dtype=torch.uint8), weights=e(N * P),
            n_queries=e((), dtype=torch.int32), status=torch.zeros((), device=dev, dtype=torch.int32) if planes else self.status)

    def buffers(self, num_targets=None) -> BatchBuffers:
        """The fixed buffers `batch(..., out=)` writes: the per-query tensors hold P_max rows."""
        return self._alloc(self.num_targets if num_targets is None else int(num_targets), self.P_max, True)

    def draw(self, seed: int):
        """Writes `num_targets_per_frame` distinct dynamic frames to `self.targets` from a hash of (seed, self.counter) and adds one to
        the counter, all on the device: a replayed graph draws new targets on every replay.  -> self.targets"""
        check(L.lib().d4gs_feed_draw(vp(self.counter), int(seed) & (2 ** 64 - 1), self.start, self.end, self.num_targets, vp(self.targets),
                                     stream_of(self.counter)), "d4gs_feed_draw")
        return self.targets

    def batch(self, index, target_inds=None, out: BatchBuffers | None = None) -> dict:
        """The reference's batch of size 1 for query frame `index` (an int, or an int32 device tensor [1]) and the target frames
        `target_inds` (a sequence of ints, an int32 device tensor [N], or None: what `draw` wrote last), plus `track_tables`, the
        arrays `losses.track_losses_from_tables` takes, `n_queries` and `status`.

        Collated keys carry the batch axis: ts [1] int64, w2cs [1,4,4], Ks [1,3,3], imgs [1,H,W,3], valid_masks, masks, depths [1,H,W],
        start [1]; target_track_imgs is [N,3,P] as the dataset returns it (run_training_dynamic.py wraps it in a list itself); the
        keys `train_collate_fn` leaves as lists are lists of one tensor: query_tracks_2d
        [P,2], target_ts [N] int64, target_w2cs [N,4,4], target_Ks [N,3,3], target_tracks_2d [N,P,2], target_visibles,
        target_invisibles [N,P] bool, target_confidences, target_track_depths [N,P].

        Without `out` the planes are views of the clip's storage, the rest is freshly allocated with P = P_q, and `index` must be an
        int (P_q and the views need it on the host).  With `out` everything is written in place, planes included, P = P_max, and
        every returned tensor is a view of `out`: the same addresses on every call.  Inside a stream capture pass `index` as an int
        or a device tensor and the targets as a device tensor or None; a sequence of ints is uploaded."""
        F = self.F
        if torch.is_tensor(index):
            if out is None:
                raise ValueError("batch(): an index in device memory needs out= (the views and P_q of a call without it need the index on the host)")
            if index.dtype != torch.int32 or index.numel() != 1 or not index.is_cuda:
                raise ValueError(f"index must be an int or an int32 device tensor [1], got {index.dtype} {tuple(index.shape)}")
            q, index_t = None, index.contiguous()
        else:
            q = int(index)
            if not 0 <= q < F:
                raise ValueError(f"index={q} outside 0..{F - 1}")
            index_t = self._frames[q:q + 1]
        if target_inds is None:
            targets = self.targets
        elif torch.is_tensor(target_inds):
            if target_inds.dtype != torch.int32 or target_inds.dim() != 1 or not target_inds.is_cuda:
                raise ValueError(f"target_inds must be an int32 device tensor [N], got {target_inds.dtype} {tuple(target_inds.shape)}")
            targets = target_inds.contiguous()
        else:
            ids = [int(t) for t in target_inds]
            if any(not 0 <= t < F for t in ids):
                raise ValueError(f"target_inds={ids} outside 0..{F - 1}")
            targets = torch.tensor(ids, dtype=torch.int32, device=self.device)
        N = targets.numel()
        if not 1 <= N <= MAX_TARGETS:
            raise ValueError(f"{N} target frames (1 <= N <= {MAX_TARGETS})")
        if out is None:
            P, b = self.P[q], self._alloc(N, self.P[q], False)  # (status: the clip's own)
        else:
            P, b = self.P_max, out
            if tuple(b.target_tracks_2d.shape) != (N, P, 2) or tuple(b.imgs.shape) != (1, self.H, self.W, 3):
                raise ValueError(f"out holds target_tracks_2d {tuple(b.target_tracks_2d.shape)} and imgs {tuple(b.imgs.shape)}; this clip "
                                 f"writes {(N, P, 2)} and {(1, self.H, self.W, 3)}: take it from buffers()")
        check(L.lib().d4gs_feed_batch(
            vp(self.imgs), vp(self.depths), vp(self.masks), vp(self.valid_masks), vp(self.Ks), vp(self.w2cs), vp(self.time_ids),
            vp(self.tracks), vp(self.offsets), self.tracks.shape[0], vp(index_t), vp(targets), F, self.H, self.W, N, P, self.end - self.start,
            vp(b.ts), vp(b.w2cs), vp(b.Ks), vp(b.imgs), vp(b.valid_masks), vp(b.masks), vp(b.depths), vp(b.query_tracks_2d), vp(b.target_ts),
            vp(b.target_w2cs), vp(b.target_Ks), vp(b.target_tracks_2d), vp(b.target_visibles), vp(b.target_invisibles),
            vp(b.target_confidences), vp(b.target_track_depths), vp(b.target_track_imgs), vp(b.pix), vp(b.rows), vp(b.vis), vp(b.weights),
            vp(b.n_queries), vp(b.status), stream_of(self.imgs)), "d4gs_feed_batch")
        planes = {k: getattr(self, k)[q:q + 1] if out is None else getattr(b, k) for k in ("imgs", "valid_masks", "masks", "depths")}
        return {"ts": b.ts, "w2cs": b.w2cs, "Ks": b.Ks, **planes, "start": self._start,
                "query_tracks_2d": [b.query_tracks_2d], "target_ts": [b.target_ts], "target_w2cs": [b.target_w2cs],
                "target_Ks": [b.target_Ks], "target_tracks_2d": [b.target_tracks_2d],
                "target_visibles": [b.target_visibles.view(torch.bool)], "target_invisibles": [b.target_invisibles.view(torch.bool)],
                "target_confidences": [b.target_confidences], "target_track_depths": [b.target_track_depths],
                "target_track_imgs": b.target_track_imgs,
                "track_tables": {"pix": b.pix, "rows": b.rows, "vis": b.vis, "weights": b.weights,
                                 "tgt_2d": b.target_tracks_2d.view(-1, 2), "tgt_depth": b.target_track_depths.view(-1),
                                 "Ks": b.target_Ks.view(-1, 9)},
                "n_queries": b.n_queries, "status": b.status}

    def check(self, out: BatchBuffers | None = None):
        """Reads the status word (of `out`, or of the calls without one) - the one host read, made when the caller decides - clears
        it, and raises if a selection was out of range since the last check."""
        status = self.status if out is None else out.status
        bits = int(status.item())
        if bits:
            status.zero_()
            raise RuntimeError("DeviceClip: a batch was written as padding: " + "; ".join(w for b, w in STATUS_BITS.items() if bits & b))
