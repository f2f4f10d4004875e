"""Observations from raw arrays: what flow3d/data/utils.py and the `get_tracks_3d` / `get_bkgd_points` bodies of the reference's
datasets do between loading a dataset and `scene_init`.

A dataset's raw arrays - aligned depth maps, foreground masks, TAPIR 2-D tracks, `Ks`, `w2cs` - become `scene_init.TrackObservations`
and `scene_init.StaticObservations`.  The three expensive steps are HIP kernels (`csrc/observations.hip`, the "Observations" block of
include/d4gs.h): the masked median blur that the reference itself marks as "very expensive", the lifting of 2-D tracks to 3-D, and
the background points with their normals.  There is no torch fallback for a kernel: a CPU tensor is refused.

    depths = filter_depths(depths, masks, valid_masks)                          # clamp, masked median blur, blend: [T,H,W]
    fg_masks = ((masks * valid_masks * (depths > 0)) > 0.5).float()              # what the reference lifts against
    tracks = tracks_3d(raw_tracks_2d, query_indices, imgs, depths, fg_masks, Ks, w2cs)    # TrackObservations
    static = bkgd_points(imgs, depths, masks, valid_masks, Ks, w2cs, 100_000, generator)  # StaticObservations

What differs from the reference, on purpose:
  * a sample is "in the mask" iff every bilinear corner with a non-zero weight is inside the image and has mask == 1.  The
    reference's `grid_sample(mask) == 1` also rejects about 1.5 % of samples whose four corners are all 1, because the rounded
    weights do not sum to 1; that is rounding, not intent;
  * the choice without replacement in `bkgd_points` comes from `torch.randperm` on a `torch.Generator` (numpy's global stream is
    no contract);
  * file loading, the `np.random.choice` over tracks and the cache file stay with the caller.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._lib import check, need_gpu, stream_of, vp
from .scene_init import StaticObservations, TrackObservations

__all__ = ["masked_median_blur", "filter_depths", "parse_tapir_track_info", "lift_tracks", "tracks_3d_for_query_frame", "tracks_3d",
           "bkgd_points_dense", "bkgd_points", "visible_count_threshold"]

WHO = "deblur4dgs_amd.observations"


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _median(image, mask, blend, kernel_size, per_image):
    """[n,H,W] fp32 contiguous each -> [n,H,W]"""
    n, H, W = image.shape
    lib = L.lib()
    nbytes = lib.d4gs_masked_median_ws_bytes(n, H, W)
    if nbytes == 0:
        raise ValueError(f"masked_median_blur: {n} images of {H} x {W} (each size >= 1, their product <= 2^31 - 1)")
    ws = torch.empty(nbytes // 4, device=image.device, dtype=torch.float32)
    out = torch.empty_like(image)
    check(lib.d4gs_masked_median_blur(vp(image), vp(mask), vp(blend), n, H, W, int(kernel_size), int(per_image), vp(out), vp(ws),
                                      stream_of(image)), "d4gs_masked_median_blur")
    return out


def masked_median_blur(image, mask, kernel_size: int = 11):
    """utils.py:207-250, exactly: image, mask [B,C,H,W] -> the lower median of every k x k window in which the entries whose mask is
    not 1 (zero padding included) are replaced alternately by min(image.min(), 0) and max(image.max(), 0), in the order the
    reference's `nonzero` visits them across the whole tensor.  Bitwise the reference's output; finite inputs."""
    need_gpu(image, WHO)
    if image.dim() != 4 or image.shape != mask.shape:
        raise ValueError(f"image and mask must be [B,C,H,W] of one shape, got {tuple(image.shape)} and {tuple(mask.shape)}")
    B, Cn, H, W = image.shape
    if image.numel() == 0:
        return _f32(image).clone()
    out = _median(_f32(image).reshape(B * Cn, H, W), _f32(mask.to(image.device)).reshape(B * Cn, H, W), None, kernel_size, False)
    return out.reshape(B, Cn, H, W)


def filter_depths(depths, masks, valid_masks, kernel_size: int = 11):
    """stereo_low_dataset.py:218-241: depths, masks, valid_masks [T,H,W] -> [T,H,W].  The depths are clamped to [0, 2.5 x the median of
    the per-frame maxima]; every frame is blurred on its own by `masked_median_blur` under mask * valid_mask * (depth > 0) and blended
    as blurred * mask + depth * (1 - mask).  All frames in one call; bitwise what one call per frame gives."""
    need_gpu(depths, WHO)
    if depths.dim() != 3 or masks.shape != depths.shape or valid_masks.shape != depths.shape:
        raise ValueError(f"depths, masks, valid_masks must be [T,H,W] of one shape, got {tuple(depths.shape)}, {tuple(masks.shape)}, "
                         f"{tuple(valid_masks.shape)}")
    d = _f32(depths)
    if d.numel() == 0:
        return d.clone()
    m, v = _f32(masks.to(d.device)), _f32(valid_masks.to(d.device))
    top = d.reshape(d.shape[0], -1).max(1).values.median() * 2.5
    d = torch.clamp(d, torch.zeros_like(top), top)
    return _median(d, (m * v * (d > 0)).contiguous(), m, kernel_size, True)


def parse_tapir_track_info(occlusions, expected_dist):
    """utils.py:53-66 on the device -> (valid_visible, valid_invisible, confidence)."""
    need_gpu(occlusions, WHO)
    vis = 1 - torch.sigmoid(occlusions)
    conf = 1 - torch.sigmoid(expected_dist)
    visible = vis * conf > 0.5
    invisible = (1 - vis) * conf > 0.5
    return visible, invisible, conf * (visible | invisible).float()


def lift_tracks(query_index: int, query_img, tracks_2d, depths, masks, inv_Ks, c2ws):
    """The kernel as it is, before any filter -> dict of xyz [N,T,3], visibles, invisibles, in_mask [N,T] bool, confidences [N,T],
    colors [N,3], visible_count [N] int32, hist [T + 1] int32 (how many tracks have each visible count)."""
    need_gpu(tracks_2d, WHO)
    if tracks_2d.dim() != 3 or tracks_2d.shape[-1] != 4:
        raise ValueError(f"tracks_2d must be [N,T,4], got {tuple(tracks_2d.shape)}")
    N, T, _ = tracks_2d.shape
    if depths.dim() != 3 or depths.shape[0] != T or masks.shape != depths.shape:
        raise ValueError(f"depths and masks must be [T,H,W] with T = {T}, got {tuple(depths.shape)} and {tuple(masks.shape)}")
    _, H, W = depths.shape
    if tuple(query_img.shape) != (H, W, 3) or tuple(inv_Ks.shape) != (T, 3, 3) or tuple(c2ws.shape) != (T, 4, 4):
        raise ValueError(f"query_img [H,W,3], inv_Ks [T,3,3], c2ws [T,4,4] expected, got {tuple(query_img.shape)}, {tuple(inv_Ks.shape)}, "
                         f"{tuple(c2ws.shape)}")
    if not 0 <= int(query_index) < T:
        raise ValueError(f"query_index={query_index} outside 0..{T - 1}")
    dev = tracks_2d.device
    tr = _f32(tracks_2d)
    out = dict(xyz=torch.empty(N, T, 3, device=dev), visibles=torch.empty(N, T, device=dev, dtype=torch.uint8),
               invisibles=torch.empty(N, T, device=dev, dtype=torch.uint8), confidences=torch.empty(N, T, device=dev),
               in_mask=torch.empty(N, T, device=dev, dtype=torch.uint8), colors=torch.empty(N, 3, device=dev),
               visible_count=torch.empty(N, device=dev, dtype=torch.int32), hist=torch.zeros(T + 1, device=dev, dtype=torch.int32))
    if N > 0:
        d, m, q, ik, cw = (_f32(x.to(dev)) for x in (depths, masks, query_img, inv_Ks, c2ws))
        check(L.lib().d4gs_lift_tracks(vp(tr), vp(d), vp(m), vp(q), vp(ik), vp(cw), N, T, H, W, int(query_index), vp(out["xyz"]),
                                       vp(out["visibles"]), vp(out["invisibles"]), vp(out["confidences"]), vp(out["in_mask"]),
                                       vp(out["colors"]), vp(out["visible_count"]), vp(out["hist"]), stream_of(tr)), "d4gs_lift_tracks")
    for k in ("visibles", "invisibles", "in_mask"):
        out[k] = out[k].bool()
    return out


def visible_count_threshold(hist, num_frames: int) -> float:
    """min(int(0.05 num_frames), the 0.1 quantile of the visible counts) from their histogram (a list of T + 1 ints): torch's linear
    quantile, position 0.1 (N - 1) between the sorted counts, interpolated in fp32 as `torch.quantile` of a float tensor does."""
    n = sum(hist)
    if n == 0:
        return float(int(0.05 * num_frames))
    pos = torch.tensor(0.1, dtype=torch.float32) * (n - 1)  # torch.quantile takes the position in the tensor's own dtype
    below, above = int(pos.floor().item()), int(pos.ceil().item())

    def at(rank):  # the count of the track of that rank among the sorted counts
        seen = 0
        for count, tracks in enumerate(hist):
            seen += tracks
            if rank < seen:
                return count
        return len(hist) - 1

    q = torch.lerp(torch.tensor(float(at(below))), torch.tensor(float(at(above))), pos - pos.floor()).item()
    return min(int(0.05 * num_frames), q)


def _kept(r, valid):
    return r["xyz"][valid], r["colors"][valid], r["visibles"][valid], r["invisibles"][valid], r["confidences"][valid]


def tracks_3d_for_query_frame(query_index: int, query_img, tracks_2d, depths, masks, inv_Ks, c2ws):
    """utils.py:69-168 -> (tracks_3d [N',T,3], colors [N',3], visibles, invisibles [N',T] bool, confidences [N',T]): the tracks that are
    in the mask at the query frame and visible in at least min(int(0.05 T), quantile_0.1(visible counts)) frames.  The quantile comes
    from the kernel's histogram of T + 1 integers: the one host read."""
    r = lift_tracks(query_index, query_img, tracks_2d, depths, masks, inv_Ks, c2ws)
    T = tracks_2d.shape[1]
    th = visible_count_threshold(r["hist"].tolist(), T)
    return _kept(r, r["in_mask"][:, int(query_index)] & (r["visible_count"] >= th))


def tracks_3d(raw_tracks_2d, query_indices, imgs, depths, masks, Ks, w2cs, num_dyn_frames=None) -> TrackObservations:
    """The loop of get_tracks_3d (stereo_low_dataset.py:415-490): raw_tracks_2d is a list of [N_i,T,4] tensors, the i-th holding the
    tracks queried in frame query_indices[i] (an index into the T frames); imgs [T,H,W,3], depths, masks [T,H,W] (masks as the caller
    wants them compared with 1: the reference passes ((masks * valid_masks * (depths > 0)) > 0.5).float()), Ks [T,3,3], w2cs [T,4,4].
    A track is kept if it is visible in at least min(int(0.05 num_dyn_frames), quantile_0.1) frames (num_dyn_frames defaults to T);
    the query-frame mask term of `tracks_3d_for_query_frame` is not applied here, as in the reference."""
    need_gpu(depths, WHO)
    if len(raw_tracks_2d) != len(query_indices):
        raise ValueError(f"{len(raw_tracks_2d)} track tensors for {len(query_indices)} query indices")
    T = depths.shape[0]
    dev = depths.device
    inv_Ks = torch.linalg.inv(Ks.to(dev).float())
    c2ws = torch.linalg.inv(w2cs.to(dev).float())
    d, m, im = _f32(depths), _f32(masks.to(dev)), _f32(imgs.to(dev))
    frames = T if num_dyn_frames is None else int(num_dyn_frames)
    lifted = [lift_tracks(int(q), im[int(q)], tr.to(dev), d, m, inv_Ks, c2ws) for q, tr in zip(query_indices, raw_tracks_2d)]
    hists = torch.stack([r["hist"] for r in lifted]).tolist() if lifted else []  # every query frame's histogram in one host read
    parts = [_kept(r, r["visible_count"] >= visible_count_threshold(h, frames)) for r, h in zip(lifted, hists)]
    if not parts:
        z = torch.zeros(0, T, device=dev)
        return TrackObservations(torch.zeros(0, T, 3, device=dev), z.bool(), z.bool(), z, torch.zeros(0, 3, device=dev))
    xyz, colors, vis, invis, conf = (torch.cat(x, 0) for x in zip(*parts))
    return TrackObservations(xyz, vis, invis, conf, colors)


def _bkgd(depths, masks, valid_masks, inv_Ks, c2ws, compact):
    if depths.dim() != 3 or masks.shape != depths.shape or valid_masks.shape != depths.shape:
        raise ValueError(f"depths, masks, valid_masks must be [T,H,W] of one shape, got {tuple(depths.shape)}, {tuple(masks.shape)}, "
                         f"{tuple(valid_masks.shape)}")
    T, H, W = depths.shape
    if tuple(inv_Ks.shape) != (T, 3, 3) or tuple(c2ws.shape) != (T, 4, 4):
        raise ValueError(f"inv_Ks [T,3,3] and c2ws [T,4,4] expected, got {tuple(inv_Ks.shape)} and {tuple(c2ws.shape)}")
    dev = depths.device
    d, m, v, ik, cw = (_f32(x.to(dev)) for x in (depths, masks, valid_masks, inv_Ks, c2ws))
    points = torch.empty(T, H, W, 3, device=dev)
    normals = torch.empty(T, H, W, 3, device=dev)
    keep = torch.empty(T, H, W, device=dev, dtype=torch.uint8)
    index = torch.empty(T, H * W, device=dev, dtype=torch.int32) if compact else None
    counts = torch.zeros(T, device=dev, dtype=torch.int32) if compact else None
    if keep.numel() > 0:
        check(L.lib().d4gs_bkgd_points(vp(d), vp(m), vp(v), vp(ik), vp(cw), T, H, W, vp(points), vp(normals), vp(keep), vp(index), vp(counts),
                                       stream_of(d)), "d4gs_bkgd_points")
    return points, normals, keep, index, counts


def bkgd_points_dense(depths, masks, valid_masks, inv_Ks, c2ws):
    """depths, masks, valid_masks [T,H,W], inv_Ks [T,3,3], c2ws [T,4,4] -> (points [T,H,W,3], normals [T,H,W,3], keep [T,H,W] bool):
    every pixel's world point, the reference's `normal_from_depth_image` (zero on the one-pixel border) and the flag
    ((1 - mask) * valid_mask * (depth > 0)) != 0."""
    need_gpu(depths, WHO)
    points, normals, keep, _, _ = _bkgd(depths, masks, valid_masks, inv_Ks, c2ws, False)
    return points, normals, keep.bool()


def bkgd_points(imgs, depths, masks, valid_masks, Ks, w2cs, num_samples: int, generator=None) -> StaticObservations:
    """get_bkgd_points (stereo_low_dataset.py:512-569): per frame, the pixels outside the foreground mask with a valid, positive depth
    become world points with normals and colours, in row-major order (the order of boolean indexing: the kernel compacts the kept
    pixels' offsets on the device, and the kept counts of all frames are the one host read); a frame contributes floor(num_samples / T)
    of them, the last frame the remainder, chosen without replacement by `torch.randperm(kept, generator=generator)[:share]` when it has
    more."""
    need_gpu(depths, WHO)
    T, H, W = depths.shape
    if tuple(imgs.shape) != (T, H, W, 3):
        raise ValueError(f"imgs must be [T,H,W,3] = {(T, H, W, 3)}, got {tuple(imgs.shape)}")
    dev = depths.device
    if not T:
        z = torch.zeros(0, 3, device=dev)
        return StaticObservations(z, z.clone(), z.clone())
    im = _f32(imgs.to(dev))
    points, normals, _, index, counts = _bkgd(depths, masks, valid_masks, torch.linalg.inv(Ks.to(dev).float()),
                                              torch.linalg.inv(w2cs.to(dev).float()), True)
    share = num_samples // T
    rows = []
    for t, kept in enumerate(counts.tolist()):
        idx = index[t, :kept]
        want = share if t != T - 1 else num_samples - (T - 1) * share
        if want < kept:
            gen_dev = "cpu" if generator is None else generator.device
            idx = idx[torch.randperm(kept, generator=generator, device=gen_dev)[:max(want, 0)].to(dev)]
        rows.append(idx.long() + t * H * W)
    rows = torch.cat(rows)
    return StaticObservations(*(x.reshape(-1, 3)[rows] for x in (points, normals, im)))
