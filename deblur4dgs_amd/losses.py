"""The reference's image-sized training losses as HIP kernels: the photometric term and the quantile-trimmed
masked L1 / depth-gradient losses of flow3d/loss_utils.py.

`photometric_loss(pred, gt, mask)` = 0.8 * L1 + 0.2 * (1 - SSIM) on `pred * mask` vs `gt * mask`, the expression the
reference evaluates three to four times per step (flow3d/trainer.py:388-392,575-586) with `pytorch_msssim.SSIM` and
~85 eager launches per evaluation; here: two kernels forward, one backward (`csrc/photometric.hip`).  Images are
channel-last [B,H,W,3] as the rasterizer returns them (no permute), the mask is [B,H,W] or [B,H,W,1].

`masked_l1_loss`, `trimmed_l1_loss` and `compute_gradient_loss` carry the names and signatures of flow3d/loss_utils.py, so
`from deblur4dgs_amd.losses import ...` replaces `from flow3d.loss_utils import ...`.  The reference finds its threshold with
`torch.quantile` (a full sort) and selects with boolean masks (`nonzero`: the host waits for the device); here the two order
statistics come from a radix select and nothing is read on the host, so the losses can sit inside a captured HIP graph
(`csrc/trimmed.hip`).  Gradients flow to `pred` only.

`track_losses` is the 2-D track loss and the mapped (track) depth loss of `Trainer.compute_dynamic_losses`
(flow3d/trainer.py:633-667,681-689) on the same machinery: one value pass gathers the rendered track points at the query pixels
and projects them, the selection runs for the 2-D term only, one kernel scatters the gradient back.

`motion_regularizers` is what is left of that function beyond the render (flow3d/trainer.py:691-728): the smoothness of the motion
bases, the smoothness of every foreground track, the acceleration along the viewing ray and the variance of the raw scales, in one
call forward and one backward on the pose kernels (`csrc/motion_regs.hip`).

`track_fit_losses` is the loss of the warm-up that runs before training (flow3d/init_utils.py:273-402, `run_initial_optim`): six terms
from one deformation per (Gaussian, frame), forward and backward on the pose kernels (`csrc/track_fit.hip`);
`scene_init.run_initial_optim` is the loop around it.

`dilate_mask`, `sharp_keep_loss` and `coverage_loss` are the passes of those two functions that the reference writes as plain torch
ops: `nn.MaxPool2d(9, 1, 4)` on the foreground mask (trainer.py:120,388,575,901), the area-reduced masked L1 between the sharp
sub-sample and the blurry target (:736-760) and `F.mse_loss` on the accumulated alpha (:621-631) (`csrc/image_terms.hip`, DESIGN.md
section 22).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from ._lib import f32c, need_gpu, stream_of, vp

_WHO = "deblur4dgs_amd.losses"  # the name a CPU tensor is refused under


class PhotometricFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask, w_l1, w_ssim):
        need_gpu(pred, _WHO)
        B, H, W, Cc = pred.shape
        p, g = f32c(pred), f32c(gt)
        m = None if mask is None else mask.detach().float().reshape(B, H, W).contiguous()
        lib = L.lib()
        if not hasattr(lib, "d4gs_photometric_maps_elems"):  # only an override library can lack it (_lib.APPENDED)
            raise RuntimeError(f"{L.LIB_PATH} predates d4gs_photometric_maps_elems: its photometric kernels use another maps layout")
        nb = lib.d4gs_photometric_blocks(B, H, W)
        maps = torch.empty(lib.d4gs_photometric_maps_elems(B, H, W), device=p.device, dtype=torch.float32)
        scratch = torch.empty(2 * nb + 3, device=p.device, dtype=torch.float32)
        stream = stream_of(p)
        L.check(lib.d4gs_photometric_fwd(vp(p), vp(g), vp(m), B, H, W, Cc, w_l1, w_ssim, vp(maps), vp(scratch),
                                         vp(scratch[2 * nb:]), stream), "d4gs_photometric_fwd")
        ctx.keep = (p, g, m, maps)
        ctx.w = (float(w_l1), float(w_ssim))
        out = scratch[2 * nb:]
        return out[0].clone(), out[1].clone(), out[2].clone()

    @staticmethod
    def backward(ctx, v_loss, v_l1, v_ssim):
        p, g, m, maps = ctx.keep
        B, H, W, Cc = p.shape
        v = v_loss.detach().float().reshape(1).contiguous()
        out = torch.empty_like(p)
        stream = stream_of(p)
        L.check(L.lib().d4gs_photometric_bwd(vp(p), vp(g), vp(m), vp(maps), vp(v), B, H, W, Cc, ctx.w[0], ctx.w[1], vp(out),
                                             stream), "d4gs_photometric_bwd")
        return out, None, None, None, None


def photometric_loss(pred, gt, mask=None, w_l1: float = 0.8, w_ssim: float = 0.2, return_terms: bool = False):
    """-> scalar loss (and, with return_terms, the detached L1 and SSIM values).  Differentiable w.r.t. `pred` only
    (the reference's `imgs` and masks are data)."""
    loss, l1, ssim = PhotometricFn.apply(pred, gt, mask, float(w_l1), float(w_ssim))
    return (loss, l1.detach(), ssim.detach()) if return_terms else loss


def _check_quantile(quantile, upper_open):
    q = float(quantile)
    if not (q > 0.0) or q == float("inf") or (not upper_open and q > 1.0):
        raise ValueError(f"quantile={quantile}: must be in (0, 1]" + (" (or above 1: nothing is trimmed)" if upper_open else ""))
    return q


def _scratch(n_max, terms, device):
    words = L.lib().d4gs_trimmed_scratch_words(n_max, terms)
    if words == 0:
        raise RuntimeError(f"trimmed losses: {n_max} elements (at most 2^31 - 1)")
    return torch.empty(words, device=device, dtype=torch.int32), words


class _TrimmedL1Fn(torch.autograd.Function):
    """mask is None: the trimmed mean (always selects); otherwise the masked forms (quantile >= 1: every element kept)."""

    @staticmethod
    def forward(ctx, pred, gt, mask, normalize, quantile):
        need_gpu(pred, _WHO)
        if pred.shape != gt.shape or pred.dim() < 1:
            raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have the same shape, at least 1-D")
        D = pred.shape[-1]
        if D < 1:
            raise ValueError("the last axis of pred is empty")
        n = pred.numel() // D
        if n == 0:
            raise ValueError("no elements (torch.quantile of an empty tensor raises too)")
        p, g = f32c(pred), f32c(gt)
        m = None
        if mask is not None:
            if mask.numel() != n:
                raise ValueError(f"mask {tuple(mask.shape)} does not match the {tuple(pred.shape[:-1])} elements of pred")
            m = f32c(mask).reshape(n)
        lib = L.lib()
        scratch, words = _scratch(n, 1, p.device)
        out = torch.empty(8, device=p.device, dtype=torch.float32)
        stream = stream_of(p)
        if m is None:
            L.check(lib.d4gs_trimmed_l1_fwd(vp(p), vp(g), n, D, quantile, vp(scratch), words, vp(out), stream), "d4gs_trimmed_l1_fwd")
        else:
            L.check(lib.d4gs_masked_l1_fwd(vp(p), vp(g), vp(m), n, D, int(bool(normalize)), quantile, vp(scratch), words, vp(out), stream),
                    "d4gs_masked_l1_fwd")
        ctx.keep = (p, g, m, scratch, out)
        ctx.args = (n, D, quantile, pred.shape, pred.dtype)
        return out[0].clone()

    @staticmethod
    def backward(ctx, v_loss):
        p, g, m, scratch, out = ctx.keep
        n, D, quantile, shape, dtype = ctx.args
        v = v_loss.detach().float().reshape(1).contiguous()
        v_pred = torch.empty_like(p)
        stream = stream_of(p)
        lib = L.lib()
        if m is None:
            L.check(lib.d4gs_trimmed_l1_bwd(vp(p), vp(g), vp(scratch), vp(out), vp(v), n, D, vp(v_pred), stream), "d4gs_trimmed_l1_bwd")
        else:
            L.check(lib.d4gs_masked_l1_bwd(vp(p), vp(g), vp(m), vp(scratch), vp(out), vp(v), n, D, quantile, vp(v_pred), stream),
                    "d4gs_masked_l1_bwd")
        return v_pred.reshape(shape).to(dtype), None, None, None, None


class _GradientLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask, quantile):
        need_gpu(pred, _WHO)
        if pred.dim() == 4 and pred.shape[-1] != 1:
            raise NotImplementedError(f"compute_gradient_loss: {pred.shape[-1]} channels (one is supported: [B,H,W] or [B,H,W,1])")
        if pred.dim() not in (3, 4) or pred.shape != gt.shape:
            raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must both be [B,H,W] or [B,H,W,1]")
        B, H, W = pred.shape[:3]
        if B * H * W == 0:
            raise ValueError("no pixels")
        if mask.numel() != B * H * W:
            raise ValueError(f"mask {tuple(mask.shape)} does not match [B,H,W] = {(B, H, W)}")
        p, g, m = f32c(pred), f32c(gt), f32c(mask).reshape(B, H, W)
        scratch, words = _scratch(B * H * W, 2, p.device)
        out = torch.empty(8, device=p.device, dtype=torch.float32)
        stream = stream_of(p)
        L.check(L.lib().d4gs_gradient_loss_fwd(vp(p), vp(g), vp(m), B, H, W, quantile, vp(scratch), words, vp(out), stream),
                "d4gs_gradient_loss_fwd")
        ctx.keep = (p, g, m, scratch, out)
        ctx.args = (B, H, W, pred.shape, pred.dtype)
        return out[0].clone()

    @staticmethod
    def backward(ctx, v_loss):
        p, g, m, scratch, out = ctx.keep
        B, H, W, shape, dtype = ctx.args
        v = v_loss.detach().float().reshape(1).contiguous()
        v_pred = torch.empty_like(p)
        stream = stream_of(p)
        L.check(L.lib().d4gs_gradient_loss_bwd(vp(p), vp(g), vp(m), vp(scratch), vp(out), vp(v), B, H, W, vp(v_pred), stream),
                "d4gs_gradient_loss_bwd")
        return v_pred.reshape(shape).to(dtype), None, None, None


def masked_l1_loss(pred, gt, mask=None, normalize=True, quantile: float = 1.0):
    """flow3d/loss_utils.py:26-42.  Elements v = |pred - gt|.mean(-1); with quantile < 1 only those strictly below
    torch.quantile(v, quantile) - taken over ALL elements, masked-out ones included - are kept.  `mask` (float or bool, shaped
    like v, with or without a trailing 1) weighs them: sum(v m) / (sum(m) + 1e-8) over the kept ones, or sum(v m) / #kept with
    normalize=False.  mask=None is `trimmed_l1_loss(pred, gt, quantile)`, as in the reference."""
    if mask is None:
        return trimmed_l1_loss(pred, gt, quantile)
    return _TrimmedL1Fn.apply(pred, gt, mask, bool(normalize), _check_quantile(quantile, upper_open=True))


def trimmed_l1_loss(pred, gt, quantile=0.9):
    """flow3d/loss_utils.py:64-68: the mean of the elements strictly below torch.quantile(v, quantile).  The quantile is always
    taken (quantile=1: the maximum, whose tie group is dropped); an empty kept set is NaN, as torch's mean of nothing."""
    return _TrimmedL1Fn.apply(pred, gt, None, False, _check_quantile(quantile, upper_open=False))


def compute_gradient_loss(pred, gt, mask, quantile=0.98):
    """flow3d/loss_utils.py:71-90.  pred, gt [B,H,W] or [B,H,W,1]; mask [B,H,W] or [B,H,W,1], bool or float.  The trimmed mean of
    |dx pred - dx gt| over horizontally adjacent pixels that are both inside the mask, plus the same vertically.  Deviation: a
    term without any valid pair is NaN here, where the reference raises (torch.quantile of an empty tensor) - raising would need
    the count on the host."""
    return _GradientLossFn.apply(pred, gt, mask, _check_quantile(quantile, upper_open=False))


class _TrackLossesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tracks_3d, pix, rows, vis, weights, tgt_2d, tgt_depth, Ks, quantile):
        n_pixels, N = tracks_3d.numel() // (3 * tracks_3d.shape[-2]), tracks_3d.shape[-2]
        t = f32c(tracks_3d)
        n = pix.numel()
        scratch, words = _scratch(n, 2, t.device)
        out = torch.empty(8, device=t.device, dtype=torch.float32)
        stream = stream_of(t)
        L.check(L.lib().d4gs_track_losses_fwd(vp(t), vp(pix), vp(rows), vp(vis), vp(weights), vp(tgt_2d), vp(tgt_depth), vp(Ks), n_pixels, N,
                                              Ks.shape[0], n, quantile, vp(scratch), words, vp(out), stream), "d4gs_track_losses_fwd")
        ctx.keep = (t, pix, rows, vis, weights, tgt_2d, tgt_depth, Ks, scratch, out)
        ctx.args = (n_pixels, N, n, quantile, tracks_3d.shape, tracks_3d.dtype)
        return out[5].clone(), out[6].clone()

    @staticmethod
    def backward(ctx, v_2d, v_depth):
        t, pix, rows, vis, weights, tgt_2d, tgt_depth, Ks, scratch, out = ctx.keep
        n_pixels, N, n, quantile, shape, dtype = ctx.args
        v = torch.stack([v_2d.detach().float().reshape(()), v_depth.detach().float().reshape(())])
        v_tracks = torch.empty_like(t)  # zeroed by the entry point, on the stream
        stream = stream_of(t)
        L.check(L.lib().d4gs_track_losses_bwd(vp(t), vp(pix), vp(rows), vp(vis), vp(weights), vp(tgt_2d), vp(tgt_depth), vp(Ks), vp(scratch),
                                              vp(out), vp(v), n_pixels, N, Ks.shape[0], n, quantile, vp(v_tracks), stream),
                "d4gs_track_losses_bwd")
        return (v_tracks.reshape(shape).to(dtype),) + (None,) * 8


def _per_batch(x, B, name):
    if torch.is_tensor(x):
        x = [x]
    if len(x) != B:
        raise ValueError(f"{name}: {len(x)} batch entries for tracks_3d of batch {B}")
    return list(x)


def track_losses(tracks_3d, query_tracks_2d, target_Ks, target_tracks_2d, target_visibles, track_weights, target_track_depths,
                 quantile: float = 0.98):
    """-> (track_2d_loss, mapped_depth_loss) of flow3d/trainer.py:633-667,681-689.

    tracks_3d [B,H,W,N,3]: the dynamic render's track points in the N target cameras' frames (`SceneModel.render`, B = 1 there).
    The batch entries of the reference, each a list of B tensors (or one tensor for B = 1): query_tracks_2d [P_b,2] (x, y),
    target_Ks [N,3,3], target_tracks_2d [N,P_b,2], target_visibles [N,P_b] bool, target_track_depths [N,P_b]; P_b may differ
    between entries.  An element is (b, n, p) in that order, sum_b N P_b of them.  track_weights: one weight per element, shaped
    [n], [n,1] or [n,M]; a trailing axis is summed, which is what the reference's masked_l1_loss makes of its [P_all, B N] product
    `confidences[..., None] * w_interval`.

    Per visible element: X = tracks_3d[b, int(y_p), int(x_p), n], P = K[b,n] X, z = max(P_z, 1e-6), xy = P_xy / z;
      track_2d_loss     = masked_l1_loss(xy, target 2-D, weights, quantile=quantile) over the visible elements - WITHOUT the
                          reference's `/ max(H, W)`: the caller divides, as the trainer does
      mapped_depth_loss = masked_l1_loss(1 / (z + 1e-5), 1 / (target depth + 1e-5), weights) over the same (quantile 1: all kept)
    Differentiable w.r.t. tracks_3d only.  Nothing is read on the host: the element tables are built with torch ops, the visible
    count is formed on the device, so the call can sit inside a captured HIP graph.

    Deviations from the reference:
      pairing - the reference pairs the i-th pixel of the queries' image mask in raster order with the i-th query; here query p
        is paired with its own pixel.  The two agree exactly when a frame's queries are distinct and in raster order; otherwise
        the reference raises or mispairs.
      no visible element - the 2-D term is NaN (with quantile >= 1: 0) and the depth term 0, where the reference raises
        (torch.quantile of nothing); raising would need the count on the host.  Same as compute_gradient_loss.
      a query outside the image - its elements are treated as not visible (the reference's indexing faults or wraps); no address
        is formed from such a pixel.
    The gradient is scattered with float atomicAdd onto a zeroed image because queries of one row may share a pixel.  With distinct
    pixels per row every address receives exactly one add onto zero, so the result is bitwise reproducible."""
    q = _check_quantile(quantile, upper_open=True)
    if not torch.is_tensor(tracks_3d) or tracks_3d.dim() != 5 or tracks_3d.shape[-1] != 3:
        raise ValueError("tracks_3d must be a [B,H,W,N,3] tensor")
    need_gpu(tracks_3d, _WHO)
    B, H, W, N, _ = tracks_3d.shape
    if B * H * W * N == 0:
        raise ValueError(f"tracks_3d {tuple(tracks_3d.shape)} is empty")
    queries, Ks = _per_batch(query_tracks_2d, B, "query_tracks_2d"), _per_batch(target_Ks, B, "target_Ks")
    tgt2d, visibles = _per_batch(target_tracks_2d, B, "target_tracks_2d"), _per_batch(target_visibles, B, "target_visibles")
    depths = _per_batch(target_track_depths, B, "target_track_depths")
    dev = tracks_3d.device
    pix, rows = [], []
    for b in range(B):
        if queries[b].dim() != 2 or queries[b].shape[1] != 2:
            raise ValueError(f"query_tracks_2d[{b}] {tuple(queries[b].shape)} must be [P,2]")
        P = queries[b].shape[0]
        for name, x, want in (("target_Ks", Ks[b], (N, 3, 3)), ("target_tracks_2d", tgt2d[b], (N, P, 2)),
                              ("target_visibles", visibles[b], (N, P)), ("target_track_depths", depths[b], (N, P))):
            if tuple(x.shape) != want:
                raise ValueError(f"{name}[{b}] {tuple(x.shape)} must be {want} (N = {N} target frames, {P} queries)")
        for x in (queries[b], Ks[b], tgt2d[b], visibles[b], depths[b]):
            need_gpu(x, _WHO)
        xy = queries[b].detach().to(torch.int64)  # truncated, as the reference's query_pixels
        x, y = xy[:, 0], xy[:, 1]
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        flat = torch.where(inside, (b * H + y) * W + x, torch.full_like(x, -1)).to(torch.int32)
        pix.append(flat[None].expand(N, P).reshape(-1))
        rows.append((b * N + torch.arange(N, device=dev, dtype=torch.int32))[:, None].expand(N, P).reshape(-1))
    pix, rows = torch.cat(pix).contiguous(), torch.cat(rows).contiguous()
    n = pix.numel()
    if n == 0:
        raise ValueError("no query tracks")
    w = track_weights
    if not torch.is_tensor(w) or w.dim() not in (1, 2) or w.shape[0] != n:
        raise ValueError(f"track_weights {tuple(w.shape) if torch.is_tensor(w) else type(w)} must be [{n}], [{n},1] or [{n},M]: one row per "
                         "(batch entry, target frame, query)")
    need_gpu(w, _WHO)
    w = f32c(w)
    if w.dim() == 2:
        w = w.sum(-1)
    vis = torch.cat([v.detach().reshape(-1) != 0 for v in visibles]).to(torch.uint8).contiguous()
    return _TrackLossesFn.apply(tracks_3d, pix, rows, vis, w.contiguous(), f32c(torch.cat([t.reshape(-1, 2) for t in tgt2d])),
                                f32c(torch.cat([d.reshape(-1) for d in depths])), f32c(torch.cat(Ks).reshape(-1, 9)), q)


_TABLE_DTYPES = (("pix", torch.int32), ("rows", torch.int32), ("vis", torch.uint8), ("weights", torch.float32), ("tgt_2d", torch.float32),
                 ("tgt_depth", torch.float32), ("Ks", torch.float32))


def track_losses_from_tables(tracks_3d, tables, quantile: float = 0.98):
    """`track_losses` for a caller that already holds the element tables - `feed.DeviceClip.batch(...)["track_tables"]` - so that no
    torch op shapes them per step.  tracks_3d [1,H,W,N,3]; tables: a dict of contiguous device tensors over n elements (n, p), n = N P:
    pix int32 [n] (the query's pixel y W + x, -1: none), rows int32 [n] (the target n), vis uint8 [n], weights fp32 [n] (already
    summed over the trailing axis), tgt_2d fp32 [n,2], tgt_depth fp32 [n], Ks fp32 [N,9].  An element with vis = 0 or pix = -1 (a
    padding row, a query outside the image) takes no part.  Same values, gradient and deviations as `track_losses`."""
    q = _check_quantile(quantile, upper_open=True)
    if not torch.is_tensor(tracks_3d) or tracks_3d.dim() != 5 or tracks_3d.shape[-1] != 3 or tracks_3d.shape[0] != 1:
        raise ValueError("tracks_3d must be a [1,H,W,N,3] tensor")
    need_gpu(tracks_3d, _WHO)
    N = tracks_3d.shape[3]
    if tracks_3d.numel() == 0:
        raise ValueError(f"tracks_3d {tuple(tracks_3d.shape)} is empty")
    n = tables["pix"].numel()
    for name, dtype in _TABLE_DTYPES:
        x = tables[name]
        need_gpu(x, _WHO)
        want = {"tgt_2d": (n, 2), "Ks": (N, 9)}.get(name, (n,))
        if x.dtype != dtype or tuple(x.shape) != want or not x.is_contiguous():
            raise ValueError(f"tables[{name!r}] must be a contiguous {dtype} tensor {want}, got {x.dtype} {tuple(x.shape)}")
    if n == 0:
        raise ValueError("no query tracks")
    return _TrackLossesFn.apply(tracks_3d, *(tables[name] for name, _ in _TABLE_DTYPES), q)


class _MotionRegsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, motion_coefs, rots, transls, scales, ts, w2cs, weight_rot, weight_transl):
        G, K, T, B = means.shape[0], rots.shape[0], rots.shape[1], ts.shape[0]
        leaves = tuple(f32c(x) for x in (means, motion_coefs, scales, rots, transls))
        t, w = f32c(ts), f32c(w2cs)
        lib = L.lib()
        nbytes = lib.d4gs_motion_regs_workspace_bytes(G, K, T, B)
        if nbytes == 0:
            raise RuntimeError(f"motion_regularizers: unsupported size G={G} K={K} T={T} B={B} (K <= 32, 9 B G <= 2^31 - 1)")
        ws = torch.empty(nbytes, device=means.device, dtype=torch.uint8)
        out = torch.empty(4, device=means.device, dtype=torch.float32)
        stream = stream_of(means)
        L.check(lib.d4gs_motion_regs_fwd(*[vp(x) for x in leaves], vp(t), vp(w), G, K, T, B, weight_rot, weight_transl, vp(ws), nbytes,
                                         vp(out), stream), "d4gs_motion_regs_fwd")
        ctx.save_for_backward(*leaves, ws)  # version-checked: a leaf changed in place before the backward raises
        ctx.args = (G, K, T, B, weight_rot, weight_transl, nbytes, tuple(x.dtype for x in (means, motion_coefs, rots, transls, scales)))
        return out[0].clone(), out[1].clone(), out[2].clone(), out[3].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, v_sb, v_st, v_za, v_sv):
        means, coefs, scales, rots, transls, ws = ctx.saved_tensors
        G, K, T, B, weight_rot, weight_transl, nbytes, dtypes = ctx.args
        v = torch.stack([x.detach().float().reshape(()) for x in (v_sb, v_st, v_za, v_sv)])
        g = dict(v_means=torch.empty_like(means), v_motion_coefs=torch.empty_like(coefs), v_scales=torch.empty_like(scales),
                 v_rots=torch.empty_like(rots), v_transls=torch.empty_like(transls))
        stream = stream_of(means)
        L.check(L.lib().d4gs_motion_regs_bwd(vp(means), vp(coefs), vp(scales), vp(rots), vp(transls), G, K, T, B, weight_rot, weight_transl,
                                             vp(ws), nbytes, vp(v), C.byref(L.fill(L.LeafGrads(), **g)), stream), "d4gs_motion_regs_bwd")
        outs = (g["v_means"], g["v_motion_coefs"], g["v_rots"], g["v_transls"], g["v_scales"])
        return tuple(o.to(dt) if need else None for o, dt, need in zip(outs, dtypes, ctx.needs_input_grad[:5])) + (None,) * 4


def motion_regularizers(means, motion_coefs, rots, transls, scales, ts, w2cs, *, weight_rot: float = 1.0, weight_transl: float = 2.0):
    """-> (smooth_bases, smooth_tracks, z_accel, scale_var), four 0-dim tensors: the regularizers of flow3d/trainer.py:691-728.

    means [G,3], raw motion_coefs [G,K] and raw scales [G,3] of the foreground, rots [K,T,6], transls [K,T,3], ts [B] frame indices
    (any real dtype), w2cs [B,4,4].  With tc = clamp(ts, 1, T-2) and m0, m1, m2 [G,B,3] the deformed means at tc-1, tc, tc+1:
      smooth_bases  = compute_se3_smoothness_loss(rots, transls, weight_rot, weight_transl)     (loss_utils.py:138-157)
      smooth_tracks = 0.5 * |2 m1 - m0 - m2|.mean()                                             (trainer.py:699-717)
      z_accel       = compute_z_acc_loss(stack(m0, m1, m2), w2cs)                               (loss_utils.py:118-135)
      scale_var     = torch.var(scales, dim=-1).mean()                                          (trainer.py:721-724)
    unweighted: the caller applies w_smooth_bases 0.1, w_smooth_tracks 2, w_z_accel 1, w_scale_var 0.01.  Gradients flow to means,
    motion_coefs, rots, transls and scales (those that require one), none to ts or w2cs, which are data in the reference too.  The
    gradient of a norm that is exactly zero is zero, as torch's.  Nothing is read on the host (the neighbour times and the camera
    centres - a cofactor inverse instead of torch.linalg.inv, whose error check waits for the device - are formed on the device), so
    the call can sit inside a captured HIP graph; forward and backward are bitwise reproducible.  T < 3 has no interior frame (the
    reference's mean over nothing is NaN) and is refused."""
    # (name, tensor, number of leading free axes, fixed trailing axes)
    for name, x, lead, tail in (("means", means, 1, (3,)), ("motion_coefs", motion_coefs, 2, ()), ("rots", rots, 2, (6,)),
                                ("transls", transls, 2, (3,)), ("scales", scales, 1, (3,)), ("ts", ts, 1, ()), ("w2cs", w2cs, 1, (4, 4))):
        if not torch.is_tensor(x) or x.dim() != lead + len(tail) or tuple(x.shape[lead:]) != tail:
            raise ValueError(f"{name} {tuple(x.shape) if torch.is_tensor(x) else type(x)}: expected "
                             "means [G,3], motion_coefs [G,K], rots [K,T,6], transls [K,T,3], scales [G,3], ts [B], w2cs [B,4,4]")
    G, K, T, B = means.shape[0], rots.shape[0], rots.shape[1], ts.shape[0]
    if G == 0:
        raise ValueError("no foreground Gaussians (G == 0)")
    if motion_coefs.shape != (G, K) or scales.shape[0] != G or transls.shape[:2] != (K, T):
        raise ValueError(f"mismatched sizes: means {tuple(means.shape)}, motion_coefs {tuple(motion_coefs.shape)}, scales {tuple(scales.shape)}, "
                         f"rots {tuple(rots.shape)}, transls {tuple(transls.shape)} (G Gaussians, K bases, T frames)")
    if K == 0:
        raise ValueError("no motion bases (K == 0)")
    if T < 3:
        raise ValueError(f"T = {T} frames: the regularizers need an interior frame (T >= 3)")
    if B == 0 or w2cs.shape[0] != B:
        raise ValueError(f"{B} times and {w2cs.shape[0]} cameras: one w2c per entry of ts, at least one")
    for x in (means, motion_coefs, rots, transls, scales, ts, w2cs):
        need_gpu(x, _WHO)
    return _MotionRegsFn.apply(means, motion_coefs, rots, transls, scales, ts, w2cs, float(weight_rot), float(weight_transl))


def scene_motion_regularizers(model, ts, w2cs, **kw):
    """`motion_regularizers` on a SceneModel's own leaves: fg.params["means" | "motion_coefs" | "scales"] and
    motion_bases.params["rots" | "transls"].  The trainer's block becomes
        sb, st, za, sv = scene_motion_regularizers(self.model, ts, w2cs)
        loss += w_smooth_bases * sb + w_smooth_tracks * st + w_z_accel * za + w_scale_var * sv"""
    fg, mb = model.fg.params, model.motion_bases.params
    return motion_regularizers(fg["means"], fg["motion_coefs"], mb["rots"], mb["transls"], fg["scales"], ts, w2cs, **kw)


class _TrackFitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, motion_coefs, rots, transls, targets, quantile):
        G, K, T = means.shape[0], rots.shape[0], rots.shape[1]
        leaves = tuple(f32c(x) for x in (means, motion_coefs, rots, transls))
        lib = L.lib()
        nbytes = lib.d4gs_track_fit_workspace_bytes(G, K, T)
        if nbytes == 0:
            raise RuntimeError(f"track_fit_losses: unsupported size G={G} K={K} T={T} (K <= 32, 3 <= T <= 65535, 9 G T <= 2^31 - 1)")
        ws = torch.empty(nbytes, device=means.device, dtype=torch.uint8)
        out = torch.empty(8, device=means.device, dtype=torch.float32)
        L.check(lib.d4gs_track_fit_fwd(*[vp(x) for x in leaves], G, K, T, quantile, None, vp(targets.buf), targets.nbytes, vp(ws), nbytes,
                                       vp(out), None, None, 0, stream_of(means)), "d4gs_track_fit_fwd")
        ctx.save_for_backward(*leaves, ws)  # version-checked: a leaf changed in place before the backward raises
        ctx.targets = targets
        ctx.args = (G, K, T, quantile, nbytes, tuple(x.dtype for x in (means, motion_coefs, rots, transls)))
        return out[1:7].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, v_terms):
        means, coefs, rots, transls, ws = ctx.saved_tensors
        G, K, T, quantile, nbytes, dtypes = ctx.args
        v = v_terms.detach().float().contiguous()
        g = dict(v_means=torch.empty_like(means), v_motion_coefs=torch.empty_like(coefs), v_rots=torch.empty_like(rots),
                 v_transls=torch.empty_like(transls))
        L.check(L.lib().d4gs_track_fit_bwd(vp(means), vp(coefs), vp(rots), vp(transls), G, K, T, quantile, vp(ctx.targets.buf),
                                           ctx.targets.nbytes, vp(ws), nbytes, vp(v), C.byref(L.fill(L.LeafGrads(), **g)), stream_of(means)),
                "d4gs_track_fit_bwd")
        outs = (g["v_means"], g["v_motion_coefs"], g["v_rots"], g["v_transls"])
        return tuple(o.to(dt) if need else None for o, dt, need in zip(outs, dtypes, ctx.needs_input_grad[:4])) + (None, None)


def track_fit_losses(means, motion_coefs, rots, transls, targets, quantile: float = 0.95):
    """-> [6]: track_3d, track_2d, coef_sparse, smooth_bases, smooth_tracks, z_accel of the reference's warm-up loop body
    (flow3d/init_utils.py:320-388), unweighted; the loop weighs them 1, 0.5, 0.01, w(i), 0.5 w(i), 0.1.

    means [G,3], raw motion_coefs [G,K], rots [K,T,6], transls [K,T,3]; `targets` = `scene_init.track_fit_targets(tracks_3d, Ks, w2cs)`,
    the prepared observations of the same G tracks and T frames.  With p[g,tau] the deformed mean at the integer frame tau:
      track_3d      = masked_l1_loss(p, xyz, visibles * confidences)
      track_2d      = masked_l1_loss(proj(p), proj(xyz), invisibles * confidences, quantile=quantile) / Ks[0,0,0]
      coef_sparse   = 1 - (softmax(motion_coefs) ** 2).sum(-1).mean()
      smooth_bases  = compute_se3_smoothness_loss(rots, transls)
      smooth_tracks = compute_accel_loss(p)                  (the mean over G (T - 2) norms: not `motion_regularizers`' 0.5 factor)
      z_accel       = compute_z_acc_loss(p at clamp(b, 1, T-2) + {-1, 0, 1}, w2cs), b = 0 .. T-1
    Every p is computed once (a composition of `motion_regularizers` with ts = arange(T) deforms each Gaussian at 3 T times).  Gradients
    flow to the four leaves; the observations are data.  The gradient of |x| at 0 and of a norm at exactly zero is zero; none flows
    through the quantile.  Nothing is read on the host, so the call can sit inside a captured HIP graph; forward and backward are
    bitwise reproducible.  T < 3 is refused (the reference's mean over nothing is NaN)."""
    q = _check_quantile(quantile, upper_open=True)
    for name, x, lead, tail in (("means", means, 1, (3,)), ("motion_coefs", motion_coefs, 2, ()), ("rots", rots, 2, (6,)),
                                ("transls", transls, 2, (3,))):
        if not torch.is_tensor(x) or x.dim() != lead + len(tail) or tuple(x.shape[lead:]) != tail:
            raise ValueError(f"{name} {tuple(x.shape) if torch.is_tensor(x) else type(x)}: expected "
                             "means [G,3], motion_coefs [G,K], rots [K,T,6], transls [K,T,3]")
    G, K, T = means.shape[0], rots.shape[0], rots.shape[1]
    if G == 0 or K == 0:
        raise ValueError(f"no foreground Gaussians or no motion bases (G = {G}, K = {K})")
    if motion_coefs.shape != (G, K) or transls.shape[:2] != (K, T):
        raise ValueError(f"mismatched sizes: means {tuple(means.shape)}, motion_coefs {tuple(motion_coefs.shape)}, rots {tuple(rots.shape)}, "
                         f"transls {tuple(transls.shape)} (G Gaussians, K bases, T frames)")
    if T < 3:
        raise ValueError(f"T = {T} frames: the fit needs an interior frame (T >= 3)")
    if (getattr(targets, "G", None), getattr(targets, "T", None)) != (G, T):
        raise ValueError(f"targets of G = {getattr(targets, 'G', None)}, T = {getattr(targets, 'T', None)} for leaves of G = {G}, T = {T} "
                         "(scene_init.track_fit_targets of the same tracks and frames)")
    for x in (means, motion_coefs, rots, transls):
        need_gpu(x, _WHO)
    return _TrackFitFn.apply(means, motion_coefs, rots, transls, targets, q)


def _mask_bhw(masks, name="masks"):
    """-> (B, H, W) of a [B,H,W] or [B,H,W,1] tensor."""
    if not torch.is_tensor(masks) or masks.dim() not in (3, 4) or (masks.dim() == 4 and masks.shape[-1] != 1) or masks.numel() == 0:
        raise ValueError(f"{name} {tuple(masks.shape) if torch.is_tensor(masks) else type(masks)}: expected a non-empty [B,H,W] or [B,H,W,1]")
    return tuple(masks.shape[:3])


def dilate_mask(masks, kernel_size: int = 9, return_complement: bool = False):
    """`nn.MaxPool2d(kernel_size, stride=1, padding=kernel_size // 2)` on a [B,H,W] or [B,H,W,1] mask (flow3d/trainer.py:120): every
    pixel becomes the maximum of its kernel_size x kernel_size window clipped to the image, bit for bit.  -> fp32, shaped like
    `masks`; with return_complement also `1 - dilated` from the same pass, the mask of the static depth losses (trainer.py:397,413).
    Masks are data: the result carries no gradient.  An even kernel_size has no centre and raises ValueError."""
    k = int(kernel_size)
    if k != kernel_size or k < 1 or k % 2 == 0:
        raise ValueError(f"kernel_size={kernel_size}: must be a positive odd integer")
    B, H, W = _mask_bhw(masks)
    need_gpu(masks, _WHO)
    m = f32c(masks)
    out = torch.empty_like(m)
    comp = torch.empty_like(m) if return_complement else None
    L.check(L.lib().d4gs_dilate_mask(vp(m), B, H, W, k // 2, vp(out), vp(comp), stream_of(m)), "d4gs_dilate_mask")
    return (out, comp) if return_complement else out


class _SharpKeepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask, reduced, factor):
        B, H, W, Cc = pred.shape
        p, t, m = f32c(pred), f32c(target), f32c(mask).reshape(B, H, W)
        lib = L.lib()
        dims = (B, H, W, Cc, factor)
        n_map, nb = lib.d4gs_area_keep_map_elems(*dims), lib.d4gs_area_keep_blocks(*dims)
        if n_map == 0:
            raise RuntimeError(f"sharp_keep_loss: unsupported size {tuple(pred.shape)} (H, W <= 32768, at most 2^31 - 1 elements)")
        gmap = torch.empty(n_map, device=p.device, dtype=torch.float32)
        partials = torch.empty(nb, device=p.device, dtype=torch.float64)
        out = torch.empty(1, device=p.device, dtype=torch.float32)
        stream = stream_of(p)
        L.check(lib.d4gs_area_keep_fwd(vp(p), vp(m), vp(t), int(reduced), *dims, vp(gmap), vp(partials), vp(out), stream), "d4gs_area_keep_fwd")
        ctx.save_for_backward(gmap)
        ctx.args = (dims, pred.dtype)
        return out.reshape(())  # (nothing else holds `out`: no clone)

    @staticmethod
    @once_differentiable
    def backward(ctx, v_loss):
        gmap, = ctx.saved_tensors
        (B, H, W, Cc, factor), dtype = ctx.args
        v = v_loss.detach().float().reshape(1).contiguous()
        v_pred = torch.empty(B, H, W, Cc, device=gmap.device, dtype=torch.float32)
        stream = stream_of(gmap)
        L.check(L.lib().d4gs_area_keep_bwd(vp(gmap), vp(v), B, H, W, Cc, factor, vp(v_pred), stream), "d4gs_area_keep_bwd")
        return v_pred.to(dtype), None, None, None, None


def sharp_keep_loss(pred_sharp, target, masks, factor: int = 4):
    """The reference's `loss_keep` (flow3d/trainer.py:736-760): `F.l1_loss(area(pred_sharp) * area(masks), area(target) * area(masks))`
    with area(x) = `F.interpolate(x, scale_factor=1 / factor, mode="area")`.  pred_sharp [B,H,W,C] channel-last, masks [B,H,W] or
    [B,H,W,1]; target is the full-size [B,H,W,C] image (the `batch4 is None` branch) or the already reduced [B,H//factor,W//factor,C]
    one (the other branch), told apart by shape; with factor == 1 the two coincide and the target is used as it is.  factor is 1, 2,
    4 or 8; H < factor or W < factor (torch: an empty tensor and a NaN loss) raises ValueError.  Differentiable w.r.t. pred_sharp
    only; sign(0) = 0 as in `F.l1_loss`."""
    if factor not in (1, 2, 4, 8):
        raise ValueError(f"factor={factor}: must be 1, 2, 4 or 8")
    if not torch.is_tensor(pred_sharp) or pred_sharp.dim() != 4 or pred_sharp.numel() == 0:
        raise ValueError(f"pred_sharp {tuple(pred_sharp.shape) if torch.is_tensor(pred_sharp) else type(pred_sharp)}: expected a non-empty [B,H,W,C]")
    B, H, W, Cc = pred_sharp.shape
    if _mask_bhw(masks) != (B, H, W):
        raise ValueError(f"masks {tuple(masks.shape)} does not match pred_sharp {tuple(pred_sharp.shape)}")
    if H < factor or W < factor:
        raise ValueError(f"H={H}, W={W} below factor={factor}: the reduced image is empty")
    if not torch.is_tensor(target) or tuple(target.shape) not in ((B, H, W, Cc), (B, H // factor, W // factor, Cc)):
        raise ValueError(f"target {tuple(target.shape) if torch.is_tensor(target) else type(target)}: expected {(B, H, W, Cc)} or the reduced "
                         f"{(B, H // factor, W // factor, Cc)}")
    for x in (pred_sharp, target, masks):
        need_gpu(x, _WHO)
    reduced = tuple(target.shape) == (B, H // factor, W // factor, Cc)  # (factor == 1: both; a 1 x 1 window's mean is the value)
    return _SharpKeepFn.apply(pred_sharp, target, masks, reduced, int(factor))


class _CoverageFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acc, target):
        a = f32c(acc)
        t = None if target is None else f32c(target)
        n = a.numel()
        lib = L.lib()
        nb = lib.d4gs_mse_blocks(n)
        if nb == 0:
            raise RuntimeError(f"coverage_loss: {n} elements (at most 2^31 - 1)")
        partials = torch.empty(nb, device=a.device, dtype=torch.float64)
        out = torch.empty(1, device=a.device, dtype=torch.float32)
        L.check(lib.d4gs_mse_fwd(vp(a), vp(t), n, vp(partials), vp(out), stream_of(a)), "d4gs_mse_fwd")
        ctx.save_for_backward(a, *(() if t is None else (t,)))
        ctx.dtype = acc.dtype
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, v_loss):
        a, *rest = ctx.saved_tensors
        t = rest[0] if rest else None
        v = v_loss.detach().float().reshape(1).contiguous()
        v_acc = torch.empty_like(a)
        L.check(L.lib().d4gs_mse_bwd(vp(a), vp(t), vp(v), a.numel(), vp(v_acc), stream_of(a)), "d4gs_mse_bwd")
        return v_acc.to(ctx.dtype), None


def coverage_loss(acc, target=None):
    """`F.mse_loss(acc, target)` on the accumulated alpha (flow3d/trainer.py:621-631).  acc [B,H,W,1] or [B,H,W]; target=None is the
    all-ones target of a scene with a background model, otherwise `masks[..., None]` (any tensor with acc's number of elements).
    Differentiable w.r.t. acc only; the gradient is exactly 0 where acc == target."""
    if not torch.is_tensor(acc) or acc.dim() not in (3, 4) or (acc.dim() == 4 and acc.shape[-1] != 1) or acc.numel() == 0:
        raise ValueError(f"acc {tuple(acc.shape) if torch.is_tensor(acc) else type(acc)}: expected a non-empty [B,H,W] or [B,H,W,1]")
    if target is not None and (not torch.is_tensor(target) or _mask_bhw(target, "target") != tuple(acc.shape[:3])):
        raise ValueError(f"target {tuple(target.shape)} does not match acc {tuple(acc.shape)}")
    for x in (acc,) if target is None else (acc, target):
        need_gpu(x, _WHO)
    return _CoverageFn.apply(acc, target)
