"""fp64 reference of gsplat's `absgrad` (`rasterization(absgrad=True)`, `info["means2d"].absgrad`):

    absgrad[g] = sum over pixels p of ( |dL_p/dx_g|, |dL_p/dy_g| ),

where L_p is pixel p's share of the loss: <v_colors[p], render_colors[p]> + v_alphas[p] * render_alphas[p], background and the
RGB+ED division included.  The per-tile composite restates oracle/raster.py::rasterize_to_pixels, except that every pixel
reads its OWN copy of each splat's centre: those copies [P, n, 2] are the differentiated leaf, so autograd returns the per-pixel
terms, which are made absolute and then summed over the pixels.  Without the abs the same sum is the oracle's means2d.grad.
The tile lists come from oracle.raster.isect_tiles."""
import math

import torch

from oracle import raster

TILE = raster.TILE


def absgrad_of_composite(means2d, conics, colors, opacities, width, height, flatten_ids, isect_offsets, v_colors, v_alphas=None,
                         background=None, ed=False):
    """means2d [N,2], conics [N,3], colors [N,D'] (the depth channel last when rendered), opacities [N] - detached, fp64;
    v_colors [H,W,D'] (the gradient of the returned image, i.e. of the DIVIDED depth channel when `ed`), v_alphas [H,W(,1)] or None,
    background [D'] or None (the depth channel's entry 0).  -> (absgrad [N,2], signed sum [N,2])."""
    dt, dev = torch.float64, means2d.device
    means2d, conics, colors, opacities = (x.detach().to(dt) for x in (means2d, conics, colors, opacities))
    v_colors = v_colors.detach().to(dt)
    v_alphas = None if v_alphas is None else v_alphas.detach().to(dt).reshape(height, width)
    bg = None if background is None else background.detach().to(dt)
    N = means2d.shape[0]
    absg = torch.zeros(N, 2, dtype=dt, device=dev)
    sgn = torch.zeros(N, 2, dtype=dt, device=dev)
    tile_w, tile_h = math.ceil(width / TILE), math.ceil(height / TILE)
    offs = isect_offsets.tolist()
    for ty in range(tile_h):
        ys0, ys1 = ty * TILE, min((ty + 1) * TILE, height)
        for tx in range(tile_w):
            t = ty * tile_w + tx
            s, e = offs[t], offs[t + 1]
            if e <= s:
                continue
            xs0, xs1 = tx * TILE, min((tx + 1) * TILE, width)
            g = flatten_ids[s:e]
            py, px = torch.meshgrid(torch.arange(ys0, ys1, device=dev, dtype=dt) + 0.5,
                                    torch.arange(xs0, xs1, device=dev, dtype=dt) + 0.5, indexing="ij")
            P = px.numel()
            m = means2d[g][None].expand(P, -1, -1).clone().requires_grad_()  # [P,n,2]: one copy per pixel
            dx = m[..., 0] - px.reshape(-1, 1)
            dy = m[..., 1] - py.reshape(-1, 1)
            cn = conics[g]
            sigma = 0.5 * (cn[:, 0] * dx * dx + cn[:, 2] * dy * dy) + cn[:, 1] * dx * dy
            alpha = torch.clamp(opacities[g][None, :] * torch.exp(-sigma), max=raster.ALPHA_MAX)
            with torch.no_grad():
                skip = (sigma < 0) | (alpha < raster.ALPHA_MIN)
            alpha = torch.where(skip, torch.zeros_like(alpha), alpha)
            T_after = torch.cumprod(1.0 - alpha, dim=1)
            T_before = torch.cat([torch.ones_like(T_after[:, :1]), T_after[:, :-1]], dim=1)
            with torch.no_grad():
                live = (T_after > raster.T_STOP) & ~skip
                alive_any = T_after > raster.T_STOP
            w = torch.where(live, alpha * T_before, torch.zeros_like(alpha))
            col = w @ colors[g]  # [P,D']
            Tf = torch.prod(torch.where(alive_any, 1.0 - alpha, torch.ones_like(alpha)), dim=1)
            if bg is not None:
                col = col + Tf[:, None] * bg
            acc = 1.0 - Tf
            if ed:
                col = torch.cat([col[:, :-1], col[:, -1:] / acc.clamp(min=1e-10)[:, None]], dim=1)
            loss = (col * v_colors[ys0:ys1, xs0:xs1].reshape(P, -1)).sum()
            if v_alphas is not None:
                loss = loss + (acc * v_alphas[ys0:ys1, xs0:xs1].reshape(P)).sum()
            (gm,) = torch.autograd.grad(loss, m, allow_unused=True)
            if gm is None:
                continue
            absg.index_add_(0, g, gm.abs().sum(0))
            sgn.index_add_(0, g, gm.sum(0))
    return absg, sgn


def absgrad_of_rasterization(means, quats, scales, opacities, colors, viewmat, K, width, height, v_colors, v_alphas=None,
                             background=None, render_mode="RGB"):
    """The oracle's projection + tile lists, then `absgrad_of_composite`.  -> (absgrad [N,2], signed [N,2], oracle info)."""
    assert render_mode in ("RGB", "RGB+D", "RGB+ED")
    with torch.no_grad():
        radii, means2d, depths, conics = raster.project(means, quats, scales, viewmat, K, width, height)
        cols = colors
        bg = background
        if render_mode != "RGB":
            cols = torch.cat([colors, depths[:, None]], dim=-1)
            if bg is not None:
                bg = torch.cat([bg, torch.zeros_like(bg[:1])], dim=-1)
        _, flatten_ids, isect_offsets = raster.isect_tiles(means2d, radii, depths, width, height)
    absg, sgn = absgrad_of_composite(means2d, conics, cols, opacities, width, height, flatten_ids, isect_offsets, v_colors,
                                     v_alphas, bg, ed=render_mode == "RGB+ED")
    return absg, sgn, dict(radii=radii, means2d=means2d, depths=depths, conics=conics, flatten_ids=flatten_ids,
                           isect_offsets=isect_offsets)
