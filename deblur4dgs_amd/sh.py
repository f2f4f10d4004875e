"""Spherical-harmonic colours on the device (`csrc/sh.hip`): gsplat 1.1.1's `spherical_harmonics` and the view-dependent
colours of its `rasterization(..., sh_degree=d)`.

`spherical_harmonics(degrees_to_use, dirs [..., 3], coeffs [..., K, 3], masks [...] = None) -> [..., 3]` evaluates
sum_{k < (d+1)^2} Y_k(dirs / |dirs|) coeffs[..., k, :] with the real SH basis in the Inria / gsplat order (degree 0..4).
Masked entries, and entries whose direction has zero length (gsplat: NaN), give 0 and zero gradients.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._lib import f32c, need_gpu, stream_of, vp


class SHFn(torch.autograd.Function):
    """rgb [N,3] from points [N,3] (direction = points - origin, or points when origin is None), coeffs [N,K,3] and
    masks uint8 [N] / None; `clamp` adds gsplat's rasterization epilogue max(rgb + 0.5, 0)."""

    @staticmethod
    def forward(ctx, degree, points, origin, coeffs, masks, clamp):
        need_gpu(points, "deblur4dgs_amd.sh", " (no CPU fallback)")
        for t in (origin, coeffs, masks):
            if t is not None and t.device != points.device:
                raise RuntimeError(f"deblur4dgs_amd.sh: every tensor must be on {points.device}, got one on {t.device}")
        p, o, c = f32c(points), f32c(origin), f32c(coeffs)
        N, K = c.shape[0], c.shape[1]
        rgb = torch.empty(N, 3, device=p.device, dtype=torch.float32)
        if N > 0:
            stream = stream_of(p)
            L.check(L.lib().d4gs_sh_fwd(N, K, degree, vp(p), vp(o), vp(c), vp(masks), int(clamp), vp(rgb), stream),
                    "d4gs_sh_fwd")
        ctx.keep = (p, o, c, masks)
        ctx.cfg = (degree, int(clamp), points.dtype, None if origin is None else origin.dtype, coeffs.dtype)
        return rgb

    @staticmethod
    def backward(ctx, v_rgb):
        p, o, c, masks = ctx.keep
        degree, clamp, p_dtype, o_dtype, c_dtype = ctx.cfg
        need_p, need_o, need_c = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        N, K = c.shape[0], c.shape[1]
        dev = p.device
        v_p = torch.empty(N, 3, device=dev, dtype=torch.float32) if need_p else None
        v_c = torch.empty(N, K, 3, device=dev, dtype=torch.float32) if need_c else None
        v_o = None
        if need_o:
            v_o = (torch.empty if N > 0 else torch.zeros)(3, device=dev, dtype=torch.float32)
        if N > 0 and (need_p or need_o or need_c):
            partials = torch.empty(L.lib().d4gs_sh_partials_elems(N), device=dev, dtype=torch.float32) if need_o else None
            stream = stream_of(p)
            L.check(L.lib().d4gs_sh_bwd(N, K, degree, vp(p), vp(o), vp(c), vp(masks), clamp, vp(f32c(v_rgb)), vp(v_c),
                                        vp(v_p), vp(v_o), vp(partials), stream), "d4gs_sh_bwd")
        cast = lambda g, dt: None if g is None else g.to(dt)  # noqa: E731
        return None, cast(v_p, p_dtype), cast(v_o, o_dtype), cast(v_c, c_dtype), None, None


def _mask_u8(masks):
    if masks is None:
        return None
    m = masks if masks.dtype in (torch.bool, torch.uint8) else masks != 0
    return m.detach().contiguous().view(torch.uint8)


def spherical_harmonics(degrees_to_use: int, dirs: torch.Tensor, coeffs: torch.Tensor, masks: torch.Tensor | None = None):
    """gsplat 1.1.1 `spherical_harmonics`: dirs [..., 3], coeffs [..., K, 3] with K >= (degrees_to_use + 1)^2, masks [...]
    (bool) or None -> colours [..., 3] (raw: no +0.5, no clamp).  Differentiable w.r.t. `dirs` and `coeffs`."""
    d = int(degrees_to_use)
    if not 0 <= d <= 4:
        raise ValueError(f"degrees_to_use must be in 0..4, got {d}")
    if dirs.shape[-1] != 3 or coeffs.dim() < 2 or coeffs.shape[-1] != 3 or dirs.shape[:-1] != coeffs.shape[:-2]:
        raise ValueError(f"expected dirs [..., 3] and coeffs [..., K, 3] with the same leading shape, got "
                         f"{tuple(dirs.shape)} and {tuple(coeffs.shape)}")
    K = coeffs.shape[-2]
    if K < (d + 1) ** 2:
        raise ValueError(f"degree {d} needs K >= {(d + 1) ** 2} coefficients, got K = {K}")
    if masks is not None and masks.shape != dirs.shape[:-1]:
        raise ValueError(f"masks must have shape {tuple(dirs.shape[:-1])}, got {tuple(masks.shape)}")
    lead = dirs.shape[:-1]
    m = _mask_u8(masks)
    rgb = SHFn.apply(d, dirs.reshape(-1, 3), None, coeffs.reshape(-1, K, 3), None if m is None else m.reshape(-1), False)
    return rgb.reshape(*lead, 3)


class CamPosFn(torch.autograd.Function):
    """campos = inverse(viewmat)[:3, 3] of a rigid world-to-camera matrix [4,4], in closed form (-R^T t), with the gradient
    torch.inverse would give (bottom row included): dL/dV = -[R v ; c.v] [c ; 1]^T for v = dL/dcampos.  No torch.inverse:
    on the device it synchronises the host to check `info`."""

    @staticmethod
    def forward(ctx, viewmat):
        R, t = viewmat[:3, :3], viewmat[:3, 3]
        c = -(R.transpose(0, 1) @ t)
        ctx.save_for_backward(viewmat, c)
        return c

    @staticmethod
    def backward(ctx, v):
        viewmat, c = ctx.saved_tensors
        left = torch.cat([viewmat[:3, :3] @ v, (c * v).sum().reshape(1)])
        right = torch.cat([c, torch.ones_like(c[:1])])
        return -torch.outer(left, right)


def sh_colors(means: torch.Tensor, viewmat: torch.Tensor, coeffs: torch.Tensor, sh_degree: int) -> torch.Tensor:
    """gsplat 1.1.1 `rasterization`'s colours for `sh_degree`: clamp_min(SH(means - campos) + 0.5, 0), [N,3].  No mask:
    see `rasterization.rasterization`."""
    return SHFn.apply(int(sh_degree), means, CamPosFn.apply(viewmat), coeffs, None, True)
