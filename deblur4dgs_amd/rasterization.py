"""Seam S1: drop-in for `gsplat.rendering.rasterization` as the reference calls it
(flow3d/scene_model.py:360-373: packed=False, C=1, render_mode in {"RGB","RGB+ED"}).

Same argument names / meaning / return triple as gsplat 1.1.1:
    render_colors [C,H,W,D(+1)] ([C,H,W,1] in the depth-only modes), render_alphas [C,H,W,1], info
render_mode: "RGB", "RGB+D", "RGB+ED", and the depth-only "D" / "ED" - the composited depth (ED: divided by max(alpha, 1e-10)), as
gsplat computes it with colors := depths[:, None] and a zero background.  Those two run the depth-only kernels (no colour table, one
channel); `colors` is validated as in the other modes but never composited (no SH evaluation, `colors.grad` stays None) and
`backgrounds` is ignored.
`info["means2d"]` is an autograd intermediate ([C,N,2], pixel units) on which callers may `.retain_grad()`;
`info["radii"]` is int32 [C,N], > 0 <=> visible.

`sh_degree=d` (0..4): `colors` are SH coefficients [N,K,3] or [1,N,K,3] with K >= (d+1)^2, evaluated per Gaussian towards
the camera centre as gsplat does (`sh.sh_colors`), then composited like [N,3] colours.

`absgrad=True`: after a backward, `info["means2d"].absgrad` [C,N,2] holds sum over pixels of (|dL_p/dx|, |dL_p/dy|) (zeros for
culled Gaussians), what gsplat's `DefaultStrategy(absgrad=True)` reads.  Computed inside the composite backward (D4GS_ABSGRAD);
up to 16 colour channels (wider renders are composited in several channel chunks: NotImplementedError).

`rasterize_mode="antialiased"`: gsplat's Mip-Splatting 2-D filter.  Every splat composites with opacity * compensation,
compensation = sqrt(max(0, det(cov2d) / det(cov2d + eps2d I))), computed by the projection kernel (D4GS_ANTIALIASED);
`info["opacities"]` is then that product [C,N] (0 where radii == 0).  Everything else in `info` keeps its classic definition.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import engine
from .engine import RenderCfg, render_instances
from .sh import sh_colors, spherical_harmonics  # noqa: F401  (re-exported: gsplat.rendering's companion)

_MODES = {"RGB": L.DEPTH_NONE, "RGB+ED": L.DEPTH_ED, "RGB+D": L.DEPTH_D, "ED": L.DEPTH_ED, "D": L.DEPTH_D}
_DEPTH_ONLY = ("D", "ED")


def rasterization(
    means: torch.Tensor,  # [N,3]
    quats: torch.Tensor,  # [N,4] wxyz
    scales: torch.Tensor,  # [N,3]
    opacities: torch.Tensor,  # [N]
    colors: torch.Tensor,  # [N,D], or SH coefficients [N,K,3] / [1,N,K,3] with sh_degree
    viewmats: torch.Tensor,  # [C,4,4]
    Ks: torch.Tensor,  # [C,3,3]
    width: int,
    height: int,
    near_plane: float = 0.01,
    far_plane: float = 1e10,
    radius_clip: float = 0.0,
    eps2d: float = 0.3,
    sh_degree=None,
    packed: bool = False,
    tile_size: int = 16,
    backgrounds: torch.Tensor | None = None,  # [C,D]
    render_mode: str = "RGB",
    sparse_grad: bool = False,
    absgrad: bool = False,
    rasterize_mode: str = "classic",
    channel_chunk: int = 32,
    exact_cull: bool = True,
    lazy_sort: bool | None = None,
    near_target: int = 0,
    exact_tiles: bool | None = None,
    **_ignored,
):
    if viewmats.shape[0] != 1 or Ks.shape[0] != 1:
        raise ValueError("C must be 1 (the reference asserts it: flow3d/scene_model.py:249)")
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"rasterize_mode {rasterize_mode!r} not supported (classic, antialiased)")
    if packed or sparse_grad or tile_size != 16:
        raise NotImplementedError("only packed=False, sparse_grad=False and tile_size=16 are implemented")
    if render_mode not in _MODES:
        raise ValueError(f"render_mode {render_mode!r} not supported (RGB, RGB+ED, RGB+D, D, ED)")
    depth_only = render_mode in _DEPTH_ONLY
    N = means.shape[0]
    if sh_degree is not None:
        d = int(sh_degree)
        if not 0 <= d <= 4:
            raise ValueError(f"sh_degree must be in 0..4, got {sh_degree}")
        if colors.dim() == 4:
            if colors.shape[0] != 1:
                raise ValueError(f"SH coefficients [C,N,K,3] need C == 1, got {tuple(colors.shape)}")
            colors = colors[0]
        if colors.dim() != 3 or colors.shape[0] != N or colors.shape[-1] != 3:
            raise ValueError(f"with sh_degree, colors must be [N,K,3] or [1,N,K,3] (N={N}), got {tuple(colors.shape)}")
        if colors.shape[1] < (d + 1) ** 2:
            raise ValueError(f"sh_degree {d} needs K >= {(d + 1) ** 2} coefficients, got K = {colors.shape[1]}")
        # gsplat masks the evaluation with radii > 0.  Unmasked here: a Gaussian that mask would drop is in no tile list,
        # so its colour is never read and its v_rgb is 0 - outputs and gradients equal the masked evaluation's, and the
        # colours need not wait for the projection.  (Depth-only modes: nothing reads the colours, nothing is evaluated.)
        if not depth_only:
            colors = sh_colors(means, viewmats[0], colors, d)
    assert quats.shape == (N, 4) and scales.shape == (N, 3) and opacities.shape == (N,) and colors.shape[0] == N
    bg = None if backgrounds is None or depth_only else backgrounds[0]
    D = colors.shape[-1]
    if depth_only:  # the depth-only kernels: no colour table, the colours are not composited (gsplat discards them)
        colors, D = None, 0
    # any channel count: the engine composites it in chunks of <= 16 channels over one projection / one set of sorted
    # tile lists (engine.channel_chunks), like gsplat's `channel_chunk`
    if lazy_sort is None:  # `info["flatten_ids"]` is part of this seam: lazy lists (unsorted behind a tile's last contributor) only on request
        lazy_sort = engine.LAZY_SORT == "1"
    if exact_tiles is None:  # likewise `tiles_per_gauss` / the lists: the per-tile ellipse test only on request (or D4GS_EXACT_TILES=1)
        exact_tiles = engine.EXACT_TILES == "1"
    cfg = RenderCfg(N=N, G=0, K=0, T=0, S=1, D=D, width=width, height=height,
                    depth_mode=_MODES[render_mode], flags=0, near_plane=near_plane, far_plane=far_plane, eps2d=eps2d,
                    radius_clip=radius_clip, exact_cull=exact_cull, lazy_sort=lazy_sort, near_target=near_target,
                    exact_tiles=exact_tiles, absgrad=bool(absgrad), antialiased=rasterize_mode == "antialiased",
                    depth_only=depth_only)
    rc, ra, means2d, radii, st = render_instances(cfg, means, quats, scales, opacities, colors, None, None, None,
                                                  None, None, viewmats[0], Ks[0], bg)
    tw, th = cfg.tiles
    opacities = st.proj_out["opac_act"][None]
    if cfg.antialiased and N > 0:  # gsplat's info["opacities"] is what was composited (N == 0: nothing was projected)
        opacities = opacities * st.proj_out["compensations"]
    info = {
        "means2d": means2d,
        "radii": radii,
        "depths": st.proj_out["depths"],
        "conics": st.proj_out["conics"],
        "opacities": opacities,
        "tiles_per_gauss": st.proj_out["tiles_touched"].view(1, N),
        "flatten_ids": st.isect["sorted_gid"][: st.n_isect],
        "isect_offsets": st.proj_out["tile_offsets"][:-1].view(1, th, tw),
        "last_ids": st.raster["last_ids"],
        "n_isect_dev": st.proj_out.get("n_isect"),  # device int64[4]: {count, longest tile list, sampled entries, sampled live entries} (include/d4gs.h)
        "width": width, "height": height, "tile_size": 16, "tile_width": tw, "tile_height": th, "n_cameras": 1,
        "n_isect": st.n_isect,
    }
    return rc, ra, info
