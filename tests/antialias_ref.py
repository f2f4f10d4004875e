"""fp64 reference of gsplat's `rasterize_mode="antialiased"` (the Mip-Splatting 2-D filter), built from the oracle's pieces:

    compensation = sqrt(max(0, det(cov2d) / det(cov2d + eps2d I)))   per visible Gaussian, 0 where radii == 0,

and the compositor (oracle.raster.rasterize_to_pixels) runs with `opacities * compensation`.  The compensation is computed from the
oracle's DIFFERENTIABLE conics Q = inv(cov2d + eps2d I) through the identity

    compensation^2 = 1 - eps2d tr(Q) + eps2d^2 det(Q),

so autograd carries every leaf gradient through it.  `rasterization` has the signature of oracle.raster.rasterization, so a test can
monkeypatch it in for `oracle.scene.render_exposure` (which looks the rasterizer up by attribute) to get the exposure oracle."""
import torch

from oracle import raster


def compensation_from_conics(conics, radii, eps2d=0.3):
    """conics [N,3] (a, b, c) of the blurred covariance, radii [N] -> [N]; 0 (with a zero gradient) where radii == 0 or the
    pre-blur determinant is not positive."""
    qa, qb, qc = conics.unbind(-1)
    c2 = 1.0 - eps2d * (qa + qc) + eps2d * eps2d * (qa * qc - qb * qb)
    ok = (radii > 0) & (c2 > 0)
    return torch.where(ok, torch.sqrt(torch.where(ok, c2, torch.ones_like(c2))), torch.zeros_like(c2))


def compensation_from_det(cov2d, eps2d=0.3):
    """cov2d [N,2,2] -> [N]: gsplat's definition, the ratio of the determinants."""
    det0 = cov2d[:, 0, 0] * cov2d[:, 1, 1] - cov2d[:, 0, 1] * cov2d[:, 1, 0]
    det1 = (cov2d[:, 0, 0] + eps2d) * (cov2d[:, 1, 1] + eps2d) - cov2d[:, 0, 1] * cov2d[:, 1, 0]
    return torch.sqrt(torch.clamp(det0 / det1, min=0.0))


def rasterization(means, quats, scales, opacities, colors, viewmat, K, width: int, height: int, background=None,
                  render_mode: str = "RGB", near_plane: float = 0.01, far_plane: float = 1e10, eps2d: float = 0.3,
                  radius_clip: float = 0.0):
    """oracle.raster.rasterization with the antialiased opacities.  -> render_colors [H,W,D(+1)], render_alphas [H,W,1], info
    (info["opacities"] = opacities * compensation, info["compensations"])."""
    assert render_mode in ("RGB", "D", "ED", "RGB+D", "RGB+ED")
    radii, means2d, depths, conics = raster.project(means, quats, scales, viewmat, K, width, height, near_plane, far_plane, eps2d,
                                                    radius_clip)
    comp = compensation_from_conics(conics, radii, eps2d)
    opac = opacities * comp
    if render_mode in ("RGB+D", "RGB+ED"):
        colors = torch.cat([colors, depths[:, None]], dim=-1)
        if background is not None:
            background = torch.cat([background, torch.zeros_like(background[:1])], dim=-1)
    elif render_mode in ("D", "ED"):
        colors = depths[:, None]
        if background is not None:
            background = torch.zeros_like(background[:1])
    tiles_per_gauss, flatten_ids, isect_offsets = raster.isect_tiles(means2d, radii, depths, width, height)
    rc, ra, last_ids = raster.rasterize_to_pixels(means2d, conics, colors, opac, width, height, flatten_ids, isect_offsets,
                                                  background)
    if render_mode in ("ED", "RGB+ED"):
        rc = torch.cat([rc[..., :-1], rc[..., -1:] / ra.clamp(min=1e-10)], dim=-1)
    info = {"radii": radii, "means2d": means2d, "depths": depths, "conics": conics, "opacities": opac, "compensations": comp,
            "tiles_per_gauss": tiles_per_gauss, "flatten_ids": flatten_ids, "isect_offsets": isect_offsets, "last_ids": last_ids,
            "n_isect": int(flatten_ids.shape[0])}
    return rc, ra, info
