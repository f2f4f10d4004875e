"""fp64 torch restatement of the SH colour model (gsplat 1.1.1 `spherical_harmonics` and `rasterization(sh_degree=d)`):
the real SH basis of degree 0..4 in the Inria / gsplat order and sign convention, the direction normalisation, masks,
the `+0.5 / clamp_min(0)` epilogue and the camera centre through `torch.inverse(viewmat)`.  The test's reference for
deblur4dgs_amd.sh; written from the basis table, evaluated on the unit vector (x, y, z)."""
import torch

# (constant, polynomial in x, y, z) for k = 0..24
BASIS = (
    (0.28209479177387814, lambda x, y, z: torch.ones_like(x)),
    (-0.4886025119029199, lambda x, y, z: y),
    (0.4886025119029199, lambda x, y, z: z),
    (-0.4886025119029199, lambda x, y, z: x),
    (1.0925484305920792, lambda x, y, z: x * y),
    (-1.0925484305920792, lambda x, y, z: y * z),
    (0.31539156525252005, lambda x, y, z: 2 * z * z - x * x - y * y),
    (-1.0925484305920792, lambda x, y, z: x * z),
    (0.5462742152960396, lambda x, y, z: x * x - y * y),
    (-0.5900435899266435, lambda x, y, z: y * (3 * x * x - y * y)),
    (2.890611442640554, lambda x, y, z: x * y * z),
    (-0.4570457994644658, lambda x, y, z: y * (4 * z * z - x * x - y * y)),
    (0.3731763325901154, lambda x, y, z: z * (2 * z * z - 3 * x * x - 3 * y * y)),
    (-0.4570457994644658, lambda x, y, z: x * (4 * z * z - x * x - y * y)),
    (1.445305721320277, lambda x, y, z: z * (x * x - y * y)),
    (-0.5900435899266435, lambda x, y, z: x * (x * x - 3 * y * y)),
    (2.5033429417967046, lambda x, y, z: x * y * (x * x - y * y)),
    (-1.7701307697799304, lambda x, y, z: y * z * (3 * x * x - y * y)),
    (0.9461746957575601, lambda x, y, z: x * y * (7 * z * z - 1)),
    (-0.6690465435572892, lambda x, y, z: y * z * (7 * z * z - 3)),
    (0.10578554691520431, lambda x, y, z: z * z * (35 * z * z - 30) + 3),
    (-0.6690465435572892, lambda x, y, z: x * z * (7 * z * z - 3)),
    (0.47308734787878004, lambda x, y, z: (x * x - y * y) * (7 * z * z - 1)),
    (-1.7701307697799304, lambda x, y, z: x * z * (x * x - 3 * y * y)),
    (0.6258357354491761, lambda x, y, z: x * x * (x * x - 3 * y * y) - y * y * (3 * x * x - y * y)),
)


def basis(degree: int, u: torch.Tensor) -> torch.Tensor:
    """Y_k(u) for k < (degree+1)^2 on unit vectors u [..., 3] -> [..., (degree+1)^2]."""
    x, y, z = u.unbind(-1)
    return torch.stack([c * f(x, y, z) for c, f in BASIS[: (degree + 1) ** 2]], -1)


def spherical_harmonics(degree: int, dirs: torch.Tensor, coeffs: torch.Tensor, masks=None) -> torch.Tensor:
    """sum_{k < (degree+1)^2} Y_k(dirs / |dirs|) coeffs[..., k, :] -> [..., 3]; masked entries are 0."""
    nb = (degree + 1) ** 2
    u = dirs / dirs.norm(dim=-1, keepdim=True)
    out = (basis(degree, u)[..., None] * coeffs[..., :nb, :]).sum(-2)
    if masks is not None:
        out = torch.where(masks[..., None], out, torch.zeros_like(out))
    return out


def campos(viewmat: torch.Tensor) -> torch.Tensor:
    """The camera centre of a world-to-camera matrix [4,4], as gsplat computes it."""
    return torch.inverse(viewmat)[:3, 3]


def sh_colors(means: torch.Tensor, viewmat: torch.Tensor, coeffs: torch.Tensor, degree: int, masks=None) -> torch.Tensor:
    """gsplat's `rasterization` colours: clamp_min(SH(means - campos) + 0.5, 0), [N,3]."""
    return torch.clamp_min(spherical_harmonics(degree, means - campos(viewmat), coeffs, masks) + 0.5, 0.0)
