"""The trainer's motion and scale regularizers restated in torch on the CPU (fp64 unless told otherwise): what
deblur4dgs_amd.losses.motion_regularizers must compute.

Written from the description in DESIGN.md section 18; tests/test_motion_ref.py pins it to values recorded from the reference's own
functions (tests/golden/motion_regs.npz).  The deformation is oracle/deform.py's.  Differentiable through torch autograd.

    tc_b = clamp(ts_b, 1, T-2);   m_j[g,b] = R(tc_b + j - 1; g) means_g + tr(tc_b + j - 1; g),  j = 0, 1, 2
    smooth_tracks = 0.5 mean |2 m_1 - m_0 - m_2|
    z_accel       = mean ((m_1 - m_0) . d)^2 + mean ((m_2 - m_1) . d)^2,   d = (m_1 - c_b) / max(|m_1 - c_b|, 1e-12),
                    c_b = -A_b^-1 t_b for w2c_b = [A_b t_b; 0 0 0 1]
    smooth_bases  = w_rot mean_{k, 1 <= tau <= T-2} |2 rots[k,tau] - rots[k,tau-1] - rots[k,tau+1]| + w_transl (the same on transls)
    scale_var     = mean_g sum_i (s_gi - mean_i s_gi)^2 / 2

The norms are written as sqrt(sum of squares) guarded at exactly zero, where value and gradient are 0 (torch.norm's convention)."""
import torch

from oracle import deform


def _norm(x):
    """|x| over the last axis; exactly 0, with a zero gradient, where x is exactly 0"""
    s = x.square().sum(-1)
    live = s > 0
    return torch.where(live, torch.where(live, s, torch.ones_like(s)).sqrt(), torch.zeros_like(s))


def neighbour_means(means, motion_coefs, rots, transls, ts):
    """-> [3, G, B, 3]: the deformed means at clamp(ts, 1, T-2) - 1, + 0, + 1"""
    T = rots.shape[1]
    tc = ts.to(means.dtype).clamp(1, T - 2)
    tf = deform.compute_transforms(torch.cat((tc - 1, tc, tc + 1)), deform.act_coefs(motion_coefs), rots, transls)  # [G, 3B, 3, 4]
    m = (tf[..., :3] @ means[:, None, :, None])[..., 0] + tf[..., 3]
    return m.reshape(m.shape[0], 3, -1, 3).permute(1, 0, 2, 3)


def camera_centres(w2cs):
    """-> [B, 3]: -A^-1 t, by the cofactor inverse the kernel uses (no torch.linalg.inv: this file is the formula, not the library)"""
    A, t = w2cs[:, :3, :3], w2cs[:, :3, 3]
    cof = torch.stack([torch.linalg.cross(A[:, (i + 1) % 3], A[:, (i + 2) % 3], dim=-1) for i in range(3)], 1)  # rows: cofactors of row i
    det = (A[:, 0] * cof[:, 0]).sum(-1)
    return -(cof.transpose(1, 2) @ t[..., None])[..., 0] / det[:, None]


def accel_norms(x):
    """[K,T,D] -> [K,T-2]"""
    return _norm(torch.diff(x, n=2, dim=1))  # x[tau+1] - 2 x[tau] + x[tau-1]: the same norm


def motion_regularizers(means, motion_coefs, rots, transls, scales, ts, w2cs, weight_rot=1.0, weight_transl=2.0):
    """-> (smooth_bases, smooth_tracks, z_accel, scale_var)"""
    m0, m1, m2 = neighbour_means(means, motion_coefs, rots, transls, ts)
    smooth_tracks = 0.5 * _norm(2 * m1 - m0 - m2).mean()
    r = m1 - camera_centres(w2cs.to(means.dtype))
    d = r / _norm(r).clamp_min(1e-12)[..., None]
    z_accel = ((m1 - m0) * d).sum(-1).square().mean() + ((m2 - m1) * d).sum(-1).square().mean()
    smooth_bases = weight_rot * accel_norms(rots).mean() + weight_transl * accel_norms(transls).mean()
    scale_var = ((scales - scales.mean(-1, keepdim=True)).square().sum(-1) / 2).mean()
    return smooth_bases, smooth_tracks, z_accel, scale_var
