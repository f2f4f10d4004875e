"""Cameras in general position for the parity tests.

`synth.make_scene` / `tests.util.static_inputs` look through `viewmat = I`, `fx = fy = W` and a centred principal point: under that
camera R and R^T, fx and fy, limx and limy, and the two sides of every cull are interchangeable.  `apply_camera` re-expresses such a
scene under one of five named cameras - the content that is in view stays (roughly) in view - and asserts, in fp64 on the oracle's
`project`, that the result is a test of what its name claims:

  rotated      V = [R0 | t0], R0 = exp([[0, -.3, .2], [.3, 0, -.1], [-.2, .1, 0]]) (0.37 rad), t0 = (0.8, -0.5, 1.5); the world becomes
               R0^T (x - t0), q(R0^T) (x) quats: the camera-space scene is the one of the identity camera.  K unchanged.
  anisotropic  fx = 1.25 W, fy = 0.85 W, centred.
  offcentre    cx = W / 2 + 5.3, cy = H / 2 - 3.7 (non-integers of opposite sign).
  general      all three.
  rolled       an exact quarter turn about the optical axis: V <- Rz V (entries 0, +-1), fx <-> fy, (cx, cy) <- (H - cy, cx),
               W <-> H.  The new image is the old one turned by 90 degrees (`unroll` turns it back).

Cameras compose: each is applied to whatever V / K the scene already carries.  The three cameras with another K also re-place the
last `4 * PROBES` Gaussians as CLAMP PROBES: large splats centred just outside x / z = +-1.3 tan(fov_x / 2) resp. y / z = +-1.3 tan(fov_y
/ 2) on each of the four sides, 30 % of a half-image off screen, wide enough to reach into the image - the Gaussians that take the
clamped branch of the projection Jacobian and of its adjoint, and that are cut by the image edge they hang over.  (make_scene's own
spread, x / z in +-0.55, reaches the x clamp of fx = 1.25 W by a hair and the y clamp never; Gaussians that are merely placed out
there are culled before the clamp can matter.)
"""
from __future__ import annotations

import math

import torch

from oracle import raster

CAMERAS = ("rotated", "anisotropic", "offcentre", "general", "rolled")
PROBES = 6  # per side
_A = torch.tensor([[0.0, -0.3, 0.2], [0.3, 0.0, -0.1], [-0.2, 0.1, 0.0]], dtype=torch.float64)
R0 = torch.linalg.matrix_exp(_A)
T0 = torch.tensor([0.8, -0.5, 1.5], dtype=torch.float64)
_w = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)  # _A = [w]_x
_th = float(_w.norm())
Q0T = torch.cat([torch.tensor([math.cos(0.5 * _th)], dtype=torch.float64), -math.sin(0.5 * _th) * _w / _th])  # wxyz of R0^T
RZ = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)  # (x, y, z) -> (-y, x, z)


def quat_mul(a, b):
    """Hamilton product, wxyz: the rotation of `a` after the rotation of `b`."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _keys(d):
    """(name of viewmat, of scales, of opacities, raw?) - a make_scene dict holds raw leaves, a static_inputs dict activated ones."""
    return ("viewmat", "scales", "opacities", True) if "viewmat" in d else ("V", "scales", "opac", False)


def _place_probes(d, W, H):
    """Overwrite the last 4 * PROBES Gaussians with the clamp probes of the camera (V, K) that `d` carries (see the module docstring)."""
    vk, sk, ok, raw = _keys(d)
    V, K = d[vk].double(), d["K"].double()
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    limx, limy = 1.3 * 0.5 * W / fx, 1.3 * 0.5 * H / fy
    N = d["means"].shape[0]
    assert N >= 8 * PROBES, "the scene is too small to carry the clamp probes"
    pc, sc = [], []
    for axis, sign in ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0)):
        for j in range(PROBES):
            out = 1.03 + 0.04 * j            # 3 % .. 23 % beyond the clamp
            along = 0.5 * (j / (PROBES - 1) - 0.5) * sign  # spread along the edge, within the middle half of the image
            z = 2.5 + 0.5 * j
            if axis == 0:
                xr, yr = sign * out * limx, along * (0.5 * H / fy)
                off = (fx * xr + cx - W) if sign > 0 else -(fx * xr + cx)  # pixels beyond the edge it hangs over
                s = (off + 4.0) / 2.0 * z / fx
            else:
                xr, yr = along * (0.5 * W / fx), sign * out * limy
                off = (fy * yr + cy - H) if sign > 0 else -(fy * yr + cy)
                s = (off + 4.0) / 2.0 * z / fy
            assert off > 0
            pc.append([xr * z, yr * z, z])
            sc.append(s)            # the image edge lies two standard deviations (minus 4 px) from the centre
    pc = torch.tensor(pc, dtype=torch.float64)
    sc = torch.tensor(sc, dtype=torch.float64)[:, None].expand(-1, 3)
    world = (pc - V[:3, 3]) @ V[:3, :3]  # R^T (p - t)
    n = pc.shape[0]
    dt = d["means"].dtype
    d["means"] = torch.cat([d["means"][:-n], world.to(dt)], 0)
    d[sk] = torch.cat([d[sk][:-n], (torch.log(sc) if raw else sc).to(dt)], 0)
    op = torch.full((n,), 0.6, dtype=torch.float64)
    d[ok] = torch.cat([d[ok][:-n], (torch.logit(op) if raw else op).to(dt)], 0)


def apply_camera(inp_or_scene, name, W, H, check=True):
    """-> (scene under the named camera: a new dict of the same kind, W', H').  `inp_or_scene`: a `static_inputs` dict (V, K,
    activated scales / opac) or a `make_scene` dict (viewmat, K, raw leaves); tensors of any dtype, none requiring grad."""
    assert name in CAMERAS, name
    d = dict(inp_or_scene)
    vk, sk, ok, raw = _keys(d)
    dt = d["means"].dtype
    V, K = d[vk].double().clone(), d["K"].double().clone()
    if name in ("rotated", "general"):
        M = torch.eye(4, dtype=torch.float64)
        M[:3, :3], M[:3, 3] = R0, T0
        V = V @ M                                        # V' x' = V x  with  x' = R0^T (x - t0)
        d["means"] = ((d["means"].double() - T0) @ R0).to(dt)
        d["quats"] = quat_mul(Q0T, d["quats"].double()).to(dt)
    if name in ("anisotropic", "general"):
        K[0, 0], K[1, 1] = 1.25 * W, 0.85 * W
    if name in ("offcentre", "general"):
        K[0, 2], K[1, 2] = K[0, 2] + 5.3, K[1, 2] - 3.7
    if name == "rolled":
        R4 = torch.eye(4, dtype=torch.float64)
        R4[:3, :3] = RZ
        V = R4 @ V
        fx, fy, cx, cy = K[0, 0].clone(), K[1, 1].clone(), K[0, 2].clone(), K[1, 2].clone()
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fy, fx, H - cy, cx
        W, H = H, W
    d[vk], d["K"] = V.to(dt), K.to(dt)
    if "W" in d:
        d["W"], d["H"] = W, H
    if name in ("anisotropic", "offcentre", "general"):
        _place_probes(d, W, H)
    if check:
        assert_is_a_test_of(d, name, W, H)
    return d, W, H


def unroll(img):
    """The image [H', W', ...] of a `rolled` camera turned back: [W', H', ...] = the unrolled camera's image."""
    return img.transpose(0, 1).flip(0)


def activated(d):
    """(means, quats, scales, opac, V, K) in fp64, scales / opacities activated."""
    vk, sk, ok, raw = _keys(d)
    sc, op = d[sk].double(), d[ok].double()
    return (d["means"].double(), d["quats"].double(), torch.exp(sc) if raw else sc, torch.sigmoid(op) if raw else op, d[vk].double(),
            d["K"].double())


def census(d, W, H):
    """fp64 facts about the canonical scene (no deformation, no camera delta) under its camera."""
    means, quats, scales, _, V, K = activated(d)
    radii, m2d, _, _ = raster.project(means, quats, scales, V, K, W, H)
    vis = radii > 0
    r = radii.double()
    pc = means @ V[:3, :3].T + V[:3, 3]
    xr, yr = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    limx, limy = 1.3 * 0.5 * W / float(K[0, 0]), 1.3 * 0.5 * H / float(K[1, 1])
    front = pc[:, 2] > 0.01
    return dict(visible=float(vis.double().mean()),
                # visible and cut by the edge / culled beyond it
                cut=dict(left=int((vis & (m2d[:, 0] - r < 0)).sum()), right=int((vis & (m2d[:, 0] + r > W)).sum()),
                         top=int((vis & (m2d[:, 1] - r < 0)).sum()), bottom=int((vis & (m2d[:, 1] + r > H)).sum())),
                # VISIBLE Gaussians beyond the clamp of the projection Jacobian (a culled one never reaches the clamped branch's output)
                clamped={"+x": int((vis & (xr > limx)).sum()), "-x": int((vis & (xr < -limx)).sum()),
                         "+y": int((vis & (yr > limy)).sum()), "-y": int((vis & (yr < -limy)).sum())},
                culled=int((front & ~vis).sum()))


def assert_is_a_test_of(d, name, W, H):
    c = census(d, W, H)
    assert c["visible"] >= 0.60, (name, c)
    assert all(v >= 1 for v in c["cut"].values()), (name, c)
    if name in ("anisotropic", "offcentre", "general"):
        assert all(v >= 5 for v in c["clamped"].values()), (name, c)
    vk = _keys(d)[0]
    V, K = d[vk].double(), d["K"].double()
    eye = torch.eye(3, dtype=torch.float64)
    if name in ("rotated", "general"):  # every entry of R differs from R^T's by far more than the tolerance
        assert float((V[:3, :3] - V[:3, :3].T).abs().max()) > 0.1 and float(V[:3, 3].abs().min()) > 0.1
    if name in ("anisotropic", "general"):
        assert abs(float(K[0, 0] / K[1, 1]) - 1.0) > 0.3
    if name in ("offcentre", "general"):
        assert abs(float(K[0, 2]) - W / 2) > 3 and abs(float(K[1, 2]) - H / 2) > 3 and (float(K[0, 2]) - W / 2) * (float(K[1, 2]) - H / 2) < 0
    if name == "rolled":
        assert bool(((V[:3, :3].abs() == 0) | (V[:3, :3].abs() == 1)).all()) and not torch.equal(V[:3, :3], eye)
    return c


# ---- the static seam under a camera: scene + fp64 oracle, shared by the CPU-twin and the GPU tests ---------------------------------
def static_case(camera, mode, D, N, W, H, seed, scale_mul=3.0):
    """`static_inputs` under `camera` through oracle.raster.rasterization in fp64, forward and backward.
    -> dict(inp, W, H (the camera's), bg, ref_c, ref_a, info, w_c, w_a, grads: means2d + every leaf + V)"""
    from tests.util import static_inputs

    inp = static_inputs(N, W, H, seed=seed, dtype=torch.float64, D=D, scale_mul=scale_mul)
    if camera is not None:
        inp, W, H = apply_camera(inp, camera, W, H)
    bg = torch.linspace(0.1, 0.9, D, dtype=torch.float64)
    t = {k: v.clone().requires_grad_(k != "K") for k, v in inp.items()}
    ref_c, ref_a, info = raster.rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"], t["K"], W, H,
                                              background=bg, render_mode=mode)
    g = torch.Generator().manual_seed(9)
    w_c = torch.randn(ref_c.shape, generator=g, dtype=torch.float64)
    w_a = torch.randn(ref_a.shape, generator=g, dtype=torch.float64)
    info["means2d"].retain_grad()
    ((ref_c * w_c).sum() + (ref_a * w_a).sum()).backward()
    grads = {k: t[k].grad for k in ("means", "quats", "scales", "opac", "colors", "V")}
    grads["means2d"] = info["means2d"].grad
    return dict(inp=inp, W=W, H=H, bg=bg, ref_c=ref_c.detach(), ref_a=ref_a.detach(), info=info, w_c=w_c, w_a=w_a, grads=grads)


# ---- the fused exposure render under a camera: scene + fp64 oracle, shared by the CPU-twin and the GPU tests ---------------------
LEAF_KEYS = ("means", "quats", "scales", "colors", "opacities")


def exposure_case(N, G, K, S, W, H, seed, camera, mask=True, depth=True, cam_jitter=0.03):
    """One dynamic (G > 0) or static (G = 0) scene under `camera`, rendered and differentiated by oracle.scene.render_exposure in
    fp64 with cotangents on the blended frame, its accumulation and every sub-sample render.
    -> dict(sc=the scene (fp64, raw leaves), ref=dict of reference tensors, grads=dict of reference leaf gradients, w=cotangents)"""
    from deblur4dgs_amd.synth import make_scene
    from oracle import scene as oscene

    sc = make_scene(N, G, max(K, 1), S, W, H, seed=seed, dtype=torch.float64, cam_jitter=cam_jitter)
    sc["scales"] = sc["scales"] + 1.2  # Gaussians big enough to overlap several pixels
    if camera is not None:
        sc, W2, H2 = apply_camera(sc, camera, W, H)
        assert (W2, H2) == (W, H)
    leaf = lambda t: t.clone().requires_grad_()
    fg = bases = bg = None
    if G:
        fg = {k: leaf(sc[k][:G]) for k in LEAF_KEYS}
        fg["motion_coefs"] = leaf(sc["motion_coefs"])
        bases = {k: leaf(sc[k]) for k in ("rots", "transls")}
    if G < N:
        bg = {k: leaf(sc[k][G:]) for k in LEAF_KEYS}
    times, RTs, w2c = leaf(sc["times"]), leaf(sc["RTs"]), leaf(sc["viewmat"])
    out = oscene.render_exposure(fg, bg, bases, times, RTs, w2c, sc["K"], (W, H), bg_color=1.0, return_depth=depth, return_mask=mask,
                                 single=(S == 1))
    blended = torch.cat([out[k] for k in ("img", "mask", "depth") if k in out], -1)[0]
    g = torch.Generator().manual_seed(1)
    w_b = torch.randn(blended.shape, generator=g, dtype=torch.float64)
    w_a = torch.randn(out["acc"][0].shape, generator=g, dtype=torch.float64)
    renders = torch.stack(out["raw_renders"], 0)[:, 0]  # [S,H,W,D']
    w_r = 0.1 * torch.randn(renders.shape, generator=g, dtype=torch.float64)
    ((blended * w_b).sum() + (out["acc"][0] * w_a).sum() + (renders * w_r).sum()).backward()
    parts = [p for p in (fg, bg) if p is not None]
    grads = {k: torch.cat([p[k].grad for p in parts], 0) for k in LEAF_KEYS}
    if G:
        grads.update(motion_coefs=fg["motion_coefs"].grad, rots=bases["rots"].grad, transls=bases["transls"].grad, times=times.grad)
    grads.update(RTs=RTs.grad, viewmat=w2c.grad)
    ref = dict(renders=renders.detach(), blended=blended.detach(), acc=out["acc"][0, ..., 0].detach())
    return dict(sc=sc, ref=ref, grads=grads, w=dict(blended=w_b, acc=w_a[..., 0], renders=w_r), N=N, G=G, S=S, W=W, H=H, mask=mask,
                depth=depth)


def exposure_leaves(case, device=None):
    """fp32 leaves of `exposure_case`'s scene (on `device`), the colour matrix with the mask channel appended, its background."""
    sc, N, G = case["sc"], case["N"], case["G"]
    mv = lambda t: (t.float() if device is None else t.float().to(device))
    L = {k: mv(sc[k]).requires_grad_() for k in LEAF_KEYS}
    for k in ("motion_coefs", "rots", "transls", "times"):
        L[k] = mv(sc[k]).requires_grad_() if G else None
    L["RTs"], L["viewmat"] = mv(sc["RTs"]).requires_grad_(), mv(sc["viewmat"]).requires_grad_()
    colors_in, bgc = L["colors"], mv(torch.ones(3))
    if case["mask"]:
        mk = torch.zeros(N, 1)
        mk[: (G if 0 < G < N else N)] = 1.0
        colors_in, bgc = torch.cat([colors_in, mv(mk)], -1), torch.cat([bgc, mv(torch.zeros(1))])
    return L, colors_in, bgc, mv(sc["K"])
