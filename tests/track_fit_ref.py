"""The warm-up's loss (flow3d/init_utils.py:320-388, the body of run_initial_optim's loop) restated on oracle/deform.py with plain
torch ops, in whatever dtype the inputs have (the tests call it in fp64) - the statement csrc/track_fit.hip is held to.  Differentiable
by autograd; `schedule` restates the loop's learning rates and smoothness weight."""
import torch

from oracle import deform

TERMS = ("track_3d", "track_2d", "coef_sparse", "smooth_bases", "smooth_tracks", "z_accel")
LR0 = (1e-2, 3e-2, 1e-2, 1e-3)  # rots, transls, motion_coefs, means


def project(x_tg, Ks, w2cs):
    """x [T,G,3] -> (uv [T,G,2], v.z [T,G]): c = A x + t, v = Ks c, uv = v.xy / max(v.z, 1e-5)."""
    c = torch.einsum("tij,tgj->tgi", w2cs[:, :3, :3], x_tg) + w2cs[:, None, :3, 3]
    v = torch.einsum("tij,tgj->tgi", Ks, c)
    return v[..., :2] / torch.clamp(v[..., 2:], min=1e-5), v[..., 2]


def positions(means, motion_coefs, rots, transls):
    """-> p [G,T,3]: the deformed means at the integer frames."""
    T = rots.shape[1]
    ts = torch.arange(T, dtype=means.dtype, device=means.device)
    tf = deform.compute_transforms(ts, deform.act_coefs(motion_coefs), rots, transls)  # [G,T,3,4]
    return torch.einsum("gtij,gj->gti", tf[..., :3], means) + tf[..., 3]


def masked_l1(pred, gt, mask, quantile=1.0):
    """loss_utils.masked_l1_loss(normalize=True) for mask [...]: -> (loss, errors, threshold or None)."""
    e = (pred - gt).abs().mean(-1)
    if quantile < 1:
        thr = torch.quantile(e.detach().reshape(-1), quantile)
        keep = e < thr
    else:
        thr, keep = None, torch.ones_like(e, dtype=torch.bool)
    return (e * mask)[keep].sum() / (mask[keep].sum() + 1e-8), e, thr


def accel(x):
    return (2 * x[:, 1:-1] - x[:, :-2] - x[:, 2:]).norm(dim=-1).mean()


def terms(means, motion_coefs, rots, transls, xyz, visibles, invisibles, conf, Ks, w2cs, quantile=0.95, detail=None):
    """-> [6] in the order of TERMS.  `detail` (a dict) receives the intermediate values the tests' gap conditions look at."""
    G, T = xyz.shape[:2]
    if T < 3:
        raise ValueError("T < 3")
    p = positions(means, motion_coefs, rots, transls)
    w3, w2 = visibles.to(p.dtype) * conf, invisibles.to(p.dtype) * conf
    t3d, _, _ = masked_l1(p, xyz, w3)
    gt2d, _ = project(xyz.transpose(0, 1), Ks, w2cs)
    uv, vz = project(p.transpose(0, 1), Ks, w2cs)
    t2d, e, thr = masked_l1(uv, gt2d, w2.transpose(0, 1), quantile)
    t2d = t2d / Ks[0, 0, 0]
    coefs = deform.act_coefs(motion_coefs)
    sparse = 1 - (coefs ** 2).sum(-1).mean()
    bases = accel(rots) + 2.0 * accel(transls)
    tracks = accel(p)
    tc = torch.arange(T, device=p.device).clamp(1, T - 2)
    m0, m1, m2 = p[:, tc - 1], p[:, tc], p[:, tc + 1]
    # centre_b = -A^-1 t, solved and not inverted: the same number, without linalg.inv's device wait
    centres = -torch.linalg.solve(w2cs[:, :3, :3], w2cs[:, :3, 3:])[..., 0]
    ray = m1 - centres
    n = ray.norm(dim=-1, keepdim=True)
    d = ray / torch.clamp(n, min=1e-12)
    z = (((m1 - m0) * d).sum(-1) ** 2).mean() + (((m2 - m1) * d).sum(-1) ** 2).mean()
    if detail is not None:
        kept = (e < thr) if thr is not None else torch.ones_like(e, dtype=torch.bool)
        detail.update(p=p.detach(), e=e.detach(), thr=thr, vz=vz.detach(), w3=w3.detach(), w2k=(w2.transpose(0, 1) * kept).detach(),
                      centre_dist=(p.detach()[:, :, None] - centres[None, None]).norm(dim=-1),
                      scale3=torch.maximum(p.detach().abs(), xyz.abs()), scale2=torch.maximum(uv.detach().abs(), gt2d.abs()),
                      track_accel=(2 * p[:, 1:-1] - p[:, :-2] - p[:, 2:]).norm(dim=-1).detach(),
                      rot_accel=(2 * rots[:, 1:-1] - rots[:, :-2] - rots[:, 2:]).norm(dim=-1).detach(),
                      transl_accel=(2 * transls[:, 1:-1] - transls[:, :-2] - transls[:, 2:]).norm(dim=-1).detach(),
                      diff3=(p - xyz).detach(), diff2=(uv - gt2d).detach())
    return torch.stack([t3d, t2d, sparse, bases, tracks, z])


def w_smooth(i, num_iters, min_v=0.01, max_v=0.1, th=400):
    """The reference's w_smooth_func (init_utils.py:303-305), in Python's doubles."""
    return min_v if i <= th else (max_v - min_v) * (i - th) / (num_iters - th) + min_v


def weights(i, num_iters):
    w = w_smooth(i, num_iters)
    return [1.0, 0.5, 0.01, w, w * 0.5, 0.1]


def total(t, i, num_iters):
    return (t * torch.tensor(weights(i, num_iters), dtype=t.dtype, device=t.device)).sum()


EPS32 = 2.0 ** -23


def gaps_ok(detail, quantile=0.95, rel=1e-5, zero_accel=False):
    """The conditions under which fp32 and fp64 take the same discrete decisions (judged on fp64 values alone):
      * the order statistics of e on both sides of thr are at least rel * max(e) apart (the same kept set);
      * every acceleration norm - tracks, rots, transls - is exactly 0 (the designed zeros; all of them with zero_accel) or >= 0.05,
        so that a / |a| is as well determined in fp32 as in fp64;
      * every point is >= 0.5 from every camera centre (the ray's normalisation);
      * no argument of an |x| that carries weight lies within 16 fp32 roundings of its larger operand of 0 unless it is exactly 0, and no
        depth within 1e-3 of the clamp at 1e-5 (the sign-like derivatives)."""
    e = detail["e"].reshape(-1)
    if quantile < 1 and e.numel() > 1:
        thr, big = detail["thr"], e.max()
        below, above = e[e < thr], e[e >= thr]
        if below.numel() and above.numel() and not bool(above.min() - below.max() >= rel * big):
            return False
    for k in ("track_accel", "rot_accel", "transl_accel"):
        a = detail[k]
        if not bool(((a == 0) if zero_accel else ((a == 0) | (a >= 0.05))).all()):
            return False
    if not bool((detail["centre_dist"] >= 0.5).all()):
        return False
    for diff, w, scale in ((detail["diff3"], detail["w3"][..., None], detail["scale3"]), (detail["diff2"], detail["w2k"][..., None], detail["scale2"])):
        dd = diff.abs()
        if not bool(((dd == 0) | (dd >= 16 * EPS32 * scale) | (w == 0)).all()):
            return False
    return bool(((detail["vz"] - 1e-5).abs() >= 1e-3).all())


def make_case(G, K, T, seed, *, general_cam=False, static=False, behind=False, blind=False, coef_scale=3.0, noise=0.1):
    """fp32 CPU inputs of one fit: bases around the identity, peaked coefficients, cameras ~7 units away looking at the scene, tracks =
    the model's own positions plus noise, about 60 % of the samples visible and 70 % of the rest `invisible`.
      general_cam  camera 1 is no rotation (a rotation + 0.1 noise), every Ks has skew and differs per frame
      static       every basis row equals its first frame: the three smoothness terms are exactly zero
      behind       Gaussian 0 is placed behind camera 1 at frame 1 (v.z = -1), where it is `invisible` with a confidence > 0
      blind        Gaussian 0 has no visible and no invisible frame"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    w2cs = torch.eye(4).repeat(T, 1, 1)
    for b in range(T):
        q, r = torch.linalg.qr(rn(3, 3))
        q = q * torch.sign(torch.diagonal(r))
        w2cs[b, :3, :3] = q * torch.linalg.det(q).sign()
        w2cs[b, :3, 3] = torch.tensor([0.0, 0.0, 7.0]) + 0.5 * rn(3)
    Ks = torch.tensor([[500.0, 0.0, 320.0], [0.0, 480.0, 240.0], [0.0, 0.0, 1.0]]).repeat(T, 1, 1)
    if general_cam:
        w2cs[1, :3, :3] += 0.1 * rn(3, 3)
        Ks[:, 0, 1] = 0.3
        Ks[:, 0, 0] += 5.0 * rn(T)
        Ks[:, 1, 1] += 5.0 * rn(T)
    rots = torch.tensor([1.0, 0, 0, 0, 1, 0]) + 0.3 * rn(K, T, 6)
    transls = 0.8 * rn(K, T, 3)
    if static:
        rots, transls = rots[:, :1].repeat(1, T, 1), transls[:, :1].repeat(1, T, 1)
    means, coefs = 2 * ru(G, 3) - 1, coef_scale * rn(G, K)
    if behind:  # means_0 = R^T (x - tr) for the point x with camera coordinates (0.3, -0.2, -1) at frame 1
        tf = deform.compute_transforms(torch.tensor([1.0], dtype=torch.float64), deform.act_coefs(coefs[:1].double()), rots.double(), transls.double())[0, 0]
        x = torch.linalg.solve(w2cs[1, :3, :3].double(), torch.tensor([0.3, -0.2, -1.0], dtype=torch.float64) - w2cs[1, :3, 3].double())
        means[0] = (tf[:, :3].T @ (x - tf[:, 3])).float()
    p = positions(means.double(), coefs.double(), rots.double(), transls.double()).float()
    xyz = p + noise * rn(G, T, 3)
    vis = ru(G, T) > 0.4
    inv = (~vis) & (ru(G, T) > 0.3)
    conf = 0.2 + 0.8 * ru(G, T)
    if behind:
        vis[0, 1], inv[0, 1] = False, True
    if blind:
        vis[0], inv[0] = False, False
    return dict(means=means, motion_coefs=coefs, rots=rots, transls=transls, xyz=xyz, visibles=vis, invisibles=inv, confidences=conf,
                Ks=Ks, w2cs=w2cs)


LEAVES = ("means", "motion_coefs", "rots", "transls")
DATA = ("xyz", "visibles", "invisibles", "confidences", "Ks", "w2cs")


def on_ref(case, mix=None, quantile=0.95, detail=None):
    """-> (terms [6] fp64, the four leaf gradients of (mix * terms).sum() or None) of a case of fp32 tensors, evaluated in fp64."""
    lv = [case[k].detach().double().requires_grad_() for k in LEAVES]
    d = [case[k].double() if case[k].is_floating_point() else case[k] for k in DATA]
    t = terms(*lv, *d, quantile=quantile, detail=detail)
    if mix is None:
        return t.detach(), None
    return t.detach(), list(torch.autograd.grad((t * torch.as_tensor(mix, dtype=t.dtype)).sum(), lv))


def conditioned_case(G, K, T, seed, quantile=0.95, attempts=400, **kw):
    """make_case with the seed advanced (by 1000 per attempt) until gaps_ok holds on the fp64 values -> (case, detail)"""
    for attempt in range(attempts):
        case = make_case(G, K, T, seed + 1000 * attempt, **kw)
        detail = {}
        on_ref(case, quantile=quantile, detail=detail)
        if gaps_ok(detail, quantile, zero_accel=kw.get("static", False)):
            return case, detail
    raise AssertionError(("no well-conditioned seed", G, K, T, seed, kw))


def simulate(case, num_iters, quantile=0.95, on_step=None):
    """The reference's loop in this file's words, in fp64: one torch.optim.Adam with four param groups, ExponentialLR, the six terms
    weighted by `weights(i, num_iters)`.  on_step(i, terms, grads, detail) sees every iteration.  -> the four leaves after num_iters."""
    lv = [case[k].detach().double().clone().requires_grad_() for k in LEAVES]
    d = [case[k].double() if case[k].is_floating_point() else case[k] for k in DATA]
    by = dict(zip(LEAVES, lv))
    opt = torch.optim.Adam([{"params": [by[k]], "lr": lr} for k, lr in zip(("rots", "transls", "motion_coefs", "means"), LR0)])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.1 ** (1 / num_iters))
    for i in range(num_iters):
        detail = {}
        t = terms(*lv, *d, quantile=quantile, detail=detail)
        opt.zero_grad()
        total(t, i, num_iters).backward()
        if on_step is not None:
            on_step(i, t.detach(), [x.grad.clone() for x in lv], detail)
        opt.step()
        sched.step()
    return [x.detach() for x in lv]


def compose_terms(means, motion_coefs, rots, transls, xyz, w3, w2, Ks, w2cs, gt2d=None, quantile=0.95):
    """The six terms composed from what the package had before csrc/track_fit.hip, on device tensors in fp32: the positions and the
    projection as torch ops, `losses.masked_l1_loss` twice, `losses.motion_regularizers` twice - once over the interior frames for the
    track acceleration (its 0.5 factor undone), once over all T frames for the z acceleration and the bases.  That is 3 T - 2
    deformations per Gaussian beside the T of the positions.  Differentiable; the measurement's third variant."""
    from deblur4dgs_amd.losses import masked_l1_loss, motion_regularizers

    T = rots.shape[1]
    p = positions(means, motion_coefs, rots, transls)
    if gt2d is None:
        gt2d = project(xyz.transpose(0, 1), Ks, w2cs)[0].transpose(0, 1).contiguous()
    uv = project(p.transpose(0, 1), Ks, w2cs)[0].transpose(0, 1)
    t3d = masked_l1_loss(p, xyz, w3[..., None])
    t2d = masked_l1_loss(uv, gt2d, w2[..., None], quantile=quantile) / Ks[0, 0, 0]
    sparse = 1 - (deform.act_coefs(motion_coefs) ** 2).sum(-1).mean()
    scales = torch.zeros_like(means)
    ts = torch.arange(T, device=means.device, dtype=torch.float32)
    sb, _, z, _ = motion_regularizers(means, motion_coefs, rots, transls, scales, ts, w2cs)
    _, st, _, _ = motion_regularizers(means, motion_coefs, rots, transls, scales, ts[1:T - 1], w2cs[1:T - 1])
    return torch.stack([t3d, t2d, sparse, sb, 2.0 * st, z])
