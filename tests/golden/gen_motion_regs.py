"""Fixture of the trainer's motion and scale regularizers: small inputs, and the four values and the leaf gradients that the
REFERENCE's own functions give for them in float64 on the CPU.

    D4GS_REFERENCE=<checkout of the reference> python tests/golden/gen_motion_regs.py   ->  tests/golden/motion_regs.npz

`MotionBases.compute_transforms` is imported from the reference (the stubs of gen_golden._import_reference), and
`compute_z_acc_loss`, `compute_se3_smoothness_loss` (with `compute_accel_loss` under it) are taken from the head of its
flow3d/loss_utils.py (gen_trimmed_losses.load_reference).  The block of Trainer.compute_dynamic_losses around them
(flow3d/trainer.py:699-716,721-724) is inline in the trainer and cannot be called on its own, so `reference_flow` below computes what
it computes in this file's own words: the clamped times and their two neighbours, the transforms applied to the means as a batched
matrix product, the norm of the second difference of each track, and the unbiased variance of the raw scales written out.  Only data
travels: the arrays below.

Every input is rounded to fp32 before use, so the GPU sees the same numbers.  So that fp32 cannot be ill-conditioned where the
reference is not, a case's seed is advanced until, outside the rows that are zero by design, every track acceleration and every basis
acceleration has norm >= 0.05, every Gaussian is >= 0.5 from every camera centre and |means| <= 4 (the inputs and the deformed
ones).  The archive is written with fixed zip timestamps: the same generator gives the same bytes."""
import io
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
from gen_trimmed_losses import load_reference  # noqa: E402

LEAVES = ("means", "motion_coefs", "rots", "transls", "scales")
TERMS = ("smooth_bases", "smooth_tracks", "z_accel", "scale_var")
MIX = (1.3, 0.7, 2.1, 0.9)  # the upstream factors of the stored gradient
#        name            G   K   T   ts                          seed
CASES = (("default_small", 333, 20, 24, [3.0], 100),
         ("block_edges", 65, 5, 8, [0.0, 3.0, 7.0], 200),
         ("one", 1, 1, 3, [1.0], 300),
         ("many_times", 130, 12, 12, [1.0, 1.0, 4.37, 10.0, 6.0], 400),
         ("static_bases", 70, 5, 6, [2.0, 4.0], 500),
         ("linear_rows", 40, 3, 7, [3.0], 600))


def _rot(g):
    """a random rotation (QR of a Gaussian matrix, det +1)"""
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    return q * torch.sign(torch.linalg.det(q))


def make_inputs(name, G, K, T, ts, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = dict(means=2.0 * torch.rand(G, 3, generator=g, dtype=torch.float64) - 1.0, motion_coefs=rn(G, K), scales=-3.0 + 0.7 * rn(G, 3),
             rots=torch.tensor([1.0, 0, 0, 0, 1, 0], dtype=torch.float64) + 0.3 * rn(K, T, 6), transls=0.8 * rn(K, T, 3))
    B = len(ts)
    w2cs = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    for b in range(B):
        w2cs[b, :3, :3] = _rot(g)
        w2cs[b, :3, 3] = torch.tensor([0.0, 0.0, 7.0], dtype=torch.float64) + 0.5 * rn(3)  # the scene ~7 in front of the camera
    if name == "block_edges":  # one camera whose 3x3 part is not orthonormal: the centre is -A^-1 t, not -A^T t
        w2cs[1, :3, :3] += 0.15 * rn(3, 3)
    if name == "static_bases":  # every basis constant in time
        c["rots"] = c["rots"][:, :1].expand(K, T, 6).clone()
        c["transls"] = c["transls"][:, :1].expand(K, T, 3).clone()
    if name == "linear_rows":  # exact midpoints of small dyadic rationals: rows (basis 0, frame 2) of transls and (basis 1, frame 3) of rots
        dy = lambda *s: torch.randint(-32, 33, s, generator=g).double() / 16.0
        a, b_ = dy(3), dy(3)
        c["transls"][0, 1], c["transls"][0, 3], c["transls"][0, 2] = a, b_, (a + b_) / 2
        a, b_ = dy(6) / 4 + c["rots"].new_tensor([1.0, 0, 0, 0, 1, 0]), dy(6) / 4 + c["rots"].new_tensor([1.0, 0, 0, 0, 1, 0])
        c["rots"][1, 2], c["rots"][1, 4], c["rots"][1, 3] = a, b_, (a + b_) / 2
    c["ts"], c["w2cs"] = torch.tensor(ts, dtype=torch.float64), w2cs
    return {k: v.float().double() for k, v in c.items()}  # what fp32 holds


def reference_flow(ref, MotionBases, c):
    """-> the four terms, the deformed means at the three neighbour times [G,3,B,3] (the layout compute_z_acc_loss takes) and the
    leaves (the bases' are the reference module's own parameters).  Three functions of the reference are called -
    MotionBases.compute_transforms, compute_se3_smoothness_loss, compute_z_acc_loss; the rest is written here."""
    bases = MotionBases(c["rots"].detach().clone(), c["transls"].detach().clone())
    c = dict(c, rots=bases.params["rots"], transls=bases.params["transls"])
    last_interior = c["rots"].shape[1] - 2
    centre_times = c["ts"].clamp(1, last_interior)
    offsets = torch.tensor([-1.0, 0.0, 1.0], dtype=centre_times.dtype)
    times = (offsets[:, None] + centre_times[None, :]).reshape(-1)  # the B times before, the B times at, the B times after
    tf = bases.compute_transforms(times, torch.softmax(c["motion_coefs"], -1))  # [G, 3B, 3, 4] = [R | t]
    deformed = (tf[..., :3] @ c["means"][:, None, :, None]).squeeze(-1) + tf[..., 3]
    groups = deformed.unflatten(1, (3, -1))  # [G, 3, B, 3]
    m0, m1, m2 = groups.unbind(1)
    accel = 2 * m1 - m0 - m2
    smooth_tracks = torch.linalg.vector_norm(accel, dim=-1).mean() / 2  # (its gradient at an exact zero is zero)
    smooth_bases = ref["compute_se3_smoothness_loss"](c["rots"], c["transls"])
    z_accel = ref["compute_z_acc_loss"](groups, c["w2cs"])
    centred = c["scales"] - c["scales"].mean(-1, keepdim=True)
    scale_var = (centred.square().sum(-1) / (c["scales"].shape[-1] - 1)).mean()
    return (smooth_bases, smooth_tracks, z_accel, scale_var), groups, c


def zero_rows(name, K, T):
    """boolean [K, T-2] masks of the basis rows that are zero by design: (rots, transls)"""
    zr, zt = torch.zeros(K, T - 2, dtype=torch.bool), torch.zeros(K, T - 2, dtype=torch.bool)
    if name == "static_bases":
        zr[:], zt[:] = True, True
    if name == "linear_rows":
        zt[0, 2 - 1], zr[1, 3 - 1] = True, True
    return zr, zt


def well_conditioned(name, c, means_nbs):
    K, T = c["rots"].shape[:2]
    accel = lambda x: torch.linalg.vector_norm(torch.diff(x, n=2, dim=1), dim=-1)  # |second difference| along the time axis
    zr, zt = zero_rows(name, K, T)
    ar, at = accel(c["rots"]), accel(c["transls"])
    if not (bool((ar[zr] == 0).all()) and bool((at[zt] == 0).all())):
        return False
    if (ar[~zr].numel() and ar[~zr].min() < 0.05) or (at[~zt].numel() and at[~zt].min() < 0.05):
        return False
    a = accel(means_nbs)[:, 0]
    if name == "static_bases":
        if not bool((a == 0).all()):
            return False
    elif a.min() < 0.05:
        return False
    centres = torch.linalg.inv(c["w2cs"])[:, :3, 3]
    if torch.linalg.vector_norm(means_nbs[:, 1] - centres, dim=-1).min() < 0.5:
        return False
    return bool(c["means"].abs().max() <= 4.0) and bool(means_nbs.abs().max() <= 4.0)


def write_npz(dst, arrays):
    """np.savez_compressed with fixed timestamps: byte-identical output for identical arrays"""
    with zipfile.ZipFile(dst, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    gen_golden.REF = os.environ["D4GS_REFERENCE"]
    MotionBases = gen_golden._import_reference()[1]
    ref = load_reference()
    arrays = {}
    for name, G, K, T, ts, seed in CASES:
        for attempt in range(200):
            c = make_inputs(name, G, K, T, ts, seed + attempt)
            with torch.no_grad():
                _, nbs, _ = reference_flow(ref, MotionBases, c)
            if well_conditioned(name, c, nbs):
                break
        else:
            raise SystemExit(f"{name}: no well-conditioned seed")
        for k in ("means", "motion_coefs", "scales"):
            c[k].requires_grad_()
        terms, _, c = reference_flow(ref, MotionBases, c)
        grads = torch.autograd.grad(sum(w * t for w, t in zip(MIX, terms)), [c[k] for k in LEAVES], retain_graph=True)
        if name == "static_bases":  # exact zeros, values and gradients (the scale term has its own)
            assert all(float(t.detach()) == 0.0 for t in terms[:3]), terms
            assert all(bool((g == 0).all()) for k, g in zip(LEAVES, grads) if k != "scales")
        assert all(bool(torch.isfinite(g).all()) for g in grads), name
        for k in LEAVES + ("ts", "w2cs"):
            arrays[f"{name}/{k}"] = c[k].detach().numpy().astype(np.float32)
        for t_name, t in zip(TERMS, terms):
            arrays[f"{name}/{t_name}"] = t.detach().numpy()
        for k, g in zip(LEAVES, grads):
            arrays[f"{name}/grad/{k}"] = g.numpy()
        if name == "block_edges":  # each term's own gradients (a term that does not reach a leaf: zeros)
            for t_name, t in zip(TERMS, terms):
                own = torch.autograd.grad(t, [c[k] for k in LEAVES], retain_graph=True, allow_unused=True)
                for k, g in zip(LEAVES, own):
                    arrays[f"{name}/grad_{t_name}/{k}"] = (torch.zeros_like(c[k]) if g is None else g).numpy()
        print(name, f"seed {seed + attempt}", [float(t.detach()) for t in terms], file=sys.stderr)
    dst = os.path.join(HERE, "motion_regs.npz")
    write_npz(dst, arrays)
    print(f"{len(arrays)} arrays -> {dst} ({os.path.getsize(dst)} bytes)", file=sys.stderr)
