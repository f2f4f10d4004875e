"""Scenes of the per-row gradient comparison, shared by the CPU test (tests/test_row_cases.py) and the GPU tests
(tests/test_gpu_row_parity.py) so that both see the same tensors.  Not a conftest: plain data plus builders, cached; the only product
code imported is the seeded scene generator the other parity tests use.

WHY ROWS.  tests/util.py `check` measures max|got - ref| / max|ref| over a whole tensor.  Per-Gaussian gradients are heavy-tailed: a few
large, bright splats set max|ref|, the median row sits 1.3 - 2.4 decades below it (quats: the lowest decile 3.5), so "1e-4 of the tensor"
holds most Gaussians to percents of their own size.  `check_rows` holds every row to its own scale; these are the scenes it is asked on.

EVERY CASE gives fp64 inputs, named row groups (index tensors) and - from `*_reference` - for both cotangent kinds the gradient of
every per-Gaussian tensor from the fp64 oracle and from the SAME oracle evaluated in fp32 (the yardstick), with the cotangents zeroed on
the fragile pixels F of oracle/margins.py (eps = 1e-4) on every side, as tests/test_gpu_flip_cause.py takes them.

  S1 random    `static_inputs` N = 600 on 64 x 48 (two tiles by a ragged third: every quadrant path): RGB+ED D = 3, RGB D = 8,
               RGB+ED D = 16 (the matrix-pipe backward), RGB+ED D = 3 with scale_mul = 8 (long lists)
  S1 strata    one hand-built scene, 616 Gaussians on 96 x 64, the groups in separate regions of the image:
                 big       large, opaque, saturated: they set every tensor's maximum
                 subpixel  projected sigma below 0.3 px: eps2d dominates the conic
                 needle    scale ratios 50 : 1 at random orientations
                 border    centres up to one radius outside an image edge
                 clamped   |x / z| (|y / z|) beyond the Jacobian clamp 1.3 (W / 2) / fx, large enough to reach into the image
                 faint     opacity 0.02 ... 0.05
                 tail      the last N mod 64 rows (the ragged group of the per-Gaussian kernels), spread under all the others as a far, soft
                           backdrop.  It is there for a reason found while building the scene: where only the rim of one small splat covers
                           a pixel, the accumulated alpha is near 1 / 255 and the gradient of the expected-depth channel sum(w z) / alpha is
                           a difference of two terms of size z / alpha - the fp32 ORACLE alone then has a fifth of the sub-pixel rows beyond
                           1e-4 of themselves (RGB alone: none).  No fp32 evaluation can be held to the caps there, so the scene has none.
  fused        `make_scene` through render_exposure (scales + 1.2, cam_jitter = 0.01, 64 x 48), one case per k_project_bwd
               instantiation and both sides of its K > 8 switch; groups dynamic (rows < G) / static (rows >= G)
"""
from __future__ import annotations

import functools

import torch

from oracle import margins, raster
from oracle import scene as oscene
from tests.util import static_inputs

EPS = 1e-4             # fragile pixels: decisions within this (relative) of their thresholds
MAX_FRAGILE = 0.05     # F may be at most this share of the pixels
KINDS = ("randn", "positive")
S1_TENSORS = ("means", "quats", "scales", "opac", "colors")
PROJ_TENSORS = ("means2d", "conics", "depths", "opacities")
FUSED_TENSORS = ("means", "quats", "scales", "colors", "opacities", "motion_coefs")

# Seeds (here, FUSED, STRATA_SEED): on each the fp32 oracle ALONE keeps half of every cap of tests/util.check_rows with room to spare
# (tests/test_row_cases.py asserts the half); a seed that could not was replaced, never a cap.
# name -> (mode, D, N, W, H, scale_mul, seed)
S1_RANDOM = {
    "rgbed3": ("RGB+ED", 3, 600, 64, 48, 3.0, 7112),
    "rgb8": ("RGB", 8, 600, 64, 48, 3.0, 7102),
    "rgbed16": ("RGB+ED", 16, 600, 64, 48, 3.0, 7104),
    "rgbed3_long": ("RGB+ED", 3, 600, 64, 48, 8.0, 7104),
}
STRATA = "strata"
S1_CASES = tuple(S1_RANDOM) + (STRATA,)
STRATA_N, STRATA_W, STRATA_H, STRATA_SEED = 616, 96, 64, 1
STRATA_GROUPS = ("big", "subpixel", "needle", "border", "clamped", "faint", "tail")

# name -> (N, G, K, S, seed): the k_project_bwd<MODE_RENDER, MFMA = K > 8, SL> instantiation each one takes
FUSED = {
    "valu_sl4": (700, 450, 6, 3, 11),
    "mfma_sl1": (650, 650, 12, 1, 4),
    "mfma_sl2": (700, 300, 20, 2, 2),
    "k8_sl4": (600, 600, 8, 4, 15),
    "k9_sl4": (600, 600, 9, 4, 32),
}
FUSED_W, FUSED_H = 64, 48


def eps_px(W, H):
    return 32 * 6e-8 * max(W, H)  # float32 evaluates a projected centre to a few ulp of the image size


def cotangents(kind: str, H: int, W: int, C: int, seed: int = 9):
    """-> (w_c [H,W,C], w_a [H,W,1]) fp64.  randn: as the parity tests draw them.  positive: smooth, in [0.5, 1.5] at every pixel and
    channel (1 + 0.5 ramp_c sin(0.37 x + 0.21 y + c), ramp_c from 0.5 to 1) - no cancellation between a colour row's pixels."""
    if kind == "randn":
        g = torch.Generator().manual_seed(seed)
        return torch.randn(H, W, C, generator=g, dtype=torch.float64), torch.randn(H, W, 1, generator=g, dtype=torch.float64)
    assert kind == "positive"
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    c = torch.arange(C, dtype=torch.float64)
    ramp = torch.linspace(0.5, 1.0, C, dtype=torch.float64)
    w_c = 1.0 + 0.5 * ramp * torch.sin(0.37 * x[..., None] + 0.21 * y[..., None] + c)
    w_a = 1.0 + 0.5 * torch.sin(0.29 * x - 0.33 * y)[..., None]
    return w_c, w_a


# ---- seam S1 ------------------------------------------------------------------------------------------------
def _strata_inputs(seed=STRATA_SEED):
    """The hand-built scene: camera at the origin looking down +z, fx = fy = W; every Gaussian is placed by its pixel and depth."""
    W, H, N = STRATA_W, STRATA_H, STRATA_N
    fx = fy = float(W)
    cx, cy = W / 2, H / 2
    g = torch.Generator().manual_seed(seed)
    u = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)
    n_of = dict(big=36, subpixel=100, needle=120, border=110, clamped=90, faint=120, tail=N % 64)
    assert sum(n_of.values()) == N
    px, py, z, sig, op, col, ratio = [], [], [], [], [], [], []

    def add(n, x, y, depth, sigma_px, opacity, colour=None, needle=False):
        px.append(x), py.append(y), z.append(depth), sig.append(sigma_px), op.append(opacity)
        col.append(torch.sigmoid(torch.randn(n, 3, generator=g, dtype=torch.float64)) if colour is None else colour)
        ratio.append(torch.full((n,), 50.0 if needle else 1.0, dtype=torch.float64))

    n = n_of["big"]      # upper right of the interior, near the camera (the world gradients carry fx / z)
    add(n, u(n, 60, 82), u(n, 10, 30), u(n, 0.6, 1.0), u(n, 3.0, 5.0), u(n, 0.9, 0.99),
        colour=torch.where(torch.rand(n, 3, generator=g) < 0.5, 0.02, 0.98).double())
    n = n_of["subpixel"]  # upper left: eps2d makes every one of them a blob of sigma ~0.55 px
    add(n, u(n, 14, 52), u(n, 9, 31), u(n, 11.0, 16.0), u(n, 0.05, 0.28), u(n, 0.3, 0.8))
    n = n_of["needle"]    # lower left
    add(n, u(n, 14, 44), u(n, 38, 55), u(n, 12.0, 16.0), u(n, 1.5, 3.0), u(n, 0.25, 0.6), needle=True)
    n = n_of["border"]    # the first half of every edge, centres outside by a fraction of the radius
    side = torch.arange(n) % 4
    sg = u(n, 2.0, 3.5)
    rad = torch.ceil(3.0 * torch.sqrt(sg * sg + 0.3))
    out = u(n, 0.05, 0.9) * rad
    along = u(n, 0.0, 1.0)
    bx = torch.where(side == 0, -out, torch.where(side == 1, W + out, torch.where(side == 2, 4 + along * (W / 2 - 8), W / 2 + 4 + along * (W / 2 - 8))))
    by = torch.where(side == 0, 4 + along * (H / 2 - 8), torch.where(side == 1, H / 2 + 4 + along * (H / 2 - 8), torch.where(side == 2, -out, H + out)))
    add(n, bx, by, u(n, 8.0, 14.0), sg, u(n, 0.4, 0.8))
    n = n_of["clamped"]   # the other half of every edge, beyond 1.3 x the half field of view
    side = torch.arange(n) % 4
    beyond = u(n, 1.32, 1.5)
    along = u(n, 0.0, 1.0)
    kx = torch.where(side == 0, cx + beyond * W / 2, torch.where(side == 1, cx - beyond * W / 2, torch.where(side == 2, W / 2 + 6 + along * (W / 2 - 12), 6 + along * (W / 2 - 12))))
    ky = torch.where(side == 0, 4 + along * (H / 2 - 8), torch.where(side == 1, H / 2 + 4 + along * (H / 2 - 8), torch.where(side == 2, cy - beyond * H / 2, cy + beyond * H / 2)))
    add(n, kx, ky, u(n, 8.0, 14.0), u(n, 7.0, 10.0), u(n, 0.1, 0.25))
    n = n_of["faint"]     # lower right
    add(n, u(n, 50, 82), u(n, 36, 55), u(n, 8.0, 14.0), u(n, 1.5, 3.0), u(n, 0.02, 0.05))
    n = n_of["tail"]      # a far, soft backdrop under all of them: a pixel that only the rim of one small splat covers has an accumulated alpha
    #                       near 1 / 255, where the expected-depth channel sum(w z) / alpha is a difference of two terms of z / alpha in float32
    add(n, u(n, 10, 86), u(n, 6, 58), u(n, 15.0, 18.0), u(n, 6.0, 9.0), u(n, 0.4, 0.6))

    px, py, z, sig, op, col, ratio = (torch.cat(v) for v in (px, py, z, sig, op, col, ratio))
    means = torch.stack([(px - cx) * z / fx, (py - cy) * z / fy, z], -1)
    s0 = sig * z / fx  # world scale of the longest axis: sigma_px at the image centre
    scales = s0[:, None] * torch.stack([torch.ones_like(ratio), 1.0 / ratio, 1.0 / ratio], -1)
    scales = scales * torch.where(ratio[:, None] > 1, torch.ones(N, 3, dtype=torch.float64), u(N * 3, 0.7, 1.0).view(N, 3))
    quats = torch.randn(N, 4, generator=g, dtype=torch.float64)
    inp = dict(means=means, quats=quats, scales=scales, opac=op, colors=col, V=torch.eye(4, dtype=torch.float64),
               K=torch.tensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=torch.float64))
    groups, at = {}, 0
    for name in STRATA_GROUPS:
        groups[name] = torch.arange(at, at + n_of[name])
        at += n_of[name]
    return inp, groups


@functools.lru_cache(maxsize=None)
def s1_case(name: str):
    """-> dict(name, mode, D, N, W, H, bg [D], inp (fp64: means, quats, scales, opac, colors, V, K), groups {name: row indices})."""
    if name == STRATA:
        inp, groups = _strata_inputs()
        mode, D, N, W, H = "RGB+ED", 3, STRATA_N, STRATA_W, STRATA_H
    else:
        mode, D, N, W, H, scale_mul, seed = S1_RANDOM[name]
        inp = static_inputs(N, W, H, seed=seed, dtype=torch.float64, D=D, scale_mul=scale_mul)
        groups = {}
    return dict(name=name, mode=mode, D=D, N=N, W=W, H=H, bg=torch.linspace(0.1, 0.9, D, dtype=torch.float64), inp=inp, groups=groups)


def _s1_oracle(case, dtype, cots):
    """The oracle in `dtype` -> (info, {kind: {tensor: grad}}); cots = {kind: (w_c, w_a)} already masked."""
    W, H = case["W"], case["H"]
    t = {k: v.to(dtype).clone().requires_grad_(k in S1_TENSORS) for k, v in case["inp"].items()}
    rc, ra, info = raster.rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"], t["K"], W, H,
                                        background=case["bg"].to(dtype), render_mode=case["mode"])
    grads = {}
    for kind, (w_c, w_a) in cots.items():
        gs = torch.autograd.grad((rc * w_c.to(dtype)).sum() + (ra * w_a.to(dtype)).sum(), [t[k] for k in S1_TENSORS], retain_graph=True)
        grads[kind] = dict(zip(S1_TENSORS, gs))
    proj = dict(radii=info["radii"], means2d=info["means2d"].detach(), conics=info["conics"].detach(), depths=info["depths"].detach(),
                opacities=torch.where(info["radii"] > 0, t["opac"].detach(), torch.zeros_like(t["opac"].detach())))
    return info, grads, proj


@functools.lru_cache(maxsize=None)
def s1_reference(name: str):
    """-> dict(F [H,W] bool, cot {kind: (w_c, w_a)} zeroed on F, g64 / g32 {kind: {tensor: grad}}, proj64 / proj32 {radii, means2d,
    conics, depths, opacities}).  Computed once per session; nobody writes into it."""
    case = s1_case(name)
    inp, W, H = case["inp"], case["W"], case["H"]
    with torch.no_grad():
        _, _, info = raster.rasterization(inp["means"], inp["quats"], inp["scales"], inp["opac"], inp["colors"], inp["V"], inp["K"], W, H,
                                          background=case["bg"], render_mode=case["mode"])
    m = margins.pixel_margins(info["means2d"], info["conics"], inp["opac"], info["depths"], info["flatten_ids"], info["isect_offsets"], W, H)
    toggles, _ = margins.gaussian_toggle_mask(inp["means"], inp["quats"], inp["scales"], inp["opac"], inp["V"], inp["K"], W, H, eps_px=eps_px(W, H))
    F = margins.fragile_pixels(m, EPS) | toggles
    keep = (~F).double()[..., None]
    C = case["D"] + (case["mode"] != "RGB")
    cot = {kind: tuple(w * keep for w in cotangents(kind, H, W, C)) for kind in KINDS}
    _, g64, proj64 = _s1_oracle(case, torch.float64, cot)
    _, g32, proj32 = _s1_oracle(case, torch.float32, cot)
    return dict(F=F, cot=cot, g64=g64, g32=g32, proj64=proj64, proj32=proj32)


# ---- the fused path -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused_case(name: str):
    """-> dict(name, N, G, K, S, W, H, sc (make_scene's fp64 dict, scales + 1.2), mask (the mask channel is rendered), groups)."""
    from deblur4dgs_amd.synth import make_scene

    N, G, K, S, seed = FUSED[name]
    W, H = FUSED_W, FUSED_H
    sc = make_scene(N, G, K, S, W, H, seed=seed, dtype=torch.float64, cam_jitter=0.01)
    sc["scales"] = sc["scales"] + 1.2  # big enough to overlap several pixels
    groups = dict(dynamic=torch.arange(0, G))
    if G < N:
        groups["static"] = torch.arange(G, N)
    return dict(name=name, N=N, G=G, K=K, S=S, W=W, H=H, sc=sc, mask=G < N, groups=groups)


def _fused_oracle(case, dtype, cots, spy=None):
    """oracle/scene.py render_exposure in `dtype` -> (out, {kind: {tensor: grad}}); cots = {kind: (w_b [H,W,C], w_a [H,W])} or a
    function of the output's channel count that makes them."""
    sc, G, N, W, H, S = case["sc"], case["G"], case["N"], case["W"], case["H"], case["S"]
    keys = ("means", "quats", "scales", "colors", "opacities")
    fg = {k: sc[k][:G].to(dtype).clone().requires_grad_() for k in keys}
    fg["motion_coefs"] = sc["motion_coefs"].to(dtype).clone().requires_grad_()
    bg = {k: sc[k][G:].to(dtype).clone().requires_grad_() for k in keys} if G < N else None
    bases = {k: sc[k].to(dtype) for k in ("rots", "transls")}
    orig = raster.project
    if spy is not None:
        raster.project = lambda *a, **kw: (spy(*a), orig(*a, **kw))[1]
    try:
        out = oscene.render_exposure(fg, bg, bases, sc["times"].to(dtype), sc["RTs"].to(dtype), sc["viewmat"].to(dtype), sc["K"].to(dtype),
                                     (W, H), bg_color=1.0, return_depth=True, return_mask=case["mask"], single=(S == 1))
    finally:
        raster.project = orig
    blended = torch.cat([out[k] for k in ("img", "mask", "depth") if k in out], -1)[0]
    if callable(cots):
        cots = cots(out, blended)
    parts = [p for p in (fg, bg) if p is not None]
    leaves = [p[k] for k in keys for p in parts] + [fg["motion_coefs"]]
    grads = {}
    for kind, (w_b, w_a) in cots.items():
        gs = list(torch.autograd.grad((blended * w_b.to(dtype)).sum() + (out["acc"][0, ..., 0] * w_a.to(dtype)).sum(), leaves, retain_graph=True))
        gd = {}
        for k in keys:
            gd[k] = torch.cat([gs.pop(0) for _ in parts], 0)
        gd["motion_coefs"] = gs.pop(0)
        grads[kind] = gd
    radii = torch.stack([inf["radii"] for inf in out["info"]], 0)  # [S,N]
    return cots, grads, radii


@functools.lru_cache(maxsize=None)
def fused_reference(name: str):
    """-> dict(F, cot {kind: (w_b [H,W,C], w_a [H,W])} zeroed on F, g64 / g32 {kind: {tensor: grad}}, radii64 / radii32 [S,N]).  F = the
    union over the sub-samples of their fragile pixels and toggling tiles, plus the pixels where the max / min blend channels tie."""
    case = fused_case(name)
    sc, G, W, H, S = case["sc"], case["G"], case["W"], case["H"], case["S"]
    opac_all = torch.sigmoid(sc["opacities"])
    calls = []

    def spy(means, quats, scales, viewmat, K, *a):
        calls.append((means.detach(), quats.detach(), scales.detach(), opac_all, viewmat.detach(), K.detach()))

    def make_cots(out, blended):
        assert len(calls) == S
        F = torch.zeros(H, W, dtype=torch.bool)
        for s in range(S):
            inf = out["info"][s]
            m = margins.pixel_margins(inf["means2d"].detach(), inf["conics"].detach(), opac_all, inf["depths"].detach(), inf["flatten_ids"],
                                      inf["isect_offsets"], W, H)
            F |= margins.fragile_pixels(m, EPS) | margins.gaussian_toggle_mask(*calls[s], W, H, eps_px=eps_px(W, H))[0]
        raw = torch.stack(out["raw_renders"], 0)[:, 0].detach()
        F |= margins.blend_tie_mask(torch.cat([raw[:-1], raw.mean(0, keepdim=True)], 0), eps=EPS)  # what the reference's max / min see
        keep = (~F).double()
        cot = {}
        for kind in KINDS:
            w_b, w_a = cotangents(kind, H, W, blended.shape[-1], seed=1)
            cot[kind] = (w_b * keep[..., None], w_a[..., 0] * keep)
        cot["F"] = F
        return cot

    holder = {}

    def first(out, blended):
        holder.update(make_cots(out, blended))
        return {k: holder[k] for k in KINDS}

    cot, g64, radii64 = _fused_oracle(case, torch.float64, first, spy=spy)
    _, g32, radii32 = _fused_oracle(case, torch.float32, cot)
    return dict(F=holder["F"], cot=cot, g64=g64, g32=g32, radii64=radii64, radii32=radii32)


def tensor_groups(case, tensor: str):
    """The row groups that index `tensor` (motion_coefs has G rows: the dynamic ones only)."""
    if tensor == "motion_coefs":
        return {}
    return case["groups"]


def below(ref: torch.Tensor, frac: float):
    """[N] bool: live rows whose largest |element| is below frac x the tensor's maximum."""
    top = ref.detach().double().reshape(ref.shape[0], -1).abs().amax(1)
    return (top > 0) & (top < frac * top.max())
