"""The forward composite's block filter (csrc/raster_fwd.hip, D4GS_BLOCK_FILTER): after a wave has built its four rows' lists of a
staged batch with the alpha >= 1/255 BOX test, the listed (splat, 4x4 block) pairs are tested with the exact ellipse test
(csrc/common.h: d4gs_block_filter_keep) and the survivors written back in place.  It may only remove steps in which no pixel of the
block passes, so with the filter on and off every output and every gradient must be BITWISE equal - and the device test itself,
reached through the A/B build's d4gs_test_block_filter, must never drop a pair that fp64 brute force over the block's 16 pixel
centres finds a valid pixel in.  (The one-call path keeps last_ids / final_T inside its workspace: there the renders, the alphas and
the gradients, which are computed from both, stand for them.)"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests.util import static_inputs

pytestmark = pytest.mark.gpu
LEAVES = ("means", "quats", "scales", "opac", "colors", "V")


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _render(inp, W, H, D, fused, lazy):
    from deblur4dgs_amd.exposure import render_exposure

    dev = torch.device("cuda:0")
    t = {k: v.to(torch.float32).to(dev) for k, v in inp.items()}
    for k in LEAVES:
        t[k].requires_grad_()
    r = render_exposure(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], 0, None, None, None, None, None, t["V"], t["K"],
                        W, H, background=torch.linspace(0.2, 0.8, D).to(dev), return_depth=True, blend=False, raw_params=False,
                        fused=fused, lazy_sort=lazy, near_target=300 if lazy else 0)
    assert bool(r["state"].frame_io) == fused
    g = torch.Generator().manual_seed(3)
    w = torch.randn(r["renders"].shape, generator=g).to(dev)
    ((r["renders"] * w).sum() + r["alphas"].sum()).backward()
    torch.cuda.synchronize()
    out = dict(renders=r["renders"], alphas=r["alphas"], **{f"g_{k}": t[k].grad for k in LEAVES})
    if not fused:
        out.update(final_T=r["state"].raster["final_T"], last_ids=r["state"].raster["last_ids"])
    return {k: _bits(v).clone() for k, v in out.items()}


def _on_equals_off(inp, W, H, D, fused, lazy, monkeypatch):
    res = {}
    for flt in ("1", "0"):
        monkeypatch.setenv("D4GS_BLOCK_FILTER", flt)
        res[flt] = _render(inp, W, H, D, fused, lazy)
    for k, a in res["1"].items():
        assert torch.equal(a, res["0"][k]), k
    assert int((res["1"]["g_means"] != 0).sum()) > 0 and float(res["1"]["alphas"].view(torch.float32).max()) > 0
    return res["1"]


@pytest.mark.parametrize("fused", [False, True], ids=["staged", "onecall"])
@pytest.mark.parametrize("lazy", [False, True], ids=["whole", "lazy"])
@pytest.mark.parametrize("seg", ["0", "1"], ids=["seg0", "seg1"])
@pytest.mark.parametrize("D", [3, 16])
@pytest.mark.parametrize("scale_mul", [1.0, 4.0])
def test_filter_on_equals_filter_off_bitwise(scale_mul, D, seg, lazy, fused, monkeypatch):
    monkeypatch.setenv("D4GS_SEG", seg)
    W, H, N = 256, 160, 6000
    inp = static_inputs(N, W, H, seed=31 + D, dtype=torch.float32, D=D, scale_mul=scale_mul)
    if lazy:
        inp["opac"] = torch.full_like(inp["opac"], 0.97)
    _on_equals_off(inp, W, H, D, fused, lazy, monkeypatch)


# ---- hand-built edge scenes -------------------------------------------------------------------------------------------------------
EW, EH, EF, EZ = 70, 50, 64.0, 4.0  # image, focal length, depth of the first splat: pixel p <- x = (p - centre) * EZ / EF, exact in fp32


def _edge_scene():
    """<= 64 splats on a 70x50 image (partial edge tiles): (pixel centre, angle, major / minor std in pixels, opacity or None = set
    from the projected conic below)."""
    rows = []
    for ang in (45.0, 135.0):
        for c in ((24.0, 20.0), (40.0, 28.0), (16.0, 32.0)):      # block corners (x, y multiples of 4), one of them a tile corner
            rows.append((c, ang, 12.0, 1.1, 0.6))
        for c in ((26.0, 20.0), (24.0, 22.0), (42.5, 16.0)):      # block edges
            rows.append((c, ang, 12.0, 1.1, 0.6))
        for c in ((24.0, 20.0), (44.0, 12.0), (26.0, 24.0), (52.0, 30.0)):  # the alpha = 1/255 contour next to a pixel centre: both sides
            rows.append((c, ang, 9.0, 0.85, None))
            rows.append((c, ang, 9.0, 0.85, None))
        rows.append(((20.0, 24.0), ang, 12.0, 1.1, (1.0 + 1e-3) / 255.0))   # tau barely positive
        rows.append(((36.0, 12.0), ang, 12.0, 1.1, 1.05 / 255.0))
        rows.append(((28.0, 36.0), ang, 12.0, 1.1, 1.0 / 255.0))            # tau = 0.02: the margin alone
        rows.append(((48.0, 20.0), ang, 12.0, 1.1, 0.999))                  # the alpha clamp
        rows.append(((12.0, 12.0), ang, 10.0, 1.1, 1.0))
        for c in ((-6.0, 10.0), (75.0, 55.0), (35.0, -8.0), (17.0, 15.0), (-20.0, -20.0)):  # outside the image / in the neighbouring tile
            rows.append((c, ang, 14.0, 1.3, 0.8))
    return rows


def _edge_inputs(rows, opac_override=None):
    n = len(rows)
    means, quats, scales, opac = torch.zeros(n, 3), torch.zeros(n, 4), torch.zeros(n, 3), torch.zeros(n)
    for i, (c, ang, smaj, smin, o) in enumerate(rows):
        z = EZ + 0.25 * i  # distinct depths (all dyadic)
        means[i] = torch.tensor([(c[0] - EW / 2) * z / EF, (c[1] - EH / 2) * z / EF, z])
        quats[i] = torch.tensor([math.cos(math.radians(ang) / 2), 0.0, 0.0, math.sin(math.radians(ang) / 2)])
        scales[i] = torch.tensor([smaj * z / EF, smin * z / EF, 1e-3])
        opac[i] = 0.5 if o is None else o
    # a degenerate conic: a needle 3 000 x 1e-4 px at 45 degrees - the fp32 determinant of its covariance (true value 1e-7 of the
    # product it is the difference of) is rounding noise, <= 0 or not
    means = torch.cat([means, torch.tensor([[0.0, 0.0, 4.0]])])
    quats = torch.cat([quats, torch.tensor([[math.cos(math.pi / 8), 0.0, 0.0, math.sin(math.pi / 8)]])])
    scales = torch.cat([scales, torch.tensor([[3000.0 * 4.0 / EF, 1e-4 * 4.0 / EF, 1e-6]])])
    opac = torch.cat([opac, torch.tensor([0.5])])
    if opac_override is not None:
        opac = opac_override
    g = torch.Generator().manual_seed(5)
    K = torch.tensor([[EF, 0.0, EW / 2], [0.0, EF, EH / 2], [0.0, 0.0, 1.0]])
    return dict(means=means, quats=quats, scales=scales, opac=opac, colors=torch.rand(n + 1, 3, generator=g), V=torch.eye(4), K=K)


def _contour_opacities(rows, inp):
    """For the rows with opacity None, in pairs: the opacity at which the alpha = 1/255 contour passes 5e-4 px outside / inside the
    centre of a pixel of a block diagonal to the splat's centre (fp64, from the projection's own fp32 conics and centres)."""
    from deblur4dgs_amd.rasterization import rasterization

    dev = torch.device("cuda:0")
    t = {k: v.to(dev) for k, v in inp.items()}
    _, _, info = rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"][None], t["K"][None], EW, EH)
    torch.cuda.synchronize()
    con, m2d = info["conics"][0].double().cpu(), info["means2d"][0].double().cpu()
    opac, side, found = inp["opac"].clone(), {}, 0
    ys, xs = np.mgrid[0:EH, 0:EW]
    for i, row in enumerate(rows):
        if row[4] is not None:
            continue
        a, b, c = con[i].tolist()
        mx, my = m2d[i].tolist()
        u, v = xs + 0.5 - mx, ys + 0.5 - my
        sig = 0.5 * (a * u * u + c * v * v) + b * u * v
        diag = ((xs // 4) != math.floor(mx / 4) if mx % 4 else np.ones_like(xs, bool)) & \
               ((ys // 4) != math.floor(my / 4) if my % 4 else np.ones_like(ys, bool))
        cand = np.argwhere(diag & (sig > 0.7) & (sig < 5.0))
        assert len(cand) > 0, i
        s = side[row[0], row[1]] = -side.get((row[0], row[1]), -1)  # +1 then -1 for the two copies
        py, px = cand[(7 * int(row[0][0] + row[0][1] + row[1])) % len(cand)]  # (the same pixel for both copies)
        grad = math.hypot(a * u[py, px] + b * v[py, px], b * u[py, px] + c * v[py, px])
        opac[i] = math.exp(sig[py, px] + s * 5e-4 * grad) / 255.0
        assert 1 / 255 < opac[i] < 0.999
        found += 1
    assert found == 16
    return opac


def test_hand_built_edge_scenes_filter_on_equals_off(monkeypatch):
    rows = _edge_scene()
    assert len(rows) + 1 <= 64
    inp = _edge_inputs(rows)
    inp = _edge_inputs(rows, _contour_opacities(rows, inp))
    for seg in ("0", "1"):
        monkeypatch.setenv("D4GS_SEG", seg)
        for fused in (False, True):
            out = _on_equals_off(inp, EW, EH, 3, fused, False, monkeypatch)
    assert float(out["alphas"].view(torch.float32).min()) < 0.5  # thin splats: most of the image stays open


# ---- the device test against brute force -------------------------------------------------------------------------------------------
def _pairs(n, seed, thin):
    """(splat, block) pairs [n, 10] fp32: centre, opacity, conic a b c, the block's pixel-centre rectangle X0 X1 Y0 Y1."""
    g = np.random.default_rng(seed)
    smaj = g.uniform(6.0, 15.0, n) if thin else np.exp(g.uniform(math.log(0.6), math.log(15.0), n))
    smin = smaj / 10.0 if thin else smaj / np.exp(g.uniform(0.0, math.log(12.0), n))
    th = np.radians(g.choice([45.0, 135.0], n)) if thin else g.uniform(0, math.pi, n)
    cs, sn = np.cos(th), np.sin(th)
    v1, v2 = smaj ** 2, smin ** 2 + 0.3
    sxx, syy, sxy = v1 * cs * cs + v2 * sn * sn, v1 * sn * sn + v2 * cs * cs, (v1 - v2) * cs * sn
    det = sxx * syy - sxy * sxy
    a, b, c = syy / det, -sxy / det, sxx / det
    opac = np.where(g.random(n) < 0.2, g.choice([1.0 / 255, 1.001 / 255, 1.05 / 255, 0.999, 1.0], n), g.uniform(0.004, 1.0, n))
    mx, my = g.uniform(0, 64, n), g.uniform(0, 64, n)
    snap = g.random(n)
    mx, my = np.where(snap < 0.3, np.round(mx / 4) * 4, mx), np.where((snap < 0.2) | (snap > 0.9), np.round(my / 4) * 4, my)
    reach = np.sqrt(2 * np.log(255 * np.maximum(opac, 1.01 / 255)) * v1) + 4  # blocks within the major axis' reach (and a little beyond)
    bx = np.floor((mx + g.uniform(-1, 1, n) * reach) / 4)
    by = np.floor((my + g.uniform(-1, 1, n) * reach) / 4)
    X0, Y0 = 4 * bx + 0.5, 4 * by + 0.5
    return np.stack([mx, my, opac, a, b, c, X0, X0 + 3, Y0, Y0 + 3], 1).astype(np.float32)


def _brute(rec):
    """Has the block a pixel the composite would take?  fp64 over the 16 pixel centres from the fp32 inputs: sigma >= 0 and
    alpha = min(0.999, opacity exp(-sigma)) >= 1/255."""
    r = rec.astype(np.float64)
    hit = np.zeros(len(r), bool)
    for i in range(4):
        for j in range(4):
            u, v = r[:, 6] + i - r[:, 0], r[:, 8] + j - r[:, 1]
            sig = 0.5 * (r[:, 3] * u * u + r[:, 5] * v * v) + r[:, 4] * u * v
            hit |= (sig >= 0) & (np.minimum(0.999, r[:, 2] * np.exp(-sig)) >= 1.0 / 255.0)
    return hit


def _device_keep(rec):
    from deblur4dgs_amd import build

    assert os.path.exists(build.VARIANTS_LIB), "run __graft_entry__.build() (builds tests/libd4gs_variants.so)"
    lib = C.CDLL(build.VARIANTS_LIB)
    lib.d4gs_test_block_filter.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.d4gs_test_block_filter.restype = C.c_int
    dev = torch.device("cuda:0")
    rd = torch.from_numpy(rec).to(dev).contiguous()
    keep = torch.full((len(rec),), -1, dtype=torch.int32, device=dev)
    assert lib.d4gs_test_block_filter(len(rec), rd.data_ptr(), keep.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    k = keep.cpu().numpy()
    assert ((k == 0) | (k == 1)).all()
    return k == 1


def _edge_pairs():
    """The edge scenes' splats (nominal 2-D shapes) against every block of their 70x50 image's tiles."""
    out = []
    for (c, ang, smaj, smin, o) in _edge_scene():
        th = math.radians(ang)
        v1, v2 = smaj ** 2, smin ** 2 + 0.3
        sxx, syy = v1 * math.cos(th) ** 2 + v2 * math.sin(th) ** 2, v1 * math.sin(th) ** 2 + v2 * math.cos(th) ** 2
        sxy = (v1 - v2) * math.cos(th) * math.sin(th)
        det = sxx * syy - sxy * sxy
        for o_ in ([o] if o is not None else [0.02, 0.3]):
            for by in range(0, 16):
                for bx in range(0, 20):
                    out.append([c[0], c[1], o_, syy / det, -sxy / det, sxx / det, 4 * bx + 0.5, 4 * bx + 3.5, 4 * by + 0.5, 4 * by + 3.5])
    return np.asarray(out, np.float32)


def test_device_test_never_drops_a_block_with_a_valid_pixel():
    sets = dict(random=_pairs(6000, 1, thin=False), thin=_pairs(3000, 2, thin=True), edge=_edge_pairs())
    shares = {}
    for name, rec in sets.items():
        hit = _brute(rec)
        assert hit.sum() >= 300 and (~hit).sum() >= 300, (name, hit.sum(), len(rec))  # the generator yields both kinds
        keep = _device_keep(rec)
        wrong = np.flatnonzero(hit & ~keep)
        assert len(wrong) == 0, (name, len(wrong), rec[wrong[:5]])
        shares[name] = float((~keep & ~hit).sum()) / float((~hit).sum())
        print(f"block filter, {name}: {len(rec)} pairs, {int(hit.sum())} with a valid pixel, "
              f"{int((~keep).sum())} dropped = {shares[name]:.3f} of the empty ones")
    assert shares["thin"] > 0 and shares["edge"] > 0
