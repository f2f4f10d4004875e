"""Every instances-per-lane arm of k_count_tiles / k_emit (csrc/host.h, FrontPlan.pt) against a render that does not depend on the arm.

A static scene rendered with S = 64 sub-samples and no camera deltas is 64 times the same render, and the one-sub-sample render of the
scene always takes one instance per lane (fewer than 256 blocks).  So every sub-sample's image, alpha, radii, means2d and per-tile sorted
Gaussian ids must equal the S = 1 render's bit for bit, whichever arm the launch plan picked.  Depths are distinct, so no tie rule takes
part in the order of a list.

The rows: instances per lane by d4gs_front_plan's rule - 1 when ceil(N / 4096) * S < 256 blocks, else the fewest of 2 ... 6 with
ceil(N / (1024 pt)) * S <= 512, else 4; always 4 (after the first test) with lazy lists.  `_pt` below restates that rule only to check
that each N still reaches the arm it was chosen for.

      N      S   arm
    8 192   64   1    (128 blocks at 4 per lane)
   16 384   64   2    (8 chunks of 2 048: 512 blocks)
   16 385   64   3    (9 chunks at 2; 6 chunks of 3 072: 384 blocks)
   32 768   64   4    (chosen by the rule: 8 chunks of 4 096)
   40 000   64   5    (8 chunks of 5 120)
   49 152   64   6    (8 chunks of 6 144)
   49 153   64   4    (the fall-back: 9 chunks even at 6 per lane)
   49 152   64   4    lazy lists
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
W = H = 64
S = 64
ROWS = [(8192, False, 1), (16384, False, 2), (16385, False, 3), (32768, False, 4), (40000, False, 5), (49152, False, 6), (49153, False, 4),
        (49152, True, 4)]


def _pt(N, S, lazy):
    blocks = lambda pt: math.ceil(N / (1024 * pt)) * S
    if blocks(4) < 256:
        return 1
    return 4 if lazy else next((pt for pt in range(2, 7) if blocks(pt) <= 512), 4)


def _scene(N):
    """N splats on distinct depths, spread so wide that a few hundred of them - from every part of the index range - reach the image"""
    g = torch.Generator().manual_seed(N)
    z = 2.0 + 8.0 * (torch.randperm(N, generator=g).double() + 0.5) / N
    half = math.sqrt(0.03 * N)
    xy = (torch.rand(N, 2, generator=g).double() * 2 - 1) * half
    quats = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=-1)
    scales = torch.log(0.1 + 0.3 * torch.rand(N, 3, generator=g))
    opac = torch.logit(0.3 + 0.6 * torch.rand(N, generator=g))
    colors = torch.rand(N, 3, generator=g)
    K = torch.tensor([[64.0, 0.0, W / 2], [0.0, 64.0, H / 2], [0.0, 0.0, 1.0]])
    dev = "cuda:0"
    return [t.float().to(dev) for t in (torch.cat([xy, z[:, None]], -1), quats, scales, opac, colors)], torch.eye(4, device=dev), K.to(dev)


def _render(leaves, w2c, K, S, lazy):
    from deblur4dgs_amd.exposure import render_exposure

    times = torch.zeros(S, device=w2c.device) if S > 1 else None  # (a static scene: only their number is read)
    with torch.no_grad():
        r = render_exposure(*leaves, 0, None, None, None, times, None, w2c, K, W, H, background=torch.tensor([0.1, 0.5, 0.9], device=w2c.device),
                            return_depth=True, blend=False, lazy_sort=lazy, exact_tiles=False)
    torch.cuda.synchronize()
    st = r["state"]
    assert st.cfg.S == S and bool(st.cfg.lazy_sort) == lazy
    return r, st.proj_out["tile_offsets"].cpu(), st.isect["sorted_gid"].cpu()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("N,lazy,arm", ROWS)
def test_every_sub_sample_equals_the_one_sub_sample_render(N, lazy, arm):
    assert _pt(N, S, lazy) == arm and _pt(N, 1, lazy) == 1, "the row no longer reaches the arm it was chosen for"
    leaves, w2c, K = _scene(N)
    one, offs1, ids1 = _render(leaves, w2c, K, 1, lazy)
    many, offs, ids = _render(leaves, w2c, K, S, lazy)
    tiles = (W // 16) * (H // 16)
    n = int(offs1[tiles])
    visible = int((one["radii"] > 0).sum())
    print(f"N={N} lazy={lazy} arm={arm}: {visible} visible splats, {n} list entries per sub-sample")
    assert 100 <= visible <= 2000 and n > visible
    assert offs.numel() == S * tiles + 1 and int(offs[-1]) == S * n
    for s in range(S):
        what = f"N={N} lazy={lazy} sub-sample {s}"
        for k in ("renders", "alphas", "means2d"):
            assert torch.equal(_bits(many[k][s]), _bits(one[k][0])), (what, k)
        assert torch.equal(many["radii"][s], one["radii"][0]), (what, "radii")
        assert torch.equal(offs[s * tiles:(s + 1) * tiles + 1] - s * n, offs1), (what, "tile_offsets")
        if not lazy:  # (lazy lists: the far part of a list whose tile saturated in its near part is never written)
            assert torch.equal(ids[s * n:(s + 1) * n], ids1[:n]), (what, "sorted ids")
