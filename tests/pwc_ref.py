"""Restatement of the pieces of the reference's flow-aligned loss that deblur4dgs_amd.pwcnet implements in HIP: the 9x9 cost volume,
get_backwarp and AlignedLoss.forward's arithmetic - in plain torch, in whatever dtype it is given (the tests give fp64).
tests/test_pwc_ref.py pins it to values recorded from the reference's own code (tests/golden/pwc.npz); the GPU tests use it as the
yardstick.  Written from the formulas, not from the reference's grid_sample call: the sample position is the closed form that call
amounts to, and the taps are gathered one by one.

Also here: the seeded weight recipe that the fixture generator and the tests share."""
import torch

RADIUS = 4
WINDOW = 2 * RADIUS + 1


def correlation(first, second, negative_slope=1.0):
    """81 shifted products: out[b, (dy+4)*9 + (dx+4), y, x] = lrelu(mean_c first[b,c,y,x] * second[b,c,y+dy,x+dx]), zero outside."""
    B, C, H, W = first.shape
    padded = torch.nn.functional.pad(second, (RADIUS, RADIUS, RADIUS, RADIUS))
    planes = [(first * padded[:, :, iy:iy + H, ix:ix + W]).sum(1) / C for iy in range(WINDOW) for ix in range(WINDOW)]
    out = torch.stack(planes, 1)
    return torch.where(out > 0, out, out * negative_slope)


def sample_positions(flow):
    """flow [B,2,H,W] -> (sx, sy) [B,H,W]: where pixel (x, y) samples.  The reference divides the flow by (W - 1) / 2 and adds it to
    an align_corners=False grid, which un-normalises to x + fx W / (W - 1)."""
    B, _, H, W = flow.shape
    xs = torch.arange(W, dtype=flow.dtype, device=flow.device).view(1, 1, W)
    ys = torch.arange(H, dtype=flow.dtype, device=flow.device).view(1, H, 1)
    return xs + flow[:, 0] * W / (W - 1), ys + flow[:, 1] * H / (H - 1)


def _taps(flow):
    """-> list of (flat index [B,H*W] clamped inside, weight [B,H*W] zeroed outside) for the four bilinear taps"""
    B, _, H, W = flow.shape
    sx, sy = sample_positions(flow)
    x0, y0 = torch.floor(sx), torch.floor(sy)
    tx, ty = sx - x0, sy - y0
    taps = []
    for j, wy in ((0, 1 - ty), (1, ty)):
        for i, wx in ((0, 1 - tx), (1, tx)):
            xi, yi = x0 + i, y0 + j
            inside = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
            taps.append((idx.reshape(B, H * W), (wy * wx * inside).reshape(B, H * W)))
    return taps


def coverage(flow):
    """[B,H,W]: the sum of the in-bounds bilinear weights of every sample"""
    B, _, H, W = flow.shape
    return sum(w for _, w in _taps(flow)).reshape(B, H, W)


def warp(inp, flow):
    """bilinear, zeros outside; no mask"""
    B, C, H, W = inp.shape
    flat = inp.reshape(B, C, H * W)
    out = 0
    for idx, w in _taps(flow):
        out = out + flat.gather(2, idx[:, None].expand(B, C, H * W)) * w[:, None]
    return out.reshape(B, C, H, W)


def get_backwarp(inp, flow):
    """-> (warped * mask [B,C,H,W], mask [B,1,H,W]), mask = coverage > 0.999"""
    mask = (coverage(flow) > 0.999).to(inp.dtype)[:, None]
    return warp(inp, flow) * mask, mask


def aligned_l1(pred, flow, target, mask=None):
    """-> [P]: per pair, mean over 3 H W of |warp(pred) m mask - target m mask| (AlignedLoss.forward after its flow network: the
    warped image arrives multiplied by m and is multiplied by it again, m being 0 or 1)."""
    aligned, m = get_backwarp(pred, flow)
    w = m if mask is None else m * mask.reshape(m.shape)
    return (aligned * w - target * w).abs().mean(dim=(1, 2, 3))


# ---- seeded weights ------------------------------------------------------------------------------------------------------------
WEIGHT_SEED = 20241
WEIGHT_GAIN = 1.0


def seeded_state(names_and_shapes, seed=WEIGHT_SEED, gain=WEIGHT_GAIN):
    """name -> fp64 tensor, drawn in the order given from one generator.  Weights: normal with the variance that keeps a leaky-ReLU
    network's activations at the scale of its input (2 / ((1 + 0.1^2) fan_in)), times `gain`; biases: normal, 0.01.  fan_in is what
    torch calls it for both convolution kinds: shape[1] * kernel area."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for name, shape in names_and_shapes:
        shape = tuple(int(s) for s in shape)
        if len(shape) == 1:
            state[name] = 0.01 * torch.randn(shape, generator=g, dtype=torch.float64)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            state[name] = gain * (2.0 / (1.01 * fan_in)) ** 0.5 * torch.randn(shape, generator=g, dtype=torch.float64)
    return state


def checksum(state):
    """(sum, sum of absolute values) over every tensor, in fp64"""
    return [float(sum(v.sum() for v in state.values())), float(sum(v.abs().sum() for v in state.values()))]


def network_inputs(seed, B, H, W):
    """Two smooth random images in [0, 1] whose second is the first shifted by about two pixels plus noise: something to align."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, 3, H // 4 + 2, W // 4 + 2, generator=g, dtype=torch.float64)
    big = torch.nn.functional.interpolate(coarse, size=(H + 8, W + 8), mode="bicubic", align_corners=False).clamp(0, 1)
    first = big[:, :, 4:4 + H, 4:4 + W]
    second = big[:, :, 2:2 + H, 6:6 + W] + 0.02 * torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
    return first.contiguous(), second.contiguous()
