"""Inputs of the photometric-loss tests, shared by the CPU discrimination test (tests/test_oracle_photometric.py) and the GPU
test (tests/test_gpu_photometric.py) so that both see the same tensors.  Not a conftest: plain functions, cached.

Every case is fp32 [2,48,60,3] with different content in the two batch items.  48x60 is 3x4 input tiles of 16 and more than
one output tile each way; 60 keeps the vertical split of "split" off a tile boundary."""
from __future__ import annotations

import functools

import torch

from oracle import photometric as ph

B, H, W = 2, 48, 60
NOISE = "noise"
# the cases on which SSIM's raw-moment formula cancels in fp32: flat, bright or converged images
FLAT = ("const_1_098", "flat_noise_both", "flat_gt", "smooth_bright", "split", "identical")
CONTENT = (NOISE, "const_03_07") + FLAT + ("alt_rows",)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _noise(g, shape=(B, H, W, 3)):
    """The input every older test uses: gt uniform, pred = gt + 0.15 randn."""
    gt = torch.rand(*shape, generator=g)
    return (gt + 0.15 * torch.randn(*shape, generator=g)).clamp(0, 1), gt


def _blob(cy, cx, sigma, amp):
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    return amp * torch.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * sigma ** 2))


@functools.lru_cache(maxsize=None)
def content(name):
    """-> (pred, gt), fp32 [2,H,W,3].  Treat as read-only (cached)."""
    g = _gen(sum(map(ord, name)))
    if name == NOISE:
        pred, gt = _noise(g)
    elif name in ("const_03_07", "const_1_098"):
        a, b = (0.3, 0.7) if name == "const_03_07" else (1.0, 0.98)
        pred, gt = torch.empty(B, H, W, 3), torch.empty(B, H, W, 3)
        pred[0], gt[0], pred[1], gt[1] = a, b, b, a  # item 1 swaps the roles: same SSIM, by symmetry
    elif name == "flat_noise_both":
        gt = 0.97 + 1e-3 * torch.randn(B, H, W, 3, generator=g)
        pred = gt + 1e-3 * torch.randn(B, H, W, 3, generator=g)
    elif name == "flat_gt":
        gt = torch.full((B, H, W, 3), 0.97)
        pred = gt + 1e-3 * torch.randn(B, H, W, 3, generator=g)
    elif name == "smooth_bright":  # 0.97 background, a soft dark blob; pred lacks a small smooth bump elsewhere
        gt0 = 0.97 - _blob(17, 40, 7.0, 0.35)
        gt1 = 0.97 - _blob(30, 15, 5.0, 0.5) - _blob(8, 50, 9.0, 0.1)
        gt = torch.stack([gt0, gt1]).unsqueeze(-1) * torch.tensor([1.0, 0.98, 0.95], dtype=torch.float64)
        bump = torch.stack([_blob(34, 14, 5.0, 0.02), _blob(12, 36, 4.0, 0.01) + _blob(40, 52, 6.0, 0.015)]).unsqueeze(-1)
        pred, gt = (gt - bump).float(), gt.float()
    elif name == "split":  # one part flat and bright (gt 0.97, pred off by 1e-3 noise), the rest the noise input
        pred, gt = _noise(g)
        fp = 0.97 + 1e-3 * torch.randn(B, H, W, 3, generator=g)
        pred[0, :, :W // 2], gt[0, :, :W // 2] = fp[0, :, :W // 2], 0.97  # item 0: left half, cut at column 30
        pred[1, 21:], gt[1, 21:] = fp[1, 21:], 0.97                        # item 1: bottom part, cut at row 21
    elif name == "identical":  # pred bitwise gt; its neighbour pred = gt + 1e-3 noise is "flat_noise_both"
        gt = content("flat_noise_both")[1]
        pred = gt.clone()
    elif name == "alt_rows":  # the noise input with pred == gt on the even rows
        pred, gt = _noise(g)
        pred[:, 0::2] = gt[:, 0::2]
    else:
        raise KeyError(name)
    return pred.contiguous(), gt.contiguous()


@functools.lru_cache(maxsize=None)
def soft_mask():
    """[2,H,W,1] soft alpha in [0,1]: smooth fractional values, a region of exact ones, and an exactly zero 16x16 input tile
    (rows 16:32, columns 16:32 of item 0; rows 0:16, columns 32:48 of item 1)."""
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    m0 = torch.sigmoid((x - 12.0) / 4.0 + (y - 24.0) / 16.0)
    m1 = torch.sigmoid((30.0 - y) / 5.0) * 0.5 + 0.5 * torch.sigmoid((x - 30.0) / 3.0)
    m = torch.stack([m0, m1]).float()
    m[0, :, 50:] = 1.0
    m[1, 40:, :10] = 1.0
    m[0, 16:32, 16:32] = 0.0
    m[1, 0:16, 32:48] = 0.0
    return m.unsqueeze(-1).contiguous()


def evaluate(pred, gt, mask, dtype):
    """oracle.photometric in `dtype` on the given fp32 tensors -> dict of python floats / [B,H,W,3] fp64 tensors:
    l1, ssim and their gradients g_l1 = d l1 / d pred, g_ssim = d ssim / d pred.  Any weighting follows from them:
    loss = w_l1 l1 + w_ssim (1 - ssim), d loss / d pred = w_l1 g_l1 - w_ssim g_ssim."""
    p = pred.detach().to(dtype, copy=True).requires_grad_()  # a copy: the cached inputs stay plain tensors
    _, l1, s = ph.photometric_loss(p, gt.to(dtype), None if mask is None else mask.to(dtype))
    g_l1, = torch.autograd.grad(l1, p, retain_graph=True)
    g_s, = torch.autograd.grad(s, p)
    return {"l1": float(l1.detach()), "ssim": float(s.detach()), "g_l1": g_l1.double(), "g_ssim": g_s.double()}


@functools.lru_cache(maxsize=None)
def reference(name, masked):
    """The fp64 oracle on the fp32-quantised inputs cast to double (the two sides differ in arithmetic only)."""
    pred, gt = content(name)
    return evaluate(pred, gt, soft_mask() if masked else None, torch.float64)
