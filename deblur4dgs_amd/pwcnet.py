"""The reference's flow-aligned exposure consistency loss (flow3d/trainer.py:599-618, flow3d/loss_utils.py AlignedLoss,
flow3d/models/pwcnet.py) on ROCm.

The reference's cost volume is CUDA C compiled through cupy, so the term cannot run on ROCm at all.  Here the 9x9 cost volume
(`correlation`, csrc/correlation.hip), the backward warp (`backwarp`, csrc/warp.hip) and the masked L1 of the warped pair
(`aligned_l1`, csrc/warp.hip) are HIP kernels; PWC-Net's convolutions stay torch (MIOpen).  `Network` and `PWCNet` restate the
reference's architecture with the same `state_dict` keys and shapes, so its pretrained blob loads unchanged.

    from deblur4dgs_amd.pwcnet import AlignedLoss, PWCNet, get_backwarp      # for flow3d.loss_utils / flow3d.models.pwcnet

`exposure_consistency_loss(exposure_imgs, alignnet)` is the trainer's loop over the 2 (S - 1) pairs as ONE batched network pass and
one loss kernel; nothing in it waits on the host, so a step that holds it can be captured in a HIP graph.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _lib as L
from ._lib import f32c, need_gpu, stream_of, vp

NEIGHBOURS = 81  # the 9 x 9 search window of the cost volume


class _CorrelationFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, first, second, slope):
        need_gpu(first, "deblur4dgs_amd.pwcnet.correlation")
        if first.dim() != 4 or first.shape != second.shape:
            raise ValueError(f"first {tuple(first.shape)} and second {tuple(second.shape)} must both be [B,C,H,W]")
        B, Cc, H, W = first.shape
        f, s = f32c(first), f32c(second)
        out = torch.empty(B, NEIGHBOURS, H, W, device=f.device, dtype=torch.float32)
        L.check(L.lib().d4gs_correlation_fwd(vp(f), vp(s), B, Cc, H, W, slope, vp(out), stream_of(f)), "d4gs_correlation_fwd")
        ctx.keep = (f, s, out if slope != 1.0 else None)
        ctx.args = (slope, first.dtype, second.dtype)
        return out

    @staticmethod
    def backward(ctx, v_out):
        f, s, out = ctx.keep
        slope, dt_first, dt_second = ctx.args
        B, Cc, H, W = f.shape
        v = f32c(v_out)
        v_first = torch.empty_like(f) if ctx.needs_input_grad[0] else None
        v_second = torch.empty_like(s) if ctx.needs_input_grad[1] else None
        L.check(L.lib().d4gs_correlation_bwd(vp(f), vp(s), vp(out), vp(v), B, Cc, H, W, slope, vp(v_first), vp(v_second), stream_of(f)),
                "d4gs_correlation_bwd")
        return (None if v_first is None else v_first.to(dt_first)), (None if v_second is None else v_second.to(dt_second)), None


def correlation(first, second, negative_slope: float = 1.0):
    """[B,C,H,W] x 2 -> [B,81,H,W]: out[b, (dy+4)*9 + (dx+4), y, x] = lrelu(mean_c first[b,c,y,x] * second[b,c,y+dy,x+dx]), second
    zero outside the image.  `negative_slope` is the leaky ReLU the network always applies to the volume, fused (1.0: none).
    Differentiable with respect to both inputs (gathers, no atomics); bitwise reproducible."""
    return _CorrelationFn.apply(first, second, float(negative_slope))


class _BackwarpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, flow):
        need_gpu(inp, "deblur4dgs_amd.pwcnet.backwarp")
        if inp.dim() != 4 or flow.dim() != 4 or flow.shape[1] != 2 or flow.shape[0] != inp.shape[0] or flow.shape[2:] != inp.shape[2:]:
            raise ValueError(f"input {tuple(inp.shape)} must be [B,C,H,W] and flow {tuple(flow.shape)} [B,2,H,W]")
        B, Cc, H, W = inp.shape
        if H < 2 or W < 2:
            raise ValueError(f"backwarp: H={H}, W={W} (each must be at least 2: the flow is scaled by W / (W - 1))")
        x, fl = f32c(inp), f32c(flow)
        out = torch.empty_like(x)
        mask = torch.empty(B, 1, H, W, device=x.device, dtype=torch.float32)
        L.check(L.lib().d4gs_backwarp_fwd(vp(x), vp(fl), B, Cc, H, W, vp(out), vp(mask), stream_of(x)), "d4gs_backwarp_fwd")
        ctx.keep = (fl,)
        ctx.args = (inp.shape, inp.dtype)
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    def backward(ctx, v_out, _v_mask):
        fl, = ctx.keep
        (B, Cc, H, W), dtype = ctx.args
        v = f32c(v_out)
        v_in = torch.empty_like(v)
        L.check(L.lib().d4gs_backwarp_bwd(vp(fl), vp(v), B, Cc, H, W, vp(v_in), stream_of(v)), "d4gs_backwarp_bwd")
        return v_in.to(dtype), None


def _no_flow_grad(flow):
    if flow.requires_grad:
        raise RuntimeError("the flow carries a gradient: the backward warp differentiates with respect to the image only (the reference "
                           "estimates the flow under torch.no_grad()); detach it")


def backwarp(input, flow):
    """get_backwarp of flow3d/models/pwcnet.py: input [B,C,H,W], flow [B,2,H,W] (x first, pixels) -> (warped * mask [B,C,H,W],
    mask [B,1,H,W]).  Bilinear, zeros outside, sampled at (x + fx W / (W - 1), y + fy H / (H - 1)); mask = 1 where the in-bounds
    bilinear weights add up to more than 0.999.  The gradient goes to `input` only."""
    _no_flow_grad(flow)
    return _BackwarpFn.apply(input, flow)


get_backwarp = backwarp  # the reference's name


class _AlignedL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, flow, target, mask):
        need_gpu(pred, "deblur4dgs_amd.pwcnet.aligned_l1")
        if pred.dim() != 4 or pred.shape[1] != 3 or target.shape != pred.shape:
            raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must both be [P,3,H,W]")
        P, _, H, W = pred.shape
        if tuple(flow.shape) != (P, 2, H, W):
            raise ValueError(f"flow {tuple(flow.shape)} must be [P,2,H,W] = {(P, 2, H, W)}")
        if H < 2 or W < 2:
            raise ValueError(f"aligned_l1: H={H}, W={W} (each must be at least 2)")
        m = None
        if mask is not None:
            if mask.numel() != P * H * W:
                raise ValueError(f"mask {tuple(mask.shape)} must hold one value per pair and pixel: [P,H,W] or [P,1,H,W]")
            m = f32c(mask).reshape(P, H, W)
        p, fl, t = f32c(pred), f32c(flow), f32c(target)
        lib = L.lib()
        partials = torch.empty(P * lib.d4gs_aligned_l1_blocks(H, W), device=p.device, dtype=torch.float64)
        losses = torch.empty(P, device=p.device, dtype=torch.float32)
        L.check(lib.d4gs_aligned_l1_fwd(vp(p), vp(fl), vp(t), vp(m), P, H, W, vp(partials), vp(losses), stream_of(p)), "d4gs_aligned_l1_fwd")
        ctx.keep = (p, fl, t, m)
        ctx.args = (pred.dtype, target.dtype)
        return losses

    @staticmethod
    def backward(ctx, v_losses):
        p, fl, t, m = ctx.keep
        P, _, H, W = p.shape
        v = f32c(v_losses).reshape(P)
        v_pred = torch.empty_like(p)
        v_target = torch.empty_like(t) if ctx.needs_input_grad[2] else None
        L.check(L.lib().d4gs_aligned_l1_bwd(vp(p), vp(fl), vp(t), vp(m), vp(v), P, H, W, vp(v_pred), vp(v_target), stream_of(p)),
                "d4gs_aligned_l1_bwd")
        return v_pred.to(ctx.args[0]), None, (None if v_target is None else v_target.to(ctx.args[1])), None


def aligned_l1(pred, flow, target, mask=None):
    """P pairs at once -> losses [P]: losses[p] = mean over 3 H W of |warp(pred_p, flow_p) m_p mask_p - target_p m_p mask_p|, m_p the
    coverage mask of `backwarp`.  pred, target [P,3,H,W]; flow [P,2,H,W]; mask [P,H,W] / [P,1,H,W] or None.  Gradients go to
    `pred` (a scatter) and `target`; the flow and the masks are data."""
    _no_flow_grad(flow)
    return _AlignedL1Fn.apply(pred, flow, target, mask)


# ---- the flow network ----------------------------------------------------------------------------------------------------------
_LEVEL_NAMES = ("netOne", "netTwo", "netThr", "netFou", "netFiv", "netSix")  # pyramid levels 1..6, and the layers of a decoder
_FEATURES = (3, 16, 32, 64, 96, 128, 196)                                   # channels of the image and of levels 1..6
_DENSE = (128, 128, 96, 64, 32)                                             # what a decoder's five dense layers add
_WARP_SCALE = {5: 0.625, 4: 1.25, 3: 2.5, 2: 5.0}                           # 20 / 2^level: network flow units -> pixels of the level
_SLOPE = 0.1


def _act():
    return nn.LeakyReLU(inplace=False, negative_slope=_SLOPE)


def _conv(cin, cout, stride=1, dilation=1):
    return nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=dilation, dilation=dilation)


def _decoder_width(level):
    """Channels entering the decoder of a level: the volume, and below level 6 the level's features, the upsampled flow (2) and the
    upsampled decoder features (2)."""
    return NEIGHBOURS if level == 6 else NEIGHBOURS + _FEATURES[level] + 2 + 2


class Extractor(nn.Module):
    """Six stride-2 stages of three 3x3 convolutions: the feature pyramid, finest first."""

    def __init__(self):
        super().__init__()
        for name, cin, cout in zip(_LEVEL_NAMES, _FEATURES[:-1], _FEATURES[1:]):
            setattr(self, name, nn.Sequential(_conv(cin, cout, stride=2), _act(), _conv(cout, cout), _act(), _conv(cout, cout), _act()))

    def forward(self, image):
        pyramid = []
        for name in _LEVEL_NAMES:
            image = getattr(self, name)(image)
            pyramid.append(image)
        return pyramid


class Decoder(nn.Module):
    """One pyramid level: cost volume of `first` against `second` warped by the coarser level's flow, then five densely connected
    convolutions and the flow head."""

    def __init__(self, level, corr_fn, warp_fn):
        super().__init__()
        self.level, self.corr_fn, self.warp_fn = level, corr_fn, warp_fn
        width = _decoder_width(level)
        if level < 6:
            self.netUpflow = nn.ConvTranspose2d(2, 2, kernel_size=4, stride=2, padding=1)
            self.netUpfeat = nn.ConvTranspose2d(_decoder_width(level + 1) + sum(_DENSE), 2, kernel_size=4, stride=2, padding=1)
        for name, cout in zip(_LEVEL_NAMES[:5], _DENSE):
            setattr(self, name, nn.Sequential(_conv(width, cout), _act()))
            width += cout
        self.netSix = nn.Sequential(_conv(width, 2))

    def forward(self, first, second, coarser):
        if coarser is None:
            feat = self.corr_fn(first, second, _SLOPE)
        else:
            flow = self.netUpflow(coarser[0])
            up = self.netUpfeat(coarser[1])
            warped = self.warp_fn(second, flow * _WARP_SCALE[self.level])[0]
            feat = torch.cat([self.corr_fn(first, warped, _SLOPE), first, flow, up], 1)
        for name in _LEVEL_NAMES[:5]:
            feat = torch.cat([getattr(self, name)(feat), feat], 1)
        return self.netSix(feat), feat


class Refiner(nn.Module):
    """The dilated context network on the finest decoder's features."""

    def __init__(self):
        super().__init__()
        plan = ((128, 1), (128, 2), (128, 4), (96, 8), (64, 16), (32, 1))
        layers, cin = [], _decoder_width(2) + sum(_DENSE)
        for cout, dilation in plan:
            layers += [_conv(cin, cout, dilation=dilation), _act()]
            cin = cout
        self.netMain = nn.Sequential(*layers, _conv(cin, 2))

    def forward(self, feat):
        return self.netMain(feat)


class Network(nn.Module):
    """PWC-Net with the reference's parameter names and shapes.  `corr_fn(first, second, negative_slope)` and
    `warp_fn(input, flow) -> (warped, mask)` default to the HIP ops; a CPU test passes restatements."""

    def __init__(self, corr_fn=None, warp_fn=None):
        super().__init__()
        corr_fn, warp_fn = corr_fn or correlation, warp_fn or backwarp
        self.netExtractor = Extractor()
        for level in (2, 3, 4, 5, 6):
            setattr(self, _LEVEL_NAMES[level - 1], Decoder(level, corr_fn, warp_fn))
        self.netRefiner = Refiner()

    def forward(self, first, second):
        a, b = self.netExtractor(first), self.netExtractor(second)
        state = None
        for level in (6, 5, 4, 3, 2):
            state = getattr(self, _LEVEL_NAMES[level - 1])(a[level - 1], b[level - 1], state)
        flow, feat = state
        return flow + self.netRefiner(feat)


class PWCNet(nn.Module):
    """The reference's wrapper: `forward(source_img, target_img)` -> flow [B,2,H,W] in pixels of the input size.  Both images are
    resized to multiples of 64, the network is called as net(target, source), and its output (at a quarter of the resized size, in
    units of 1/20 pixel) is resized back, multiplied by 20 and rescaled per axis."""

    def __init__(self, load_pretrained=True, weights_path=None, rgb2bgr=False, corr_fn=None, warp_fn=None):
        super().__init__()
        self.net = Network(corr_fn, warp_fn)
        self.rgb2bgr = rgb2bgr
        if load_pretrained:
            if weights_path is None:
                raise ValueError("PWCNet(load_pretrained=True) needs weights_path")
            self.load_reference_state(torch.load(weights_path, map_location="cpu"))

    def load_reference_state(self, weights):
        """The published blob names its modules 'module...'; the network here (as the reference's) 'net...'."""
        self.net.load_state_dict({k.replace("module", "net"): v for k, v in weights.items()})

    def forward(self, source_img, target_img):
        if source_img.shape[-2:] != target_img.shape[-2:]:
            raise ValueError(f"source {tuple(source_img.shape)} and target {tuple(target_img.shape)} differ in size")
        H, W = source_img.shape[-2:]
        source, target = source_img.reshape(-1, 3, H, W), target_img.reshape(-1, 3, H, W)
        if self.rgb2bgr:
            source, target = source.flip(1), target.flip(1)
        H64, W64 = 64 * math.ceil(H / 64), 64 * math.ceil(W / 64)
        resize = lambda t, size: nn.functional.interpolate(t, size=size, mode="bilinear", align_corners=False)
        flow = 20.0 * resize(self.net(resize(target, (H64, W64)), resize(source, (H64, W64))), (H, W))
        return torch.stack((flow[:, 0] * (float(W) / float(W64)), flow[:, 1] * (float(H) / float(H64))), dim=1)


class AlignedLoss(nn.Module):
    """flow3d/loss_utils.py AlignedLoss with the flow network passed in (the reference builds a pretrained PWCNet itself).
    forward(pred, target, mask=None): pred, target [B,3,H,W], mask [B,1,H,W] -> the mean over B 3 H W of the masked L1 between
    `pred` warped onto `target` and `target`."""

    def __init__(self, alignnet, loss_weight=1.0):
        super().__init__()
        self.alignnet = alignnet.eval()
        self.loss_weight = loss_weight

    def forward(self, pred, target, mask=None):
        with torch.no_grad():
            offset = self.alignnet(pred, target)
        return aligned_l1(pred, offset, target, mask).mean()  # equal element counts: the mean of the pairs' means is the mean


def exposure_consistency_loss(exposure_imgs, alignnet):
    """The exposure consistency term of flow3d/trainer.py:599-618 (the caller applies its weight of 2).  exposure_imgs [S,1,H,W,D']
    (`SceneModel.render(...)["exposure_imgs"]`: RGB in channels 0..2, alpha in channel 3).  Every sub-sample e < S - 1 is compared
    with its successor (target img[e+1], which receives a gradient; mask alpha[e+1]) and every e >= 1 with sub-sample 0 (target and
    mask detached): 2 (S - 1) pairs in one PWC-Net pass under no_grad and one loss kernel.  -> sum of the pairs' losses / (S - 1)."""
    if exposure_imgs.dim() != 5 or exposure_imgs.shape[1] != 1 or exposure_imgs.shape[-1] < 4 or exposure_imgs.shape[0] < 2:
        raise ValueError(f"exposure_imgs {tuple(exposure_imgs.shape)} must be [S,1,H,W,D'] with S >= 2 and D' >= 4")
    S = exposure_imgs.shape[0]
    img = exposure_imgs[:, 0, :, :, 0:3].permute(0, 3, 1, 2)
    alpha = exposure_imgs[:, 0, :, :, 3].detach()
    pred = torch.cat([img[:-1], img[1:]], 0)
    target = torch.cat([img[1:], img[:1].detach().expand(S - 1, -1, -1, -1)], 0)
    mask = torch.cat([alpha[1:], alpha[:1].expand(S - 1, -1, -1)], 0)
    with torch.no_grad():
        flow = alignnet(pred, target)
    return aligned_l1(pred, flow, target, mask).sum() / (S - 1)
