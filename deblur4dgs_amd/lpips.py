"""LPIPS (AlexNet, version 0.1): the validator's ninth metric and the score of the reference's result table.

    from deblur4dgs_amd.lpips import LPIPS, mLPIPS        # for flow3d.metrics.mLPIPS and run_compute_metrics.py's lpips model

    net = LPIPS("alexnet-owt-7be5be79.pth", "alex.pth")   # torchvision's AlexNet weights, and the LPIPS v0.1 linear heads
    ValidationMetrics(lpips=net)                           # nine val/* keys instead of six

The package ships NO weights.  The two files are public: the trunk is torchvision's `alexnet(weights="IMAGENET1K_V1")` state dict
(`features.*`; its classifier keys are ignored), the heads are `lpips/weights/v0.1/alex.pth` of the LPIPS repository
(richzhang/PerceptualSimilarity), which the reference carries as `models/weights/v0.1/alex.pth`.

The trunk's five convolutions are torch's (MIOpen) in fp32, restricted to its deterministic algorithms.  Everything else is HIP (`csrc/lpips.hip`): one launch builds the trunk's
input from channel-last images and masks, one launch per layer turns two feature tensors into the layer's distance map, and one call
upsamples, adds, masks and sums.  The trunk runs once per side and mask on B images (identical problems, identical arithmetic: a
mask scores bitwise the same alone and among the validator's three).  Forward only: no output requires a
gradient.  The reference takes its network from torchmetrics' `_NoTrainLpips`; this module follows the reference's own PNetLin.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import re
import threading

import torch
from torch import nn

from . import _lib as L
from ._lib import f32c, need_gpu, stream_of, vp
from .metrics import _Metric

__all__ = ["alex_sizes", "LPIPS", "mLPIPS", "prepare", "layer_distance", "score", "mean_score", "deterministic_convolutions", "CHANNELS"]

CHANNELS = (64, 192, 384, 256, 256)
MIN_SIZE = 31
# index in torchvision's `features` -> (slice of the LPIPS layout, c_in, c_out, kernel, stride, padding)
_CONVS = {0: (1, 3, 64, 11, 4, 2), 3: (2, 64, 192, 5, 1, 2), 6: (3, 192, 384, 3, 1, 1), 8: (4, 384, 256, 3, 1, 1), 10: (5, 256, 256, 3, 1, 1)}
_POOLS = (2, 5)
_SLICES = ((0, 2), (2, 5), (5, 8), (8, 10), (10, 12))


def alex_sizes(H: int, W: int):
    """The five feature-map sizes (h, w) of an H x W image: conv 11/4 pad 2, two 3/2 max-pools, three size-preserving convolutions."""
    if H < MIN_SIZE or W < MIN_SIZE:
        raise ValueError(f"LPIPS needs H and W >= {MIN_SIZE} (the deepest map would be empty), got H={H} W={W}")
    first = lambda n: (n - 7) // 4 + 1
    pool = lambda n: (n - 3) // 2 + 1
    s1 = (first(H), first(W))
    s2 = (pool(s1[0]), pool(s1[1]))
    s3 = (pool(s2[0]), pool(s2[1]))
    return (s1, s2, s3, s3, s3)


class _Trunk(nn.Module):
    """torchvision's AlexNet features[0:12] cut into the five slices of the LPIPS layout; forward returns the five ReLU outputs"""

    def __init__(self):
        super().__init__()
        layers = {}
        for i, (_, cin, cout, k, s, p) in _CONVS.items():
            layers[i], layers[i + 1] = nn.Conv2d(cin, cout, k, stride=s, padding=p), nn.ReLU()
        for i in _POOLS:
            layers[i] = nn.MaxPool2d(3, 2)
        for n, (lo, hi) in enumerate(_SLICES):
            seq = nn.Sequential()
            for i in range(lo, hi):
                seq.add_module(str(i), layers[i])
            self.add_module(f"slice{n + 1}", seq)

    def forward(self, x):
        feats = []
        for n in range(5):
            x = getattr(self, f"slice{n + 1}")(x)
            feats.append(x)
        return feats


class _Lin(nn.Module):
    """one head: `model.1` is the 1x1 convolution (`model.0` is the reference's dropout, the identity in eval mode)"""

    def __init__(self, channels):
        super().__init__()
        self.model = nn.Sequential(nn.Identity(), nn.Conv2d(channels, 1, 1, bias=False))


_FLAGS_LOCK = threading.RLock()  # LPIPS calls of several threads take their turns at the two switches


@contextlib.contextmanager
def deterministic_convolutions():
    """torch.backends.cudnn.{deterministic, benchmark} = True, False inside (the MIOpen backend reads the same two switches), restored
    on the way out.  The switches are process-wide: a convolution that ANOTHER thread issues while a trunk call is inside this
    context (a trainer thread's PWC-Net beside a validating one, say) also runs with MIOpen's deterministic algorithms - slower,
    never wrong.  Calls from several threads are serialised by a lock, so one's restore never undoes another's setting."""
    cudnn = torch.backends.cudnn
    with _FLAGS_LOCK:
        saved = cudnn.deterministic, cudnn.benchmark
        cudnn.deterministic, cudnn.benchmark = True, False
        try:
            yield
        finally:
            cudnn.deterministic, cudnn.benchmark = saved


def _load(source, what):
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        source = torch.load(source, map_location="cpu")
    if not isinstance(source, dict):
        raise ValueError(f"LPIPS: {what} must be a path or a state dict, got {type(source).__name__}")
    return source


def _trunk_state(source):
    """a state dict in torchvision's or the LPIPS layout -> {net.slice{n}.{i}.{weight,bias}: tensor}; ValueError names a bad key"""
    out = {}
    for key, v in source.items():
        m = re.fullmatch(r"features\.(\d+)\.(weight|bias)", key) or re.fullmatch(r"net\.slice(\d)\.(\d+)\.(weight|bias)", key)
        if m is None:
            if key.startswith("classifier."):  # torchvision's whole-model state dict: the classifier is not part of the metric
                continue
            raise ValueError(f"LPIPS trunk: stray key {key!r}")
        i = int(m.groups()[-2])
        if i not in _CONVS or (len(m.groups()) == 3 and int(m.group(1)) != _CONVS[i][0]):
            raise ValueError(f"LPIPS trunk: stray key {key!r}")
        n, cin, cout, k = _CONVS[i][:4]
        want = (cout, cin, k, k) if m.groups()[-1] == "weight" else (cout,)
        if tuple(v.shape) != want:
            raise ValueError(f"LPIPS trunk: {key!r} has shape {tuple(v.shape)}, expected {want}")
        mine = f"net.slice{n}.{i}.{m.groups()[-1]}"
        if mine in out:
            raise ValueError(f"LPIPS trunk: {key!r} is given twice (both layouts)")
        out[mine] = v
    for i, (n, *_rest) in _CONVS.items():
        for leaf in ("weight", "bias"):
            if f"net.slice{n}.{i}.{leaf}" not in out:
                raise ValueError(f"LPIPS trunk: missing key 'features.{i}.{leaf}' (or 'net.slice{n}.{i}.{leaf}')")
    return out


def _lins_state(source):
    out = {}
    for key, v in source.items():
        m = re.fullmatch(r"lin([0-4])\.model\.1\.weight", key)
        if m is None:
            raise ValueError(f"LPIPS heads: stray key {key!r}")
        want = (1, CHANNELS[int(m.group(1))], 1, 1)
        if tuple(v.shape) != want:
            raise ValueError(f"LPIPS heads: {key!r} has shape {tuple(v.shape)}, expected {want}")
        out[key] = v
    for k in range(5):
        if f"lin{k}.model.1.weight" not in out:
            raise ValueError(f"LPIPS heads: missing key 'lin{k}.model.1.weight'")
    return out


def layer_distance(f0, f1, weights):
    """f0, f1 [n,C,h,w], weights [C] -> [n,h,w] fp32: sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2, one launch."""
    need_gpu(f0, "deblur4dgs_amd.lpips")
    if f0.dim() != 4 or f1.shape != f0.shape or weights.numel() != f0.shape[1]:
        raise ValueError(f"f0 {tuple(f0.shape)} and f1 {tuple(f1.shape)} must both be [n,C,h,w] and weights {tuple(weights.shape)} hold C values")
    a, b, w = f32c(f0), f32c(f1), f32c(weights.to(f0.device)).reshape(-1)
    n, Cn, h, wd = a.shape
    out = torch.empty(n, h, wd, device=a.device, dtype=torch.float32)
    L.check(L.lib().d4gs_lpips_layer(vp(a), vp(b), vp(w), n, Cn, h, wd, vp(out), stream_of(a)), "d4gs_lpips_layer")
    return out


def _host_tables(layers):
    """(host array of the maps' device pointers, host array of their sizes) as d4gs_lpips_score / d4gs_lpips_mean take them"""
    if len(layers) != 5:
        raise ValueError(f"LPIPS: five layer maps expected, got {len(layers)}")
    ptrs = (C.c_void_p * 5)(*[t.data_ptr() for t in layers])
    sizes = (C.c_int32 * 10)(*[s for t in layers for s in t.shape[-2:]])
    return ptrs, sizes


def _masks(masks, B, H, W, device):
    """None, [B,H,W] or [M,B,H,W] (a trailing 1 allowed) -> (fp32 contiguous [M,B,H,W] or None, M)"""
    if masks is None:
        return None, 1
    if masks.dim() >= 4 and masks.shape[-1] == 1 and tuple(masks.shape[-4:-1]) == (B, H, W):
        masks = masks[..., 0]
    if masks.dim() not in (3, 4) or tuple(masks.shape[-3:]) != (B, H, W):
        raise ValueError(f"masks must be [B,H,W] or [M,B,H,W] (a trailing 1 allowed) for images {(B, H, W, 3)}, got {tuple(masks.shape)}")
    m = f32c(masks.to(device))
    return m.reshape(-1, B, H, W), (m.shape[0] if m.dim() == 4 else 1)


def prepare(preds, targets, masks=None, normalize: bool = False):
    """preds, targets [B,H,W,3], masks None / [B,H,W] / [M,B,H,W] -> the trunk's input [2,M,B,3,H,W] fp32 (preds first), one launch:
    (image * mask), `* 2 - 1` when `normalize`, then the scaling layer, rounded as torch rounds each step."""
    return _prepare(preds, targets, masks, normalize)[0]


def _prepare(preds, targets, masks, normalize):
    """-> (the trunk's input, the masks as the kernels read them: fp32 [M,B,H,W] or None)"""
    need_gpu(preds, "deblur4dgs_amd.lpips")
    if preds.dim() != 4 or preds.shape[-1] != 3 or targets.shape != preds.shape:
        raise ValueError(f"preds and targets must both be [B,H,W,3], got {tuple(preds.shape)} and {tuple(targets.shape)}")
    B, H, W, _ = preds.shape
    alex_sizes(H, W)
    p, t = f32c(preds), f32c(targets.to(preds.device))
    m, M = _masks(masks, B, H, W, p.device)
    out = torch.empty(2, M, B, 3, H, W, device=p.device, dtype=torch.float32)
    L.check(L.lib().d4gs_lpips_prepare(vp(p), vp(t), vp(m), M, B, H, W, int(bool(normalize)), vp(out), stream_of(p)), "d4gs_lpips_prepare")
    return out, m


def score(layers, H: int, W: int, masks=None, want_map: bool = False):
    """layers: five maps [M*B,h_k,w_k] (or [M,B,h_k,w_k]); masks None (M = 1), [B,H,W] (M = 1) or [M,B,H,W] -> (sum score * mask, sum mask, map or None):
    float64 [M,B] twice and fp32 [M,B,H,W].  Two launches."""
    need_gpu(layers[0], "deblur4dgs_amd.lpips")
    maps = [f32c(t) for t in layers]
    if masks is None:
        M, B, m = 1, maps[0].numel() // (maps[0].shape[-2] * maps[0].shape[-1]), None
    else:
        if masks.dim() not in (3, 4) or tuple(masks.shape[-2:]) != (H, W):
            raise ValueError(f"masks must be [B,H,W] or [M,B,H,W] with H={H} W={W}, got {tuple(masks.shape)}")
        m = f32c(masks.to(maps[0].device))
        m = m[None] if m.dim() == 3 else m
        M, B = m.shape[0], m.shape[1]
    for k, t in enumerate(maps):
        if t.numel() != M * B * t.shape[-2] * t.shape[-1]:
            raise ValueError(f"layer map {k} {tuple(t.shape)} does not hold M*B = {M * B} images")
    lib = L.lib()
    nb = lib.d4gs_lpips_score_blocks(M, B, H, W)
    if nb == 0:
        raise ValueError(f"LPIPS score: sizes M={M} B={B} H={H} W={W} are too small (H, W >= {MIN_SIZE}) or beyond the grid")
    dev = maps[0].device
    scratch = torch.empty(2 * nb + 2 * M * B, device=dev, dtype=torch.float64)
    out = scratch[2 * nb:]
    smap = torch.empty(M, B, H, W, device=dev, dtype=torch.float32) if want_map else None
    ptrs, sizes = _host_tables(maps)
    L.check(lib.d4gs_lpips_score(ptrs, sizes, vp(m), M, B, H, W, vp(smap), vp(scratch), vp(out), stream_of(maps[0])), "d4gs_lpips_score")
    out = out.view(M, B, 2)
    return out[..., 0].clone(), out[..., 1].clone(), smap


def mean_score(layers):
    """layers: five maps [n,h_k,w_k] -> float64 [n]: the layer means added in layer order (the reference's spatial=False form)."""
    need_gpu(layers[0], "deblur4dgs_amd.lpips")
    maps = [f32c(t) for t in layers]
    n = maps[0].shape[0]
    if any(t.dim() != 3 or t.shape[0] != n for t in maps):
        raise ValueError(f"layer maps must all be [n,h,w] with one n, got {[tuple(t.shape) for t in maps]}")
    out = torch.empty(n, device=maps[0].device, dtype=torch.float64)
    ptrs, sizes = _host_tables(maps)
    L.check(L.lib().d4gs_lpips_mean(ptrs, sizes, n, vp(out), stream_of(maps[0])), "d4gs_lpips_mean")
    return out


class LPIPS(nn.Module):
    """PNetLin(pnet_type='alex', version='0.1') in eval mode.  `trunk`: a path or state dict in torchvision's layout
    (`features.{0,3,6,8,10}.{weight,bias}`) or the LPIPS one (`net.slice{1..5}.*`); `lins`: a path or state dict with
    `lin{0..4}.model.1.weight`.  A missing, stray or misshapen key raises ValueError naming it.  `state_dict()` is in the LPIPS layout."""

    def __init__(self, trunk, lins):
        super().__init__()
        self.net = _Trunk()
        for k, c in enumerate(CHANNELS):
            self.add_module(f"lin{k}", _Lin(c))
        state = {**_trunk_state(_load(trunk, "trunk")), **_lins_state(_load(lins, "lins"))}
        self.load_state_dict({k: v.detach().float() for k, v in state.items()}, strict=True)
        self.requires_grad_(False)
        self.eval()

    def train(self, mode: bool = True):
        return super().train(False)  # a metric: never in training mode

    @torch.no_grad()
    def layer_maps(self, x):
        """x: the trunk's input [2,M,B,3,H,W] (or [2,B,3,H,W]) -> the five distance maps [M*B,h_k,w_k] between x[0] and x[1].
        The trunk runs once per side and mask, on B images each time: 2 M calls of one and the same convolution problem.  MIOpen
        chooses its algorithm by problem size and lays a batch out over its workgroups as it likes, so only identical problems are
        promised identical arithmetic; with deterministic algorithms (no atomics) that makes a result independent of M, equal from call
        to call, and exactly 0 for identical images, by construction and not by MIOpen's grace."""
        H, W = x.shape[-2:]
        x = x.reshape(2, -1, x.shape[-4], 3, H, W)
        M, B = x.shape[1], x.shape[2]
        with deterministic_convolutions():
            feats = [[self.net(x[side, m]) for m in range(M)] for side in range(2)]
        maps = []
        for k in range(5):
            f0, f1 = (feats[side][0][k] if M == 1 else torch.cat([feats[side][m][k] for m in range(M)]) for side in range(2))
            maps.append(layer_distance(f0, f1, getattr(self, f"lin{k}").model[1].weight))
        return maps

    def distance(self, img0, img1, normalize: bool = False):
        """img0, img1 [B,H,W,3] in [-1, 1] ([0, 1] with normalize) -> [B]: the reference's spatial=False score, one number per pair."""
        return mean_score(self.layer_maps(prepare(img0, img1, None, normalize))).float()

    def score_map(self, img0, img1, normalize: bool = False):
        """-> [B,H,W]: the reference's spatial=True score."""
        H, W = img0.shape[1:3]
        return score(self.layer_maps(prepare(img0, img1, None, normalize)), H, W, None, want_map=True)[2][0]

    def masked_sums(self, preds, targets, masks=None):
        """preds, targets [B,H,W,3] in [0, 1]; masks None, [B,H,W] or [M,B,H,W] -> (sum_scores, mask_sum) float64 [M,B]: what one
        mLPIPS.update adds up per mask and image (flow3d/metrics.py:264-272: the images are multiplied by the mask, scaled to
        [-1, 1], scored spatially, and the score map is summed under the mask).  A mask's result is bitwise what it is alone (see layer_maps)."""
        x, m = _prepare(preds, targets, masks, True)
        s, t, _ = score(self.layer_maps(x), x.shape[-2], x.shape[-1], m)
        return s, t

    forward = distance


class mLPIPS(_Metric):
    """flow3d/metrics.py:220-279 around an `LPIPS`.  One entry per update: the masked sum of the score map over the whole batch and
    total = int64(sum mask) (the truncation matters for fractional masks); compute() is the mean of their ratios, nan for an empty mask."""
    _states = ("sum_scores", "total")

    def __init__(self, net: LPIPS, **kwargs):
        self.net = net
        super().__init__(**kwargs)

    def __len__(self) -> int:
        return len(self.total)

    def _append(self, sum_scores, mask_sum):
        self.sum_scores.append(sum_scores.sum())
        self.total.append(mask_sum.sum().to(torch.int64))

    @torch.no_grad()
    def update(self, preds, targets, masks=None):
        """preds, targets [B,H,W,3] in [0, 1]; masks [B,H,W] or None"""
        self._append(*self.net.masked_sums(preds, targets, masks))

    def compute(self) -> torch.Tensor:
        return (torch.stack(self.sum_scores) / torch.stack(self.total)).mean()
