"""The LPIPS metric (AlexNet, version 0.1) restated in fp64 with plain torch: what tests/golden/lpips.npz records of the reference's
PNetLin, and what the kernels of csrc/lpips.hip are held to.  The rules also stand on explicit feature tensors and layer maps
(`layer_map`, `score_map`, `mean_score`), for the tests of the head alone.

    scaling layer   (x - shift) / scale per channel, x in [-1, 1]
    trunk           conv 3->64 11x11 s4 p2, ReLU | maxpool 3/2, conv 64->192 5x5 p2, ReLU | maxpool 3/2, conv 192->384 3x3 p1, ReLU |
                    conv 384->256 3x3 p1, ReLU | conv 256->256 3x3 p1, ReLU; the five ReLU outputs are the features
    per layer       g = f / (sqrt(sum_c f_c^2) + 1e-10);  d = sum_c w_c (g0_c - g1_c)^2
    spatial score   every d bilinearly upsampled to H x W (align_corners=False, source = (dst + 0.5) / (1. * H / h) - 0.5 clamped at 0),
                    added in layer order
    mean score      the mean over h x w of every d, added in layer order
    mLPIPS          images * mask, 2 x - 1, spatial score; one entry per update: sum(score * mask) / int64(sum mask)

The trunk of the tests is not a trained one (about 10 MB): `seeded_trunk` draws every tensor from its own generator seed, rounded to
fp32; the fixture stores its checksum.  The head weights are the reference's (1 152 floats, in the fixture)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips.npz")
CHANNELS = (64, 192, 384, 256, 256)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
#         features index, c_in, c_out, kernel, stride, padding, max-pool in front
CONVS = ((0, 3, 64, 11, 4, 2, False), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, True), (8, 384, 256, 3, 1, 1, False),
         (10, 256, 256, 3, 1, 1, False))
TRUNK_SEED = 7100
SHAPES = ((1, 31, 31), (1, 35, 35), (2, 47, 64), (1, 64, 99))
VALIDATOR_SHAPE = SHAPES[2]
IMAGES = ("uniform", "same")
MASKS = ("none", "ones", "zero", "bernoulli", "dyadic")


def shape_name(s):
    return "x".join(str(v) for v in s)


def alex_sizes(H, W):
    h1, w1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return ((h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3))


def seeded_trunk(seed=TRUNK_SEED):
    """torchvision's key layout -> fp32 tensor.  Tensor j (weight, bias of each convolution in turn) comes from the generator seeded
    seed + j: weights normal with variance 2 / fan_in (what keeps a ReLU network's activations at the scale of its input), biases
    normal with deviation 0.05."""
    state, j = {}, 0
    for i, cin, cout, k, _, _, _ in CONVS:
        for leaf, shape, dev in (("weight", (cout, cin, k, k), (2.0 / (cin * k * k)) ** 0.5), ("bias", (cout,), 0.05)):
            g = torch.Generator().manual_seed(seed + j)
            state[f"features.{i}.{leaf}"] = (dev * torch.randn(shape, generator=g, dtype=torch.float64)).float()
            j += 1
    return state


def checksum(state):
    """(sum, sum of absolute values) over every tensor, in fp64"""
    return [float(sum(v.double().sum() for v in state.values())), float(sum(v.double().abs().sum() for v in state.values()))]


def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def head_weights(fx, dtype=torch.float64):
    return [torch.from_numpy(fx[f"lin{k}"]).to(dtype) for k in range(5)]


def lins_state(fx):
    """the recorded head weights under the reference's keys"""
    return {f"lin{k}.model.1.weight": torch.from_numpy(fx[f"lin{k}"]).reshape(1, -1, 1, 1) for k in range(5)}


def images_of(fx, sname, kind):
    pred = torch.from_numpy(fx[f"{sname}/pred"])
    return (pred, pred.clone()) if kind == "same" else (pred, torch.from_numpy(fx[f"{sname}/target"]))


def mask_of(fx, sname, mk):
    B, H, W = (int(v) for v in sname.split("x"))
    if mk == "none":
        return None
    if mk in ("ones", "zero"):
        return torch.full((B, H, W), 1.0 if mk == "ones" else 0.0)
    return torch.from_numpy(fx[f"{sname}/mask/{mk}"])


def validator_masks(fx):
    valid, fg = torch.from_numpy(fx["validator/valid_mask"]), torch.from_numpy(fx["validator/fg_mask"])
    return valid, fg, {"main": valid, "fg": fg * valid, "bg": (1 - fg) * valid}


# ---- the rules -------------------------------------------------------------------------------------------------------------------

def scaling(x):
    """x [n,3,H,W].  The constants are fp32 numbers (the reference holds them in float32 buffers), whatever x's precision"""
    shift, scale = (torch.tensor(v, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1) for v in (SHIFT, SCALE))
    return (x - shift) / scale


def trunk(x, state):
    """x [n,3,H,W] (scaled) -> the five features, in x's dtype"""
    feats = []
    for i, _, _, _, stride, pad, pool in CONVS:
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, state[f"features.{i}.weight"].to(x.dtype), state[f"features.{i}.bias"].to(x.dtype), stride=stride, padding=pad))
        feats.append(x)
    return feats


def layer_terms(f0, f1, w):
    """f0, f1 [n,C,h,w], w [C] -> (d, sum_c |w_c| (g0_c - g1_c)^2), each [n,h,w], in fp64"""
    f0, f1, w = f0.double(), f1.double(), w.double().view(1, -1, 1, 1)
    g0 = f0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10)
    g1 = f1 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + 1e-10)
    sq = (g0 - g1) ** 2
    return (w * sq).sum(1), (w.abs() * sq).sum(1)


def layer_map(f0, f1, w):
    return layer_terms(f0, f1, w)[0]


def _source(dst_size, src_size, dtype):
    src = ((torch.arange(dst_size, dtype=dtype) + 0.5) * (1.0 / (1.0 * dst_size / src_size)) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=src_size - 1)
    return i0, (i0 + 1).clamp(max=src_size - 1), src - i0


def upsample(d, H, W):
    """d [n,h,w] -> [n,H,W], bilinear, align_corners=False"""
    y0, y1, ly = _source(H, d.shape[1], d.dtype)
    x0, x1, lx = _source(W, d.shape[2], d.dtype)
    ly = ly.view(1, H, 1)
    row = lambda y: (1 - lx) * d[:, y][:, :, x0] + lx * d[:, y][:, :, x1]
    return (1 - ly) * row(y0) + ly * row(y1)


def score_map(layer_maps, H, W):
    out = upsample(layer_maps[0].double(), H, W)
    for d in layer_maps[1:]:
        out = out + upsample(d.double(), H, W)
    return out


def mean_score(layer_maps):
    out = layer_maps[0].double().mean((1, 2))
    for d in layer_maps[1:]:
        out = out + d.double().mean((1, 2))
    return out


def layer_maps_of(img0, img1, state, lins, normalize=False):
    """img0, img1 [B,H,W,3] -> the five [B,h,w] maps, fp64"""
    x0, x1 = (v.double().permute(0, 3, 1, 2) for v in (img0, img1))
    if normalize:
        x0, x1 = 2 * x0 - 1, 2 * x1 - 1
    f0, f1 = trunk(scaling(x0), state), trunk(scaling(x1), state)
    return [layer_map(a, b, w) for a, b, w in zip(f0, f1, lins)]


def masked_sums(preds, targets, masks, state, lins):
    """one mLPIPS update: preds, targets [B,H,W,3] in [0, 1], masks [B,H,W] or None -> (sum of score * mask, int64(sum mask))"""
    m = torch.ones_like(preds[..., 0]) if masks is None else masks
    maps = layer_maps_of(preds * m[..., None], targets * m[..., None], state, lins, normalize=True)
    scores = score_map(maps, preds.shape[1], preds.shape[2])
    return (scores * m.double()).sum(), m.sum().to(torch.int64)
