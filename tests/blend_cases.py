"""Inputs of the exposure-blend edge tests, shared by the CPU test (tests/test_blend_ref.py) and the GPU tests
(tests/test_gpu_blend_edges.py) so that both see the same tensors.  Not a conftest: plain functions, cached.  Imports no product code.

THE GRID.  Every render and alpha value is a multiple of 2^-10 in [0, 1]; every cotangent a multiple of 2^-6 in [-4, 4], never zero.
For S <= 25 a sum of S such values is an integer multiple of 2^-10 below 25 * 1024 < 2^24: exact in fp32 in any order.  The mean
sum / S either equals a grid value (then the division is exact) or differs from every grid value by at least 1 / (1024 * S) > 3.9e-5,
far above an fp32 ulp, so every comparison the blend makes falls the same way in fp32 and in fp64 - no flip allowance.

THE CLASSES.  On a max / min channel each pixel carries one hand-built class (the label names it), the rest are random grid values.
The columns are built for a max channel in integer units of 2^-10; a min channel gets the mirror image 1024 - v, which turns every
max statement into the min statement (the mean mirrors too).  `zeros` is built per policy (a mirror would leave no zero).
  winner:j      the unique extreme sits at sub-sample j <= S - 2                                      -> j takes the whole gradient
  last_mean     the raw extreme sits at s = S - 1 (which the blend replaces by the mean) and the mean
                beats every candidate                                                                -> the gradient spreads, g / S each
  last_lower    the raw extreme sits at s = S - 1, but a candidate still beats the mean (S >= 3)      -> that candidate
  tie:a,b       candidates a < b hold the same extreme                                                -> a
  all_equal     all S values equal (the mean equals them exactly on this grid)                        -> raw_0, first in stack order
  mean_eq_cand  the mean equals the extreme candidate, not all equal (S >= 3; (0.5, 0.25, 0.75))      -> that candidate
  zeros         +0.0 and -0.0 among the candidates that hold the extreme 0                            -> the first of them
                (max: every value is a zero, raw_0 = +0.0; min: the first zero candidate is -0.0 - with these orders the blended
                zero carries the winner's sign whether the hardware's max / min orders -0 < +0 or keeps its first operand)
"""
from __future__ import annotations

import functools

import torch

UNIT = 1024            # renders, alphas: k / UNIT, k = 0 .. UNIT
COT_UNIT, COT_MAX = 64, 4
MEAN, MAX, MIN = 0, 1, 2
S_LIST = (1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 16, 17, 18, 25)
SHARD_S = (2, 3, 9, 11, 17)
RANDOM = "random"
TIES = ((0, None), (7, 8), (8, 9), (15, 16))  # (0, None): (0, S - 2)


def policy_of(shape: str, C: int) -> list[int]:
    p = [MEAN] * C
    if shape == "ref":  # the reference's: channel 3 max, channel 16 min
        if C > 3:
            p[3] = MAX
        if C > 16:
            p[16] = MIN
    elif shape == "ends":  # max on channel 0, min on the last one (C = 1: max only; "min0" is its twin)
        p[0] = MAX
        if C > 1:
            p[C - 1] = MIN
    elif shape == "min0":
        p[0] = MIN
    elif shape == "multi":  # several of each, neighbours included, the last two channels among them
        for c, v in ((0, MIN), (1, MAX), (2, MAX), (C // 2, MIN), (C - 2, MAX), (C - 1, MIN)):
            if 0 <= c < C:
                p[c] = v
    else:
        assert shape == "mean"
    return p


def classes_of(S: int) -> list[str]:
    """The hand-built classes that S admits."""
    if S < 2:
        return []
    cl = [f"winner:{j}" for j in range(S - 1)] + ["last_mean"]
    if S >= 3:
        cl.append("last_lower")
        for a, b in TIES:
            b = S - 2 if b is None else b
            if a < b <= S - 2 and f"tie:{a},{b}" not in cl:
                cl.append(f"tie:{a},{b}")
    cl.append("all_equal")
    if S >= 3:
        cl.append("mean_eq_cand")
    cl.append("zeros")
    return cl


def _column(cls: str, S: int, pol: int, k: int, g: torch.Generator) -> tuple[torch.Tensor, int]:
    """-> (the S values of one pixel of a `pol` channel as fp32, the winner: a sub-sample index, or -1 for the mean)."""
    ri = lambda lo, hi, n=1: torch.randint(lo, hi, (n,), generator=g)
    if cls == "zeros":
        sign = torch.where(ri(0, 2, S) == 1, -0.0, 0.0).float()
        if pol == MAX:  # all zeros, raw_0 = +0.0, at least one -0.0 behind it
            sign[0] = 0.0
            sign[S - 1 if S == 2 else 1 + k % (S - 2)] = -0.0
            return sign, 0
        v = ri(64, 512, S).float() / UNIT  # min: positive values, the zeros at z1 < z2 (and wherever else the coin says), z1 holds -0.0
        if S == 2:
            v[0] = -0.0
            return v, 0
        z1 = k % (S - 2)
        z2 = z1 + 1 + (k // (S - 2)) % (S - 2 - z1)
        for s in range(z1 + 1, S - 1):
            if int(ri(0, 4)) == 0:
                v[s] = sign[s]
        v[z1], v[z2] = -0.0, 0.0
        return v, z1
    v = ri(64, 512, S)  # "low"
    if cls.startswith("winner:"):
        w = int(cls[7:])
        v[w] = 900
    elif cls == "last_mean":  # candidates < 1024 / S <= the mean
        v = ri(0, UNIT // S, S)
        v[S - 1], w = UNIT, -1
    elif cls == "last_lower":
        v = ri(0, 100, S)
        w = k % (S - 1)
        v[S - 1], v[w] = 1000, 990  # mean <= (1990 + 100 (S - 2)) / S < 990
    elif cls.startswith("tie:"):
        w, b = (int(x) for x in cls[4:].split(","))
        v[w] = v[b] = 900
    elif cls == "all_equal":
        v[:] = ri(0, UNIT + 1)
        w = 0
    else:
        assert cls == "mean_eq_cand"
        w = k % (S - 1)
        d = ri(1, 21, S) if S > 3 else torch.full((S,), 256)  # S = 3: (0.5, 0.25, 0.75) and its orders
        v = 512 - d
        v[w], v[S - 1] = 512, 512 + int(d.sum() - d[w] - d[S - 1])
    assert 0 <= int(v.min()) and int(v.max()) <= UNIT
    if pol == MIN:
        v = UNIT - v
    return v.float() / UNIT, w


def _cot(g, *shape):
    k = torch.randint(-COT_MAX * COT_UNIT, COT_MAX * COT_UNIT + 1, shape, generator=g)
    return torch.where(k == 0, 1, k).float() / COT_UNIT


def _grid(g, *shape):
    return torch.randint(0, UNIT + 1, shape, generator=g).float() / UNIT


@functools.lru_cache(maxsize=None)
def case(S: int, H: int, W: int, C: int, shape: str) -> dict:
    """Treat as read-only (cached).  renders [S,H,W,C], alphas [S,H,W], w_out [H,W,C], w_acc [H,W], add_r, add_a (fp32, CPU); `label`
    [H,W] indexes `classes` (the last entry is RANDOM); `winner` [H,W,C] is what the construction promises on the hand-built pixels of a
    policy channel (-1: the mean), -2 wherever nothing is promised."""
    g = torch.Generator().manual_seed(1000 * S + 10 * C + H + sum(map(ord, shape)))
    policy = policy_of(shape, C)
    renders, alphas = _grid(g, S, H, W, C), _grid(g, S, H, W)
    classes = classes_of(S) + [RANDOM]
    n = len(classes) - 1
    period = n + max(1, n // 4)  # of every `period` pixels, the last n // 4 stay random
    label = torch.full((H * W,), n, dtype=torch.int64)
    winner = torch.full((H * W, C), -2, dtype=torch.int64)
    pol_ch = [c for c, p in enumerate(policy) if p != MEAN]
    for px in range(H * W if pol_ch else 0):
        i = px % period
        if i >= n:
            continue
        label[px] = i
        for c in pol_ch:
            col, w = _column(classes[i], S, policy[c], px // period, g)
            renders.view(S, H * W, C)[:, px, c] = col
            winner[px, c] = w
    return dict(S=S, H=H, W=W, C=C, shape=shape, policy=policy, renders=renders, alphas=alphas, w_out=_cot(g, H, W, C),
                w_acc=_cot(g, H, W), add_r=_cot(g, S, H, W, C), add_a=_cot(g, S, H, W), classes=classes, label=label.view(H, W),
                winner=winner.view(H, W, C))


def _table():
    """Per S: one case with the reference's policy and two others, rotating through the channel counts, policy shapes and image sizes.
    H * W * C is never a multiple of 256 and always more than one 256-lane block; 8 x 9 has a pixel count that is a multiple of 4."""
    ref = ((7, 9, 17), (8, 9, 5), (7, 9, 64))
    other = ((19, 27, 5, "multi"), (19, 27, 1, "min0"), (7, 9, 64, "ends"), (8, 9, 17, "multi"), (19, 27, 1, "ends"), (19, 27, 64, "multi"),
             (7, 9, 5, "mean"), (19, 27, 17, "ends"))
    keys = []
    for i, S in enumerate(S_LIST):
        keys.append((S, *ref[i % 3], "ref"))
        keys += [(S, *other[(2 * i + j) % 8]) for j in ((0, 1) if S in SHARD_S + (1, 12, 18, 25) else (0,))]
    # the sharded tests want a min channel and a many-channel policy at every SHARD_S, and the reference's two policy channels at S = 2
    keys += [(2, 7, 9, 17, "ref"), (3, 19, 27, 1, "min0"), (9, 19, 27, 1, "min0")]
    assert len(set(keys)) == len(keys)
    for S, H, W, C, _ in keys:
        assert (H * W * C) % 256 != 0 and H * W * C > 256, (H, W, C)
    return tuple(keys)


KEYS = _table()
IDS = [f"S{S}-{H}x{W}-C{C}-{shape}" for S, H, W, C, shape in KEYS]
SHARD_KEYS = tuple(k for k in KEYS if k[0] in SHARD_S)
SHARD_IDS = [IDS[KEYS.index(k)] for k in SHARD_KEYS]
