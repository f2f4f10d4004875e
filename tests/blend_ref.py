"""The exposure blend (csrc/blend.hip) restated in fp64 for an ARBITRARY per-channel policy, forward and adjoint.  It routes
explicitly - the winner is the first index of the extreme over the stack [raw_0 .. raw_{S-2}, mean] - and does not rely on what
autograd does at a tie.  tests/test_blend_ref.py pins it to oracle.scene.blend_exposure (the literal restatement of the reference's
scene_model.py:386-397) on the reference's policy.  Imports no product code."""
from __future__ import annotations

import torch

MEAN, MAX, MIN = 0, 1, 2


def forward(renders: torch.Tensor, alphas: torch.Tensor, policy) -> dict:
    """renders [S,H,W,C], alphas [S,H,W] -> fp64 out [H,W,C], acc [H,W], mean [H,W,C] and winner int64 [H,W,C]: the sub-sample whose raw
    value the blend takes (and hands the whole gradient to), -1 where it takes the mean (every mean channel; everything at S = 1)."""
    r = renders.double()
    S = r.shape[0]
    mean = r[0].clone() if S == 1 else r.sum(0) / S
    winner = torch.full(mean.shape, -1, dtype=torch.int64)
    out = mean.clone()
    if S > 1:
        idx = torch.arange(S).view(S, 1, 1)
        for c, p in enumerate(policy):
            if p == MEAN:
                continue
            stack = torch.cat([r[:S - 1, ..., c], mean[None, ..., c]], 0)  # the last slot holds the mean: the reference's in-place write
            ext = stack.max(0).values if p == MAX else stack.min(0).values
            first = torch.where(stack == ext, idx, S).min(0).values  # (-0.0 == +0.0: the first of them)
            assert int(first.max()) < S
            winner[..., c] = torch.where(first == S - 1, -1, first)
            out[..., c] = torch.gather(stack, 0, first[None])[0]
    return dict(out=out, acc=alphas.double().sum(0) / S if S > 1 else alphas[0].double().clone(), mean=mean, winner=winner)


def backward(S: int, winner: torch.Tensor, v_out, v_acc, add_r=None, add_a=None):
    """-> fp64 v_renders [S,H,W,C], v_alphas [S,H,W] for cotangents v_out [H,W,C], v_acc [H,W] (None: zero) and the optional
    cotangents add_r / add_a held on the sub-sample images themselves."""
    H, W, C = winner.shape
    g = torch.zeros(H, W, C, dtype=torch.float64) if v_out is None else v_out.double()
    s = torch.arange(S).view(S, 1, 1, 1)
    v_r = torch.where(winner[None] < 0, (g / S)[None].expand(S, H, W, C), torch.where(winner[None] == s, g[None], 0.0))
    ga = torch.zeros(H, W, dtype=torch.float64) if v_acc is None else v_acc.double()
    v_a = (ga / S)[None].expand(S, H, W).clone()
    if add_r is not None:
        v_r = v_r + add_r.double()
    if add_a is not None:
        v_a = v_a + add_a.double()
    return v_r, v_a
