"""GPU: the exposure blend (csrc/blend.hip) on exactly representable inputs, at every unroll edge of its sums and scans and at every
kind of tie - against the general-policy fp64 reference tests/blend_ref.py (pinned to the oracle's blend on the CPU,
tests/test_blend_ref.py), case by case from tests/blend_cases.py.

On that grid every S-term sum is exact in fp32 and no comparison of the blend can fall differently in fp32 and in fp64, so nothing here
carries a flip allowance: a max / min channel is compared bit for bit, the routing of its gradient exactly, a mean to one ulp.

Outside the contract and untested: NaN or infinite renders (fmaxf drops a NaN where torch.max propagates it)."""
import ctypes as C
import functools

import pytest
import torch

from tests import blend_cases as bc
from tests import blend_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ulps(a, b):
    """Distance of two fp32 tensors in units in the last place (the floats in order as integers; -0.0 and +0.0 coincide)."""
    def key(t):
        i = _bits(t).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)

    return (key(a) - key(b)).abs()


def _classes_at(cs, bad):
    """The class labels of the pixels where `bad` ([..., H, W, C] or [..., H, W]) is set."""
    if bad.dim() > 2 and bad.shape[-1] == cs["C"] and bad.shape[-3:-1] == cs["label"].shape:
        bad = bad.any(-1)
    while bad.dim() > 2:
        bad = bad.any(0)
    return sorted({cs["classes"][i] for i in cs["label"][bad].tolist()})


@functools.lru_cache(maxsize=None)
def _ref(key):
    cs = bc.case(*key)
    ref = blend_ref.forward(cs["renders"], cs["alphas"], cs["policy"])
    ref["v_r"], ref["v_a"] = blend_ref.backward(cs["S"], ref["winner"], cs["w_out"], cs["w_acc"])
    return ref


@functools.lru_cache(maxsize=None)
def _blend_fn(key):
    """exposure.BlendFn on the case, forward and backward -> CPU tensors.  Computed once per case; read-only."""
    from deblur4dgs_amd.exposure import BlendFn

    cs = bc.case(*key)
    r, a = cs["renders"].to(DEV).requires_grad_(), cs["alphas"].to(DEV).requires_grad_()
    out, acc = BlendFn.apply(r, a, cs["policy"])
    torch.autograd.backward([out, acc], [cs["w_out"].to(DEV), cs["w_acc"].to(DEV)])
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), acc=acc.detach().cpu(), v_r=r.grad.cpu(), v_a=a.grad.cpu())


@pytest.mark.parametrize("key", bc.KEYS, ids=bc.IDS)
def test_blend_fn_equals_the_fp64_reference_on_the_grid(key):
    """d4gs_blend_fwd / d4gs_blend_bwd through BlendFn.  Where a raw value wins, `out` is that fp32 input bit for bit; where the mean
    does - and on every mean channel and `acc` - it is within 1 ulp of the fp64 mean rounded to fp32 (an exact sum, one correctly
    rounded division; the ulp is the reference's double rounding).  The gradient routing is exact: zero where the reference is zero,
    exactly g on the winner; a spread entry is within 4 * 2^-24 |g| / S of g / S (the kernel multiplies by a rounded 1 / S: two
    roundings), v_alphas within 1 ulp of v_acc / S."""
    cs, ref, got = bc.case(*key), _ref(key), _blend_fn(key)
    S = cs["S"]
    win = ref["winner"]
    raw = win >= 0
    want_raw = torch.gather(cs["renders"], 0, win.clamp(min=0)[None])[0]
    bad = raw & (_bits(got["out"]) != _bits(want_raw))
    assert not bool(bad.any()), ("out, a raw value wins", int(bad.sum()), _classes_at(cs, bad))
    u = _ulps(got["out"], ref["out"].float())
    print(f"{key}: out where the mean wins: max {int(u[~raw].max()) if bool((~raw).any()) else 0} ulp; "
          f"acc: max {int(_ulps(got['acc'], ref['acc'].float()).max())} ulp")
    bad = ~raw & (u > 1)
    assert not bool(bad.any()), ("out, the mean", int(u[~raw].max()), _classes_at(cs, bad))
    assert int(_ulps(got["acc"], ref["acc"].float()).max()) <= 1

    g = cs["w_out"].double()
    v_r = got["v_r"]
    zero = ref["v_r"] == 0  # (the cotangents are never zero: a zero is a sub-sample that lost)
    bad = zero & (v_r != 0)
    assert not bool(bad.any()), ("v_renders, must be zero", int(bad.sum()), _classes_at(cs, bad))
    s = torch.arange(S).view(S, 1, 1, 1)
    takes = win[None] == s
    bad = takes & (_bits(v_r) != _bits(cs["w_out"])[None])
    assert not bool(bad.any()), ("v_renders, the winner takes g", int(bad.sum()), _classes_at(cs, bad))
    assert torch.equal(takes | zero, raw[None].expand_as(zero))
    spread = ~raw[None].expand_as(zero)
    err = (v_r.double() - (g / S)[None]).abs()
    bad = spread & (err > 4 * 2.0 ** -24 * (g.abs() / S)[None])
    print(f"{key}: spread entries: max |got - g/S| / (2^-24 |g|/S) = "
          f"{float((err / (2.0 ** -24 * (g.abs() / S)[None]))[spread].max()) if bool(spread.any()) else 0.0:.3f}")
    assert not bool(bad.any()), ("v_renders, spread", int(bad.sum()), _classes_at(cs, bad))
    ua = _ulps(got["v_a"], (cs["w_acc"].double() / S).float()[None].expand(S, -1, -1))
    assert int(ua.max()) <= 1, ("v_alphas", int(ua.max()))


NULL_KEYS = [k for k in bc.KEYS if k[0] in (1, 2, 11, 25)]


@pytest.mark.parametrize("key", NULL_KEYS, ids=[bc.IDS[bc.KEYS.index(k)] for k in NULL_KEYS])
def test_blend_bwd_takes_a_null_cotangent_for_either_output(key):
    """d4gs_blend_bwd through ctypes with v_out = NULL, then with v_acc = NULL: the missing half gives exact zeros, the other half is
    the full call's bit for bit."""
    from deblur4dgs_amd import _lib as L
    from deblur4dgs_amd.engine import _stream

    cs = bc.case(*key)
    S, H, W, Cn = cs["S"], cs["H"], cs["W"], cs["C"]
    lib = L.lib()
    pol = (C.c_int32 * Cn)(*cs["policy"])
    r, a = cs["renders"].to(DEV), cs["alphas"].to(DEV)
    out, acc = torch.empty(H, W, Cn, device=DEV), torch.empty(H, W, device=DEV)
    L.check(lib.d4gs_blend_fwd(S, H * W, Cn, pol, L.ptr(r), L.ptr(a), L.ptr(out), L.ptr(acc), _stream()), "d4gs_blend_fwd")
    v_out, v_acc = cs["w_out"].to(DEV), cs["w_acc"].to(DEV)

    def bwd(vo, va):
        v_r, v_a = torch.full_like(r, float("nan")), torch.full_like(a, float("nan"))
        L.check(lib.d4gs_blend_bwd(S, H * W, Cn, pol, L.ptr(r), L.ptr(out), L.ptr(vo), L.ptr(va), L.ptr(v_r), L.ptr(v_a), _stream()),
                "d4gs_blend_bwd")
        torch.cuda.synchronize()
        return v_r.cpu(), v_a.cpu()

    full_r, full_a = bwd(v_out, v_acc)
    fn = _blend_fn(key)
    assert torch.equal(_bits(full_r), _bits(fn["v_r"])) and torch.equal(_bits(full_a), _bits(fn["v_a"]))
    no_out_r, no_out_a = bwd(None, v_acc)
    assert bool((no_out_r == 0).all()) and torch.equal(_bits(no_out_a), _bits(full_a))
    no_acc_r, no_acc_a = bwd(v_out, None)
    assert bool((no_acc_a == 0).all()) and torch.equal(_bits(no_acc_r), _bits(full_r))


@pytest.mark.parametrize("Cn", [0, 65])
def test_blend_entry_points_reject_a_channel_count_out_of_range(Cn):
    """C = 0 and C = 65 (the policy travels as 64 bytes): D4GS_EINVAL with the error string set, nothing launched, the outputs untouched."""
    from deblur4dgs_amd import _lib as L
    from deblur4dgs_amd.engine import _stream

    S, P = 3, 70
    lib = L.lib()
    pol = (C.c_int32 * 65)(*([0] * 65))
    mk = lambda *shape: torch.full(shape, 7.0, device=DEV)  # (every buffer holds 65 channels: whatever ran would stay inside)
    r, a, out, acc = mk(S, P, 65), mk(S, P), mk(P, 65), mk(P)
    v_out, v_acc, v_r, v_a = mk(P, 65), mk(P), mk(S, P, 65), mk(S, P)
    rc = lib.d4gs_blend_fwd(S, P, Cn, pol, L.ptr(r), L.ptr(a), L.ptr(out), L.ptr(acc), _stream())
    assert rc == -1 and f"blend: C={Cn} out of range".encode() in lib.d4gs_last_error(), (rc, lib.d4gs_last_error())
    rc = lib.d4gs_blend_bwd(S, P, Cn, pol, L.ptr(r), L.ptr(out), L.ptr(v_out), L.ptr(v_acc), L.ptr(v_r), L.ptr(v_a), _stream())
    assert rc == -1 and f"blend: C={Cn} out of range".encode() in lib.d4gs_last_error(), (rc, lib.d4gs_last_error())
    torch.cuda.synchronize()
    for t in (out, acc, v_r, v_a):
        assert bool((t == 7.0).all())


def _worlds(S):
    return sorted({2, 3, 4, S, S + 1})


SHARD_PARAMS = [(k, w) for k in bc.SHARD_KEYS for w in _worlds(k[0])]


@pytest.mark.parametrize("key,world", SHARD_PARAMS, ids=[f"{bc.IDS[bc.KEYS.index(k)]}-world{w}" for k, w in SHARD_PARAMS])
def test_shard_kernels_of_every_rank_equal_the_single_gpu_blend_bitwise(key, world):
    """d4gs_blend_shard_*, all `world` ranks emulated on one GPU, the all-reduces as tensor ops (SUM of the parts, MAX of the candidates,
    MIN of the winners).  On the grid the rank-local partial sums are exact, so the sharded blend equals BlendFn bit for bit: policy
    channels, mean channels, acc and every gradient - for the min policy and many policy channels too, with ranks that own nothing
    (world = S + 1: their candidate stays -inf and never wins) and ranks that own only the last sub-sample (never a candidate).
    One allowance: on the `zeros` pixels the blended zero is compared by value - a MAX all-reduce, RCCL's or a tensor op's, leaves the
    sign of max(-0.0, +0.0) open.  The routing there is still exact."""
    from deblur4dgs_amd import _lib as L
    from deblur4dgs_amd.engine import _stream
    from deblur4dgs_amd.parallel import _shard_desc, owned_subsamples

    cs, want = bc.case(*key), _blend_fn(key)
    S, H, W, Cn, pol = cs["S"], cs["H"], cs["W"], cs["C"], cs["policy"]
    npol = sum(1 for p in pol if p)
    renders, alphas = cs["renders"].to(DEV), cs["alphas"].to(DEV)
    v_out, v_acc = cs["w_out"].to(DEV), cs["w_acc"].to(DEV)
    lib = L.lib()
    parts, cands, descs, locs = [], [], [], []
    for r in range(world):
        own = owned_subsamples(S, world, r)
        lr, la = renders[own].contiguous(), alphas[own].contiguous()
        desc, keep = _shard_desc(len(own), S, own, Cn, H * W, pol)
        part = torch.empty(H, W, Cn + 1, device=DEV)
        cand = torch.empty(H, W, max(npol, 1), device=DEV)
        L.check(lib.d4gs_blend_shard_partial_fwd(C.byref(desc), L.ptr(lr), L.ptr(la), L.ptr(part), L.ptr(cand), _stream()), "partial")
        if npol and not any(s <= S - 2 for s in own):
            assert bool((cand == -float("inf")).all()), r  # nothing to offer: the empty rank, the rank of the last sub-sample
        parts.append(part), cands.append(cand), descs.append((desc, keep)), locs.append((own, lr, la))
    part = torch.stack(parts).sum(0)              # all-reduce SUM
    cand = torch.stack(cands).amax(0)             # all-reduce MAX
    out, acc = torch.empty(H, W, Cn, device=DEV), torch.empty(H, W, device=DEV)
    L.check(lib.d4gs_blend_shard_finish_fwd(C.byref(descs[0][0]), L.ptr(part), L.ptr(cand), L.ptr(out), L.ptr(acc), _stream()), "finish")
    torch.cuda.synchronize()
    zeros = (cs["label"] == cs["classes"].index("zeros"))[..., None].expand(H, W, Cn) if "zeros" in cs["classes"] else \
        torch.zeros(H, W, Cn, dtype=torch.bool)
    bad = torch.where(zeros, out.cpu() != want["out"], _bits(out) != _bits(want["out"]))
    assert not bool(bad.any()), ("out", int(bad.sum()), [c for c in range(Cn) if bool(bad[..., c].any())], _classes_at(cs, bad))
    assert torch.equal(_bits(acc), _bits(want["acc"]))
    wins = []
    for r in range(world):
        own, lr, la = locs[r]
        win = torch.full((H, W, max(npol, 1)), S, dtype=torch.int32, device=DEV)
        # (each rank compares with the REDUCED image, as after the forward collectives)
        L.check(lib.d4gs_blend_shard_winner(C.byref(descs[r][0]), L.ptr(lr), L.ptr(out), L.ptr(win), _stream()), "winner")
        wins.append(win)
    win = torch.stack(wins).amin(0)  # all-reduce MIN
    for r in range(world):
        own, lr, la = locs[r]
        v_r, v_a = torch.empty_like(lr), torch.empty_like(la)
        L.check(lib.d4gs_blend_shard_bwd(C.byref(descs[r][0]), L.ptr(v_out), L.ptr(v_acc), L.ptr(win), L.ptr(v_r), L.ptr(v_a),
                                         _stream()), "bwd")
        torch.cuda.synchronize()
        if len(own):
            bad = _bits(v_r) != _bits(want["v_r"][own])
            assert not bool(bad.any()), ("v_renders", r, own, int(bad.sum()), _classes_at(cs, bad))
            assert torch.equal(_bits(v_a), _bits(want["v_a"][own])), ("v_alphas", r)
