"""CPU: the case table of the exposure-blend edge tests (tests/blend_cases.py) is what it claims to be, and the general-policy fp64
reference the GPU tests compare with (tests/blend_ref.py) equals the literal restatement of the reference's blend
(oracle.scene.blend_exposure) wherever that one applies - the reference's policy - value and gradients, exactly."""
import pytest
import torch

from tests import blend_cases as bc
from tests import blend_ref


def _case(key):
    return bc.case(*key)


def test_the_table_covers_every_size_channel_count_and_policy_shape():
    assert {k[0] for k in bc.KEYS} == set(bc.S_LIST)
    assert {k[3] for k in bc.KEYS} == {1, 5, 17, 64}
    assert {k[4] for k in bc.KEYS} == {"ref", "ends", "min0", "multi", "mean"}
    assert {(7, 9), (19, 27)} <= {k[1:3] for k in bc.KEYS}
    px = {k[1] * k[2] for k in bc.KEYS}
    assert any(p % 4 == 0 for p in px) and any(p % 4 for p in px)
    assert 35 <= len(bc.KEYS) <= 45
    assert bc.policy_of("ends", 64)[63] == bc.MIN and bc.policy_of("ends", 64)[0] == bc.MAX
    for S in bc.SHARD_S:  # what the sharded tests count on
        pols = [bc.policy_of(k[4], k[3]) for k in bc.SHARD_KEYS if k[0] == S]
        assert any(bc.MIN in p for p in pols) and any(sum(1 for v in p if v) >= 3 for p in pols), S
        assert any(k[0] == S and k[4] == "ref" and k[3] >= 17 for k in bc.SHARD_KEYS), S  # the reference's max AND min channel
    # each tie class at each S that admits it (every S has a case with a policy channel, and every such case carries all its classes)
    assert "tie:0,1" in bc.classes_of(3) and "tie:7,8" in bc.classes_of(10) and "tie:7,8" not in bc.classes_of(9)
    assert "tie:8,9" in bc.classes_of(11) and "tie:8,9" not in bc.classes_of(10)
    assert "tie:15,16" in bc.classes_of(18) and "tie:15,16" not in bc.classes_of(17)
    assert bc.classes_of(25)[:24] == [f"winner:{j}" for j in range(24)] and bc.classes_of(1) == []
    assert "last_lower" not in bc.classes_of(2) and "mean_eq_cand" not in bc.classes_of(2)
    for S in bc.S_LIST:
        assert any(k[0] == S and any(bc.policy_of(k[4], k[3])) for k in bc.KEYS), S


@pytest.mark.parametrize("key", bc.KEYS, ids=bc.IDS)
def test_case_is_on_the_grid_and_carries_its_classes(key):
    """The grid conditions that make every fp32 comparison of the blend fall as in fp64 (derived in blend_cases.py, asserted here), the
    promised classes where promised, and at least half of the policy-channel pixels hand-built."""
    cs = _case(key)
    S, H, W, C, pol = cs["S"], cs["H"], cs["W"], cs["C"], cs["policy"]
    assert cs["renders"].shape == (S, H, W, C) and cs["alphas"].shape == (S, H, W) and cs["renders"].dtype == torch.float32
    for name in ("renders", "alphas"):
        k = cs[name].double() * bc.UNIT
        assert torch.equal(k, k.round()) and float(k.min()) >= 0 and float(k.max()) <= bc.UNIT, name
        tot = cs[name].double().sum(0) * bc.UNIT
        assert torch.equal(tot, tot.round()) and float(tot.max()) < 2 ** 24, name  # the S-term sum: an integer of 2^-10, exact in fp32
    for name in ("w_out", "w_acc", "add_r", "add_a"):
        k = cs[name].double() * bc.COT_UNIT
        assert torch.equal(k, k.round()) and float(k.abs().max()) <= bc.COT_MAX * bc.COT_UNIT and float(k.abs().min()) >= 1, name
    pc = [c for c, p in enumerate(pol) if p]
    r = cs["renders"].double()
    mean = r.sum(0) / S
    for c in pc:
        d = (mean[..., c][None] - r[..., c]).abs()
        assert bool(((d == 0) | (d >= 1.0 / (bc.UNIT * S) * (1 - 1e-9))).all()), c  # equal, or apart by far more than an fp32 ulp
    lab, classes = cs["label"], cs["classes"]
    assert classes[-1] == bc.RANDOM and classes[:-1] == bc.classes_of(S)
    if not pc:
        assert bool((lab == len(classes) - 1).all())
        return
    present = set(lab.unique().tolist())
    assert present == set(range(len(classes))), [classes[i] for i in set(range(len(classes))) - present]
    if S >= 3:
        assert float((lab != len(classes) - 1).double().mean()) >= 0.5
    # the label tells the truth: the fp64 reference finds the promised winner on every hand-built pixel of every policy channel
    ref = blend_ref.forward(cs["renders"], cs["alphas"], pol)
    for c in pc:
        built = cs["winner"][..., c] != -2
        assert torch.equal(built, lab != len(classes) - 1)
        bad = built & (ref["winner"][..., c] != cs["winner"][..., c])
        assert not bool(bad.any()), (c, sorted({classes[i] for i in lab[bad].tolist()}))
    # ... and the classes are what their names say
    cols = r.view(S, H * W, C)
    flat = lab.view(-1)
    for i, name in enumerate(classes[:-1]):
        for px in (flat == i).nonzero().view(-1).tolist():
            for c in pc:
                col = cols[:, px, c] if pol[c] == bc.MAX else -cols[:, px, c]  # (as a max problem)
                w = int(cs["winner"].view(-1, C)[px, c])
                cand, m = col[:S - 1], col.sum() / S
                if name.startswith("winner:"):
                    assert w == int(name[7:]) and int((cand == cand.max()).sum()) == 1 and cand[w] > max(m, col[S - 1])
                elif name == "last_mean":
                    assert w == -1 and col[S - 1] > cand.max() and m > cand.max()
                elif name == "last_lower":
                    assert col[S - 1] > cand.max() and cand[w] > m and int((cand == cand.max()).sum()) == 1
                elif name.startswith("tie:"):
                    a, b = (int(x) for x in name[4:].split(","))
                    assert w == a and cand[a] == cand[b] == cand.max() and int((cand == cand.max()).sum()) == 2 and cand[a] > m
                elif name == "all_equal":
                    assert w == 0 and bool((col == col[0]).all()) and m == col[0]
                elif name == "mean_eq_cand":
                    assert m == cand[w] and int((cand == cand.max()).sum()) == 1 and cand[w] == cand.max() and not bool((col == col[0]).all())
                else:
                    assert name == "zeros"
                    z = cols[:, px, c]
                    zero_c = (z[:S - 1] == 0).nonzero().view(-1).tolist()
                    assert zero_c and w == zero_c[0] and cand[w] == cand.max() and cand[w] >= m
                    sb = torch.signbit(z[z == 0])
                    assert bool(sb.any()) and (S == 2 and pol[c] == bc.MIN or not bool(sb.all()))  # both signs (one zero only: -0.0)
                    assert bool(torch.signbit(z[w])) == (pol[c] == bc.MIN)


REF_KEYS = [k for k in bc.KEYS if k[4] == "ref"]


@pytest.mark.parametrize("key", REF_KEYS, ids=[bc.IDS[bc.KEYS.index(k)] for k in REF_KEYS])
def test_blend_ref_equals_the_oracle_blend_on_the_reference_policy(key):
    from oracle import scene as oscene

    cs = _case(key)
    S = cs["S"]
    r, a = cs["renders"].double().requires_grad_(), cs["alphas"].double().requires_grad_()
    out, acc, _ = oscene.blend_exposure([r[s][None] for s in range(S)], [a[s][None] for s in range(S)], single=(S == 1))
    ((out[0] * cs["w_out"].double()).sum() + (acc[0] * cs["w_acc"].double()).sum() + (r * cs["add_r"].double()).sum()
     + (a * cs["add_a"].double()).sum()).backward()
    ref = blend_ref.forward(cs["renders"], cs["alphas"], cs["policy"])
    v_r, v_a = blend_ref.backward(S, ref["winner"], cs["w_out"], cs["w_acc"], cs["add_r"], cs["add_a"])
    assert torch.equal(ref["out"], out[0].detach()) and torch.equal(ref["acc"], acc[0].detach())
    assert torch.equal(v_r, r.grad) and torch.equal(v_a, a.grad)
    v_r0, v_a0 = blend_ref.backward(S, ref["winner"], cs["w_out"], cs["w_acc"])
    assert torch.equal(v_r0 + cs["add_r"].double(), v_r) and torch.equal(v_a0 + cs["add_a"].double(), v_a)
    assert int((v_r0 == 0).sum()) == (S - 1) * int((ref["winner"] >= 0).sum())  # a raw winner takes it all
