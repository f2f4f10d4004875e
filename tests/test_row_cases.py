"""The per-row comparison proved before any device is involved: the scenes of tests/row_cases.py and the checker tests/util.check_rows.

  reference margin   on every case, cotangent kind, tensor and group the fp32 oracle against the fp64 oracle passes `check_rows` with
                     every cap HALVED: what the device is held to, the reference's own arithmetic keeps with room;
  groups             the strata really are below the tensor's maximum (that is what makes the row norm bite where the tensor norm
                     does not), and every group has rows to speak of;
  mutation           a gradient whose small rows are all 0.5 % off passes `check` at (1e-4, 0) and fails `check_rows`; negated tail
                     rows fail it too;
  dtype              the oracle of the fused path runs in fp32 end to end (no fp64 constant sneaks in)."""
import pytest
import torch

from tests import row_cases as rc
from tests import util
from tests.util import check, check_rows, row_errors

CASES = [("s1", n) for n in rc.S1_CASES] + [("fused", n) for n in rc.FUSED]


def _load(seam, name):
    if seam == "s1":
        return rc.s1_case(name), rc.s1_reference(name), rc.S1_TENSORS
    return rc.fused_case(name), rc.fused_reference(name), rc.FUSED_TENSORS


@pytest.fixture(autouse=True)
def _keep_the_parity_table_for_the_device():
    """`check` / `check_rows` log what they compare; oracle against oracle does not belong in the device's parity table."""
    n = len(util.PARITY_LOG)
    yield
    del util.PARITY_LOG[n:]


@pytest.mark.parametrize("seam,name", CASES)
def test_the_fp32_oracle_alone_keeps_half_of_every_cap(seam, name):
    case, ref, tensors = _load(seam, name)
    assert float(ref["F"].float().mean()) <= rc.MAX_FRAGILE
    for kind in rc.KINDS:
        for t in tensors:
            g64, g32 = ref["g64"][kind][t], ref["g32"][kind][t]
            assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and g64.shape == g32.shape
            e = check_rows(f"{name} {kind}", t, g32, g64, cap_scale=0.5)
            assert e["live_rows"] >= 200 and e["norm"] == "per row"
            for gname, idx in rc.tensor_groups(case, t).items():
                check_rows(f"{name} {kind} [{gname}]", t, g32[idx], g64[idx], cap_scale=0.5)
        # the colour rows are the well-conditioned ones: under positive cotangents nothing cancels
        r, _ = row_errors(ref["g32"]["positive"]["colors"], ref["g64"]["positive"]["colors"])
        assert r.max() <= 0.5e-4, r.max()


@pytest.mark.parametrize("name", rc.S1_CASES)
def test_the_projection_of_the_fp32_oracle_is_exact_to_rounding(name):
    ref = rc.s1_reference(name)
    p64, p32 = ref["proj64"], ref["proj32"]
    both = (p64["radii"] > 0) & (p32["radii"] > 0)
    assert int(both.sum()) >= 0.9 * len(both)
    for t in rc.PROJ_TENSORS:
        check_rows(f"{name} projection", t, p32[t][both], p64[t][both], cap_scale=0.5)


def test_the_strata_sit_below_the_maximum_they_hide_beside():
    case, ref = rc.s1_case(rc.STRATA), rc.s1_reference(rc.STRATA)
    assert tuple(case["groups"]) == rc.STRATA_GROUPS and len(case["groups"]["tail"]) == rc.STRATA_N % 64
    assert int(case["groups"]["tail"][-1]) == rc.STRATA_N - 1
    for kind in rc.KINDS:
        for t in rc.S1_TENSORS:
            g = ref["g64"][kind][t]
            top = g.reshape(g.shape[0], -1).abs().amax(1)
            for gname, idx in case["groups"].items():
                assert int((top[idx] > 0).sum()) >= 30, (kind, t, gname)
                if gname != "big" and t in ("means", "scales"):
                    assert float(top[idx].max()) < 1e-1 * float(top.max()), (kind, t, gname, float(top[idx].max() / top.max()))
    # what the groups are by construction
    inp, proj = case["inp"], ref["proj64"]
    W, H, fx = case["W"], case["H"], float(case["inp"]["K"][0, 0])
    gr = case["groups"]
    assert float((inp["scales"][gr["subpixel"]].amax(1) * fx / inp["means"][gr["subpixel"], 2]).max()) < 0.3
    s = inp["scales"][gr["needle"]]
    assert float((s.amax(1) / s.amin(1)).min()) >= 49.9
    assert 0.02 <= float(inp["opac"][gr["faint"]].min()) and float(inp["opac"][gr["faint"]].max()) <= 0.05
    m = inp["means"][gr["clamped"]]
    lim = 1.3 * torch.tensor([0.5 * W / fx, 0.5 * H / fx], dtype=torch.float64)
    assert bool(((m[:, :2] / m[:, 2:3]).abs() > lim).any(1).all())
    vis = proj["radii"][gr["border"]] > 0
    m2 = proj["means2d"][gr["border"]][vis]
    outside = (m2[:, 0] < 0) | (m2[:, 0] > W) | (m2[:, 1] < 0) | (m2[:, 1] > H)
    assert bool(outside.all()) and int(vis.sum()) >= 30


@pytest.mark.parametrize("name", tuple(rc.S1_RANDOM))
def test_most_quaternion_rows_of_a_random_scene_lie_decades_below_the_maximum(name):
    ref = rc.s1_reference(name)
    for kind in rc.KINDS:
        g = ref["g64"][kind]["quats"]
        live = int(row_errors(g, g)[1].sum())
        assert int(rc.below(g, 1e-2).sum()) >= 0.30 * live, (kind, int(rc.below(g, 1e-2).sum()), live)


@pytest.mark.parametrize("seam,name", CASES)
def test_small_rows_half_a_percent_off_pass_the_tensor_norm_and_fail_the_row_norm(seam, name):
    case, ref, tensors = _load(seam, name)
    for kind in rc.KINDS:
        for t in tensors:
            g = ref["g64"][kind][t]
            small = rc.below(g, 1e-2)
            assert int(small.sum()) > 0.02 * g.shape[0], (kind, t, int(small.sum()))
            bad = g.clone()
            bad[small] *= 1.005
            check(f"{name} {kind} mutated", t, bad, g, 1e-4, 0.0)  # 0.5 % of a row below 1e-2 of the maximum: 5e-5 of the maximum
            with pytest.raises(AssertionError, match="live rows off by"):
                check_rows(f"{name} {kind} mutated", t, bad, g)
            check_rows(f"{name} {kind} unmutated", t, g, g)


def test_negated_tail_rows_fail_the_row_norm():
    """The ragged last group with its sign flipped.  The rows of the tail sit at 1e-2 ... 3e-2 of the tensor's maximum on this scene, so the
    tensor norm sees this one as well (twice a row is 2e-2 ... 6e-2 of the maximum); scaled to the small rows' level it is the mutation above.
    What is asserted here is that the row norm fails it on the GROUP and on the whole tensor alike."""
    case, ref = rc.s1_case(rc.STRATA), rc.s1_reference(rc.STRATA)
    tail = case["groups"]["tail"]
    for kind in rc.KINDS:
        for t in rc.S1_TENSORS:
            g = ref["g64"][kind][t]
            bad = g.clone()
            bad[tail] = -bad[tail]
            with pytest.raises(AssertionError, match="live rows off by"):
                check_rows(f"strata {kind} tail negated", t, bad, g)
            with pytest.raises(AssertionError, match="live rows off by"):
                check_rows(f"strata {kind} tail negated [tail]", t, bad[tail], g[tail])
            # ... and hidden behind the tensor norm once the maximum is a few decades up: the same rows beside one large one
            big = torch.cat([g, 1e5 * g.abs().max() * torch.ones_like(g[:1])])
            bad = big.clone()
            bad[tail] = -bad[tail]
            check(f"strata {kind} tail negated beside a large row", t, bad, big, 1e-4, 0.0)
            with pytest.raises(AssertionError, match="live rows off by"):
                check_rows(f"strata {kind} tail negated beside a large row", t, bad, big)


def test_check_rows_yardstick_floor_dead_rows_and_small_groups():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(300, 3, generator=g, dtype=torch.float64)
    ref[:5] = 0.0  # not live
    noise = lambda s: ref * (1 + s * torch.randn(300, 3, generator=g, dtype=torch.float64))
    e = check_rows("unit", "t", noise(1e-6), ref, yard=noise(1e-6))
    assert e["live_rows"] == 295 and e["share_1e4"] == 0 and 0 < e["median"] < 1e-5 and e["yard_median"] > 0 and e["norm"] == "per row"
    check_rows("unit", "t", noise(2e-6), ref, yard=noise(1e-9))  # the yardstick is never taken below 2.5e-6
    with pytest.raises(AssertionError, match="fp32 oracle"):
        check_rows("unit", "t", noise(3e-5), ref, yard=noise(1e-6))  # within every cap, 30 x the yardstick
    check_rows("unit", "t", noise(3e-5), ref, yard=noise(1e-6), ratio=None)
    dead = torch.zeros(300, dtype=torch.bool)
    dead[:5] = True
    got = ref.clone()
    check_rows("unit", "t", got, ref, dead=dead)
    got[2, 1] = 1e-30
    with pytest.raises(AssertionError, match="culled rows"):
        check_rows("unit", "t", got, ref, dead=dead)
    # caps: 1 % beyond 1e-3 - three rows of 295 are too many, two are not; a group under 200 rows may have one more
    for n_bad, ok in ((2, True), (3, False)):
        got = ref.clone()
        got[10:10 + n_bad] *= 1.002
        if ok:
            check_rows("unit", "t", got, ref)
        else:
            with pytest.raises(AssertionError, match="live rows off by"):
                check_rows("unit", "t", got, ref)
    small, got = ref[100:140], ref[100:140].clone()
    got[0] *= 1.5
    check_rows("unit", "t", got, small)
    got[1] *= 1.5
    with pytest.raises(AssertionError, match="live rows off by"):
        check_rows("unit", "t", got, small)
