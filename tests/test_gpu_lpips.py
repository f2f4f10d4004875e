"""LPIPS on the device (csrc/lpips.hip, deblur4dgs_amd/lpips.py):
  1. the layer kernel alone on synthetic features, against the fp64 statement of tests/lpips_ref.py, by a bound from the statement;
  2. the score kernel alone on synthetic layer maps: the map, the masked sums, the zero mask, independence of M;
  3. the prepare kernel, bit for bit what torch's fp32 operations give;
  4. the whole path (MIOpen trunk from seeded weights, the recorded head weights) against what tests/golden/lpips.npz records of the
     reference, within 8 x the reference's own fp32-against-fp64 gap;
  5. bitwise repeatability and independence of the number of masks, and the nine keys of ValidationMetrics(lpips=...) through validate_with_pose_refinement."""
import pytest
import torch

from tests import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def net(fx):
    from deblur4dgs_amd.lpips import LPIPS

    return LPIPS(R.seeded_trunk(), R.lins_state(fx)).to(DEV)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- 1. the layer kernel ------------------------------------------------------------------------------------------------------
def _features(case, n, C, h, w, g):
    """two ReLU-like feature tensors (about half the values zero) and C weights"""
    f0 = torch.randn(n, C, h, w, generator=g).clamp(min=0) * 3
    f1 = (f0 + 0.5 * torch.randn(n, C, h, w, generator=g)).clamp(min=0)
    wts = torch.rand(C, generator=g) * 1.3
    if case == "same":
        f1 = f0.clone()
    elif case == "mixed":
        wts = wts - 0.6
    elif case == "dead":  # all-zero columns: in one input at the even pixels of a row, in both at every third pixel
        f0 = f0.permute(0, 2, 3, 1).reshape(-1, C).clone()
        f1 = f1.permute(0, 2, 3, 1).reshape(-1, C).clone()
        f0[0::2] = 0
        f0[0::3], f1[0::3] = 0, 0
        f0, f1 = (v.reshape(n, h, w, C).permute(0, 3, 1, 2).contiguous() for v in (f0, f1))
    return f0, f1, wts


@pytest.mark.parametrize("C", [1, 3, 64, 65, 192, 256, 384])
def test_layer_kernel_against_the_fp64_statement(C):
    """Bound per element: 4 C 2^-24 sum_c |w_c| (g0_c - g1_c)^2 from the statement - the worst case of a C-term fp32 sum whose terms
    each carry a few roundings (the kernel accumulates in double and rounds once: it holds with room)."""
    from deblur4dgs_amd.lpips import layer_distance

    worst = 0.0
    for si, (h, w) in enumerate(((1, 1), (3, 5), (8, 67), (17, 31))):
        for n in (1, 3):
            for ci, case in enumerate(("nonneg", "mixed", "dead", "same")):
                f0, f1, wts = _features(case, n, C, h, w, gen(100 * C + 10 * si + ci + n))
                got = layer_distance(f0.to(DEV), f1.to(DEV), wts.to(DEV)).cpu().double()
                want, scale = R.layer_terms(f0, f1, wts)
                assert got.shape == want.shape == (n, h, w) and bool(torch.isfinite(got).all())
                if case == "same":
                    assert bool((got == 0).all()), (C, h, w, n)  # exactly 0.0, as the reference's direct form gives
                    continue
                bound = 4 * C * EPS * scale
                ratio = ((got - want).abs() / bound.clamp(min=1e-300))[bound > 0]
                assert bool((got[bound == 0] == 0).all())  # both columns dead (or equal): nothing to sum
                worst = max(worst, float(ratio.max()) if ratio.numel() else 0.0)
                assert bool(((got - want).abs() <= bound).all()), (C, h, w, n, case, float(ratio.max()))
    print(f"layer kernel C={C}: largest error / bound {worst:.3e}")


def test_layer_kernel_refuses_what_it_cannot_take():
    from deblur4dgs_amd.lpips import layer_distance

    f = torch.rand(1, 4, 3, 3, device=DEV)
    with pytest.raises(ValueError, match="weights"):
        layer_distance(f, f, torch.rand(5, device=DEV))
    with pytest.raises(RuntimeError, match="C=4097"):
        layer_distance(torch.rand(1, 4097, 1, 1, device=DEV), torch.rand(1, 4097, 1, 1, device=DEV), torch.rand(4097, device=DEV))


# ---- 2. the score kernel ------------------------------------------------------------------------------------------------------
def _score_masks(kind, M, B, H, W, g):
    if kind == "none":
        return None
    if kind == "ones":
        return torch.ones(M, B, H, W)
    if kind == "zero":
        return torch.zeros(M, B, H, W)
    if kind == "bernoulli":
        return (torch.rand(M, B, H, W, generator=g) < 0.7).float()
    if kind == "dyadic":
        return torch.randint(0, 3, (M, B, H, W), generator=g).float() / 2
    valid, fg = (torch.rand(B, H, W, generator=g) < 0.9).float(), torch.zeros(B, H, W)  # the validator's three
    fg[:, H // 4:H // 2 + 5, 3:W // 2] = 1
    return torch.stack((valid, fg * valid, (1 - fg) * valid))[:M]


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_name)
def test_score_kernel_against_the_fp64_statement(shape):
    """Map within 2e-6 of its maximum (five 4-tap interpolations and four additions), sums to rtol 2e-6; the zero mask gives sums of
    exactly 0 and an mLPIPS of nan; every (m, b) is bitwise the same alone and inside M = 3."""
    from deblur4dgs_amd.lpips import mLPIPS, mean_score, score

    B, H, W = shape
    sizes = R.alex_sizes(H, W)
    worst_map = worst_sum = 0.0
    for M in (1, 3):
        g = gen(700 + M + H)
        maps = [torch.rand(M * B, h, w, generator=g) * (0.2 + k) for k, (h, w) in enumerate(sizes)]
        dev_maps = [m.to(DEV) for m in maps]
        want_map = R.score_map(maps, H, W).reshape(M, B, H, W)
        for kind in ("none", "ones", "zero", "bernoulli", "dyadic", "validator"):
            if kind == "none" and M != 1:
                continue
            masks = _score_masks(kind, M, B, H, W, g)
            s, t, smap = score(dev_maps, H, W, None if masks is None else masks.to(DEV), want_map=True)
            s2, t2, none = score(dev_maps, H, W, None if masks is None else masks.to(DEV))
            assert none is None and torch.equal(s, s2) and torch.equal(t, t2)  # the map is optional and changes nothing
            assert s.dtype == t.dtype == torch.float64 and s.shape == t.shape == (M, B) and smap.shape == (M, B, H, W)
            err = float((smap.cpu().double() - want_map).abs().max() / want_map.abs().max())
            worst_map = max(worst_map, err)
            assert err <= 2e-6, (kind, M, err)
            mk = torch.ones(M, B, H, W) if masks is None else masks
            want_s, want_t = (want_map * mk.double()).sum((2, 3)), mk.double().sum((2, 3))
            assert torch.equal(t.cpu(), want_t)  # sums of 0, 0.5 and 1: exact
            if kind == "zero":
                assert bool((s == 0).all()) and bool((t == 0).all())
                one = mLPIPS(None)
                one._append(s, t)
                assert bool(torch.isnan(one.compute()))
            else:
                rel = float(((s.cpu() - want_s).abs() / want_s.abs()).max())
                worst_sum = max(worst_sum, rel)
                assert rel <= 2e-6, (kind, M, rel)
            if M == 3:
                for m in range(3):
                    alone = score([d.view(M, B, *d.shape[1:])[m].contiguous() for d in dev_maps], H, W, masks[m:m + 1].to(DEV), want_map=True)
                    assert torch.equal(alone[0][0], s[m]) and torch.equal(alone[1][0], t[m]) and torch.equal(alone[2][0], smap[m]), (kind, m)
        # the mean form on the same maps
        got = mean_score(dev_maps).cpu()
        want = R.mean_score(maps)
        assert got.dtype == torch.float64 and float(((got - want).abs() / want.abs()).max()) <= 1e-12
    print(f"score kernel {R.shape_name(shape)}: map error / max {worst_map:.3e} (2e-6 allowed), sums relative {worst_sum:.3e} (2e-6 allowed)")


# ---- 3. the prepare kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("M", [0, 1, 3])  # 0: no masks
def test_prepare_is_torch_fp32_bit_for_bit(M, normalize):
    from deblur4dgs_amd.lpips import prepare

    B, H, W = 2, 33, 47
    g = gen(40 + M)
    pred = torch.rand(B, 3, H, W, generator=g).permute(0, 2, 3, 1)  # channel-last view of NCHW storage: not contiguous
    target = torch.rand(B, H, 2 * W, 3, generator=g)[:, :, ::2]     # a strided view
    assert not pred.is_contiguous() and not target.is_contiguous()
    masks = None if M == 0 else (torch.rand(M, B, H, W, generator=g) * (torch.rand(M, B, H, W, generator=g) < 0.8))
    shift, scale = (torch.tensor(v, dtype=torch.float32).view(1, 1, 1, 3, 1, 1) for v in (R.SHIFT, R.SCALE))
    x = torch.stack((pred, target)).permute(0, 1, 4, 2, 3)[:, None]  # [2,1,B,3,H,W]
    if masks is not None:
        x = x * masks[None, :, :, None]
    if normalize:
        x = x * 2 - 1
    want = ((x - shift) / scale).contiguous()
    got = prepare(pred.to(DEV), target.to(DEV), None if masks is None else masks.to(DEV), normalize=normalize)
    assert got.shape == want.shape == (2, max(M, 1), B, 3, H, W) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    if M == 1:  # [B,H,W] masks are M = 1
        assert torch.equal(prepare(pred.to(DEV), target.to(DEV), masks[0].to(DEV), normalize=normalize), got)


# ---- 4. the whole path against the fixture ------------------------------------------------------------------------------------
def _tol(fx, key, recorded):
    return 8 * float(fx[key]) * float(abs(recorded).max())


@pytest.mark.parametrize("kind", R.IMAGES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_name)
def test_whole_path_matches_the_reference(fx, net, shape, kind):
    """Tolerance: 8 x the recorded gap of the reference's own fp32 run against its fp64 run, relative to the largest recorded value -
    the factor test_network_matches_the_reference_flows grants MIOpen's convolution algorithms over the CPU's direct ones."""
    from deblur4dgs_amd.lpips import mLPIPS

    sname = R.shape_name(shape)
    p, t = (v.to(DEV) for v in R.images_of(fx, sname, kind))
    want_mean, want_map = fx[f"{sname}/{kind}/mean"], fx[f"{sname}/{kind}/map"]
    mean, smap = net.distance(p, t, normalize=True), net.score_map(p, t, normalize=True)
    assert mean.shape == want_mean.shape and smap.shape == want_map.shape
    assert torch.equal(net.distance(2 * p - 1, 2 * t - 1), mean)  # torch's 2 x - 1 rounds as the kernel's does: the same trunk input
    if kind == "same":
        assert bool((mean == 0).all()) and bool((smap == 0).all())
    else:
        e_mean = float((mean.cpu().double() - torch.from_numpy(want_mean)).abs().max())
        e_map = float((smap.cpu().double() - torch.from_numpy(want_map)).abs().max())
        print(f"{sname}: mean error / allowed {e_mean / _tol(fx, 'ref_gap_mean', want_mean):.3f}, map error / allowed {e_map / _tol(fx, 'ref_gap_map', want_map):.3f}")
        assert e_mean <= _tol(fx, "ref_gap_mean", want_mean) and e_map <= _tol(fx, "ref_gap_map", want_map)
    for mk in R.MASKS:
        mask = R.mask_of(fx, sname, mk)
        s, total = net.masked_sums(p, t, None if mask is None else mask.to(DEV))
        want_s, want_total = fx[f"{sname}/{kind}/{mk}/sum"], int(fx[f"{sname}/{kind}/{mk}/total"])
        assert s.shape == total.shape == (1, shape[0]) and s.dtype == torch.float64
        assert int(total.sum().to(torch.int64)) == want_total
        one = mLPIPS(net)
        value = one(p, t, None if mask is None else mask.to(DEV))
        assert len(one) == 1 and int(one.total[0]) == want_total and one.total[0].dtype == torch.int64
        if kind == "same" or mk == "zero":
            assert float(s.abs().sum()) == 0.0
            assert bool(torch.isnan(value)) if mk == "zero" else float(value) == 0.0
        else:
            err = abs(float(s.sum()) - float(want_s))
            print(f"{sname}/{mk}: sum error / allowed {err / _tol(fx, 'ref_gap_map', want_s):.3f}")
            assert err <= _tol(fx, "ref_gap_map", want_s)
            assert abs(float(value) - float(want_s) / want_total) <= _tol(fx, "ref_gap_map", want_s / want_total)


def test_sequence_and_validation_metrics_match_the_reference(fx, net):
    from deblur4dgs_amd.lpips import mLPIPS
    from deblur4dgs_amd.metrics import ValidationMetrics

    one = mLPIPS(net)
    for step in fx["sequence/steps"]:
        sname, kind, mk = str(step).split("/")
        mask = R.mask_of(fx, sname, mk)
        one.update(*(v.to(DEV) for v in R.images_of(fx, sname, kind)), None if mask is None else mask.to(DEV))
    assert len(one) == 3 and [int(v) for v in one.total] == [int(v) for v in fx["sequence/totals"]]
    assert abs(float(one.compute()) - float(fx["sequence/compute"])) <= _tol(fx, "ref_gap_map", fx["sequence/compute"])
    one.reset()
    assert len(one) == 0

    sname = R.shape_name(R.VALIDATOR_SHAPE)
    p, t = (v.to(DEV) for v in R.images_of(fx, sname, "uniform"))
    valid, fg, three = R.validator_masks(fx)
    both, plain = ValidationMetrics(lpips=net), ValidationMetrics()
    both.update(p, t, valid.to(DEV), fg.to(DEV)), plain.update(p, t, valid.to(DEV), fg.to(DEV))
    out, old = both.compute(), plain.compute()
    assert tuple(out) == ValidationMetrics.KEYS + ValidationMetrics.LPIPS_KEYS and tuple(old) == ValidationMetrics.KEYS
    assert all(torch.equal(out[k], old[k]) for k in old)  # the six old numbers: the same bits
    for key, name in (("main", "val/lpips"), ("fg", "val/fg_lpips"), ("bg", "val/bg_lpips")):
        want = float(fx[f"validator/{key}/sum"]) / int(fx[f"validator/{key}/total"])
        print(f"{name}: error / allowed {abs(float(out[name]) - want) / (8 * float(fx['ref_gap_map']) * want):.3f}")
        assert abs(float(out[name]) - want) <= 8 * float(fx["ref_gap_map"]) * want
    # bitwise repeatability of the three-mask call, and each mask alone is what it is among the three
    masks = torch.stack(tuple(three.values())).to(DEV)
    a, b = net.masked_sums(p, t, masks), net.masked_sums(p, t, masks)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape == (3, 2)
    for m in range(3):
        alone = net.masked_sums(p, t, masks[m])
        assert torch.equal(alone[0][0], a[0][m]) and torch.equal(alone[1][0], a[1][m]), m
    # which side an image is on does not matter: targets against preds is the same distance, bit for bit
    assert torch.equal(net.masked_sums(t, p, masks)[0], a[0])
    # without a background: the fg mask is the main one, the other two stay nan
    lone = ValidationMetrics(has_bg=False, lpips=net)
    lone.update(p, t, valid.to(DEV), fg.to(DEV))
    res = lone.compute()
    assert torch.equal(res["val/lpips"], out["val/fg_lpips"])  # one mask or three: the same bits
    assert bool(torch.isnan(res["val/fg_lpips"])) and bool(torch.isnan(res["val/bg_lpips"])) and bool(torch.isnan(res["val/bg_psnr"]))


# ---- 5. through the validation loop -------------------------------------------------------------------------------------------
def test_nine_keys_through_validate_with_pose_refinement(net):
    """The six old keys are bitwise what lpips=None gives.  The three new ones EQUAL, bit for bit, what three mLPIPS objects give for
    the same renders, one mask each: the trunk runs per side and mask, so a mask alone and a mask among the validator's three are the
    same convolution problems and the head does not depend on M."""
    from deblur4dgs_amd.lpips import mLPIPS
    from deblur4dgs_amd.metrics import ValidationMetrics
    from deblur4dgs_amd.pose_refine import validate_with_pose_refinement
    from tests import pose_refine_ref as P

    model, sc = P.build_model(DEV)
    img = P.target_image().float().to(DEV)
    g = gen(9)
    valid = (torch.rand(P.H, P.W, generator=g) < 0.9).float().to(DEV)
    fg = torch.zeros(P.H, P.W, device=DEV)
    fg[10:30, 20:50] = 1
    frame = dict(t=P.T_FRAME, w2c=sc["viewmat"].to(DEV), K=sc["K"].to(DEV), img=img, valid_mask=valid, fg_mask=fg)

    class Keeping(ValidationMetrics):  # remembers the renders it was fed
        def update(self, rendered_img, img, valid_mask, fg_mask):
            self.seen = getattr(self, "seen", []) + [(rendered_img.clone(), img.clone(), valid_mask.clone(), fg_mask.clone())]
            super().update(rendered_img, img, valid_mask, fg_mask)

    kw = dict(iters=3, lr=P.LR, eta_min=P.ETA_MIN, graph=False)
    nine = Keeping(has_bg=model.has_bg, lpips=net)
    out = validate_with_pose_refinement(model, [frame], metrics=nine, **kw)
    six = validate_with_pose_refinement(model, [frame], metrics=ValidationMetrics(has_bg=model.has_bg), **kw)
    assert tuple(six) == ValidationMetrics.KEYS and tuple(out) == ValidationMetrics.KEYS + ValidationMetrics.LPIPS_KEYS
    assert all(torch.equal(out[k], six[k]) or (bool(torch.isnan(out[k])) and bool(torch.isnan(six[k]))) for k in six)
    (render, target, v, f), = nine.seen
    masks = (v, f * v, (1 - f) * v) if model.has_bg else (f * v,)
    for name, m in zip(("val/lpips", "val/fg_lpips", "val/bg_lpips"), masks):
        one = mLPIPS(net)
        one.update(render, target, m)
        assert bool(torch.isfinite(out[name])) and float(out[name]) > 0, name
        assert torch.equal(one.compute(), out[name]), (name, float(one.compute()), float(out[name]))
