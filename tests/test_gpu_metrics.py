"""deblur4dgs_amd.metrics on the device: csrc/metrics.hip against the reference's recorded values (tests/golden/metrics.npz), against
the fp64 restatement (tests/metrics_ref.py), and against answers that need no oracle.

Bounds.  Against the fixture: the reference's own fp32 error, ten times the gap the generator measured for the case's image kind
(tests/test_metrics_ref.py).  Against the restatement both sides are double arithmetic on the same fp32 inputs (eps 1.1e-16, sums of
121 terms, the variance cancellation amplified by 1 / c2 = 1.1e3: ~1e-11 at the very worst, ~1e-13 typical): SSIM within 1e-9
absolute, SSE within 1e-12 relative, the mask sum exact.  The largest shape is 64x48; 26x26 and 27x38 are the tile edges."""
import numpy as np
import pytest
import torch

from tests import metrics_ref as R
from tests.metrics_cases import CASES, check_against_fixture, load_case, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
C1 = 1e-4


@pytest.fixture(scope="module")
def M():
    from deblur4dgs_amd import metrics

    return metrics


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def restated(golden):
    """the fp64 restatement of every case, computed once on the CPU: name -> (sse, msum, ssim) [1,B]"""
    with torch.no_grad():
        return {c: R.masked_image_metrics(*load_case(golden, *c)) for c in CASES}


def exact_case(kind, mk):
    return kind == "same" or mk == "zero"


@pytest.mark.parametrize("sname,kind,mk", CASES, ids=["-".join(c) for c in CASES])
def test_every_case_against_the_fixture_and_the_restatement(M, golden, restated, sname, kind, mk):
    pred, target, mask = load_case(golden, sname, kind, mk, DEV)
    sse, msum, ssim = M.masked_image_metrics(pred, target, mask)
    assert all(v.dtype == torch.float64 and v.shape == (1, pred.shape[0]) and v.is_cuda and not v.requires_grad for v in (sse, msum, ssim))
    sse, msum, ssim = sse.cpu(), msum.cpu(), ssim.cpu()
    e_fix = check_against_fixture(golden, f"{sname}/{kind}/{mk}", kind, sse[0], msum[0], ssim[0], exact_case(kind, mk))
    r_sse, r_msum, r_ssim = restated[(sname, kind, mk)]
    e_ssim = float((ssim - r_ssim).abs().max())
    e_sse = float(((sse - r_sse).abs() / r_sse.clamp(min=1e-300)).max())
    print(f"{sname}/{kind}/{mk}: against the fixture SSIM {e_fix[0]:.2e} SSE {e_fix[1]:.2e}; against fp64 SSIM {e_ssim:.2e} SSE {e_sse:.2e}")
    assert torch.equal(msum, r_msum)
    assert e_ssim <= 1e-9 and e_sse <= 1e-12
    if exact_case(kind, mk):
        assert bool((ssim == 1).all()) and bool((sse == 0).all())
    sse_only, msum_only, none = M.masked_image_metrics(pred, target, mask, ssim=False)  # the PSNR-only kernel: the same two sums
    assert none is None and torch.equal(sse_only.cpu(), sse) and torch.equal(msum_only.cpu(), msum)


def test_pred_equal_target_is_exactly_one_and_a_zero_mask_gives_nan_psnr(M, golden):
    pred, _, mask = load_case(golden, "2x27x38", "flat", "dyadic", DEV)
    sse, msum, ssim = M.masked_image_metrics(pred, pred.clone(), mask)
    assert bool((ssim == 1.0).all()) and bool((sse == 0.0).all()) and bool((msum > 0).all())
    _, target, _ = load_case(golden, "2x27x38", "uniform", "none", DEV)
    sse, msum, ssim = M.masked_image_metrics(pred, target, torch.zeros_like(mask))
    assert bool((ssim == 1.0).all()) and bool((sse == 0.0).all()) and bool((msum == 0.0).all())
    ps = M.mPSNR()
    ps.update(pred, target, torch.zeros_like(mask))
    assert int(ps.total[0]) == 0 and ps.total[0].dtype == torch.int64 and bool(torch.isnan(ps.compute()))


@pytest.mark.parametrize("shape", [(1, 11, 11), (2, 27, 38), (1, 64, 48)])
@pytest.mark.parametrize("a,b", [(0.25, 0.75), (0.9, 0.8999), (0.1, 1.0), (0.3, 0.3)])
def test_constant_images_have_closed_forms(M, shape, a, b):
    B, H, W = shape
    a32, b32 = float(np.float32(a)), float(np.float32(b))  # what the kernel is given
    pred, target = torch.full((B, H, W, 3), a, device=DEV), torch.full((B, H, W, 3), b, device=DEV)
    sse, msum, ssim = (v.cpu() for v in M.masked_image_metrics(pred, target, torch.ones(B, H, W, device=DEV)))
    want_ssim, want_sse = (2 * a32 * b32 + C1) / (a32 * a32 + b32 * b32 + C1), 3 * H * W * (a32 - b32) ** 2
    assert bool((msum == H * W).all())
    assert float((ssim - want_ssim).abs().max()) <= 1e-12 * want_ssim
    assert float((sse - want_sse).abs().max()) <= 1e-12 * want_sse
    none = M.masked_image_metrics(pred, target)  # no mask = the mask of ones, bitwise
    assert torch.equal(none[0].cpu(), sse) and torch.equal(none[1].cpu(), msum) and torch.equal(none[2].cpu(), ssim)


def validator_inputs(golden, device=DEV):
    pred, target, _ = load_case(golden, "1x64x48", "uniform", "none", device)
    return pred, target, torch.tensor(golden["validator/valid_mask"], device=device), torch.tensor(golden["validator/fg_mask"], device=device)


def test_three_masks_in_one_call_equal_three_calls_and_calls_repeat_bitwise(M, golden):
    pred, target, valid, fg = validator_inputs(golden)
    masks = torch.stack((valid, fg * valid, (1 - fg) * valid))
    three = M.masked_image_metrics(pred, target, masks)
    again = M.masked_image_metrics(pred, target, masks)
    assert all(v.shape == (3, 1) for v in three) and all(torch.equal(x, y) for x, y in zip(three, again))
    for i in range(3):
        one = M.masked_image_metrics(pred, target, masks[i])
        assert all(torch.equal(x[i], y[0]) for x, y in zip(three, one)), i
    p2, t2, m2 = load_case(golden, "2x27x38", "uniform", "bernoulli", DEV)  # two images, two masks: [M,B] is laid out mask-major
    both = M.masked_image_metrics(p2, t2, torch.stack((m2, 1 - m2)))
    for m_i, m in enumerate((m2, 1 - m2)):
        for b in range(2):
            one = M.masked_image_metrics(p2[b:b + 1], t2[b:b + 1], m[b:b + 1])
            assert all(torch.equal(x[m_i, b], y[0, 0]) for x, y in zip(both, one)), (m_i, b)


def test_other_dtypes_and_strides_equal_their_fp32_contiguous_copies(M, golden):
    pred, target, mask = load_case(golden, "1x43x27", "uniform", "dyadic", DEV)
    want = M.masked_image_metrics(pred, target, mask)
    nc_pred = pred.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)  # channel-first storage
    wide = torch.zeros(1, 43, 40, 3, device=DEV)
    wide[:, :, 5:32] = target
    nc_mask = mask.transpose(1, 2).contiguous().transpose(1, 2)
    assert not nc_pred.is_contiguous() and not wide[:, :, 5:32].is_contiguous() and not nc_mask.is_contiguous()
    for got in (M.masked_image_metrics(nc_pred, wide[:, :, 5:32], nc_mask), M.masked_image_metrics(pred.double(), target.double(), mask.double()),
                M.masked_image_metrics(pred, target, mask[..., None]), M.masked_image_metrics(pred, target, mask[None]),
                M.masked_image_metrics(pred.requires_grad_(), target, mask)):
        assert all(torch.equal(x, y) and not x.requires_grad for x, y in zip(got, want))
    binary = M.masked_image_metrics(pred, target, mask > 0.25)  # a bool mask is its 0 / 1 float
    assert all(torch.equal(x, y) for x, y in zip(binary, M.masked_image_metrics(pred, target, (mask > 0.25).float())))
    with pytest.raises(ValueError):
        M.masked_image_metrics(pred, target, mask[:, :-1])
    with pytest.raises(ValueError):
        M.masked_image_metrics(pred, target[:, :-1], mask)
    with pytest.raises(RuntimeError, match="want_ssim"):
        M.masked_image_metrics(pred[:, :10], target[:, :10])
    assert M.masked_image_metrics(pred[:, :10], target[:, :10], ssim=False)[2] is None  # the sums need no window


def test_classes_accumulate_return_the_batch_value_and_reset(M, golden):
    ps, ss = M.mPSNR(), M.mSSIM()
    batch_psnr, batch_ssim = [], []
    for step in golden["sequence/steps"]:
        pred, target, mask = load_case(golden, *str(step).split("/"), DEV)
        batch_psnr.append(ps(pred, target, mask))  # forward: this batch's value, and the state grows
        batch_ssim.append(ss(pred, target, mask))
        alone = M.mPSNR()
        alone.update(pred, target, mask)
        assert torch.equal(alone.compute(), batch_psnr[-1]) and len(alone) == 1
        sse, msum, ssim = M.masked_image_metrics(pred, target, mask)
        assert torch.equal(batch_ssim[-1], ssim[0].mean())
        assert abs(M.compute_psnr(pred, target, mask) - float(batch_psnr[-1])) <= 1e-12 * abs(float(batch_psnr[-1]))
    assert len(ps) == 3 and len(ss) == 4 and all(v.is_cuda and v.dim() == 0 for v in ps.sum_squared_error + ps.total)
    assert abs(float(ps.compute()) - float(torch.stack(batch_psnr).mean())) <= 1e-13 * float(ps.compute())
    assert abs(float(ps.compute()) - float(golden["sequence/psnr"])) <= 1e-5 * float(golden["sequence/psnr"])  # fp32 reference
    assert abs(float(ss.compute()) - float(golden["sequence/ssim"])) <= 10 * float(golden["ref_gap_ssim/flat"])
    ps.reset(), ss.reset()
    assert len(ps) == 0 and len(ss) == 0
    # compute_psnr clamps the mask sum at 1 where mPSNR divides by zero
    pred, target, mask = load_case(golden, "1x26x26", "uniform", "zero", DEV)
    assert M.compute_psnr(pred, target, mask) == float("inf")
    flat = M.compute_psnr(pred.reshape(-1, 3), target.reshape(-1, 3))  # [N,3] points, as flow3d/metrics.py allows
    assert abs(flat - M.compute_psnr(pred, target)) <= 1e-12 * abs(flat)


@pytest.mark.parametrize("has_bg", [True, False])
def test_validation_metrics_keys_and_values(M, golden, has_bg):
    pred, target, valid, fg = validator_inputs(golden)
    vm = M.ValidationMetrics(has_bg)
    vm.update(pred, target, valid, fg)
    out = vm.compute()
    assert tuple(out) == ("val/psnr", "val/ssim", "val/fg_psnr", "val/fg_ssim", "val/bg_psnr", "val/bg_ssim") == M.ValidationMetrics.KEYS
    names = {"": "main", "fg_": "fg", "bg_": "bg"} if has_bg else {"": "fg"}
    for prefix, key in names.items():
        assert abs(float(out[f"val/{prefix}psnr"]) - float(golden[f"validator/{key}/psnr"])) <= 1e-5 * float(golden[f"validator/{key}/psnr"])
        assert abs(float(out[f"val/{prefix}ssim"]) - float(golden[f"validator/{key}/ssim"][0])) <= 10 * float(golden["ref_gap_ssim/uniform"])
    if not has_bg:  # the reference never updates these without a background
        assert all(bool(torch.isnan(out[k])) for k in ("val/fg_psnr", "val/fg_ssim", "val/bg_psnr", "val/bg_ssim"))
    vm.update(pred, target, valid, fg)
    assert abs(float(vm.compute()["val/ssim"]) - float(out["val/ssim"])) <= 1e-15  # the mean of two equal frames
    vm.reset()
    assert all(bool(torch.isnan(v)) for v in vm.compute().values())


def test_capture_on_a_side_stream_replays_on_new_inputs_bitwise(M, golden):
    first = load_case(golden, "2x27x38", "uniform", "bernoulli", DEV)
    second = load_case(golden, "2x27x38", "flat", "rows", DEV)
    want = M.masked_image_metrics(*second)
    bufs = [t.clone() for t in first]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.masked_image_metrics(*bufs)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = M.masked_image_metrics(*bufs)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, M.masked_image_metrics(*first)))
    for buf, new in zip(bufs, second):
        buf.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want))
