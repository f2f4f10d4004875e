"""The batch feed on the GPU (csrc/feed.hip through deblur4dgs_amd.feed) against tests/golden/feed.npz, which tests/golden/gen_feed.py
records from the reference's own functions in float64.

Inputs are fp32 and both sides see the same numbers.  The bounds:
  flags, pix, rows, vis, n_queries, target_ts   EQUAL (the fixture's samples stay 1e-3 away from the flags' edge)
  planes, Ks, w2cs, the 2-D tracks              bitwise the clip's own data: they are copied, never computed
  depth and image samples, confidences, weights within 1e-4 max|ref| of the fp64 fixture (the project's standing bound)
The fixture's sizes: P_q = 1, 63, 64, 65 (around one wave) and 257 (one past a block of 256 lanes), N = 1 and 4; 24 x 32 frames start
on 16-byte lines, 13 x 17 frames (663 floats) do not, and test_planes_on_every_copy_path walks every head, body and tail of the copy.
Past the fixture: N = 16, 17, 28, 29 and 64 targets of a 66-frame clip with permuted time ids (the 256 lanes that write the target
cameras take a second turn from N = 17 for the 4 x 4 matrices and from N = 29 for the 3 x 3), and draws of n = 63 and 64 frames, the
last lanes of the one wave that draws."""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from deblur4dgs_amd import feed, losses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPS = ("24x32", "13x17")
CASES = ("q0_n4", "q1_n1", "q2_n4", "q3_n1", "q4_n4", "q5_n1")
FRAMES, START, END = 6, 1, 5
P_Q = (65, 1, 63, 64, 65, 257)
TOL = 1e-4
PLANES = ("imgs", "valid_masks", "masks", "depths")
PER_QUERY = ("target_tracks_2d", "target_visibles", "target_invisibles", "target_confidences", "target_track_depths")


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "feed.npz"))
    return {k: z[k] for k in z.files}


def case(prefix):
    return {k[len(prefix) + 1:]: v for k, v in golden().items() if k.startswith(prefix + "/") and "/" not in k[len(prefix) + 1:]}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


@functools.lru_cache(maxsize=None)
def fixture_clip(name):
    c = case(name)
    clip = feed.DeviceClip(dev(c["imgs"]), dev(c["depths"]), dev(c["masks"]), dev(c["valid_masks"]), dev(c["Ks"]), dev(c["w2cs"]),
                           dev(c["time_ids"], torch.int64), [dev(c[f"tracks_{q}"]) for q in range(FRAMES)], START, END)
    return clip, c


def same(t, a):
    """bit for bit (fp32 as their words; everything else as it is)"""
    t, a = t.detach().cpu().numpy(), np.ascontiguousarray(a)
    if t.dtype == np.float32:
        return t.shape == a.shape and np.array_equal(t.view(np.uint32), a.astype(np.float32).view(np.uint32))
    return t.shape == a.shape and np.array_equal(t, a.astype(t.dtype))


def err(what, got, ref):
    """max |got - ref| / max |ref|"""
    ref = np.asarray(ref, np.float64)
    e = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-30)
    print(f"{what}: relative error {e:.3e}")
    return e


def bits(t):
    """the tensor's bytes"""
    return t.contiguous().view(-1).view(torch.uint8)


def flat(batch):
    """every tensor of a batch dict by name (list entries unwrapped, the tables prefixed)"""
    out = {}
    for k, v in batch.items():
        if k == "track_tables":
            out.update({f"tables/{n}": t for n, t in v.items()})
        else:
            out[k] = v[0] if isinstance(v, list) else v
    return out


def synthetic_clip(F, H, W, P, seed, time_ids=None, start=0, end=None, n=2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    tracks = []
    for q in range(F):
        t = torch.cat([r(F, P, 1) * (W - 1), r(F, P, 1) * (H - 1), torch.randn(F, P, 2, generator=g) * 2], -1)
        pixels = torch.randperm(H * W, generator=g)[:P].sort().values
        t[q, :, 0], t[q, :, 1] = (pixels % W).float(), (pixels // W).float()
        tracks.append(t.to(DEV))
    ids = torch.arange(F) if time_ids is None else torch.tensor(time_ids)
    return feed.DeviceClip(r(F, H, W, 3).to(DEV), (r(F, H, W) + 1).to(DEV), (r(F, H, W) < 0.5).float().to(DEV), (r(F, H, W) < 0.9).float().to(DEV),
                           (r(F, 3, 3) + torch.eye(3)).to(DEV), r(F, 4, 4).to(DEV), ids.to(DEV), tracks, start, F if end is None else end, n)


# ------------------------------------------------------------------------------------------------------------- the fixture

@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("clip_name", CLIPS)
def test_batch_equals_the_fixture(clip_name, name):
    clip, c = fixture_clip(clip_name)
    ref = case(f"{clip_name}/{name}")
    q, targets = int(ref["query"]), [int(t) for t in ref["targets"]]
    N, P, H, W = len(targets), P_Q[q], clip.H, clip.W
    b = clip.batch(q, targets)
    t = flat(b)
    # the reference's keys and shapes for a batch of one
    shapes = dict(ts=(1,), w2cs=(1, 4, 4), Ks=(1, 3, 3), imgs=(1, H, W, 3), valid_masks=(1, H, W), masks=(1, H, W), depths=(1, H, W),
                  start=(1,), query_tracks_2d=(P, 2), target_ts=(N,), target_w2cs=(N, 4, 4), target_Ks=(N, 3, 3),
                  target_tracks_2d=(N, P, 2), target_visibles=(N, P), target_invisibles=(N, P), target_confidences=(N, P),
                  target_track_depths=(N, P), target_track_imgs=(N, 3, P))
    assert {k: tuple(t[k].shape) for k in shapes} == shapes
    for k in ("query_tracks_2d", "target_ts", "target_w2cs", "target_Ks", "target_tracks_2d", "target_visibles", "target_invisibles",
              "target_confidences", "target_track_depths"):
        assert isinstance(b[k], list) and len(b[k]) == 1, k  # the keys train_collate_fn leaves as lists
    assert t["target_visibles"].dtype == t["target_invisibles"].dtype == torch.bool and t["ts"].dtype == t["target_ts"].dtype == torch.int64
    # decisions and integers: equal
    assert same(t["target_visibles"], ref["visibles"]) and same(t["target_invisibles"], ref["invisibles"])
    assert same(t["tables/pix"], np.tile(ref["pix"], N)) and same(t["tables/rows"], np.repeat(np.arange(N), P))
    assert same(t["tables/vis"], ref["visibles"].reshape(-1))  # (every query of the fixture is inside the image)
    assert int(t["n_queries"]) == P and same(t["target_ts"], ref["target_ts"]) and int(t["start"]) == START
    assert int(t["ts"]) == int(c["time_ids"][q]) and int(t["status"]) == 0
    # copies: bitwise the clip's own data; without `out` the planes are views of its storage
    for k in PLANES:
        assert same(t[k][0], c[k][q]) and t[k].data_ptr() == getattr(clip, k)[q].data_ptr(), k
    tt = c["time_ids"][targets]
    assert same(t["Ks"][0], c["Ks"][q]) and same(t["w2cs"][0], c["w2cs"][q])
    assert same(t["target_Ks"], c["Ks"][tt]) and same(t["target_w2cs"], c["w2cs"][tt])  # at the TIME id, as the reference
    tracks = c[f"tracks_{q}"]
    assert same(t["query_tracks_2d"], tracks[q][:, :2]) and same(t["target_tracks_2d"], tracks[targets][..., :2])
    assert same(t["tables/tgt_2d"], tracks[targets][..., :2].reshape(-1, 2)) and same(t["tables/Ks"], c["Ks"][tt].reshape(N, 9))
    assert t["tables/tgt_depth"].data_ptr() == t["target_track_depths"].data_ptr()
    # computed in fp32 against float64
    assert err("depth samples", t["target_track_depths"], ref["track_depths"]) < TOL
    assert err("image samples", t["target_track_imgs"], ref["track_imgs"]) < TOL
    assert err("confidences", t["target_confidences"], ref["confidences"]) < TOL
    assert err("weights", t["tables/weights"], ref["weights"].reshape(-1)) < TOL
    zero = ref["confidences"] == 0
    assert (t["target_confidences"].cpu().numpy()[zero] == 0).all() and (t["tables/weights"].cpu().numpy()[zero.reshape(-1)] == 0).all()

    # with out=: the same on the first P_q columns, padding behind them, planes copied
    out = clip.buffers(N)
    for f in dataclasses.fields(out):  # (whatever was there before is overwritten)
        x = getattr(out, f.name)
        x.fill_(1) if x.dtype in (torch.uint8, torch.int32, torch.int64) else x.fill_(float("nan"))
    out.status.zero_()
    o = flat(clip.batch(q, targets, out=out))
    PM = clip.P_max
    assert PM == 257 and tuple(o["target_tracks_2d"].shape) == (N, PM, 2) and tuple(o["target_track_imgs"].shape) == (N, 3, PM)
    for k in ("ts", "w2cs", "Ks", "target_ts", "target_w2cs", "target_Ks") + PLANES:
        assert same(o[k], t[k].cpu().numpy()), k
    assert same(o["query_tracks_2d"][:P], t["query_tracks_2d"].cpu().numpy()) and (o["query_tracks_2d"][P:] == -1).all()
    for k in PER_QUERY:
        assert same(o[k][:, :P], t[k].cpu().numpy()) and not o[k][:, P:].any(), k  # zero coordinates, depth, confidence; flags false
    assert same(o["target_track_imgs"][..., :P], t["target_track_imgs"].cpu().numpy()) and not o["target_track_imgs"][..., P:].any()
    for k, pad in (("pix", -1), ("vis", 0), ("weights", 0)):
        x = o[f"tables/{k}"].view(N, PM)
        assert same(x[:, :P], t[f"tables/{k}"].view(N, P).cpu().numpy()) and (x[:, P:] == pad).all(), k
    assert same(o["tables/rows"], np.repeat(np.arange(N), PM)) and int(o["n_queries"]) == P and int(o["status"]) == 0
    clip.check(out), clip.check()


def test_out_buffers_keep_their_addresses():
    clip, _ = fixture_clip("13x17")
    out = clip.buffers()
    a = flat(clip.batch(0, [1, 2, 3, 4], out=out))
    ptrs = {k: v.data_ptr() for k, v in a.items()}
    kept = {k: v.clone() for k, v in a.items()}
    b = flat(clip.batch(5, [4, 3, 2, 1], out=out))
    assert {k: v.data_ptr() for k, v in b.items()} == ptrs
    assert all(b[k].data_ptr() == getattr(out, k.split("/")[-1]).data_ptr() for k in ("imgs", "target_tracks_2d", "tables/pix", "n_queries"))
    assert not torch.equal(kept["imgs"], b["imgs"]) and not torch.equal(kept["target_tracks_2d"], b["target_tracks_2d"])  # new contents
    assert int(kept["n_queries"]) == 65 and int(b["n_queries"]) == 257
    with pytest.raises(ValueError, match="needs out="):
        clip.batch(torch.zeros(1, dtype=torch.int32, device=DEV))


def test_planes_on_every_copy_path():
    """37 x 41 frames: 1 517 floats, so frame q starts 4 q bytes into a 16-byte line and the image (4 551 floats) takes two blocks.
    Destinations 0 .. 3 floats into a line meet every frame once on the same offset (16-byte words behind a head of 0 .. 3 dwords,
    tails of 0 .. 3) and three times on another (dwords).  The floats around every destination keep their sentinel."""
    F, H, W = 4, 37, 41
    clip = synthetic_clip(F, H, W, 5, seed=3)
    for shift in range(4):
        out = clip.buffers()
        store = {k: torch.full((getattr(out, k).numel() + 8,), -7.0, device=DEV) for k in PLANES}
        for k in PLANES:
            setattr(out, k, store[k][shift:shift + getattr(out, k).numel()].view(getattr(out, k).shape))
            assert getattr(out, k).data_ptr() % 16 == 4 * shift
        for q in range(F):
            b = clip.batch(q, [0, 1], out=out)
            for k in PLANES:
                assert torch.equal(b[k][0], getattr(clip, k)[q]), (shift, q, k)
                n = b[k].numel()
                assert (store[k][:shift] == -7).all() and (store[k][shift + n:] == -7).all(), (shift, q, k)


# ------------------------------------------------------------------------------------------------- many targets: the strides

FB = 256  # feed.hip: constexpr int FB = 256, the lanes by which feed_small strides over N 16 and N 9 values


@functools.lru_cache(maxsize=None)
def permuted_clip():
    ids = torch.randperm(66, generator=torch.Generator().manual_seed(66))
    assert int((ids != torch.arange(66)).sum()) > 60
    return synthetic_clip(66, 5, 6, 3, seed=66, time_ids=ids.tolist()), ids.numpy()


@pytest.mark.parametrize("N", (16, 17, 28, 29, 64))
def test_target_cameras_of_many_targets_are_the_clip_rows_at_the_time_ids(N):
    """feed_small writes target_w2cs with `i < N * 16` and target_Ks with `i < N * 9`, strided by 256 lanes: N = 16 and 28 are the last
    sizes of one turn, 17 and 29 the first of two, 64 (the most a batch takes) has four and three.  The time ids are a permutation,
    so a row taken at the frame and not at its time id, or at the wrong n, shows."""
    assert (N * 16 > FB) == (N >= 17) and (N * 9 > FB) == (N >= 29) and N <= feed.MAX_TARGETS == 64
    clip, ids = permuted_clip()
    targets = torch.randperm(66, generator=torch.Generator().manual_seed(N))[:N].tolist()
    q = N % 7
    tt = ids[targets]
    assert (tt != np.array(targets)).any()
    w2cs, Ks = clip.w2cs.cpu().numpy(), clip.Ks.cpu().numpy()
    t = flat(clip.batch(q, targets))
    out = clip.buffers(N)
    for f in dataclasses.fields(out):
        x = getattr(out, f.name)
        x.fill_(1) if x.dtype in (torch.uint8, torch.int32, torch.int64) else x.fill_(float("nan"))
    out.status.zero_()
    o = flat(clip.batch(q, targets, out=out))
    for b in (t, o):
        assert tuple(b["target_w2cs"].shape) == (N, 4, 4) and tuple(b["target_Ks"].shape) == (N, 3, 3)
        assert same(b["target_w2cs"], w2cs[tt]) and same(b["target_Ks"], Ks[tt]) and same(b["target_ts"], tt)
        assert same(b["tables/Ks"], Ks[tt].reshape(N, 9)) and int(b["ts"]) == int(ids[q]) and int(b["status"]) == 0
    for k, v in o.items():
        if v.is_floating_point():
            assert not torch.isnan(v).any(), k  # every element of the buffers was written
    clip.check(out), clip.check()


# ---------------------------------------------------------------------------------------------------------------- the draw

@pytest.mark.parametrize("n", (63, 64))
def test_draw_of_a_whole_wave_equals_its_cpu_twin(n):
    """k_feed_draw is one wave whose lane k keeps pick k: n = 63 and 64 (the most) use lanes 62 and 63.  From a range of exactly n
    frames every draw is a permutation of the range; from n + 1 frames the picks are distinct and one frame is left out."""
    assert n <= feed.MAX_TARGETS == 64  # feed.hip: FEED_MAX_TARGETS = 64, "one wave holds a draw"
    for extra in (0, 1):
        start, end = 1, 1 + n + extra
        clip = synthetic_clip(66, 5, 6, 3, seed=n, start=start, end=end, n=n)
        got = [clip.draw(31 + n).cpu().tolist() for _ in range(20)]
        assert int(clip.counter) == 20
        assert got == [feed.draw_cpu(31 + n, step, start, end, n) for step in range(20)]
        assert all(len(t) == n and len(set(t)) == n and all(start <= x < end for x in t) for t in got)
        if extra == 0:  # (Floyd's picks give a set: pick k is a new frame or frame k, so the whole range comes out in order)
            assert all(sorted(t) == list(range(start, end)) for t in got)
        else:  # the frame left out moves: 20 uniform picks among n + 1 frames hit about 17 different ones, a stuck draw one
            assert len({sum(range(start, end)) - sum(t) for t in got}) > 10


def test_draw_equals_its_cpu_twin_for_50_steps():
    clip, _ = fixture_clip("24x32")
    clip.counter.zero_()
    drawn = []
    for _ in range(50):
        drawn.append(clip.draw(2024).clone())
    assert int(clip.counter) == 50
    got = torch.stack(drawn).cpu().tolist()
    assert got == [feed.draw_cpu(2024, step, START, END, 4) for step in range(50)]
    assert all(len(set(t)) == 4 and all(START <= x < END for x in t) for t in got)
    wide = synthetic_clip(24, 5, 6, 3, seed=5, start=2, end=23, n=4)  # more frames than targets: the draws differ from step to step
    got = [wide.draw(7).cpu().tolist() for _ in range(50)]
    assert got == [feed.draw_cpu(7, step, 2, 23, 4) for step in range(50)] and len({tuple(t) for t in got}) > 40


def test_a_captured_draw_and_batch_sees_new_targets_on_every_replay():
    clip, _ = fixture_clip("24x32")
    wide = synthetic_clip(12, 24, 32, 70, seed=9, start=1, end=11, n=4)
    for c, q in ((clip, 2), (wide, 5)):
        out, eager = c.buffers(), c.buffers()
        c.draw(99), c.batch(q, out=out)  # (the kernels are loaded before the capture)
        c.counter.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # one stream, no parallel branches; a host read in here would raise
            c.draw(99)
            b = c.batch(q, out=out)
        replayed = flat(b)
        assert int(c.counter) == 0  # captured, not run
        seen = set()
        for step in range(12):
            g.replay()
            targets = feed.draw_cpu(99, step, c.start, c.end, 4)
            seen.add(tuple(targets))
            assert c.targets.cpu().tolist() == targets and int(c.counter) == step + 1
            want = flat(c.batch(q, targets, out=eager))
            for k, v in replayed.items():
                assert torch.equal(bits(v), bits(want[k])), (step, k)
        assert c is clip or len(seen) > 8
        c.check(out)


# ------------------------------------------------------------------------------------------------------------ track losses

def test_track_losses_from_tables_equals_track_losses_bit_for_bit():
    clip, _ = fixture_clip("24x32")
    b = clip.batch(0, [1, 4, 2, 3])
    tables = b["track_tables"]
    g = torch.Generator().manual_seed(11)
    base = torch.cat([torch.randn(1, 24, 32, 4, 2, generator=g), torch.rand(1, 24, 32, 4, 1, generator=g) + 1.5], -1).to(DEV)
    results = []
    for fn in (lambda t: losses.track_losses_from_tables(t, tables),
               lambda t: losses.track_losses(t, b["query_tracks_2d"], b["target_Ks"], b["target_tracks_2d"], b["target_visibles"],
                                             tables["weights"], b["target_track_depths"])):
        t = base.clone().requires_grad_()
        l2d, ldepth = fn(t)
        (l2d * 0.7 + ldepth * 1.3).backward()
        results.append((l2d.detach(), ldepth.detach(), t.grad))
    (a2d, adepth, agrad), (b2d, bdepth, bgrad) = results
    print(f"track_2d {float(a2d):.6f}, mapped depth {float(adepth):.6f}, |grad| {float(agrad.abs().sum()):.6f}")
    assert torch.isfinite(a2d) and torch.isfinite(adepth) and float(a2d) > 0 and float(agrad.abs().sum()) > 0
    for x, y in ((a2d, b2d), (adepth, bdepth), (agrad, bgrad)):
        assert torch.equal(x.view(-1).view(torch.int32), y.view(-1).view(torch.int32))
    # the padded tables of an out= batch give the same values: padding takes no part
    out = clip.buffers()
    padded = clip.batch(0, [1, 4, 2, 3], out=out)["track_tables"]
    p2d, pdepth = losses.track_losses_from_tables(base, padded)
    assert abs(float(p2d) - float(a2d)) <= 1e-5 * float(a2d) and abs(float(pdepth) - float(adepth)) <= 1e-5 * float(adepth)


# ------------------------------------------------------------------------------------------------------------------ status

def test_a_selection_out_of_range_on_the_device_gives_padding_and_a_status_bit():
    clip, _ = fixture_clip("13x17")
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    for index, targets, bit, word in ((i32(6), i32(1, 2, 3, 4), 1, "index"), (i32(-1), i32(1, 2, 3, 4), 1, "index"),
                                      (i32(2 ** 31 - 1), i32(1, 2, 3, 4), 1, "index"), (i32(2), i32(1, 2, 6, 4), 2, "a target is"),
                                      (i32(2), i32(1, -2 ** 31, 3, 4), 2, "a target is"), (i32(7), i32(9, 2, 3, 4), 3, "index")):
        out = clip.buffers()
        for f in dataclasses.fields(out):
            x = getattr(out, f.name)
            x.fill_(1) if x.dtype in (torch.uint8, torch.int32, torch.int64) else x.fill_(float("nan"))
        out.status.zero_()
        o = flat(clip.batch(index, targets, out=out))
        assert int(o["status"]) == bit and int(o["n_queries"]) == 0
        assert (o["tables/pix"] == -1).all() and (o["query_tracks_2d"] == -1).all() and same(o["tables/rows"], np.repeat(np.arange(4), 257))
        for k in PER_QUERY + PLANES + ("ts", "w2cs", "Ks", "target_ts", "target_w2cs", "target_Ks", "target_track_imgs", "tables/vis",
                                       "tables/weights"):
            assert not o[k].any(), k
        with pytest.raises(RuntimeError, match=word):
            clip.check(out)
        clip.check(out)  # read and cleared
    # a legal call after a refused one: the bit stays until it is read
    out = clip.buffers()
    clip.batch(i32(6), i32(1, 2, 3, 4), out=out)
    o = flat(clip.batch(i32(3), i32(1, 2, 3, 4), out=out))
    assert int(o["n_queries"]) == 64 and int(o["status"]) == 1
    # a time id outside the clip: target_w2cs = w2cs[target_ts] has nothing to take
    odd = synthetic_clip(3, 6, 7, 4, seed=1, time_ids=(0, 1, 7))
    out = odd.buffers()
    assert int(flat(odd.batch(0, [1, 0], out=out))["status"]) == 0 and int(flat(odd.batch(0, [1, 2], out=out))["status"]) == 4
    with pytest.raises(RuntimeError, match="time id"):
        odd.check(out)
    with pytest.raises(ValueError, match="outside"):
        clip.batch(6, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="outside"):
        clip.batch(0, [1, 2, 3, 6])


def test_a_query_outside_the_image_has_no_pixel_no_flag_and_no_weight():
    clip = synthetic_clip(3, 6, 7, 8, seed=2)
    q, P = 1, 8
    rows = clip.tracks[int(clip.offsets[q]):int(clip.offsets[q + 1])].view(3, P, 4)
    rows[:, :, 2:] = -4.0  # every sample visible and confident
    outside = {0: (-3.0, 2.0), 2: (7.0, 1.0), 3: (1.5, -1.0), 5: (2.0, 6.0), 6: (float("nan"), 1.0), 7: (-0.5, 5.5)}
    for p, xy in outside.items():
        rows[q, p, 0], rows[q, p, 1] = xy
    b = clip.batch(q, [0, 2])
    t = b["track_tables"]
    pix, vis, w = t["pix"].view(2, P).cpu(), t["vis"].view(2, P).cpu(), t["weights"].view(2, P).cpu()
    gone = torch.tensor([p in outside and p != 7 for p in range(P)])  # (-0.5, 5.5) truncates to the pixel (0, 5)
    assert (pix[:, gone] == -1).all() and not vis[:, gone].any() and not w[:, gone].any()
    assert (pix[:, ~gone] >= 0).all() and vis[:, ~gone].all() and (w[:, ~gone] > 0).all() and int(pix[0, 7]) == 5 * 7
    assert b["target_visibles"][0].all()  # the batch's own flags do not know about the query's pixel


# ----------------------------------------------------------------------------------------------------------------- example

def test_the_example_trains_every_frame_from_a_graph_of_its_own():
    """examples/train_clip.py on a small scene: four dynamic frames, each with two eager steps and one captured graph (draw, batch,
    three renders, photometric and track losses, backward, one-launch Adam), then 12 replays in an order the host picks.  Every
    eager step and every replay drew once; no selection was out of range; the losses are finite."""
    import importlib.util
    import math

    spec = importlib.util.spec_from_file_location("train_clip_example", os.path.join(ROOT, "examples", "train_clip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, _, clip = mod.train(steps=12, W=128, H=96, F=6, start=1, end=5, n_tracks=200, n_fg=3000, n_bg=5000, K=6, verbose=False)
    print("losses", losses, "| draws", int(clip.counter))
    assert len(losses) == 12 and all(math.isfinite(x) and x > 0 for x in losses)
    assert clip.P_max == 200 and clip.num_targets == 4 and int(clip.counter) >= 4 * 2 + 12 and int(clip.status) == 0
