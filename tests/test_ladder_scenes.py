"""The ladder scenes (tests/ladder.py) come out as designed: run through the scalar-C oracle, every tile's list has exactly the
designed length and members, every tie group shares one float32 depth and sits in its list contiguously in Gaussian-id order, and the
scenes together put a list on every boundary length of the kernels and reach every sort regime.  No GPU: this keeps the GPU tests of
tests/test_gpu_list_edges.py on the edges they are meant to hit."""
import numpy as np
import pytest

from oracle import cref
from tests import ladder


def _run(sc):
    return cref.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opac"], sc["colors"], sc["V"], sc["K"], sc["W"], sc["H"],
                              render_mode="RGB+ED", dtype=np.float64)


@pytest.mark.parametrize("name", list(ladder.SCENES) + ["grid"])
def test_ladder_lists_come_out_as_designed(name):
    sc = ladder.build(name, D=3)
    _, al, ctx = _run(sc)
    N = sc["means"].shape[0]
    assert (ctx["radii"] > 0).all() and ctx["radii"].max() <= ladder.MAX_RADIUS, ctx["radii"].max()
    assert (ctx["tiles_per_gauss"] == 1).all()
    offs, flat = ctx["offs"].astype(np.int64), ctx["flat"][: ctx["n_isect"]]
    assert ctx["n_isect"] == N and offs[-1] == N
    assert np.array_equal(np.diff(offs), sc["counts"])
    for t in np.nonzero(sc["counts"])[0]:
        members = flat[offs[t]:offs[t + 1]]
        assert np.array_equal(np.sort(members), np.nonzero(sc["tile_of"] == t)[0]), t
    z32 = ctx["dep"].astype(np.float32)
    pos = np.empty(N, np.int64)
    pos[flat] = np.arange(N)
    for g in sc["ties"]:
        assert len(g) >= 3 and (z32[g] == z32[g[0]]).all()
        assert np.array_equal(pos[g], pos[g[0]] + np.arange(len(g))), "tie group not contiguous in id order"
        assert (np.diff(g) > 1).any() or len(g) == N  # ids interleaved with other splats
    # every other pair of list neighbours: depths at least ~5e-5 apart (relative), far from any float32 near-tie
    for t in np.nonzero(sc["counts"] > 1)[0]:
        z = ctx["dep"][flat[offs[t]:offs[t + 1]]]
        rel = np.diff(z) / z[1:]
        assert (rel >= 0).all() and ((rel == 0) | (rel > 4e-5)).all()
    if ladder.SCENES.get(name, {}).get("regime") == "translucent":
        assert al.max() < 1.0 - 2e-4  # no pixel's transmittance near the 1e-4 stop
    if name == "chunks":  # one tie group in a list of the 4 096-key class, one in the 16 384-key class, each across a 512-key chunk boundary
        assert sorted(sc["counts"][sc["counts"] > 0].tolist()) == [2560, 2561, 3584, 3585, 4608, 4609, 6144, 6145, 12288, 12289, 16383]
        assert ladder.sort_launches(N, sc["counts"].size, 16383) == ("merge_short", 0, 4)
        for g, (lo, hi) in zip(sc["ties"], ((2048, 4096), (8192, 16384))):
            t = sc["tile_of"][g[0]]
            p = pos[g] - offs[t]
            assert lo < sc["counts"][t] <= hi and len(g) >= 600 and p[0] // 512 != p[-1] // 512
    if name == "long":  # mixed regime: the long lists stop early, at steps that differ inside a 2x2 quad of one tile
        last = ctx["last"]
        t = int(np.argmax(sc["counts"]))
        ty, tx = divmod(t, sc["tw"])
        blk = last[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] - offs[t]
        assert 0 < blk.max() < sc["counts"][t] - 1
        h, w = blk.shape[0] // 2 * 2, blk.shape[1] // 2 * 2
        q = blk[:h, :w].reshape(h // 2, 2, w // 2, 2)
        assert (q.max(axis=(1, 3)) != q.min(axis=(1, 3))).any()
        assert ((blk % 255 != 254) & (blk % 256 != 255) & (blk > 0)).any()  # some stop falls inside a forward batch


def test_ladder_covers_every_edge_and_every_sort_regime():
    lens = set()
    seen = set()
    for name in list(ladder.SCENES) + ["grid"]:
        sc = ladder.build(name)
        c = sc["counts"]
        lens |= set(c[c > 0].tolist())
        T, n, longest = c.size, int(c.sum()), int(c.max())
        for cap, hint in ((n, longest), (ladder.warm_capacity(n), ladder.sort_class(longest))):
            seen.add(ladder.sort_launches(cap, T, hint)[0])
        seen.add(ladder.sort_launches(n, T, longest, merge_long_allowed=False)[0])
    assert set(ladder.EDGES) <= lens, sorted(set(ladder.EDGES) - lens)
    assert {L % 4 for L in ladder.EDGES} == {0, 1, 2, 3}
    assert seen == {"merge_short", "merge_long", "neither"}
    # the designed regime of each scene (tests/test_gpu_list_edges.py asserts the same numbers from the device's launch counts)
    assert ladder.sort_launches(3659 + 6 + 7 + 66 + 130 + 258, 104, 513) == ("merge_long", 1, 0)
    assert ladder.sort_launches(15552, 24, 4097) == ("neither", 1, 3)
    assert ladder.sort_launches(ladder.warm_capacity(15552), 24, ladder.sort_class(4097)) == ("merge_short", 0, 3)


@pytest.mark.parametrize("D", [1, 2, 16])
def test_ladder_colour_channels(D):
    sc = ladder.recolor(ladder.build("short"), D, seed=3, subnormal=True)
    col = sc["colors"]
    assert col.shape[1] == D
    if D >= 2:
        sub = col[:, -1].astype(np.float32)
        assert (sub > 0).all() and (sub < np.finfo(np.float32).tiny).all()  # subnormal in float32, not flushed by the cast
    if D == 16:
        assert col[:, 1].min() > 40 and col[:, 2].max() < 0 and col[:, 3].max() <= 1e-3
