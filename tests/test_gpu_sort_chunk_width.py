"""The LDS sort of 513 .. 2 048-key tile lists at every length where a chunk width or a chunk count changes.

`sort_list_lds` (csrc/binning.hip) sorts lists of 513 .. 1 024 keys as three or four register chunks of 256 keys and lists of 1 025 ..
2 048 keys as three or four chunks of 512; a wave loads its chunks from global memory and writes the sorted list out of its registers.
k_tile_sort's first class calls it for one list per workgroup, k_tile_sort_w<LONG> for up to four lists one after the other in one
workgroup, through the same 16 KB of LDS at either chunk width.  The edges are therefore 512 | 513 (one wave, no LDS | LDS), 768 | 769 (three | four 256-key chunks), 1 024 | 1 025
(256-key | 512-key chunks; two | three of them), 1 536 | 1 537 (three | four) and 2 048 (the last full chunk, no padding), plus the
lengths one short of a full chunk (767, 1 023, 1 535, 2 047).  The ladder scenes of tests/test_gpu_list_edges.py hit only some of them.
A scene in the merge_short regime takes the k_tile_sort path, one in merge_long the k_tile_sort_w<LONG> path, where every workgroup
holds lists on both sides of 1 024 keys.  Lists must EQUAL the scalar-C oracle's, every entry, cold and warm; depth ties are broken by
emission index."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import cref
from tests import ladder

gpu = pytest.mark.gpu
# interleaved so that four consecutive tiles (one k_tile_sort_w workgroup) hold lists on both sides of 1 024 keys
LENGTHS = (512, 1025, 513, 2048, 767, 1535, 768, 1537, 769, 2047, 1023, 1024)
# tie groups inside one chunk, across a 256-key chunk boundary's worth of keys, and in a four-chunk list of either width
TIES = ((2, 5), (8, 40), (10, 300), (7, 9), (3, 17))
SCENES = {
    # 16 tiles, 848 keys per tile on average: merge_short - one k_tile_sort launch of the (0, 2 048] class sorts every list
    "merge_short": dict(W=64, H=64, seed=21, tiles=None),
    # 36 tiles, 377 per tile (warm capacity 585 per tile): merge_long - k_tile_sort_w<LONG>; tiles 0 .. 11 are three whole workgroups
    "merge_long": dict(W=96, H=96, seed=22, tiles=tuple(range(12))),
}


def _oracle(sc):
    return cref.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opac"], sc["colors"], sc["V"], sc["K"], sc["W"], sc["H"],
                              render_mode="RGB", dtype=np.float64)


def _render(sc):
    import torch

    from deblur4dgs_amd.rasterization import rasterization

    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.asarray(sc[k])).float().to(dev) for k in ("means", "quats", "scales", "opac", "colors", "V", "K")}
    return rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"][None], t["K"][None], sc["W"], sc["H"],
                         render_mode="RGB", lazy_sort=False, exact_tiles=False)[2]


def _launches(fn):
    """-> (fn(), {kernel name: launches}) from the library's launch recorder."""
    import torch

    from deblur4dgs_amd import _lib as L

    lib = L.lib()
    buf = C.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    lib.d4gs_profile_collect(buf, C.c_size_t(len(buf)))  # (drops anything recorded before)
    lib.d4gs_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.d4gs_profile_enable(0)
    lib.d4gs_profile_collect(buf, C.c_size_t(len(buf)))
    return out, {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines()}


@functools.lru_cache(maxsize=None)
def _scene(name):
    """-> (scene, oracle lists, oracle offsets, n): built and run through the oracle once, shared (read-only) by the tests."""
    p = SCENES[name]
    sc = ladder.ladder_scene(p["W"], p["H"], LENGTHS, p["seed"], ties=TIES, tiles=p["tiles"])
    _, _, ctx = _oracle(sc)
    n = int(ctx["n_isect"])
    flat, offs = ctx["flat"][:n].copy(), ctx["offs"].copy()
    flat.setflags(write=False), offs.setflags(write=False)
    return sc, flat, offs, n


@pytest.mark.parametrize("name", list(SCENES))
def test_the_oracle_alone_gives_lists_of_the_intended_lengths(name):
    """No GPU: the scenes put exactly one list on every length of LENGTHS, with the designed members, ties contiguous in id order."""
    sc, flat, offs, n = _scene(name)
    N = sc["means"].shape[0]
    assert n == N == sum(LENGTHS) and offs[-1] == N
    got = np.diff(offs.astype(np.int64))
    assert np.array_equal(got, sc["counts"])
    assert sorted(got[got > 0].tolist()) == sorted(LENGTHS)
    for t in np.nonzero(sc["counts"])[0]:
        assert np.array_equal(np.sort(flat[offs[t]:offs[t + 1]]), np.nonzero(sc["tile_of"] == t)[0]), t
    pos = np.empty(N, np.int64)
    pos[flat] = np.arange(N)
    assert len(sc["ties"]) == len(TIES)
    for g in sc["ties"]:
        assert np.array_equal(pos[g], pos[g[0]] + np.arange(len(g))), "tie group not contiguous in id order"
        assert (np.diff(g) > 1).any()  # ids interleaved with the other splats: the depth alone does not order them
    # ids shuffled against depth order: no list is already sorted by id
    assert all((np.diff(flat[offs[t]:offs[t + 1]]) < 0).any() for t in np.nonzero(sc["counts"])[0])
    T = sc["counts"].size
    for cap, hint in ((n, max(LENGTHS)), (ladder.warm_capacity(n), ladder.sort_class(max(LENGTHS)))):  # cold, warm
        assert ladder.sort_launches(cap, T, hint)[0] == name
    if name == "merge_long":  # every workgroup of k_tile_sort_w (four consecutive tiles) holds lists on both sides of 1 024 keys
        for w in range(3):
            four = sc["counts"][4 * w:4 * w + 4]
            assert ((four > 512) & (four <= 1024)).any() and (four > 1024).any(), four


def _check(name, what, info, launches, warm):
    sc, flat, offs, n = _scene(name)
    assert info["n_isect"] == n, what
    assert np.array_equal(info["isect_offsets"].flatten().cpu().numpy(), offs[:-1]), what
    got = info["flatten_ids"].cpu().numpy()
    assert got.shape == flat.shape, (what, got.shape)
    if not np.array_equal(got, flat):
        bad = np.nonzero(got != flat)[0]
        tiles = np.unique(np.searchsorted(offs, bad, side="right") - 1)
        raise AssertionError(f"{what}: {bad.size} list entries differ from the oracle, first at {bad[:8].tolist()}, "
                             f"in lists of {sc['counts'][tiles].tolist()} keys")
    longest, T = max(LENGTHS), sc["counts"].size
    cap, hint = (ladder.warm_capacity(n), ladder.sort_class(longest)) if warm else (n, longest)
    regime, n_w, n_s = ladder.sort_launches(cap, T, hint)
    assert regime == name, (what, regime)
    assert launches.get("k_tile_sort_w", 0) == n_w and launches.get("k_tile_sort", 0) == n_s, (what, regime, launches)
    return got


@gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_lists_equal_the_oracle_at_every_chunk_edge(name):
    from deblur4dgs_amd import engine

    sc = _scene(name)[0]
    engine._SIZE_GUESS.clear()
    for warm in (False, True):
        info, launches = _launches(lambda: _render(sc))
        _check(name, f"{name} {'warm' if warm else 'cold'}", info, launches, warm)


@gpu
def test_two_renders_give_byte_identical_lists():
    from deblur4dgs_amd import engine

    sc = _scene("merge_short")[0]
    engine._SIZE_GUESS.clear()
    got = []
    for warm in (False, True):
        info, launches = _launches(lambda: _render(sc))
        got.append(_check("merge_short", f"determinism render {len(got)}", info, launches, warm).tobytes())
    assert got[0] == got[1]
