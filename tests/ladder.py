"""Scenes whose per-tile list lengths are chosen exactly (test infrastructure, no GPU needed to build or check them).

The composite, the sort and the depth segmentation change behaviour at fixed list lengths: the forward's batches of 255 / 256 / 127
splats, the backward's 64-splat batches, the 256-multiple segment unit, the register sorts of 64 .. 512 keys, the register-chunk LDS
sort beyond them (k_tile_sort_w's 513 .. 2 048-key lists and the classes at 2 048 / 4 096 / 8 192 / 16 384 keys: 256-key chunks up to
1 024 keys, 512-key chunks dealt round-robin to 4 / 8 / 16 waves beyond) and the global-memory fallback past 16 384.  A random scene crosses
some of those edges by chance; a ladder scene puts a list on each edge on purpose.

Construction (identity view matrix): every splat of a tile has its projected centre within 0.5 px of the tile's centre and a screen
radius of at most 7 px, so its rectangle - gsplat's floor / ceil rule and the exact ellipse cull alike - is that one tile.  The focal
length keeps every centre near the optical axis (|x / z| <= 1/4), so the depth extent of a splat adds little to its footprint.
Depths within a tile are distinct and at least ~5e-5 apart relatively, or bit-identical inside a designed tie group; Gaussian ids are
shuffled against depth order, so a tie group's ids are interleaved with the other splats of its tile.

`tests/test_ladder_scenes.py` runs every scene through the scalar-C oracle and checks that the lists come out as designed."""
from __future__ import annotations

import numpy as np

TILE = 16
MAX_RADIUS = 7


def _colors(rng, n, D, subnormal):
    """[n, D]: channel c % 4 = 0 in (0, 1), 1 at scale 1e3, 2 negative, 3 at scale 1e-3; `subnormal`: the last channel (D >= 2) holds
    positive values of about 1e-39 (subnormal in float32)."""
    u = rng.uniform(0.05, 1.0, size=(n, D))
    scale = np.array([(1.0, 1e3, -1.0, 1e-3)[c % 4] for c in range(D)])
    col = u * scale
    if subnormal and D >= 2:
        col[:, -1] = rng.uniform(0.5, 2.0, size=n) * 1e-39
    return col


def ladder_scene(W: int, H: int, lengths, seed: int, *, ties=(), regime: str = "mixed", D: int = 3, subnormal: bool = False,
                 tiles=None, zrange=(2.0, 10.0)):
    """-> dict(means, quats, scales, opac, colors, V, K [float64 numpy], W, H, tile_of [N], counts [tiles], ties [list of id arrays]).

    lengths  list length of each populated tile (placed on tiles in a shuffled order; the bottom-right tile - partial when W or H is not
             a multiple of 16 - always gets the first length);
    ties     (index into `lengths`, group size) pairs: that many splats of that tile share one float32 depth;
    regime   "translucent": opacities low enough that no pixel's transmittance reaches 1e-4 (every list <= 513);
             "mixed": opacities in (0.05, 0.6) with one splat in ten at 0.95 .. 0.99, so pixels stop at different steps;
    tiles    explicit tile indices for `lengths` (default: shuffled)."""
    rng = np.random.default_rng(seed)
    tw, th = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    T = tw * th
    lengths = [int(x) for x in lengths]
    if tiles is None:
        rest = rng.permutation(T - 1)[: len(lengths) - 1]
        tiles = [T - 1] + rest.tolist()
    tiles = [int(t) for t in tiles]
    assert len(tiles) == len(lengths) <= T and len(set(tiles)) == len(tiles)
    f = float(max(200.0, 2.0 * max(W, H)))
    cx, cy = W / 2.0, H / 2.0
    tie_of = {}
    for li, g in ties:
        tie_of.setdefault(li, []).append(g)
    px, py, z, tile_of, groups = [], [], [], [], []
    start = 0
    for li, (t, L) in enumerate(zip(tiles, lengths)):
        ty, tx = divmod(t, tw)
        px.append(TILE * tx + 8.0 + rng.uniform(-0.5, 0.5, size=L))
        py.append(TILE * ty + 8.0 + rng.uniform(-0.5, 0.5, size=L))
        # distinct, evenly spaced depths (relative spacing >= (z1 - z0) / (L z1)), shuffled against the splats' order
        zz = np.float32(zrange[0] + (zrange[1] - zrange[0]) * (np.arange(L) + 0.5) / L)
        zz = zz[rng.permutation(L)].astype(np.float64)
        pos = 0
        for g in tie_of.get(li, []):
            assert pos + g <= L
            zz[pos:pos + g] = zz[pos]  # one float32 value, exact under the identity view
            groups.append(start + np.arange(pos, pos + g))
            pos += g
        z.append(zz)
        tile_of.append(np.full(L, t))
        start += L
    px, py, z, tile_of = (np.concatenate(a) for a in (px, py, z, tile_of))
    N = px.shape[0]
    # Gaussian id = perm position: ids shuffled against depth order and against tiles
    perm = rng.permutation(N)
    inv = np.empty(N, np.int64)
    inv[perm] = np.arange(N)
    px, py, z, tile_of = px[perm], py[perm], z[perm], tile_of[perm]
    groups = [np.sort(inv[g]) for g in groups]
    means = np.stack([(px - cx) * z / f, (py - cy) * z / f, z], -1)
    q = rng.normal(size=(N, 4))
    quats = q / np.linalg.norm(q, axis=-1, keepdims=True)
    # 1.3 .. 1.8 px on screen per axis: radius 5 .. 7, so a splat of a partial edge tile whose centre lies up to 4.5 px beyond the
    # image still reaches into it (the 1300 x 1000 grid's last column is 4 px wide)
    scales = rng.uniform(1.3, 1.8, size=(N, 3)) * (z / f)[:, None]
    if regime == "translucent":
        per = np.array([min(0.5, 6.0 / L) for L in lengths])  # sum of the alphas at a pixel < 6: T > e^-6.2 > 1e-4
        lut = dict(zip(tiles, per))
        opac = np.array([lut[t] for t in tile_of]) * rng.uniform(0.5, 1.0, size=N)
        assert opac.min() > 1.0 / 255.0 * 1.2
    else:
        opac = rng.uniform(0.05, 0.6, size=N)
        hard = rng.random(N) < 0.1
        opac[hard] = rng.uniform(0.95, 0.99, size=int(hard.sum()))
    counts = np.zeros(T, np.int64)
    for t, L in zip(tiles, lengths):
        counts[t] = L
    V = np.eye(4)
    K = np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
    return dict(means=means, quats=quats, scales=scales, opac=opac, colors=_colors(rng, N, D, subnormal), V=V, K=K, W=W, H=H,
                tile_of=tile_of, counts=counts, ties=groups, tw=tw, th=th)


def recolor(sc: dict, D: int, seed: int, subnormal: bool = False) -> dict:
    """The same geometry with D colour channels."""
    rng = np.random.default_rng(seed)
    return dict(sc, colors=_colors(rng, sc["means"].shape[0], D, subnormal))


def sort_launches(n_cap: int, n_tiles: int, longest: int, merge_long_allowed: bool = True):
    """-> (regime, k_tile_sort_w launches, k_tile_sort launches) of binning.hip `launch_sorts` (pass 0) for a list capacity `n_cap`,
    `n_tiles` lists and a longest-list bound `longest` (0 = unknown: the capacity)."""
    CHUNK = 512
    longest = longest if longest > 0 else n_cap
    merge_short = longest > CHUNK and n_cap >= 768 * n_tiles
    merge_long = not merge_short and merge_long_allowed and longest > CHUNK and n_cap < 640 * n_tiles
    lows = [0 if merge_short else CHUNK, 2048, 4096, 8192, 16384]
    n = 0
    for lo in lows[1 if merge_long else 0:]:
        if longest <= lo:
            break
        n += 1
    regime = "merge_short" if merge_short else "merge_long" if merge_long else "neither"
    return regime, 0 if merge_short else 1, n


def sort_class(max_tile: int) -> int:
    """engine._sort_class: the longest-list bound a warm render launches with (0 = unknown)."""
    for c in (512, 2048, 4096, 8192, 16384):
        if 3 * max_tile <= 2 * c:
            return c
    return 0


def warm_capacity(n: int) -> int:
    """engine._sized_launch: the capacity a render launches with once an earlier render of its shape measured n intersections."""
    return n + n // 4 + 4096


# The designed scenes.  Every boundary length of the kernels appears in at least one of them (tests/test_ladder_scenes.py checks it).
EDGES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 254, 255, 256, 257, 510, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8192, 8193,
         16384, 16385)
SCENES = {
    # 104 tiles, every list <= 513: k_tile_sort_w sorts all of them (LONG form for the 513-key list), no pixel saturates
    "short": dict(W=203, H=117, seed=11, regime="translucent", ties=((12, 5), (18, 7)),
                  lengths=(1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 254, 255, 256, 257, 510, 511, 512, 513, 6, 7, 66, 130, 258)),
    # 104 tiles, lists to 2 049: merge_long (k_tile_sort_w sorts 513 .. 2 048 keys in LDS) plus the 2 048 .. 4 096 class
    "mid": dict(W=203, H=117, seed=12, ties=((3, 9), (7, 4), (9, 16)),
                lengths=(3, 65, 129, 255, 513, 1023, 1024, 1025, 1536, 2047, 2048, 2049, 64, 256, 511)),
    # 24 tiles (4 x 6, ragged), the longest lists: merge_short, every LDS class and the global-memory fallback
    "long": dict(W=91, H=53, seed=13, ties=((11, 6), (13, 300)),
                 lengths=(1, 2, 4, 64, 257, 512, 513, 2048, 2049, 4095, 4096, 4097, 8192, 8193, 16384, 16385)),
    # 24 tiles, 640 x 24 <= intersections < 768 x 24 on a cold render: neither merge (k_tile_sort_w + classes 0 .. 2); a warm render's
    # capacity crosses 768 per tile: merge_short
    "between": dict(W=91, H=53, seed=14, ties=((6, 3), (9, 11)),
                    lengths=(5, 63, 127, 254, 510, 2047, 2048, 2049, 4095, 4097, 128, 129)),
    # 16 tiles, merge_short: the chunk counts inside the larger LDS classes - five | six and seven | eight 512-key chunks on the eight waves
    # of the 4 096-key class, nine | ten and twelve | thirteen on the sixteen waves of the 8 192-key class, a second chunk per wave
    # (24 | 25) and a single key of padding (16 383) in the 16 384-key class; each tie group spans a chunk boundary
    "chunks": dict(W=64, H=64, seed=16, ties=((3, 600), (9, 640)),
                   lengths=(2560, 2561, 3584, 3585, 4608, 4609, 6144, 6145, 12288, 12289, 16383)),
}
# 1300 x 1000: 82 x 63 = 5 166 tiles (more than D4GS_SEG_TILES_MAX_NARROW, not a multiple of 4 or 8): no depth segments at any width
GRID = dict(W=1300, H=1000, seed=15, ties=((5, 3),), lengths=(1, 2, 3, 4, 5, 513, 64, 65, 256, 257))


def build(name: str, D: int = 3, subnormal: bool = False) -> dict:
    p = dict(GRID if name == "grid" else SCENES[name])
    W, H, seed, lengths = p.pop("W"), p.pop("H"), p.pop("seed"), p.pop("lengths")
    if name == "grid":  # one splat in every third tile besides the designed lists
        rng = np.random.default_rng(99)
        T = 82 * 63
        designed = [T - 1, 0, 81, T - 82, 2000, 3000, 4100, 17, 1234, 4321]
        others = [t for t in rng.permutation(T).tolist() if t not in designed][: T // 3]
        lengths = tuple(lengths) + (1,) * len(others)
        p["tiles"] = designed + others
    return ladder_scene(W, H, lengths, seed, D=D, subnormal=subnormal, **p)
