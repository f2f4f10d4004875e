"""Binning, sorting and compositing at every list-length boundary (tests/ladder.py scenes).

The kernels change behaviour at fixed list lengths: the forward's batches (255 splats + a null record for narrow widths, 127 + one for
16 channels, 256 for 5 / 8 channels and in the segmented kernels), the backward's 64-splat batches, the segment unit
256 x ceil(len / 2048), wave_sort_list<1, 2, 4, 8> at 64 .. 512 keys, k_tile_sort_w<LONG> to 2 048 keys, the LDS classes at 4 096 / 8 192 /
16 384 keys and the global-memory fallback, and the three dispatch regimes of launch_sorts (merge_short, merge_long, neither).  The
ladder scenes put a list on each of those lengths, with depth ties and Gaussian ids shuffled against depth order, and:

  - the device's tile lists EQUAL the scalar-C oracle's, tile by tile, cold and warm, with exact_cull on and off, in every sort regime,
    with the regime and size classes each render launched asserted from the recorded launches;
  - the forward equals the plain variants (one wave per tile, quads) bit for bit at every instantiated width and channel chunking, with
    and without depth segments, lazy and eager, with a subnormal colour channel that must not be flushed;
  - forward and backward match the fp64 oracle with NO allowance, normalised per output channel and per gradient column, once the
    pixels with a decision within 1e-5 of its threshold (oracle/margins.py) are masked on both sides - tie groups get no exemption;
  - the backward is the same with and without depth segments."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cref, margins
from tests import ladder
from tests.util import check_columns, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
EPS = 1e-5  # the ladder scenes sit away from every threshold: a decision margin below 1e-5 is all that is masked
SEG_TOL = 2e-5  # segmented vs whole-list backward (test_depth_segmented_backward_equals_the_whole_list_replay)
# The view-matrix gradient is a sum over every Gaussian (66 k in the "long" scene) whose terms cancel: its translation column is a
# small difference of large float32 partial sums, and the segmented replay hands those partial sums off in a different order.  Measured
# on "long", D = 16: 2.7e-5 unsegmented, 1.2e-4 segmented against the fp64 oracle; every other column of every tensor stays below 1.1e-5.
# (test_depth_segmented_backward_equals_the_whole_list_replay allows the same 4e-4 for the same reason.)
VTOL = 4e-4
CHILD_TIMEOUT = 300


def _oracle(sc, mode="RGB+ED", bg=None):
    return cref.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opac"], sc["colors"], sc["V"], sc["K"], sc["W"], sc["H"],
                              background=bg, render_mode=mode, dtype=np.float64)


def _render(sc, mode, bg=None, grad=False, **kw):
    from deblur4dgs_amd.rasterization import rasterization

    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.asarray(sc[k])).float().to(dev) for k in ("means", "quats", "scales", "opac", "colors", "V", "K")}
    if grad:
        for k in ("means", "quats", "scales", "opac", "colors", "V"):
            t[k].requires_grad_()
    kw = dict(dict(lazy_sort=False, exact_tiles=False), **kw)
    rc, ra, info = rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"][None], t["K"][None], sc["W"], sc["H"],
                                 backgrounds=None if bg is None else torch.tensor(bg, device=dev).float()[None], render_mode=mode, **kw)
    return rc, ra, info, t


def _launches(fn):
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


def lists_case(name, merge_long_allowed=True):
    """Render the scene cold and warm with exact_cull on and off; the lists must equal the oracle's and the launches the regime's.
    -> the regimes seen.  (Also run in a child process with D4GS_SORT_NO_MERGE_LONG set.)"""
    from deblur4dgs_amd import engine

    sc = ladder.build(name)
    _, _, ctx = _oracle(sc)
    n, T = ctx["n_isect"], sc["counts"].size
    want_ids, want_offs = ctx["flat"][:n], ctx["offs"][:-1]
    longest = int(sc["counts"].max())
    seen = []
    for exact_cull in (True, False):
        engine._SIZE_GUESS.clear()
        for warm in (False, True):
            (rc, ra, info, _), launches = _launches(lambda: _render(sc, "RGB", exact_cull=exact_cull))
            what = f"{name} exact_cull={exact_cull} {'warm' if warm else 'cold'}"
            assert info["n_isect"] == n, what
            assert np.array_equal(info["isect_offsets"].flatten().cpu().numpy(), want_offs), what
            got = info["flatten_ids"].cpu().numpy()
            if not np.array_equal(got, want_ids):
                bad = np.nonzero(got != want_ids)[0]
                raise AssertionError(f"{what}: {bad.size} list entries differ from the oracle, first at {bad[:8].tolist()}")
            cap, hint = (ladder.warm_capacity(n), ladder.sort_class(longest)) if warm else (n, longest)
            regime, n_w, n_s = ladder.sort_launches(cap, T, hint, merge_long_allowed)
            assert launches.get("k_tile_sort_w", 0) == n_w and launches.get("k_tile_sort", 0) == n_s, (what, regime, launches)
            seen.append((regime, n_s))
    return seen


@pytest.mark.parametrize("name", list(ladder.SCENES) + ["grid"])
def test_tile_lists_equal_the_oracle_in_every_sort_regime(name):
    seen = lists_case(name)
    designed = {"short": ("merge_long", 0), "mid": ("merge_long", 1), "long": ("merge_short", 5), "between": ("neither", 3),
                "chunks": ("merge_short", 4), "grid": ("merge_long", 0)}[name]
    assert seen[0] == designed, seen  # the cold render ran the regime and classes the scene was designed for
    if name == "between":
        assert seen[1] == ("merge_short", 3), seen


def test_tile_lists_without_merge_long():
    """D4GS_SORT_NO_MERGE_LONG (read once per process): the 513 .. 2 048-key lists of a mostly-short scene go to the first LDS class."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_list_edges import lists_case\n"
            "seen = lists_case('mid', merge_long_allowed=False)\n"
            "assert seen[0] == ('neither', 2), seen\n"
            "print('ok', seen)\n") % ROOT
    env = dict(os.environ, D4GS_SORT_NO_MERGE_LONG="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- forward: bit for bit against the plain variants -----------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 4, 5, 8, 16, 17, 20, 33)
MODES = ("RGB", "RGB+D", "RGB+ED")
FWD_CASES = ([("mid", D, m) for D in WIDTHS for m in MODES] + [(s, D, "RGB+ED") for s in ("short", "long", "between") for D in (3, 16)]
             + [("grid", 16, "RGB+ED")])


def _bg(D):
    bg = np.linspace(0.1, 0.9, D)
    if D >= 2:
        bg[-1] = 0.0  # the subnormal channel: what is there is the splats' contribution
    return bg


def fwd_cases_run(out_path, kind):
    """Child process: render FWD_CASES with the library / variant of this process's environment and save what was rendered (large
    images as digests).  kind "product": with D4GS_SEG 0 and 1 and with lazy_sort; the subnormal channel is checked here."""
    res = {}
    for name, D, mode in FWD_CASES:
        sc = ladder.build(name, D=D, subnormal=True)
        runs = (("seg0", "0", False), ("seg1", "1", False), ("lazy", None, True)) if kind == "product" else (("plain", None, False),)
        for tag, seg, lazy in runs:
            if seg is None:
                os.environ.pop("D4GS_SEG", None)
            else:
                os.environ["D4GS_SEG"] = seg
            rc, ra, info, _ = _render(sc, mode, bg=_bg(D), lazy_sort=lazy)
            torch.cuda.synchronize()
            out = (rc[0].cpu(), ra[0].cpu(), info["last_ids"][0].cpu())
            if D >= 2:  # not flushed: every pixel some splat reaches carries a non-zero subnormal channel
                sub, hit = out[0][..., D - 1], out[1][..., 0] > 0
                assert bool(hit.any()) and bool((sub[hit] != 0).all()), (name, D, mode, tag, int((sub[hit] == 0).sum()))
                assert float(sub.abs().max()) < 1e-37
            if name == "grid":
                out = tuple(hashlib.sha256(x.numpy().tobytes()).hexdigest() for x in out)
            res[(name, D, mode, tag)] = out
    os.environ.pop("D4GS_SEG", None)
    torch.save(res, out_path)


def test_forward_bitwise_equal_to_the_plain_variants_at_every_edge(tmp_path):
    from deblur4dgs_amd import build

    assert os.path.exists(build.VARIANTS_LIB), "run __graft_entry__.build() (builds tests/libd4gs_variants.so)"
    var = {"D4GS_LIB_PATH": build.VARIANTS_LIB}
    outs = {}
    for kind, extra in (("product", {}), ("A", {**var, "D4GS_FWD_WAVE_PER_TILE": "1"}), ("B", {**var, "D4GS_FWD_QUADS": "1"})):
        path = str(tmp_path / f"fwd_{kind}.pt")
        env = {k: v for k, v in os.environ.items() if not k.startswith("D4GS_FWD_") and k != "D4GS_SEG"}
        env.update(extra)
        code = "import sys; sys.path.insert(0, %r)\nfrom tests.test_gpu_list_edges import fwd_cases_run\nfwd_cases_run(sys.argv[1], sys.argv[2])\n" % ROOT
        r = subprocess.run([sys.executable, "-c", code, path, "product" if kind == "product" else "variant"], env=env,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        assert r.returncode == 0, (kind, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        outs[kind] = torch.load(path)
    bad = []
    for name, D, mode in FWD_CASES:
        ref = outs["A"][(name, D, mode, "plain")]
        others = {"B": outs["B"][(name, D, mode, "plain")], **{t: outs["product"][(name, D, mode, t)] for t in ("seg0", "seg1", "lazy")}}
        for who, got in others.items():
            for what, x, y in zip(("render_colors", "render_alphas", "last_ids"), got, ref):
                if not (x == y if isinstance(x, str) else torch.equal(x, y)):
                    bad.append((name, D, mode, who, what))
    assert not bad, bad


# ---- forward and backward against the fp64 oracle, no allowance -----------------------------------------------------------------
def _eps_px(W, H):
    return 32 * 6e-8 * max(W, H)  # (tests/test_gpu_flip_cause.py: float32 evaluates a projected centre to a few ulp of the image size)


ORACLE_CASES = [(s, D) for s in ("short", "mid", "long") for D in (3, 8, 16, 20)]


@pytest.mark.parametrize("name,D", ORACLE_CASES)
def test_forward_and_backward_match_the_fp64_oracle_per_column(name, D, monkeypatch):
    sc = ladder.build(name, D=D)
    W, H, N = sc["W"], sc["H"], sc["means"].shape[0]
    bg = np.linspace(0.1, 0.9, D)
    out, al, ctx = _oracle(sc, bg=bg)
    n = ctx["n_isect"]
    mg = margins.pixel_margins(torch.from_numpy(ctx["m2d"]), torch.from_numpy(ctx["con"]), torch.from_numpy(sc["opac"]),
                               torch.from_numpy(ctx["dep"]), torch.from_numpy(ctx["flat"][:n]).long(), torch.from_numpy(ctx["offs"]).long(), W, H)
    dt = lambda k: torch.from_numpy(np.asarray(sc[k], np.float64))
    toggles, _ = margins.gaussian_toggle_mask(dt("means"), dt("quats"), dt("scales"), dt("opac"), dt("V"), dt("K"), W, H, eps_px=_eps_px(W, H))
    # eps_order 0: tie groups and list neighbours are NOT fragile - their order must simply match
    F = margins.fragile_pixels(mg, EPS, eps_order=0.0) | toggles
    assert float(F.float().mean()) <= 0.05, float(F.float().mean())
    keep = (~F).double().numpy()[..., None]
    g = np.random.default_rng(7)
    wc, wa = g.standard_normal(out.shape), g.standard_normal(al.shape)
    ref = cref.backward(ctx, wc * keep, wa * keep)
    ref_img, ref_al = torch.from_numpy(out), torch.from_numpy(al)
    names = ("means", "quats", "scales", "opac", "colors")
    dev = torch.device("cuda:0")
    got = {}
    for seg in ("0", "1"):
        monkeypatch.setenv("D4GS_SEG", seg)
        rc, ra, info, t = _render(sc, "RGB+ED", bg=bg, grad=True)
        info["means2d"].retain_grad()
        k = torch.from_numpy(keep).float().to(dev)
        ((rc[0] * torch.from_numpy(wc).float().to(dev) * k).sum() + (ra[0] * torch.from_numpy(wa).float().to(dev) * k).sum()).backward()
        torch.cuda.synchronize()
        case = f"list edges {name} D={D} RGB+ED D4GS_SEG={seg} ({int(F.sum())} fragile px masked, eps {EPS:g})"
        img, alp = rc[0].detach().cpu().double(), ra[0].detach().cpu().double()
        # image: a miss outside the fragile pixels is a failure (per output channel)
        den = ref_img.abs().amax(dim=(0, 1)).clamp(min=1e-30)
        miss = (((img - ref_img).abs() > TOL * den).any(-1) | ((alp - ref_al).abs() > TOL * float(ref_al.abs().max())).any(-1)) & ~F
        assert not bool(miss.any()), (case, int(miss.sum()), miss.nonzero()[:8].tolist())
        kk = (~F)[..., None].double()
        check_columns(case, "render_colors (unmasked px)", img * kk, ref_img * kk, TOL)
        check_columns(case, "render_alphas (unmasked px)", alp * kk, ref_al * kk, TOL)
        gd = dict({n_: t[n_].grad.cpu() for n_ in names}, viewmat=t["V"].grad.cpu()[:3], means2d=info["means2d"].grad[0].cpu())
        gr = dict({n_: torch.from_numpy(ref[n_]) for n_ in names}, viewmat=torch.from_numpy(ref["viewmat"][:3]),
                  means2d=torch.from_numpy(ref["means2d"]))
        for n_ in gd:
            check_columns(case, n_ + ".grad", gd[n_], gr[n_], VTOL if n_ == "viewmat" else TOL)
        got[seg] = gd
    for n_ in got["0"]:  # segmented and whole-list backward: the hand-off's rounding and nothing more
        a, b = (x.reshape(-1, x.shape[-1] if x.dim() > 1 else 1) for x in (got["0"][n_], got["1"][n_]))
        for c in range(a.shape[1]):
            assert rel_err(b[:, c], a[:, c]) <= (VTOL if n_ == "viewmat" else SEG_TOL), (name, D, n_, c, rel_err(b[:, c], a[:, c]))
