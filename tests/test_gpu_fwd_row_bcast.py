"""The narrow forward composites (csrc/raster_fwd.hip, D <= 4 and the depth-only kernels) against the plain forward of the A/B library
(tests/libd4gs_variants.so, one wave per tile), BITWISE, through rasterization(): renders, alphas, last_ids, final_T and every leaf
gradient of a forward + backward.  What the narrow step reads from the staged records, and how (whole 16-byte records, or any other
form of getting a row's splat to its 16 lanes), must not show in a single bit.

Cases: D = 1 .. 4 without and with the depth channel ("RGB", "RGB+D" / "RGB+ED"), the depth-only modes "D" / "ED"; depth segments on and
off (D4GS_SEG), the block filter on and off (D4GS_BLOCK_FILTER), lazy lists.

Scenes: 40 x 24 pixels - 3 x 2 tiles, the right column 8 pixels wide and the bottom row 8 pixels high, so waves and rows contain lanes
outside the image.  Every tile holds a designed number of small splats about its centre (tests/ladder.py) and 24 large opaque splats
in front of everything, centred on tile 0, reach every tile: tile 0 saturates inside its first batch, the other lists are one below,
at and one above the batch sizes of the kernels (a 128-slot and a 256-slot batch; the unsegmented narrow kernels stage 255 splats and
a null record, which puts 254 / 255 / 256 on their boundary as well), and two lists span three batches.  The list lengths are asserted
from the device's own offsets.

The A/B library has no plain depth-only forward (its variants composite colours): for "D" / "ED" the forward is held against the depth
channel, the alphas, last_ids and final_T of the plain "RGB+D" / "RGB+ED" render of one colour channel - the same per-pixel operations -
and the gradients against the A/B library's own depth-only render.

With depth segments on, the composite BACKWARD replays a list of more than 256 entries segment by segment from the boundary states the
forward stored, and hands partial sums over in another order than the whole-list replay of the plain library (which neither writes nor
reads boundary states): there the forward's four outputs are still held bitwise, the gradients to the hand-off's rounding - SEG_TOL and
VTOL of tests/test_gpu_list_edges.py, per column - and bitwise between filter on and filter off."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ladder
from tests.util import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
W, H = 40, 24
N_BIG = 24
SEG_TOL, VTOL = 2e-5, 4e-4  # segmented against whole-list backward (tests/test_gpu_list_edges.py); VTOL: the view matrix' cancelling sums
FWD = ("renders", "alphas", "last_ids", "final_T")
# list length of tiles 0 .. 5 (row-major), the large splats included
SCENES = {"a": (64, 127, 128, 129, 255, 256), "b": (64, 257, 254, 130, 511, 513)}
LEAVES = ("means", "quats", "scales", "opac", "colors", "V")
CONFIGS = [(D, mode) for D in (1, 2, 3, 4) for mode in ("RGB", "RGB+ED" if D % 2 else "RGB+D")] + [(0, "D"), (0, "ED")]
# (name, D4GS_SEG, D4GS_BLOCK_FILTER, lazy_sort)
VARIANTS = [("seg0", "0", "1", False), ("seg1", "1", "1", False), ("seg0_nofilter", "0", "0", False), ("seg1_nofilter", "1", "0", False),
            ("lazy", "0", "1", True)]


def _scene(name, D):
    lengths = SCENES[name]
    sc = ladder.ladder_scene(W, H, [n - N_BIG for n in lengths], seed=5 + len(name) + ord(name), tiles=list(range(6)), D=max(D, 1))
    rng = np.random.default_rng(17)
    f, cx, cy = sc["K"][0, 0], sc["K"][0, 2], sc["K"][1, 2]
    z = np.float32(1.0 + 0.9 * (np.arange(N_BIG) + 0.5) / N_BIG).astype(np.float64)  # in front of the ladder's 2 .. 10
    px, py = 8.0 + rng.uniform(-0.5, 0.5, N_BIG), 8.0 + rng.uniform(-0.5, 0.5, N_BIG)
    big = dict(means=np.stack([(px - cx) * z / f, (py - cy) * z / f, z], -1), quats=np.tile([1.0, 0.0, 0.0, 0.0], (N_BIG, 1)),
               scales=np.tile((12.0 * z / f)[:, None], (1, 3)), opac=np.full(N_BIG, 0.99), colors=rng.uniform(0.05, 1.0, (N_BIG, max(D, 1))))
    out = {k: np.concatenate([sc[k], big[k]]) for k in big}
    out.update(V=sc["V"], K=sc["K"])
    return out


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _render(sc, D, mode, lazy):
    import deblur4dgs_amd.rasterization as R

    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.asarray(v)).float().to(dev) for k, v in sc.items()}
    for k in LEAVES:
        t[k].requires_grad_()
    kept = {}
    inner = R.render_instances

    def keep_state(*a, **kw):  # (final_T is not part of rasterization()'s info)
        out = inner(*a, **kw)
        kept["st"] = out[4]
        return out
    R.render_instances = keep_state
    try:
        bg = torch.linspace(0.2, 0.8, D).to(dev)[None] if D else None
        rc, ra, info = R.rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["colors"], t["V"][None], t["K"][None], W, H,
                                       backgrounds=bg, render_mode=mode, lazy_sort=lazy, near_target=64 if lazy else 0, exact_tiles=False)
    finally:
        R.render_instances = inner
    g = torch.Generator().manual_seed(3)
    wc, wa = torch.randn(rc.shape, generator=g).to(dev), torch.randn(ra.shape, generator=g).to(dev)
    ((rc * wc).sum() + (ra * wa).sum()).backward()
    torch.cuda.synchronize()
    out = dict(renders=rc, alphas=ra, last_ids=info["last_ids"], final_T=kept["st"].raster["final_T"],
               offsets=info["isect_offsets"].flatten(), n_isect=torch.tensor(info["n_isect"]))
    out.update({f"g_{k}": t[k].grad for k in LEAVES if t[k].grad is not None})  # (depth only: the colours take no gradient)
    return {k: _bits(v).clone() for k, v in out.items()}


def run_cases(out_path, kind):
    """Child process (the library is chosen when the package loads): every case with this process's library, saved as bit patterns."""
    res = {}
    for name in SCENES:
        for D, mode in CONFIGS + ([(1, "RGB+D"), (1, "RGB+ED")] if kind == "plain" else []):
            sc = _scene(name, D)
            for tag, seg, flt, lazy in (VARIANTS if kind == "product" else [("plain", None, "1", False)]):
                for k, v in (("D4GS_SEG", seg), ("D4GS_BLOCK_FILTER", flt)):  # (read per call)
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
                res[(name, D, mode, tag)] = _render(sc, D, mode, lazy)
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def outs(tmp_path_factory):
    from deblur4dgs_amd import build

    assert os.path.exists(build.VARIANTS_LIB), "run __graft_entry__.build() (builds tests/libd4gs_variants.so)"
    tmp = tmp_path_factory.mktemp("fwd_row_bcast")
    got = {}
    for kind, extra in (("product", {}), ("plain", {"D4GS_LIB_PATH": build.VARIANTS_LIB, "D4GS_FWD_WAVE_PER_TILE": "1"})):
        path = str(tmp / f"{kind}.pt")
        env = {k: v for k, v in os.environ.items() if not k.startswith(("D4GS_FWD_", "D4GS_BWD_")) and k not in ("D4GS_SEG", "D4GS_BLOCK_FILTER", "D4GS_LIB_PATH")}
        env.update(extra)
        code = "import sys; sys.path.insert(0, %r)\nfrom tests.test_gpu_fwd_row_bcast import run_cases\nrun_cases(sys.argv[1], sys.argv[2])\n" % ROOT
        r = subprocess.run([sys.executable, "-c", code, path, kind], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        assert r.returncode == 0, (kind, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        got[kind] = torch.load(path)
    return got


def test_the_scenes_put_the_lists_on_the_batch_boundaries(outs):
    for name, lengths in SCENES.items():
        o = outs["plain"][(name, 3, "RGB", "plain")]
        offs = o["offsets"].tolist() + [int(o["n_isect"])]
        assert tuple(b - a for a, b in zip(offs[:-1], offs[1:])) == lengths, (name, offs)
        # tile 0 (all of it inside the image) saturates inside its first batch: every pixel stops before the end of the 64-entry list
        last, fT = o["last_ids"].view(H, W)[:16, :16], o["final_T"].view(torch.float32).view(H, W)[:16, :16]
        assert int(last.max()) < offs[0] + lengths[0] - 1 and float(fT.max()) < 0.02, (name, int(last.max()), float(fT.max()))
        # and the longest list is walked past its first batch: some pixel of tile 4 takes its last contribution from a later one
        if lengths[4] > 256:
            reach = int(o["last_ids"].view(H, W)[16:, 16:32].max()) - offs[4]
            print(f"scene {name}: tile 4's last contributor at list position {reach} of {lengths[4]}")
            assert reach >= 256, (name, reach)
    assert {127, 128, 129, 254, 255, 256, 257} <= set(SCENES["a"]) | set(SCENES["b"])


@pytest.mark.parametrize("variant", [v[0] for v in VARIANTS])
@pytest.mark.parametrize("D,mode", CONFIGS)
def test_narrow_forward_equals_the_plain_forward_bitwise(D, mode, variant, outs):
    for name in SCENES:
        got, ref = outs["product"][(name, D, mode, variant)], outs["plain"][(name, D, mode, "plain")]
        assert set(got) == set(ref) and {"g_" + k for k in LEAVES if k != "colors" or D} <= set(got)
        fwd = ref
        if D == 0:  # the plain forward of the same per-pixel operations: one colour channel and the depth, its last channel
            rgbd = outs["plain"][(name, 1, "RGB+" + mode, "plain")]
            fwd = dict(ref, renders=rgbd["renders"][..., 1:], alphas=rgbd["alphas"], last_ids=rgbd["last_ids"], final_T=rgbd["final_T"])
        segmented = variant.startswith("seg1")
        bad = [k for k in got if (k in FWD or not segmented) and not torch.equal(got[k], (fwd if k in FWD else ref)[k])]
        assert not bad, (name, D, mode, variant, bad)
        if segmented:
            twin = outs["product"][(name, D, mode, "seg1" if variant != "seg1" else "seg1_nofilter")]
            for k in (k for k in got if k.startswith("g_")):
                assert torch.equal(got[k], twin[k]), (name, D, mode, variant, k)
                a, b = (x.view(torch.float32).reshape(-1, x.shape[-1] if x.dim() > 1 else 1) for x in (ref[k], got[k]))
                for c in range(a.shape[1]):
                    err = rel_err(b[:, c], a[:, c])
                    assert err <= (VTOL if k == "g_V" else SEG_TOL), (name, D, mode, variant, k, c, err)
        assert int((got["g_means"] != 0).sum()) > 0 and int((got["renders"] != 0).sum()) > 0
