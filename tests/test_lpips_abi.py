"""The entry points of csrc/lpips.hip are declared under D4GS_LPIPS_API behind the feed block, parsed into a table of their own (the
seventh), bound and exported, and validate their arguments on the host before any launch: fake addresses - nothing is dereferenced; no
GPU needed.  The Python surface refuses CPU tensors, loads both key layouts of the trunk and names a missing, stray or misshapen key."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from tests import lpips_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d4gs_lpips_prepare", "d4gs_lpips_layer", "d4gs_lpips_score_blocks", "d4gs_lpips_score", "d4gs_lpips_mean")
A = 0x10000  # a fake, 16-byte aligned device address
SIZES = [s for hw in R.alex_sizes(47, 64) for s in hw]


def tables(ptrs=(A,) * 5, sizes=SIZES):
    return (C.c_void_p * 5)(*ptrs), (C.c_int32 * 10)(*sizes)


#                                 pred target masks M B H W normalize out stream
CALLS = {"d4gs_lpips_prepare": ([A, A, A, 3, 2, 47, 64, 1, A, None], {0: (b"pred", True, 4), 1: (b"target", True, 4), 2: (b"masks", False, 4),
                                                                      8: (b"out", True, 4)}),
         #                      f0 f1 weights n C h w out stream
         "d4gs_lpips_layer": ([A, A, A, 2, 192, 5, 7, A, None], {0: (b"f0", True, 4), 1: (b"f1", True, 4), 2: (b"weights", True, 4),
                                                                 7: (b"out", True, 4)}),
         #                      layers sizes masks M B H W score_map partials out stream
         "d4gs_lpips_score": ([None, None, A, 3, 2, 47, 64, A, A, A, None], {2: (b"masks", False, 4), 7: (b"score_map", False, 4),
                                                                             8: (b"partials", True, 8), 9: (b"out", True, 8)}),
         #                      layers sizes n out stream
         "d4gs_lpips_mean": ([None, None, 2, A, None], {3: (b"out", True, 8)})}
OFFSETS = {4: (1, 2, 3), 8: (1, 2, 4)}


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import _lib as L

    return L.lib()


def call(lib, fn, args, layers=None, sizes=None):
    args = list(args)
    if fn in ("d4gs_lpips_score", "d4gs_lpips_mean"):
        keep = tables()  # alive until the call returns
        args[0] = keep[0] if layers is None else layers
        args[1] = keep[1] if sizes is None else sizes
    return getattr(lib, fn)(*args)


def bad(lib, fn, args, *words, **kw):
    assert call(lib, fn, args, **kw) == -1, (fn, args)  # D4GS_EINVAL
    err = lib.d4gs_last_error()
    assert fn.encode() in err and all(w in err for w in words), err


def put(fn, i, v):
    base = CALLS[fn][0]
    return base[:i] + [v] + base[i + 1:]


def test_the_block_is_declared_parsed_bound_and_exported_in_a_table_of_its_own(lib):
    from deblur4dgs_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    assert lib.d4gs_version() == 305 and "#define D4GS_VERSION 305" in header and len(L.EXPORTS) == 79 and len(L.STRUCTS) == 16
    init, ev, data, fit, feed, lp = {}, {}, {}, {}, {}, {}
    _, structs, prototypes = L.parse(header, init, eval=ev, data=data, fit=fit, feed=feed, lpips=lp)
    assert tuple(lp) == NEW == tuple(L.LPIPS_PROTOTYPES)  # in the header's order
    others = (L.EXPORTS, L.INIT_PROTOTYPES, L.EVAL_PROTOTYPES, L.DATA_PROTOTYPES, L.FIT_PROTOTYPES, L.FEED_PROTOTYPES)
    assert all(not set(NEW) & set(t) for t in others) and tuple(prototypes) == L.EXPORTS  # disjoint from the other six tables
    assert (tuple(init), tuple(ev), tuple(data), tuple(fit), tuple(feed)) == tuple(tuple(t) for t in others[1:])
    assert set(structs) == set(L.STRUCT_NAMES.values())  # no new struct
    assert tuple(L.parse(header)[2]) == L.EXPORTS  # the keyword is optional: the block is read and counted all the same
    assert header.count("D4GS_LPIPS_API") >= len(NEW) + 1 and header.index("#define D4GS_LPIPS_API") > header.index("#define D4GS_FEED_API")
    dyn = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert hasattr(lib, name) and f"{name}(" in header and f" T {name}\n" in dyn, name
        assert getattr(lib, name).argtypes == L.LPIPS_PROTOTYPES[name][1] and getattr(lib, name).restype is L.LPIPS_PROTOTYPES[name][0], name
    score = L.LPIPS_PROTOTYPES["d4gs_lpips_score"][1]
    assert score[0]._type_ is C.c_void_p and score[1]._type_ is C.c_int32 and score[2] is C.c_void_p  # host tables, device pointers
    assert L.LPIPS_PROTOTYPES["d4gs_lpips_score_blocks"][0] is C.c_int64


def test_the_lpips_block_is_parsed_as_strictly_as_the_rest():
    from deblur4dgs_amd import _lib as L

    old = "D4GS_LPIPS_API int64_t d4gs_lpips_score_blocks(int32_t M, int32_t B, int32_t H, int32_t W);"
    text = open(os.path.join(ROOT, "include", "d4gs.h")).read()
    assert text.count(old) == 1
    for new, word in ((old[:-1], "D4GS_LPIPS_API prototypes"), (old.replace("int32_t M", "unsigned long M"), "d4gs_lpips_score_blocks"),
                      (old.replace("int64_t d4gs", "unsigned d4gs"), "d4gs_lpips_score_blocks")):
        with pytest.raises(ValueError) as e:
            L.parse(text.replace(old, new))
        assert word in str(e.value), str(e.value)


def test_null_and_misaligned_pointers_are_refused(lib):
    for fn, (base, ptrs) in CALLS.items():
        for i, (name, required, align) in ptrs.items():
            if required:
                bad(lib, fn, put(fn, i, None), name, b"NULL")
            for off in OFFSETS[align]:
                bad(lib, fn, put(fn, i, A + off), name, b"misaligned")
    for fn in ("d4gs_lpips_score", "d4gs_lpips_mean"):
        base = CALLS[fn][0]
        for k in range(5):
            bad(lib, fn, base, f"layers[{k}]".encode(), b"NULL", layers=tables(tuple(None if j == k else A for j in range(5)))[0])
            bad(lib, fn, base, f"layers[{k}]".encode(), b"misaligned", layers=tables(tuple(A + 2 if j == k else A for j in range(5)))[0])
        assert getattr(lib, fn)(None, tables()[1], *base[2:]) == -1 and b"layers is NULL" in lib.d4gs_last_error()
        assert getattr(lib, fn)(tables()[0], None, *base[2:]) == -1 and b"sizes is NULL" in lib.d4gs_last_error()


def test_bad_sizes_are_refused(lib):
    for fn, where in (("d4gs_lpips_prepare", {3: b"M=", 4: b"B=", 5: b"H=", 6: b"W="}), ("d4gs_lpips_layer", {3: b"n=", 4: b"C=", 5: b"h=", 6: b"w="}),
                      ("d4gs_lpips_score", {3: b"M=", 4: b"B=", 5: b"H=", 6: b"W="}), ("d4gs_lpips_mean", {2: b"n="})):
        for i, name in where.items():
            for v in (0, -1, -2 ** 31):
                bad(lib, fn, put(fn, i, v), b"bad size", name + str(v).encode())
    for fn in ("d4gs_lpips_prepare", "d4gs_lpips_score"):
        bad(lib, fn, put(fn, 5, 30), b"H=30", b">= 31")
        bad(lib, fn, put(fn, 6, 30), b"W=30", b">= 31")
        bad(lib, fn, put(fn, 2, None), b"masks == NULL", b"M must be 1")  # M = 3 without masks
    bad(lib, "d4gs_lpips_layer", put("d4gs_lpips_layer", 4, 4097), b"C=4097")
    assert call(lib, "d4gs_lpips_layer", put("d4gs_lpips_layer", 4, 4096)[:3] + [2 ** 20, 4096, 2 ** 10, 2 ** 10, A, None]) == -1
    assert b"overflows" in lib.d4gs_last_error() and b"n=1048576" in lib.d4gs_last_error()
    bad(lib, "d4gs_lpips_prepare", put("d4gs_lpips_prepare", 5, 2 ** 24)[:6] + [2 ** 24, 1, A, None], b"overflows", b"H=16777216")
    bad(lib, "d4gs_lpips_score", put("d4gs_lpips_score", 3, 65536), b"overflows", b"M=65536")
    for fn in ("d4gs_lpips_score", "d4gs_lpips_mean"):
        for k in range(10):
            sizes = list(SIZES)
            sizes[k] = 0
            bad(lib, fn, CALLS[fn][0], f"sizes[{k // 2}]".encode(), b"bad size", sizes=tables(sizes=sizes)[1])
    assert lib.d4gs_lpips_score_blocks(3, 2, 47, 64) == 3 * 2 * ((47 * 64 + 255) // 256)
    for args in ((0, 1, 47, 64), (1, 0, 47, 64), (1, 1, 30, 64), (1, 1, 64, 30), (65536, 1, 47, 64), (2 ** 15, 1, 2 ** 15, 2 ** 15)):
        assert lib.d4gs_lpips_score_blocks(*args) == 0, args


def test_every_public_call_refuses_a_cpu_tensor():
    from deblur4dgs_amd import lpips
    from deblur4dgs_amd.metrics import ValidationMetrics

    fx = R.load_fixture()
    net = lpips.LPIPS(R.seeded_trunk(), R.lins_state(fx))
    img, mask = torch.rand(1, 31, 33, 3), torch.ones(1, 31, 33)
    maps = [torch.rand(1, h, w) for h, w in lpips.alex_sizes(31, 33)]
    calls = (lambda: net.distance(img, img), lambda: net.score_map(img, img), lambda: net.masked_sums(img, img, mask), lambda: net(img, img),
             lambda: lpips.mLPIPS(net).update(img, img, mask), lambda: lpips.mLPIPS(net)(img, img), lambda: lpips.prepare(img, img, mask),
             lambda: lpips.layer_distance(torch.rand(1, 4, 3, 3), torch.rand(1, 4, 3, 3), torch.rand(4)), lambda: lpips.score(maps, 31, 33),
             lambda: lpips.mean_score(maps), lambda: ValidationMetrics(lpips=net).update(img, img, mask, mask))
    for f in calls:
        with pytest.raises(RuntimeError, match="ROCm"):  # no CPU fallback
            f()


def test_state_dicts_both_layouts_load_and_bad_keys_are_named():
    from deblur4dgs_amd import lpips

    fx = R.load_fixture()
    trunk, lins = R.seeded_trunk(), R.lins_state(fx)
    net = lpips.LPIPS(trunk, lins)
    state = net.state_dict()
    slices = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}
    own = {f"net.slice{slices[int(k.split('.')[1])]}.{k.split('.', 1)[1]}": v for k, v in trunk.items()}
    assert set(state) == set(own) | set(lins)  # the LPIPS layout, and nothing else
    assert all(torch.equal(state[k], v) for k, v in {**own, **lins}.items())
    assert not any(p.requires_grad for p in net.parameters()) and not net.training and not net.train().training
    again = lpips.LPIPS({k: v for k, v in state.items() if k.startswith("net.")}, {k: v for k, v in state.items() if k.startswith("lin")})
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in state.items())  # the round trip
    lpips.LPIPS({**trunk, "classifier.1.weight": torch.zeros(2, 2)}, lins)  # torchvision's whole model: the classifier is passed over
    for key in trunk:
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            lpips.LPIPS({k: v for k, v in trunk.items() if k != key}, lins)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            lpips.LPIPS({**trunk, key: trunk[key][..., :-1] if trunk[key].dim() > 1 else trunk[key][:-1]}, lins)
    for key in lins:
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            lpips.LPIPS(trunk, {k: v for k, v in lins.items() if k != key})
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            lpips.LPIPS(trunk, {**lins, key: lins[key][:, :-1]})
    for stray in ("features.1.weight", "features.12.bias", "net.slice1.3.weight", "net.slice6.0.weight", "scaling.shift"):
        with pytest.raises(ValueError, match=stray.replace(".", r"\.")):
            lpips.LPIPS({**trunk, stray: torch.zeros(1)}, lins)
    for stray in ("lin5.model.1.weight", "lin0.model.0.weight", "net.slice1.0.weight"):
        with pytest.raises(ValueError, match=stray.replace(".", r"\.")):
            lpips.LPIPS(trunk, {**lins, stray: torch.zeros(1, 64, 1, 1)})
    with pytest.raises(ValueError, match="given twice"):
        lpips.LPIPS({**trunk, "net.slice1.0.weight": trunk["features.0.weight"]}, lins)
    with pytest.raises(ValueError, match="path or a state dict"):
        lpips.LPIPS(3, lins)


def test_weight_files_load_from_paths(tmp_path):
    from deblur4dgs_amd import lpips

    fx = R.load_fixture()
    trunk, lins = R.seeded_trunk(), R.lins_state(fx)
    torch.save(trunk, tmp_path / "alexnet.pth"), torch.save(lins, tmp_path / "alex.pth")
    net = lpips.LPIPS(str(tmp_path / "alexnet.pth"), tmp_path / "alex.pth")
    assert torch.equal(net.state_dict()["net.slice3.6.weight"], trunk["features.6.weight"])
    assert torch.equal(net.state_dict()["lin2.model.1.weight"], lins["lin2.model.1.weight"])


def test_validation_metrics_without_lpips_are_unchanged_and_the_old_import_still_fails():
    from deblur4dgs_amd.metrics import ValidationMetrics

    keys = ("val/psnr", "val/ssim", "val/fg_psnr", "val/fg_ssim", "val/bg_psnr", "val/bg_ssim")
    assert ValidationMetrics().KEYS == keys and tuple(ValidationMetrics().compute()) == keys
    assert ValidationMetrics.LPIPS_KEYS == ("val/lpips", "val/fg_lpips", "val/bg_lpips")
    net = object()  # compute() before any update touches no network: nine keys, all nan
    out = ValidationMetrics(has_bg=False, lpips=net).compute()
    assert tuple(out) == keys + ValidationMetrics.LPIPS_KEYS and all(bool(torch.isnan(v)) for v in out.values())
    with pytest.raises(ImportError, match=r"AlexNet.*deblur4dgs_amd\.lpips\.mLPIPS"):
        from deblur4dgs_amd.metrics import mLPIPS  # noqa: F401
