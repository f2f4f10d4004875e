"""ctypes binding of libd4gs.so, derived at import from include/d4gs.h: the header is the one statement of the C ABI.

Appending an entry point, a struct or a constant means editing the header and nothing here (a new struct: one line of
STRUCT_NAMES).  The type rules and the [host] / [device] marks are in `_ctype`; DESIGN.md section 23 has them as a table.
Prototypes under D4GS_API are PROTOTYPES / EXPORTS; the scene-initialisation block under D4GS_INIT_API is INIT_PROTOTYPES, the
evaluation-time block (test-time pose refinement) under D4GS_EVAL_API is EVAL_PROTOTYPES, the data-preparation block (observations
from raw arrays) under D4GS_DATA_API is DATA_PROTOTYPES, the warm-up block (the track fit) under D4GS_FIT_API is FIT_PROTOTYPES, the
per-step block (batch assembly from a device-resident clip) under D4GS_FEED_API is FEED_PROTOTYPES, the LPIPS block (the metric's
passes around its convolutions) under D4GS_LPIPS_API is LPIPS_PROTOTYPES.

The product path has NO fallback: if the HIP library is missing this module raises at first use, and every
entry point raises RuntimeError on a non-zero return code with `d4gs_last_error()`.
"""
from __future__ import annotations

import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("D4GS_LIB_PATH") or os.path.join(HERE, "libd4gs.so")  # override: A/B builds (scripts/)
HEADER = os.path.join(HERE, "..", "include", "d4gs.h")

F = C.c_void_p  # device pointers travel as void*

# C name -> the name the package uses
STRUCT_NAMES = {
    "D4gsDims": "Dims", "D4gsProjIn": "ProjIn", "D4gsProjOut": "ProjOut", "D4gsIsect": "Isect", "D4gsRaster": "Raster",
    "D4gsRasterGrads": "RasterGrads", "D4gsLeafGrads": "LeafGrads", "D4gsSizes": "Sizes", "D4gsPoses": "Poses",
    "D4gsMoveModelParams": "MoveModelParams", "D4gsMoveModelOut": "MoveModelOut", "D4gsMoveModelGrads": "MoveModelGrads",
    "D4gsFrameIO": "FrameIO", "D4gsFrameGrads": "FrameGrads", "D4gsShardBlend": "ShardBlend", "D4gsAdamRec": "AdamRec",
}
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "int8_t": C.c_int8,
            "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_STARS = r"((?:\*\s*(?:const\b\s*)?)*)"  # `*`, `* const *`, ...: only the count matters
_PARAM = re.compile(rf"(?:const\s+)?(\w+)\b\s*{_STARS}\b(\w+)\s*(?:@(host|device))?")
_DECLARATOR = re.compile(rf"{_STARS}\b(\w+)\s*(?:\[(\d+)\])?")
_FIELD = r"\s*([^;@{}]+?)\s*;((?:\s*@\w+)*)"  # one declaration (one or more declarators) and the marks of its inline comment


def _ctype(base, stars, mark, structs, text):
    """The ctypes type of one parameter or field: `base` with `stars` levels of pointer and the declaration's mark."""
    n = stars.count("*")
    if base in structs:  # a descriptor travels by host pointer, unless it is marked as a table in device memory
        if n == 1:
            return C.c_void_p if mark == "device" else C.POINTER(structs[base])
    elif n == 0 and base in _SCALARS:
        return _SCALARS[base]
    elif n == 1 and base == "char":
        return C.c_char_p
    elif n == 1 and (base == "void" or base in _SCALARS):  # a device pointer, unless marked [host]
        return C.POINTER(_SCALARS[base]) if mark == "host" and base != "void" else C.c_void_p
    elif n == 2 and (base == "void" or base in _SCALARS):  # a host array of pointers
        return C.POINTER(C.c_void_p)
    raise ValueError(f"d4gs.h: cannot bind the type of `{text}`")


def parse(text, init=None, *, eval=None, data=None, fit=None, feed=None, lpips=None):
    """-> (constants, structs, prototypes) of the header `text`: {name without D4GS_: int}, {Python name: ctypes.Structure},
    {entry point: (restype, argtypes)}.  Strict: whatever is left of the header once every enum, struct and prototype has been
    taken out, and every declaration that does not parse completely, raises ValueError with the offending text.
    `prototypes` is the D4GS_API table.  The declarations under D4GS_INIT_API (scene initialisation) are read
    by the same rules, counted in the same way, and land in the dict `init` when one is given; so do those under D4GS_EVAL_API
    (test-time pose refinement) and the dict `eval`, and those under D4GS_DATA_API (observations from raw
    arrays) and the dict `data`, and those under D4GS_FIT_API (the track fit) and the dict
    `fit`, and those under D4GS_FEED_API (batch assembly) and the dict `feed`, and those under D4GS_LPIPS_API
    (the LPIPS passes) and the dict `lpips`."""
    def comment(m):  # an inline comment (code before it on its line) leaves its mark as a token; every other comment is blank
        inline = text[text.rfind("\n", 0, m.start()) + 1:m.start()].strip()
        found = re.search(r"\[(host|device)\]", m.group()) if inline else None
        return f" @{found.group(1)} " if found else " "

    code = re.sub(r"/\*.*?\*/", comment, text, flags=re.S)
    constants = {k: int(v) for k, v in re.findall(r"^#define D4GS_(\w+)[ \t]+(-?\d+)[ \t]*$", code, flags=re.M)}
    n_api, n_structs = len(re.findall(r"\bD4GS_API\b", code)) - 1, len(re.findall(r"\btypedef\s+struct\b", code))
    n_init = max(len(re.findall(r"\bD4GS_INIT_API\b", code)) - 1, 0)  # (a header without the block: none)
    n_eval = max(len(re.findall(r"\bD4GS_EVAL_API\b", code)) - 1, 0)
    n_data = max(len(re.findall(r"\bD4GS_DATA_API\b", code)) - 1, 0)
    n_fit = max(len(re.findall(r"\bD4GS_FIT_API\b", code)) - 1, 0)
    n_feed = max(len(re.findall(r"\bD4GS_FEED_API\b", code)) - 1, 0)
    n_lpips = max(len(re.findall(r"\bD4GS_LPIPS_API\b", code)) - 1, 0)
    code = re.sub(r"^[ \t]*#.*$", "", code, flags=re.M)
    structs, by_c_name, prototypes, init, eval = {}, {}, {}, {} if init is None else init, {} if eval is None else eval
    data, fit, feed = {} if data is None else data, {} if fit is None else fit, {} if feed is None else feed
    lpips = {} if lpips is None else lpips

    def enum(m):
        for item in filter(None, (x.strip() for x in m.group(1).split(","))):
            e = re.fullmatch(r"D4GS_(\w+)\s*=\s*(-?\d+)", item)
            if not e:
                raise ValueError(f"d4gs.h: cannot parse the enumerator `{item}`")
            constants[e.group(1)] = int(e.group(2))
        return ""

    def struct(m):
        body, name = m.groups()
        if name not in STRUCT_NAMES or not re.fullmatch(f"(?:{_FIELD})*\\s*", body):
            raise ValueError(f"d4gs.h: cannot parse struct {name} (or it has no entry in STRUCT_NAMES): `{body.strip()}`")
        fields = []
        for decl, marks in re.findall(_FIELD, body):
            d = re.fullmatch(r"(?:const\s+)?(\w+)\b\s*(.*)", decl, flags=re.S)
            for one in d.group(2).split(",") if d else [""]:
                f = _DECLARATOR.fullmatch(one.strip())
                if not f:
                    raise ValueError(f"d4gs.h: cannot parse the field `{decl}` of {name}")
                t = _ctype(d.group(1), f.group(1), marks.strip()[1:] or None, by_c_name, decl)
                fields.append((f.group(2), t * int(f.group(3)) if f.group(3) else t))
        by_c_name[name] = structs[STRUCT_NAMES[name]] = type(STRUCT_NAMES[name], (C.Structure,), {"_fields_": fields})
        return ""

    def prototype(m, table=prototypes):
        ret, name, params = (x.strip() for x in m.groups())
        restype = C.c_char_p if re.fullmatch(r"const\s+char\s*\*", ret) else None if ret == "void" else _SCALARS.get(ret)
        if restype is None and ret != "void":
            raise ValueError(f"d4gs.h: cannot bind the return type of `{m.group().strip()}`")
        argtypes = None  # f(void): ctypes' default, as for a function that was never given argtypes
        if params != "void":
            found = [_PARAM.fullmatch(p.strip()) for p in params.split(",")]
            if not all(found):
                raise ValueError(f"d4gs.h: cannot parse a parameter of `{m.group().strip()}`")
            argtypes = [_ctype(p.group(1), p.group(2), p.group(4), by_c_name, p.group()) for p in found]
        table[name] = (restype, argtypes)
        return ""

    code = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, code)
    code = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, code)
    code = re.sub(r"\bD4GS_API\b([^;()]*?)\b(\w+)\s*\(([^;()]*)\)\s*;", prototype, code)
    code = re.sub(r"\bD4GS_INIT_API\b([^;()]*?)\b(\w+)\s*\(([^;()]*)\)\s*;", lambda m: prototype(m, init), code)
    code = re.sub(r"\bD4GS_EVAL_API\b([^;()]*?)\b(\w+)\s*\(([^;()]*)\)\s*;", lambda m: prototype(m, eval), code)
    code = re.sub(r"\bD4GS_DATA_API\b([^;()]*?)\b(\w+)\s*\(([^;()]*)\)\s*;", lambda m: prototype(m, data), code)
    code = re.sub(r"\bD4GS_FIT_API\b([^;()]*?)\b(\w+)\s*\(([^;()]*)\)\s*;", lambda m: prototype(m, fit), code)
    code = re.sub(r"\bD4GS_FEED_API\b([^;()]*?)\b(\w+)\s*\(([^;()]*)\)\s*;", lambda m: prototype(m, feed), code)
    code = re.sub(r"\bD4GS_LPIPS_API\b([^;()]*?)\b(\w+)\s*\(([^;()]*)\)\s*;", lambda m: prototype(m, lpips), code)
    for block, table, n in (("INIT", init, n_init), ("EVAL", eval, n_eval), ("DATA", data, n_data), ("FIT", fit, n_fit),
                            ("FEED", feed, n_feed), ("LPIPS", lpips, n_lpips)):
        if len(table) != n:
            raise ValueError(f"d4gs.h: {len(table)} of {n} D4GS_{block}_API prototypes parsed; not understood: `{' '.join(code.split())}`")
    if code.split() != ["extern", '"C"', "{", "}"] or len(prototypes) != n_api or len(structs) != n_structs:
        raise ValueError(f"d4gs.h: {len(prototypes)} of {n_api} prototypes and {len(structs)} of {n_structs} structs parsed; "
                         f"not understood: `{' '.join(code.split())}`")
    return constants, structs, prototypes


INIT_PROTOTYPES = {}  # the D4GS_INIT_API block: scene_init.py's entry points, bound like the rest
EVAL_PROTOTYPES = {}  # the D4GS_EVAL_API block: pose_refine.py's
DATA_PROTOTYPES = {}  # the D4GS_DATA_API block: observations.py's
FIT_PROTOTYPES = {}   # the D4GS_FIT_API block: the track fit of losses.py / scene_init.py
FEED_PROTOTYPES = {}  # the D4GS_FEED_API block: feed.py's
LPIPS_PROTOTYPES = {}  # the D4GS_LPIPS_API block: lpips.py's
with open(HEADER) as _f:
    CONSTANTS, STRUCTS, PROTOTYPES = parse(_f.read(), INIT_PROTOTYPES, eval=EVAL_PROTOTYPES, data=DATA_PROTOTYPES, fit=FIT_PROTOTYPES,
                                           feed=FEED_PROTOTYPES, lpips=LPIPS_PROTOTYPES)
# the package's names: VERSION, TILE, GEOM_STRIDE, ADAM_CHUNK, RAW_PARAMS ... ANTIALIASED, DEPTH_*, ROWS_*; Dims ... AdamRec
globals().update(CONSTANTS)
globals().update(STRUCTS)
EXPORTS = tuple(PROTOTYPES)

# Appended to ABI 305 after A/B libraries of older trees were built.  The product library must have them (as every export; build()
# checks it too); a library named by D4GS_LIB_PATH is held only to the entry points its run calls, so a raster A/B library
# that predates one of these still loads, and calling the missing entry point through it raises.
APPENDED = ("d4gs_photometric_maps_elems",)

_lib = None


def bind(cdll: C.CDLL) -> C.CDLL:
    """Give every entry point of the header its restype and argtypes on a loaded library."""
    later = {**INIT_PROTOTYPES, **EVAL_PROTOTYPES, **DATA_PROTOTYPES, **FIT_PROTOTYPES, **FEED_PROTOTYPES, **LPIPS_PROTOTYPES}
    for name, (restype, argtypes) in {**PROTOTYPES, **later}.items():
        if (name in APPENDED or name in later) and os.environ.get("D4GS_LIB_PATH") and not hasattr(cdll, name):
            continue
        fn = getattr(cdll, name)  # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = restype, argtypes
    return cdll


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
                "Build it with `python -m deblur4dgs_amd.build` (hipcc, --offload-arch=gfx950)."
            )
        import torch  # noqa: F401  -- torch's bundled HIP runtime must be the one both sides use: load it first
        L = bind(C.CDLL(LIB_PATH))
        if L.d4gs_version() != CONSTANTS["VERSION"]:
            raise RuntimeError(f"libd4gs.so version {L.d4gs_version()} != {CONSTANTS['VERSION']} (stale build?)")
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().d4gs_last_error().decode()}")


def ptr(t):
    """Device pointer of a contiguous tensor (or NULL for None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "d4gs expects contiguous tensors"
    return t.data_ptr()


def vp(t):
    """The same as a c_void_p, without the contiguity check (callers that made the tensor themselves)."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def f32c(t):
    """Detached, fp32, contiguous (None stays None): what an entry point reads."""
    return None if t is None else t.detach().float().contiguous()


def need_gpu(t, who: str, note: str = ""):
    """The refusal of a CPU tensor, in `who`'s name."""
    if not t.is_cuda:
        raise RuntimeError(f"{who} runs on an MI355X (ROCm) device only; got a CPU tensor{note}")


def fill(struct, **tensors):
    for k, v in tensors.items():
        setattr(struct, k, ptr(v))
    return struct


_RAW_STREAM = None


def raw_stream(index=None) -> int:
    """The current HIP stream of device `index` (default: the current device) as an integer handle.  One C call:
    torch.cuda.current_stream() builds a Python Stream object every time (~12 us, six times per rendered frame)."""
    global _RAW_STREAM
    import torch

    if _RAW_STREAM is None:
        _RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    if index is None:
        index = torch.cuda.current_device()
    if _RAW_STREAM:
        return _RAW_STREAM(index)
    return torch.cuda.current_stream(index).cuda_stream


def stream_of(t):
    """The current stream of tensor `t`'s device, as an entry point takes it."""
    return C.c_void_p(raw_stream(t.device.index))
