"""deblur4dgs_amd/_lib.py derives the ctypes binding from include/d4gs.h.  Three checks, none needs a GPU:
the compiler's reading of the header agrees with the parser's (sizes, offsets, field widths of all 16 structs), the parser refuses
what it does not understand instead of skipping it, and the [host] / [device] marks give exactly the pointer kinds they stand for."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import pytest

from deblur4dgs_amd import _lib as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "d4gs.h")


# ---- the compiler probe ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compiled_layouts():
    """{"Dims": size, "Dims.N": (offset, size), ...} as the compiler lays the header's structs out: a host-only C++ program, written
    from the parsed struct and field names, compiled with the compiler of deblur4dgs_amd/build.py and run."""
    c_names = {py: c for c, py in L.STRUCT_NAMES.items()}
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{HEADER}"', "int main() {"]
    for py, cls in L.STRUCTS.items():
        lines.append(f'  printf("{py} %zu\\n", sizeof({c_names[py]}));')
        for name, _ in cls._fields_:
            lines.append(f'  printf("{py}.{name} %zu %zu\\n", offsetof({c_names[py]}, {name}), sizeof((({c_names[py]} *)0)->{name}));')
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.cpp"), os.path.join(d, "probe")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.run(["hipcc", "-x", "c++", "-std=c++17", "-Wall", "-Werror", src, "-o", exe], check=True, capture_output=True, text=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = {}
    for ln in out.splitlines():
        key, *numbers = ln.split()
        table[key] = int(numbers[0]) if len(numbers) == 1 else tuple(int(x) for x in numbers)
    return table


def check_struct_layouts():
    table = compiled_layouts()
    assert len(L.STRUCTS) == len(L.STRUCT_NAMES) == 16
    derived = {}
    for py, cls in L.STRUCTS.items():
        derived[py] = C.sizeof(cls)
        for name, _ in cls._fields_:
            derived[f"{py}.{name}"] = (getattr(cls, name).offset, getattr(cls, name).size)
    assert derived == table, sorted(k for k in set(derived) | set(table) if derived.get(k) != table.get(k))


def test_struct_layouts_match_the_compiler():
    check_struct_layouts()


# ---- strict parsing ----------------------------------------------------------------------------------------------------------
def _damaged(old, new):
    text = open(HEADER).read()
    assert text.count(old) == 1, old
    return text.replace(old, new)


def test_the_header_parses_and_every_declaration_is_counted():
    constants, structs, prototypes = L.parse(open(HEADER).read())
    assert tuple(prototypes) == L.EXPORTS and len(prototypes) == 79 and list(structs) == list(L.STRUCTS)
    assert constants["VERSION"] == L.VERSION == 305 and (L.TILE, L.GEOM_STRIDE, L.ADAM_CHUNK) == (16, 8, 2048)
    assert (L.RAW_PARAMS, L.RAW_COLORS, L.EXACT_CULL, L.LAZY_SORT, L.EXACT_TILES, L.ABSGRAD, L.ANTIALIASED) == (1, 2, 4, 8, 16, 32, 64)
    assert (L.DEPTH_NONE, L.DEPTH_ED, L.DEPTH_D) == (0, 1, 2) and (L.ROWS_AUTO, L.ROWS_DENSE, L.ROWS_SPARSE) == (0, 1, 2)


@pytest.mark.parametrize("old,new,word", [
    # an unknown type, in a struct and in a prototype
    ("  int32_t G;  ", "  int33_t G;  ", "int33_t"),
    ("D4GS_API size_t d4gs_scan_ws_elems(int64_t n_instances);", "D4GS_API size_t d4gs_scan_ws_elems(long n_instances);", "long n_instances"),
    ("D4GS_API int64_t d4gs_adam_blocks(int64_t n);", "D4GS_API unsigned d4gs_adam_blocks(int64_t n);", "d4gs_adam_blocks"),
    # a missing semicolon inside a struct
    ("  int32_t g_major;\n", "  int32_t g_major\n", "D4gsPoses"),
    ("  float *quats;       /* [S,N,4]", "  float *quats        /* [S,N,4]", "quats"),
    # prototypes the pattern would miss: valid C in another shape, and two fused by a lost semicolon
    ("D4GS_API int d4gs_version(void);", "D4GS_API int (d4gs_version)(void);", "78 of 79 prototypes"),
    ("D4GS_API int d4gs_version(void);", "D4GS_API int d4gs_version(void)", "78 of 79 prototypes"),
    ("D4GS_API void d4gs_profile_enable(int on);", "D4GS_API void d4gs_profile_enable(int on, void (*done)(int));", "d4gs_profile_enable"),
    # a struct the name map does not know, and a mark where no declaration owns it
    ("} D4gsPoses;", "} D4gsPose;", "STRUCT_NAMES"),
    ("D4GS_API const char *d4gs_last_error(void);", "D4GS_API const char *d4gs_last_error(void); /* [host] */", "@host"),
])
def test_a_damaged_header_raises_at_import(old, new, word):
    with pytest.raises(ValueError) as e:
        L.parse(_damaged(old, new))
    assert word in str(e.value), str(e.value)


# ---- marks -------------------------------------------------------------------------------------------------------------------
def test_marks_give_exactly_the_documented_pointer_kinds():
    vp, P = C.c_void_p, C.POINTER
    sig = {name: argtypes for name, (_, argtypes) in L.PROTOTYPES.items()}
    # [host] scalars: the blend policy wherever it appears, and the peaks' result
    assert dict(L.FrameIO._fields_)["policy"] is P(C.c_int32) and dict(L.ShardBlend._fields_)["policy"] is P(C.c_int32)
    assert sig["d4gs_blend_fwd"][3] is P(C.c_int32) and sig["d4gs_blend_bwd"][3] is P(C.c_int32)
    assert sig["d4gs_measure_peaks"] == [vp, C.c_size_t, P(C.c_double), vp]
    # the Adam table: [device] on the launches, a host descriptor array for the CPU twin; grads is a host array of pointers
    assert sig["d4gs_adam_step"] == [vp, C.c_int32, vp, C.c_int32, vp, vp]
    assert sig["d4gs_adam_set_grads"] == [vp, C.c_int32, P(vp), vp]
    assert sig["d4gs_adam_step_cpu"] == [P(L.AdamRec), C.c_int32]
    # char * is a host string
    assert L.PROTOTYPES["d4gs_profile_enable"] == (None, [C.c_int])
    assert L.PROTOTYPES["d4gs_profile_collect"] == (C.c_int, [C.c_char_p, C.c_size_t])
    assert L.PROTOTYPES["d4gs_last_error"] == (C.c_char_p, None)
    # and nothing else: every other pointer is a device pointer (c_void_p) or a descriptor passed by host pointer
    descriptors = {P(cls) for cls in L.STRUCTS.values()}
    typed = {(name, i) for name, a in sig.items() for i, t in enumerate(a or ()) if t not in descriptors and hasattr(t, "contents")}
    assert typed == {("d4gs_blend_fwd", 3), ("d4gs_blend_bwd", 3), ("d4gs_measure_peaks", 2), ("d4gs_adam_set_grads", 2)}
    typed = {(py, f) for py, cls in L.STRUCTS.items() for f, t in cls._fields_ if hasattr(t, "contents")}
    assert typed == {("FrameIO", "policy"), ("ShardBlend", "policy")}
    arrays = {(py, f): t._length_ for py, cls in L.STRUCTS.items() for f, t in cls._fields_ if hasattr(t, "_length_")}
    assert arrays == {("MoveModelParams", "w"): 9, ("MoveModelParams", "b"): 9, ("MoveModelGrads", "v_w"): 9, ("MoveModelGrads", "v_b"): 9}


def test_bind_applies_the_signatures_to_any_handle():
    from deblur4dgs_amd import build

    raw = L.bind(C.CDLL(build.build()))
    for name, (restype, argtypes) in L.PROTOTYPES.items():
        fn = getattr(raw, name)
        assert fn.restype is restype and (fn.argtypes is None if argtypes is None else list(fn.argtypes) == argtypes), name
