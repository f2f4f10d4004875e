"""The fixed-order sum of the loss and metric kernels (csrc/reduce.h), checked bit for bit against a NumPy restatement of the order
that the header's opening comment states.  The "two runs are bitwise equal" tests of the losses rest on that order; their value
tests (1e-5-class tolerances) would not notice a reordered tree.  Two hooks of the A/B build only (tests/libd4gs_variants.so) run
the block sum and the ordered total, one block each.

Inputs are randn * 10 ** uniform(-6, 6): twelve decades of magnitude, so that a different association shows in the bits
(test_the_inputs_tell_the_order_from_a_sequential_sum holds the inputs to that)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NT = 256
DTYPES = {"float": np.float32, "double": np.float64}


@pytest.fixture(scope="module")
def lib():
    from deblur4dgs_amd import build

    assert os.path.exists(build.VARIANTS_LIB), "run __graft_entry__.build() (builds tests/libd4gs_variants.so)"
    lib = C.CDLL(build.VARIANTS_LIB)
    lib.d4gs_test_block_sum.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.d4gs_test_block_sum.restype = C.c_int
    lib.d4gs_test_ordered_total.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.d4gs_test_ordered_total.restype = C.c_int
    return lib


def wide_range(rng, shape, dtype):
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 6, shape)).astype(dtype)


# ---- the order, restated from the comment at the head of csrc/reduce.h ----

def ordered_total(partials):
    """partials [n,R] of float or double -> [R] doubles.  Thread t starts from 0.0 and adds partials t, t + 256, ... in increasing index,
    each converted to double first; then the halving tree o = 128 ... 1, r[t] += r[t + o] for t < o."""
    n, R = partials.shape
    a = np.zeros((NT, R), np.float64)
    for start in range(0, n, NT):
        chunk = partials[start:start + NT].astype(np.float64)
        a[:len(chunk)] += chunk
    o = NT // 2
    while o:
        a[:o] += a[o:2 * o]
        o //= 2
    return a[0]


def block_sum(x):
    """x [256,R] of T -> [R] of T.  Per wave of 64 lanes the butterfly a = a + a[lane ^ o], o = 32 ... 1; then (s0 + s1) + (s2 + s3)."""
    idx = np.arange(64)
    s = []
    for w in range(4):
        a = x[64 * w:64 * w + 64].copy()
        for o in (32, 16, 8, 4, 2, 1):
            a = a + a[idx ^ o]
        s.append(a[0])
    out = (s[0] + s[1]) + (s[2] + s[3])
    assert out.dtype == x.dtype
    return out


def sequential(partials):
    a = np.zeros(partials.shape[1], np.float64)
    for row in partials.astype(np.float64):
        a = a + row
    return a


# ---- the device side ----

def gpu_ordered_total(lib, buf, n, R, stride):
    dev = torch.device("cuda:0")
    x = torch.from_numpy(buf).to(dev)
    out = torch.full((R,), float("nan"), device=dev, dtype=torch.float64)
    rc = lib.d4gs_test_ordered_total(R, int(buf.dtype == np.float64), x.data_ptr(), n, stride, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu()


def gpu_block_sum(lib, x):
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(x).to(dev).contiguous()
    out = torch.full((x.shape[1],), float("nan"), device=dev, dtype=xd.dtype)
    rc = lib.d4gs_test_block_sum(x.shape[1], int(x.dtype == np.float64), xd.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("pad", [0, 1])  # element stride R and R + 1
@pytest.mark.parametrize("R", [1, 2, 3, 5])
@pytest.mark.parametrize("tin", ["float", "double"])
def test_ordered_total_has_the_stated_bits(lib, tin, R, pad):
    stride = R + pad
    for n in (1, 2, 255, 256, 257, 511, 513, 1000):
        rng = np.random.default_rng([n, R, pad, tin == "double"])
        buf = wide_range(rng, (n, stride), DTYPES[tin])  # with pad: a column between the partials that no sum may touch
        want = torch.from_numpy(ordered_total(buf[:, :R]))
        got = gpu_ordered_total(lib, buf.reshape(-1), n, R, stride)
        assert torch.equal(got, want), (tin, R, stride, n, got, want)


@pytest.mark.parametrize("tin", ["float", "double"])
def test_the_inputs_tell_the_order_from_a_sequential_sum(lib, tin):
    n, R = 513, 3
    rng = np.random.default_rng([n, R, 0, tin == "double"])  # the inputs of the case above
    buf = wide_range(rng, (n, R), DTYPES[tin])
    want = ordered_total(buf)
    assert (sequential(buf) != want).any(), "these inputs would not show a sum taken in another order"
    assert torch.equal(gpu_ordered_total(lib, buf.reshape(-1), n, R, R), torch.from_numpy(want))


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("t", ["float", "double"])
def test_block_sum_has_the_stated_bits(lib, t, R):
    rng = np.random.default_rng([R, t == "double"])
    for trial in range(3):
        x = wide_range(rng, (NT, R), DTYPES[t])
        want = torch.from_numpy(block_sum(x))
        got = gpu_block_sum(lib, x)
        assert torch.equal(got, want), (t, R, trial, got, want)


@pytest.mark.parametrize("t", ["float", "double"])
def test_block_sum_keeps_every_wave(lib, t):
    """one non-zero, in lane 0 of wave 3: a dropped wave cannot hide behind rounding"""
    for R in (1, 2, 3):
        x = np.zeros((NT, R), DTYPES[t])
        x[3 * 64] = np.arange(1, R + 1) * 0.3
        got = gpu_block_sum(lib, x)
        assert torch.equal(got, torch.from_numpy(x[3 * 64])), (t, R, got)
        assert torch.equal(got, torch.from_numpy(block_sum(x)))
