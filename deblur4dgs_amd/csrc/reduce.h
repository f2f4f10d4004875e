// reduce.h -- the one fixed-order sum of the loss and metric kernels (photometric, metrics, warp, trimmed, motion_regs, sh, lpips): device
// code only, and nothing on the frame's hot path includes it.  Every float sum that these kernels promise bit for
// bit, on every run and graph replay, is associated in this order and no other (tests/test_gpu_ordered_sum.py restates it in NumPy
// from this comment and compares the bits):
//
//   Block sum -- 256 threads = 4 waves of 64 lanes, thread 64 w + l is lane l of wave w; each holds R running sums of type T (float
//   or double), and every one of the R is summed on its own, in T:
//     1. butterfly inside each wave, o = 32, 16, 8, 4, 2, 1 in that order: every lane replaces its a[l] by a[l] + a[l ^ o].  After
//        the six steps every lane of wave w holds the wave's sum s_w (block_sum_store, which leaves s_w in LDS);
//     2. behind ONE __syncthreads() of the caller the block's sum is (s_0 + s_1) + (s_2 + s_3) (block_sum_combine).  A kernel that
//        sums two types (k_photo_fwd: a double and a float) stores both before that one barrier.
//
//   Ordered total -- one block of 256 threads adds n partials of type Tin (float or double) into R sums; partial i of sum k is
//   p[i * stride + k]:
//     1. thread t starts from 0.0 (double) and adds the partials i = t, t + 256, t + 512, ... < n in increasing i, each converted
//        to double before it is added;
//     2. halving tree over the 256 thread sums, o = 128, 64, ..., 2, 1 in that order: r[t] = r[t] + r[t + o] for every t < o, all
//        from the values of before the step.  r[0] is the total; every thread gets it.
#pragma once
#include "common.h"

constexpr int REDUCE_NT = 256;
static_assert(REDUCE_NT == 4 * D4GS_WAVE, "the block sum is written for four waves");

template <int R, class T>
__device__ __forceinline__ void block_sum_store(T (&v)[R], T *red) {  // red: 4 R values of T in LDS; all 256 threads call
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < R; k++) v[k] += __shfl_xor(v[k], o);
  if ((threadIdx.x & (D4GS_WAVE - 1)) == 0)
#pragma unroll
    for (int k = 0; k < R; k++) red[(threadIdx.x / D4GS_WAVE) * R + k] = v[k];
}
template <int R, class T>
__device__ __forceinline__ T block_sum_combine(const T *red, int k) {  // the block's sum of value k
  return (red[k] + red[R + k]) + (red[2 * R + k] + red[3 * R + k]);
}

template <int R, class Tin>
__device__ __forceinline__ void ordered_total(const Tin *__restrict__ p, int64_t n, int64_t stride, double (&total)[R]) {
  __shared__ double r[R][REDUCE_NT];
  const int t = threadIdx.x;
  double a[R] = {};
  for (int64_t i = t; i < n; i += REDUCE_NT)
#pragma unroll
    for (int k = 0; k < R; k++) a[k] += (double)p[i * stride + k];
#pragma unroll
  for (int k = 0; k < R; k++) r[k][t] = a[k];
  __syncthreads();
  for (int o = REDUCE_NT / 2; o > 0; o >>= 1) {
    if (t < o)
#pragma unroll
      for (int k = 0; k < R; k++) r[k][t] += r[k][t + o];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < R; k++) total[k] = r[k][0];
  __syncthreads();  // r is written again (the next call, the next turn of a caller's loop) only after every thread has read it
}

// Zeroes n floats.  Scatter targets are zeroed by this kernel and not by hipMemsetAsync: a memset node did not take effect when a
// captured graph was replayed (tests/test_gpu_pwc.py::test_graph_capture_and_replay saw the scatter land on uninitialised memory).
// A template so that only the translation units that launch it (k_zero_f32<>) emit it, and static like their own kernels.
template <int NT = REDUCE_NT>
static __global__ void __launch_bounds__(NT) k_zero_f32(float *__restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) p[i] = 0.f;
}
