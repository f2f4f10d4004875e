// adam.hip -- multi-tensor Adam: one launch over a device-resident table of tensors (include/d4gs.h, "Multi-tensor Adam"), and
// its CPU twin.  Memory bound: 16 B read + 12 B written per element, ~20 fp32 operations.
//
// Mapping.  Workgroup b finds its record r by a binary search of block_prefix (wave-uniform: scalar loads, <= log2(records)
// steps) and serves chunk b - block_prefix[r], D4GS_ADAM_CHUNK = 2048 elements: 256 threads x 2 x float4 per array, all eight
// 16-byte loads of a thread issued before the first use.  A 4-element tensor costs one workgroup that retires after one load
// round; a 4 M-element tensor is 2048 workgroups, one residency round of the chip - the same code, no per-tensor launch.
// The bias corrections want beta^t: an fp64 square-and-multiply on the integer step (<= 24 rounds, once per thread, while the
// loads are in flight), so the CPU twin gets the same bits without trusting two libm pow() to agree.
#include "adam_math.h"  // AdamCoef, adam_coef, adam_update: the per-element update, shared with pose_refine.hip
#include "common.h"

namespace {

constexpr int ADAM_BLOCK = 256;
constexpr int ADAM_VEC_ITERS = D4GS_ADAM_CHUNK / (4 * ADAM_BLOCK);
constexpr int ADAM_DWORD_ITERS = D4GS_ADAM_CHUNK / ADAM_BLOCK;
constexpr int ADAM_PATCH = 64;  // gradient pointers per k_adam_set_grads launch (512 B of kernel arguments)
static_assert(D4GS_ADAM_CHUNK % (4 * ADAM_BLOCK) == 0, "a chunk is a whole number of float4 rounds of the block");

__device__ __forceinline__ void adam_update4(float4 &p, float4 &m, float4 &v, const float4 g, const AdamCoef &c) {
  adam_update(p.x, m.x, v.x, g.x, c);
  adam_update(p.y, m.y, v.y, g.y, c);
  adam_update(p.z, m.z, v.z, g.z, c);
  adam_update(p.w, m.w, v.w, g.w, c);
}

__global__ void __launch_bounds__(ADAM_BLOCK) k_adam(const D4gsAdamRec *__restrict__ table, int n_records,
                                                     const int32_t *__restrict__ block_prefix, float *__restrict__ block_steps) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int lo = 0, hi = n_records;  // the last r with block_prefix[r] <= b
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (block_prefix[mid] <= b) lo = mid;
    else hi = mid;
  }
  const D4gsAdamRec r = table[lo];
  if (!r.grad) return;  // no gradient: nothing written, the step does not advance
  const int64_t start = (int64_t)(b - block_prefix[lo]) * D4GS_ADAM_CHUNK;
  if (start > 0 && start >= r.n) return;  // (chunk 0 of an empty record still counts the step)
  const int64_t end = start + D4GS_ADAM_CHUNK < r.n ? start + D4GS_ADAM_CHUNK : r.n;
  const float t = block_steps[b] + 1.0f;
  const bool vec = (((uintptr_t)r.param | (uintptr_t)r.grad | (uintptr_t)r.exp_avg | (uintptr_t)r.exp_avg_sq) & 15) == 0;
  if (vec) {
    const int64_t q0 = start / 4 + tid, q1 = end / 4;  // whole quads of this chunk; start % 4 == 0
    float4 *p4 = reinterpret_cast<float4 *>(r.param), *m4 = reinterpret_cast<float4 *>(r.exp_avg),
           *v4 = reinterpret_cast<float4 *>(r.exp_avg_sq);
    const float4 *g4 = reinterpret_cast<const float4 *>(r.grad);
    float4 p[ADAM_VEC_ITERS], g[ADAM_VEC_ITERS], m[ADAM_VEC_ITERS], v[ADAM_VEC_ITERS];
#pragma unroll
    for (int k = 0; k < ADAM_VEC_ITERS; k++) {
      const int64_t q = q0 + k * ADAM_BLOCK;
      if (q < q1) p[k] = p4[q], g[k] = g4[q], m[k] = m4[q], v[k] = v4[q];
    }
    const AdamCoef c = adam_coef(r.lr, r.beta1, r.beta2, r.eps, t);
#pragma unroll
    for (int k = 0; k < ADAM_VEC_ITERS; k++) {
      const int64_t q = q0 + k * ADAM_BLOCK;
      if (q < q1) {
        adam_update4(p[k], m[k], v[k], g[k], c);
        p4[q] = p[k], m4[q] = m[k], v4[q] = v[k];
      }
    }
    const int64_t i = 4 * q1 + tid;  // the n % 4 tail, in the record's last chunk only
    if (i < end) {
      float pi = r.param[i], mi = r.exp_avg[i], vi = r.exp_avg_sq[i];
      adam_update(pi, mi, vi, r.grad[i], c);
      r.param[i] = pi, r.exp_avg[i] = mi, r.exp_avg_sq[i] = vi;
    }
  } else {
    const AdamCoef c = adam_coef(r.lr, r.beta1, r.beta2, r.eps, t);
#pragma unroll 4
    for (int k = 0; k < ADAM_DWORD_ITERS; k++) {
      const int64_t i = start + tid + k * ADAM_BLOCK;
      if (i < end) {
        float pi = r.param[i], mi = r.exp_avg[i], vi = r.exp_avg_sq[i];
        adam_update(pi, mi, vi, r.grad[i], c);
        r.param[i] = pi, r.exp_avg[i] = mi, r.exp_avg_sq[i] = vi;
      }
    }
  }
  if (tid == 0) {
    block_steps[b] = t;
    if (start == 0) *r.step = t;
  }
}

struct AdamGradArgs {
  const float *g[ADAM_PATCH];
};

__global__ void __launch_bounds__(ADAM_PATCH) k_adam_set_grads(D4gsAdamRec *table, int count, AdamGradArgs a) {
  const int i = threadIdx.x;
  if (i < count) table[i].grad = a.g[i];
}

}  // namespace

extern "C" {

int64_t d4gs_adam_blocks(int64_t n) { return n > D4GS_ADAM_CHUNK ? (n + D4GS_ADAM_CHUNK - 1) / D4GS_ADAM_CHUNK : 1; }

int d4gs_adam_step(const D4gsAdamRec *table, int32_t n_records, const int32_t *block_prefix, int32_t n_blocks, float *block_steps,
                   void *stream) {
  if (n_records < 0 || n_blocks < n_records) {
    d4gs_set_error("d4gs_adam_step: bad counts n_records=%d n_blocks=%d (every record has at least one block)", n_records, n_blocks);
    return D4GS_EINVAL;
  }
  if (n_records == 0) return D4GS_OK;
  if (!table || !block_prefix || !block_steps) {
    d4gs_set_error("d4gs_adam_step: NULL argument (table, block_prefix and block_steps are required)");
    return D4GS_EINVAL;
  }
  if ((uintptr_t)table % 8 || (uintptr_t)block_prefix % 4 || (uintptr_t)block_steps % 4) {
    d4gs_set_error("d4gs_adam_step: misaligned argument (table 8-byte, block_prefix and block_steps 4-byte)");
    return D4GS_EINVAL;
  }
  D4GS_LAUNCH("k_adam", k_adam, dim3((unsigned)n_blocks), dim3(ADAM_BLOCK), 0, (hipStream_t)stream, table, (int)n_records,
              block_prefix, block_steps);
  return d4gs_check_launch("k_adam");
}

int d4gs_adam_set_grads(D4gsAdamRec *table, int32_t n_records, const float *const *grads, void *stream) {
  if (n_records < 0) {
    d4gs_set_error("d4gs_adam_set_grads: n_records=%d", n_records);
    return D4GS_EINVAL;
  }
  if (n_records == 0) return D4GS_OK;
  if (!table || !grads || (uintptr_t)table % 8) {
    d4gs_set_error("d4gs_adam_set_grads: NULL or misaligned argument");
    return D4GS_EINVAL;
  }
  for (int32_t first = 0; first < n_records; first += ADAM_PATCH) {
    const int count = n_records - first < ADAM_PATCH ? n_records - first : ADAM_PATCH;
    AdamGradArgs a = {};
    for (int i = 0; i < count; i++) {
      if ((uintptr_t)grads[first + i] % 4) {
        d4gs_set_error("d4gs_adam_set_grads: grads[%d] is not 4-byte aligned", first + i);
        return D4GS_EINVAL;
      }
      a.g[i] = grads[first + i];
    }
    D4GS_LAUNCH("k_adam_set_grads", k_adam_set_grads, dim3(1), dim3(ADAM_PATCH), 0, (hipStream_t)stream, table + first, count, a);
    if (int rc = d4gs_check_launch("k_adam_set_grads")) return rc;
  }
  return D4GS_OK;
}

int d4gs_adam_step_cpu(const D4gsAdamRec *table, int32_t n_records) {
  if (n_records < 0 || (n_records > 0 && !table)) {
    d4gs_set_error("d4gs_adam_step_cpu: NULL table or n_records=%d", n_records);
    return D4GS_EINVAL;
  }
  for (int32_t r = 0; r < n_records; r++) {  // validate everything before anything is written
    const D4gsAdamRec &a = table[r];
    if (!a.param || !a.exp_avg || !a.exp_avg_sq || !a.step || a.n < 0) {
      d4gs_set_error("d4gs_adam_step_cpu: record %d: NULL param / exp_avg / exp_avg_sq / step, or n=%lld", r, (long long)a.n);
      return D4GS_EINVAL;
    }
    if (((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq | (uintptr_t)a.step) % 4) {
      d4gs_set_error("d4gs_adam_step_cpu: record %d: misaligned pointer (fp32 tensors)", r);
      return D4GS_EINVAL;
    }
  }
  for (int32_t r = 0; r < n_records; r++) {
    const D4gsAdamRec &a = table[r];
    if (!a.grad) continue;
    const float t = *a.step + 1.0f;
    const AdamCoef c = adam_coef(a.lr, a.beta1, a.beta2, a.eps, t);
    for (int64_t i = 0; i < a.n; i++) adam_update(a.param[i], a.exp_avg[i], a.exp_avg_sq[i], a.grad[i], c);
    *a.step = t;
  }
  return D4GS_OK;
}

}  // extern "C"
