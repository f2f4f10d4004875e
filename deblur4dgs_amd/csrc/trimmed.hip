// trimmed.hip -- the reference's quantile-trimmed losses (flow3d/loss_utils.py: masked_l1_loss, trimmed_l1_loss,
// compute_gradient_loss) without a sort, a host read or a data-dependent launch (include/d4gs.h, "Trimmed losses"),
// and the trainer's 2-D track / mapped-depth pair built on them (flow3d/trainer.py:633-667,681-689).
//
// One value pass per mode writes the elements v >= 0 to scratch (the depth-gradient mode: two terms, one slot per pixel and term,
// a slot without a valid pair holds TRIM_EMPTY and the valid ones are counted on the device; the track mode: two terms, one slot per
// (target frame, query) and term, live where the query is visible).  Everything after it is the same for every mode and runs once
// per term (blockIdx.y); the terms that select come first, the others (term >= sel_terms) skip the selection and keep every live slot:
//   4 x { k_trim_hist: LDS histogram of one 8-bit digit of the keys under the current prefix, merged into 256 global bins with
//                      integer atomics;  k_trim_narrow: one block scans the bins and extends the prefix }
// Non-negative floats order like their bit patterns, so after the four digits the prefix IS the order statistic.  torch.quantile
// interpolates between the order statistics floor(r) and ceil(r): two prefixes are narrowed side by side (they share a histogram
// until they part, after which the upper one is the minimum of its bin).  k_trim_sum then adds v * m, m and the count over v < t
// into per-block partials and k_trim_finish adds those in a fixed order in double.  Integer adds commute and every float sum has a
// fixed order: the same input gives the same bits on every run and every graph replay.
//
// LDS atomics on one address serialise, and a depth map puts every key of a wave into one bin of the first digit (often of the
// first two), so a wave first peels off up to TRIM_PEEL groups of lanes that share a digit - one add of the group's size each - and
// only the lanes left after that add one by one (keys spread over many bins, where lanes rarely meet).
#include "common.h"
#include "reduce.h"

namespace {

constexpr int TB = REDUCE_NT;                      // threads per block, all kernels
constexpr int TRIM_ITEMS = 8;                // elements per thread before the grid stops growing
constexpr int TRIM_MAX_BLOCKS = 1024;        // 4 per CU; beyond that the data passes stride
constexpr int TRIM_PEEL = 4;
constexpr uint32_t TRIM_EMPTY = 0xFFFFFFFFu;  // a slot without an element: a NaN pattern, above every key, `v < t` false
constexpr int TRIM_PASSES = 4;
// control words per term (uint32): the state, then two 256-bin histograms (lower / upper order statistic)
enum { C_COUNT = 0, C_PREFIX_LO, C_RANK_LO, C_PREFIX_HI, C_RANK_HI, C_FRAC, C_T, C_PAD, C_HIST, C_WORDS = C_HIST + 512 };
constexpr int PARTIAL_DOUBLES = 3;  // sum v * m, sum m, count

__host__ __device__ inline int64_t trim_blocks(int64_t n_max) {
  const int64_t b = (n_max + (int64_t)TB * TRIM_ITEMS - 1) / ((int64_t)TB * TRIM_ITEMS);
  return b < 1 ? 1 : (b > TRIM_MAX_BLOCKS ? TRIM_MAX_BLOCKS : b);
}
// scratch layout in 32-bit words: values [terms * n_max] (padded to even) | control [terms * C_WORDS] | partials (doubles)
__host__ __device__ inline int64_t trim_ctrl_offset(int64_t n_max, int terms) { return ((int64_t)terms * n_max + 1) & ~(int64_t)1; }
__host__ __device__ inline int64_t trim_partials_offset(int64_t n_max, int terms) {
  return trim_ctrl_offset(n_max, terms) + (int64_t)terms * C_WORDS;
}
__host__ __device__ inline int64_t trim_scratch_words(int64_t n_max, int terms) {
  return trim_partials_offset(n_max, terms) + 2 * (int64_t)terms * trim_blocks(n_max) * PARTIAL_DOUBLES;
}

__global__ void __launch_bounds__(TB) k_trim_init(uint32_t *ctrl, int terms, uint32_t count) {
  for (int i = threadIdx.x; i < terms * C_WORDS; i += TB) ctrl[i] = (i % C_WORDS) == C_COUNT ? count : 0u;
}

// v[i] = mean over the last axis of |pred - gt|
__global__ void __launch_bounds__(TB) k_trim_l1_values(const float *__restrict__ pred, const float *__restrict__ gt, int64_t n, int D,
                                                       float *__restrict__ values) {
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
    float s = 0.f;
    for (int d = 0; d < D; d++) s += fabsf(pred[i * D + d] - gt[i * D + d]);
    values[i] = D == 1 ? s : s / (float)D;
  }
}

// the finite differences of one pixel towards its right (x term) and lower (y term) neighbour, and whether each pair is valid
struct GradPairs {
  float dx, dy;
  bool vx, vy;
};
__device__ __forceinline__ GradPairs grad_pairs(const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ mask,
                                                int64_t p, int H, int W) {
  const int x = (int)(p % W), y = (int)((p / W) % H);
  GradPairs g;
  const bool m0 = mask[p] != 0.f;
  g.vx = m0 && x + 1 < W && mask[p + 1] != 0.f;
  g.vy = m0 && y + 1 < H && mask[p + W] != 0.f;
  g.dx = g.vx ? (pred[p + 1] - pred[p]) - (gt[p + 1] - gt[p]) : 0.f;
  g.dy = g.vy ? (pred[p + W] - pred[p]) - (gt[p + W] - gt[p]) : 0.f;
  return g;
}

__global__ void __launch_bounds__(TB) k_trim_grad_values(const float *__restrict__ pred, const float *__restrict__ gt,
                                                         const float *__restrict__ mask, int64_t P, int H, int W,
                                                         float *__restrict__ values, uint32_t *ctrl) {
  __shared__ uint32_t cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  uint32_t cx = 0, cy = 0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x; p < P; p += stride) {
    const GradPairs g = grad_pairs(pred, gt, mask, p, H, W);
    values[p] = g.vx ? fabsf(g.dx) : __uint_as_float(TRIM_EMPTY);
    values[P + p] = g.vy ? fabsf(g.dy) : __uint_as_float(TRIM_EMPTY);
    cx += g.vx, cy += g.vy;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cx += __shfl_xor(cx, o), cy += __shfl_xor(cy, o);
  if ((threadIdx.x & 63) == 0) atomicAdd(&cnt[0], cx), atomicAdd(&cnt[1], cy);
  __syncthreads();
  if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&ctrl[threadIdx.x * C_WORDS + C_COUNT], cnt[threadIdx.x]);
}

// one wave adds its lanes' digits to an LDS histogram (header comment); called by all 64 lanes together
__device__ __forceinline__ void wave_hist_add(uint32_t *h, uint32_t digit, bool active) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(active);
  for (int round = 0; round < TRIM_PEEL && todo; round++) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t d = __shfl(digit, leader);
    const bool mine = active && digit == d;
    const unsigned long long same = __ballot(mine);
    if (lane == leader) atomicAdd(&h[d], (uint32_t)__popcll(same));
    active = active && !mine;
    todo &= ~same;
  }
  if (active) atomicAdd(&h[digit], 1u);
}

// pass p counts bits [24 - 8p, 32 - 8p) of the keys whose higher bits equal the prefix of the lower / of the upper order statistic
__global__ void __launch_bounds__(TB) k_trim_hist(const float *__restrict__ values, int64_t n_max, uint32_t *ctrl_all, int pass) {
  __shared__ uint32_t h[TB / 64][2][256];
  const int term = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
  uint32_t *ctrl = ctrl_all + (int64_t)term * C_WORDS;
  const uint32_t *keys = reinterpret_cast<const uint32_t *>(values) + (int64_t)term * n_max;
  for (int i = tid; i < (TB / 64) * 2 * 256; i += TB) (&h[0][0][0])[i] = 0;
  const int shift = 24 - 8 * pass;
  const uint32_t high = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
  const uint32_t pre_lo = ctrl[C_PREFIX_LO], pre_hi = ctrl[C_PREFIX_HI];
  const bool split = pre_lo != pre_hi;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t base = (int64_t)blockIdx.x * TB; base < n_max; base += stride) {  // block-uniform trip count: the ballots need whole waves
    const int64_t i = base + tid;
    const uint32_t key = i < n_max ? keys[i] : TRIM_EMPTY;
    const uint32_t digit = (key >> shift) & 255u;
    const bool live = key != TRIM_EMPTY;
    wave_hist_add(h[wave][0], digit, live && (key & high) == pre_lo);
    if (split) wave_hist_add(h[wave][1], digit, live && (key & high) == pre_hi);
  }
  __syncthreads();
  for (int i = tid; i < 512; i += TB) {
    const int track = i >> 8, bin = i & 255;
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < TB / 64; w++) s += h[w][track][bin];
    if (s) atomicAdd(&ctrl[C_HIST + i], s);
  }
}

// torch.lerp's formula in fp32 (ATen/native/Lerp.h)
__device__ __forceinline__ float trim_lerp(float a, float b, float w) {
#pragma clang fp contract(off)
  const float d = b - a;
  return w < 0.5f ? a + w * d : b - d * (1.f - w);
}

// one block per term: bin of the histogram that holds the wanted rank -> next 8 bits of the prefix.  Before the first pass: the
// ranks from the live count, r = q (n - 1) in fp32 as torch.quantile evaluates it for fp32 input.  After the last: the threshold.
__global__ void __launch_bounds__(TB) k_trim_narrow(uint32_t *ctrl_all, int pass, float q) {
  __shared__ uint32_t scan[2][TB];
  __shared__ uint32_t st[8];
  uint32_t *ctrl = ctrl_all + (int64_t)blockIdx.x * C_WORDS;
  const int tid = threadIdx.x;
  const uint32_t n = ctrl[C_COUNT];
  if (tid == 0) {
    if (pass == 0) {
      float r = 0.f;
      uint32_t lo = 0, hi = 0;
      if (n > 0) {
        r = q * (float)(n - 1);
        const float fl = floorf(r), ce = ceilf(r);
        lo = fl >= (float)(n - 1) ? n - 1 : (uint32_t)fl;  // (float)(n - 1) can round up: stay inside
        hi = ce >= (float)(n - 1) ? n - 1 : (uint32_t)ce;
        r = r - fl;
      }
      st[C_PREFIX_LO] = 0, st[C_PREFIX_HI] = 0, st[C_RANK_LO] = lo, st[C_RANK_HI] = hi, st[C_FRAC] = __float_as_uint(r);
    } else {
      for (int k = C_PREFIX_LO; k <= C_FRAC; k++) st[k] = ctrl[k];
    }
  }
  const uint32_t ha = ctrl[C_HIST + tid], hb_raw = ctrl[C_HIST + 256 + tid];
  __syncthreads();
  ctrl[C_HIST + tid] = 0, ctrl[C_HIST + 256 + tid] = 0;  // ready for the next pass (and for the next call)
  const bool split = st[C_PREFIX_LO] != st[C_PREFIX_HI];
  const uint32_t hb = split ? hb_raw : ha;
  const uint32_t rank_lo = st[C_RANK_LO], rank_hi = st[C_RANK_HI];
  scan[0][tid] = ha, scan[1][tid] = hb;
  __syncthreads();
  for (int o = 1; o < TB; o <<= 1) {  // inclusive scans of both histograms
    const uint32_t a = tid >= o ? scan[0][tid - o] : 0, b = tid >= o ? scan[1][tid - o] : 0;
    __syncthreads();
    scan[0][tid] += a, scan[1][tid] += b;
    __syncthreads();
  }
  const int shift = 24 - 8 * pass;
  const uint32_t ea = scan[0][tid] - ha, eb = scan[1][tid] - hb;  // exclusive
  if (ha && ea <= rank_lo && rank_lo - ea < ha) st[C_PREFIX_LO] |= (uint32_t)tid << shift, st[C_RANK_LO] = rank_lo - ea;
  __syncthreads();  // (the two updates touch different words, but C_PREFIX_LO above was read for `split`: keep them apart)
  if (hb && eb <= rank_hi && rank_hi - eb < hb) st[C_PREFIX_HI] |= (uint32_t)tid << shift, st[C_RANK_HI] = rank_hi - eb;
  __syncthreads();
  if (tid == 0) {
    for (int k = C_PREFIX_LO; k <= C_FRAC; k++) ctrl[k] = st[k];
    if (pass == TRIM_PASSES - 1) {
      const float t = n > 0 ? trim_lerp(__uint_as_float(st[C_PREFIX_LO]), __uint_as_float(st[C_PREFIX_HI]), __uint_as_float(st[C_FRAC]))
                            : __uint_as_float(0x7FC00000u);  // no element: NaN, nothing is below it
      ctrl[C_T] = __float_as_uint(t);
    }
  }
}

__device__ __forceinline__ bool trim_kept(float v, float t, bool keep_all) { return keep_all ? v == v : v < t; }

__global__ void __launch_bounds__(TB) k_trim_sum(const float *__restrict__ values, const float *__restrict__ weights, int64_t n_max,
                                                 const uint32_t *__restrict__ ctrl_all, int sel_terms, double *__restrict__ partials) {
  __shared__ double red[PARTIAL_DOUBLES * (TB / 64)];
  const int term = blockIdx.y, tid = threadIdx.x;
  const bool keep_all = term >= sel_terms;
  const float t = __uint_as_float(ctrl_all[(int64_t)term * C_WORDS + C_T]);
  const float *v = values + (int64_t)term * n_max;
  double s_vm = 0.0, s_m = 0.0, cnt = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + tid; i < n_max; i += stride) {
    const float vi = v[i];
    if (trim_kept(vi, t, keep_all)) {
      const float m = weights ? weights[i] : 1.f;
      s_vm += (double)(vi * m), s_m += (double)m, cnt += 1.0;
    }
  }
  double s[PARTIAL_DOUBLES] = {s_vm, s_m, cnt};
  block_sum_store(s, red);
  __syncthreads();
  if (tid < PARTIAL_DOUBLES)
    partials[((int64_t)term * gridDim.x + blockIdx.x) * PARTIAL_DOUBLES + tid] = block_sum_combine<PARTIAL_DOUBLES>(red, tid);
}

// out[0] = sum of the terms' losses; per term k: out[1 + 2k] = threshold, out[2 + 2k] = 1 / denominator (what the backward scales by),
// out[5 + k] = the term's own loss
// denominators: mode 0 sum of kept m + 1e-8 (normalize=True), mode 1 the kept count (normalize=False, no mask), mode 2 as mode 0 but
// a term that selected among no live slot at all (its threshold is NaN) is NaN, as the mean forms are
__global__ void __launch_bounds__(TB) k_trim_finish(const double *__restrict__ partials, int n_blocks, int terms, int mode,
                                                    const uint32_t *__restrict__ ctrl_all, float *out) {
  double total = 0.0;
  for (int term = 0; term < terms; term++) {
    double r[PARTIAL_DOUBLES];  // every thread gets the term's sums: sum v * m, sum m, count
    ordered_total(partials + (int64_t)term * n_blocks * PARTIAL_DOUBLES, n_blocks, PARTIAL_DOUBLES, r);
    const double den = mode == 1 ? r[2] : r[1] + 1e-8;
    const float t = __uint_as_float(ctrl_all[(int64_t)term * C_WORDS + C_T]);
    double loss = r[0] / den;  // 0 / 0 = NaN: an empty kept set, as torch's mean of nothing
    if (mode == 2 && t != t) loss = (double)t;
    total += loss;
    if (threadIdx.x == 0) out[1 + 2 * term] = t, out[2 + 2 * term] = (float)(1.0 / den), out[5 + term] = (float)loss;
  }
  if (threadIdx.x == 0) out[0] = (float)total;
}

__global__ void __launch_bounds__(TB) k_trim_l1_bwd(const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ mask,
                                                    const float *__restrict__ values, const float *__restrict__ out,
                                                    const float *__restrict__ v_loss, int64_t n, int D, int keep_all, float *__restrict__ v_pred) {
  const float t = out[1], scale = v_loss[0] * out[2] / (float)D;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
    const float c = trim_kept(values[i], t, keep_all) ? scale * (mask ? mask[i] : 1.f) : 0.f;
    for (int d = 0; d < D; d++) {
      const float x = pred[i * D + d], y = gt[i * D + d];
      v_pred[i * D + d] = x > y ? c : (x < y ? -c : 0.f);
    }
  }
}

__device__ __forceinline__ float trim_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// one thread per pixel gathers from the (at most) four pairs it belongs to: no atomics, a fixed order
__global__ void __launch_bounds__(TB) k_trim_grad_bwd(const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ mask,
                                                      const float *__restrict__ values, const float *__restrict__ out,
                                                      const float *__restrict__ v_loss, int64_t P, int H, int W, float *__restrict__ v_pred) {
  const float tx = out[1], ty = out[3], sx = v_loss[0] * out[2], sy = v_loss[0] * out[4];
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x; p < P; p += stride) {
    const int x = (int)(p % W), y = (int)((p / W) % H);
    float g = 0.f;
    const GradPairs own = grad_pairs(pred, gt, mask, p, H, W);  // pairs (p, p + 1) and (p, p + W): p is the subtracted end
    if (own.vx && values[p] < tx) g -= sx * trim_sign(own.dx);
    if (x > 0) {
      const GradPairs l = grad_pairs(pred, gt, mask, p - 1, H, W);
      if (l.vx && values[p - 1] < tx) g += sx * trim_sign(l.dx);
    }
    if (own.vy && values[P + p] < ty) g -= sy * trim_sign(own.dy);
    if (y > 0) {
      const GradPairs u = grad_pairs(pred, gt, mask, p - W, H, W);
      if (u.vy && values[P + p - W] < ty) g += sy * trim_sign(u.dy);
    }
    v_pred[p] = g;
  }
}

// ---- the 2-D track loss and the mapped-depth loss (trainer.py:633-667,681-689) over elements e = (row r = b N + n, query p) ----
// One query of one target frame: the point the dynamic render composited at the query's pixel, in the target camera's frame, and
// its projection by the row's intrinsics.
struct TrackPoint {
  const float *K;    // the row's 3 x 3 intrinsics
  int64_t at;        // offset of the point's three floats in tracks_3d [pixels, N, 3]
  float pz, z, x, y; // (K X)_z, max(pz, 1e-6), (K X)_xy / z
};
// false: not a live element (not visible, or a pixel / row outside the tables' range - no address is formed from such an index)
__device__ __forceinline__ bool track_point(const float *__restrict__ tracks, const int32_t *__restrict__ pix, const int32_t *__restrict__ rows,
                                            const uint8_t *__restrict__ visible, const float *__restrict__ Ks, int64_t e, int64_t n_pixels,
                                            int N, int n_rows, TrackPoint &t) {
  if (!visible[e]) return false;
  const int32_t p = pix[e], r = rows[e];
  if (p < 0 || (int64_t)p >= n_pixels || r < 0 || r >= n_rows) return false;
  t.K = Ks + (int64_t)r * 9;
  t.at = ((int64_t)p * N + r % N) * 3;
  const float X = tracks[t.at], Y = tracks[t.at + 1], Z = tracks[t.at + 2];
  const float px = t.K[0] * X + t.K[1] * Y + t.K[2] * Z, py = t.K[3] * X + t.K[4] * Y + t.K[5] * Z;
  t.pz = t.K[6] * X + t.K[7] * Y + t.K[8] * Z;
  t.z = fmaxf(t.pz, 1e-6f);
  t.x = px / t.z, t.y = py / t.z;
  return true;
}
__device__ __forceinline__ float track_disparity(float depth) { return 1.f / (depth + 1e-5f); }

// term 0: mean over (x, y) of |projected - target|; term 1: |1 / (z + 1e-5) - 1 / (target depth + 1e-5)|; both share the live count
__global__ void __launch_bounds__(TB) k_track_values(const float *__restrict__ tracks, const int32_t *__restrict__ pix,
                                                     const int32_t *__restrict__ rows, const uint8_t *__restrict__ visible,
                                                     const float *__restrict__ target_2d, const float *__restrict__ target_depth,
                                                     const float *__restrict__ Ks, int64_t n_pixels, int N, int n_rows, int64_t n,
                                                     float *__restrict__ values, uint32_t *ctrl) {
  __shared__ uint32_t cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  uint32_t c = 0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x; e < n; e += stride) {
    TrackPoint t;
    const bool live = track_point(tracks, pix, rows, visible, Ks, e, n_pixels, N, n_rows, t);
    float v0 = __uint_as_float(TRIM_EMPTY), v1 = v0;
    if (live) {
      v0 = 0.5f * (fabsf(t.x - target_2d[2 * e]) + fabsf(t.y - target_2d[2 * e + 1]));
      v1 = fabsf(track_disparity(t.z) - track_disparity(target_depth[e]));
    }
    values[e] = v0, values[n + e] = v1;
    c += live;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x < 2 && cnt) atomicAdd(&ctrl[threadIdx.x * C_WORDS + C_COUNT], cnt);
}

// one thread per live element adds K^T dL/d(K X) to its point.  torch.clamp(min) passes the gradient where its input is >= the
// bound: pz > 1e-6f here, fp32's 1e-6 lying just below the real one.  Below it x and y still divide by the clamped 1e-6.
__global__ void __launch_bounds__(TB) k_track_bwd(const float *__restrict__ tracks, const int32_t *__restrict__ pix,
                                                  const int32_t *__restrict__ rows, const uint8_t *__restrict__ visible,
                                                  const float *__restrict__ weights, const float *__restrict__ target_2d,
                                                  const float *__restrict__ target_depth, const float *__restrict__ Ks,
                                                  const float *__restrict__ values, const float *__restrict__ out,
                                                  const float *__restrict__ v_losses, int64_t n_pixels, int N, int n_rows, int64_t n,
                                                  int keep_all, float *v_tracks) {
  const float t0 = out[1], s0 = v_losses[0] * out[2], s1 = v_losses[1] * out[4];
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x; e < n; e += stride) {
    TrackPoint t;
    if (!track_point(tracks, pix, rows, visible, Ks, e, n_pixels, N, n_rows, t)) continue;
    const float w = weights[e];
    const float c0 = trim_kept(values[e], t0, keep_all) ? 0.5f * s0 * w : 0.f;
    const float gx = c0 * trim_sign(t.x - target_2d[2 * e]), gy = c0 * trim_sign(t.y - target_2d[2 * e + 1]);
    const float a = track_disparity(t.z);
    const float gz = -(gx * t.x + gy * t.y) / t.z - s1 * w * trim_sign(a - track_disparity(target_depth[e])) * a * a;
    const float dx = gx / t.z, dy = gy / t.z, dz = t.pz > 1e-6f ? gz : 0.f;
#pragma unroll
    for (int j = 0; j < 3; j++) atomicAdd(&v_tracks[t.at + j], t.K[j] * dx + t.K[3 + j] * dy + t.K[6 + j] * dz);
  }
}

// [selection of the first sel_terms terms at quantile q], sum, finish over values already in scratch (control words initialised)
int trim_reduce(float *values, const float *weights, int64_t n_max, int terms, int sel_terms, int mode, float q, uint32_t *ctrl,
                double *partials, float *out, hipStream_t stream) {
  const int nb = (int)trim_blocks(n_max);
  const dim3 grid(nb, terms);
  if (sel_terms > 0) {
    for (int pass = 0; pass < TRIM_PASSES; pass++) {
      D4GS_LAUNCH("k_trim_hist", k_trim_hist, dim3(nb, sel_terms), dim3(TB), 0, stream, (const float *)values, n_max, ctrl, pass);
      if (int rc = d4gs_check_launch("k_trim_hist")) return rc;
      D4GS_LAUNCH("k_trim_narrow", k_trim_narrow, dim3(sel_terms), dim3(TB), 0, stream, ctrl, pass, q);
      if (int rc = d4gs_check_launch("k_trim_narrow")) return rc;
    }
  }
  D4GS_LAUNCH("k_trim_sum", k_trim_sum, grid, dim3(TB), 0, stream, (const float *)values, weights, n_max, (const uint32_t *)ctrl,
              sel_terms, partials);
  if (int rc = d4gs_check_launch("k_trim_sum")) return rc;
  D4GS_LAUNCH("k_trim_finish", k_trim_finish, dim3(1), dim3(TB), 0, stream, (const double *)partials, nb, terms, mode,
              (const uint32_t *)ctrl, out);
  return d4gs_check_launch("k_trim_finish");
}

bool bad_quantile(float q) { return !(q > 0.f) || !(q <= 3.0e38f); }  // NaN, <= 0, inf

int l1_fwd(const char *who, const float *pred, const float *gt, const float *mask, int64_t n, int32_t D, bool keep_all, int mode,
           float quantile, void *scratch, int64_t scratch_words, float *out, void *stream) {
  if (!pred || !gt || !scratch || !out) {
    d4gs_set_error("%s: NULL argument (pred, gt, scratch and out are required)", who);
    return D4GS_EINVAL;
  }
  if (n < 0 || n > INT32_MAX || D < 1) {
    d4gs_set_error("%s: bad size n=%lld D=%d (0 <= n <= 2^31 - 1, D >= 1)", who, (long long)n, D);
    return D4GS_EINVAL;
  }
  if (bad_quantile(quantile)) {
    d4gs_set_error("%s: quantile=%g (finite and > 0)", who, (double)quantile);
    return D4GS_EINVAL;
  }
  if (scratch_words < trim_scratch_words(n, 1) || (uintptr_t)scratch % 8) {
    d4gs_set_error("%s: scratch of %lld words (8-byte aligned) needed, %lld given at %p", who, (long long)trim_scratch_words(n, 1),
                   (long long)scratch_words, scratch);
    return D4GS_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  float *values = (float *)scratch;
  uint32_t *ctrl = (uint32_t *)scratch + trim_ctrl_offset(n, 1);
  double *partials = (double *)((uint32_t *)scratch + trim_partials_offset(n, 1));
  D4GS_LAUNCH("k_trim_init", k_trim_init, dim3(1), dim3(TB), 0, s, ctrl, 1, (uint32_t)n);
  if (int rc = d4gs_check_launch("k_trim_init")) return rc;
  D4GS_LAUNCH("k_trim_l1_values", k_trim_l1_values, dim3((unsigned)trim_blocks(n)), dim3(TB), 0, s, pred, gt, n, (int)D, values);
  if (int rc = d4gs_check_launch("k_trim_l1_values")) return rc;
  return trim_reduce(values, mask, n, 1, keep_all ? 0 : 1, mode, quantile, ctrl, partials, out, s);
}

int l1_bwd(const char *who, const float *pred, const float *gt, const float *mask, const float *values, const float *out,
           const float *v_loss, int64_t n, int32_t D, bool keep_all, float *v_pred, void *stream) {
  if (!pred || !gt || !values || !out || !v_loss || !v_pred) {
    d4gs_set_error("%s: NULL argument (only the mask is optional)", who);
    return D4GS_EINVAL;
  }
  if (n < 0 || n > INT32_MAX || D < 1) {
    d4gs_set_error("%s: bad size n=%lld D=%d (0 <= n <= 2^31 - 1, D >= 1)", who, (long long)n, D);
    return D4GS_EINVAL;
  }
  if (n == 0) return D4GS_OK;
  D4GS_LAUNCH("k_trim_l1_bwd", k_trim_l1_bwd, dim3((unsigned)trim_blocks(n)), dim3(TB), 0, (hipStream_t)stream, pred, gt, mask, values,
              out, v_loss, n, (int)D, (int)keep_all, v_pred);
  return d4gs_check_launch("k_trim_l1_bwd");
}

int track_check(const char *who, const void *const *ptrs, int n_ptrs, int64_t n_pixels, int32_t N, int32_t n_rows, int64_t n_elements,
                float quantile) {
  for (int i = 0; i < n_ptrs; i++)
    if (!ptrs[i]) {
      d4gs_set_error("%s: NULL argument (every pointer is required)", who);
      return D4GS_EINVAL;
    }
  if (N < 1 || n_rows < 1 || n_rows % N || n_elements < 1 || n_elements > INT32_MAX || n_pixels < 1 || n_pixels > INT32_MAX ||
      n_pixels > ((int64_t)1 << 40) / N) {
    d4gs_set_error("%s: bad size n_pixels=%lld N=%d n_rows=%d n_elements=%lld (N >= 1, n_rows a positive multiple of N, 1 <= n_pixels, "
                   "n_elements <= 2^31 - 1, n_pixels N <= 2^40)", who, (long long)n_pixels, N, n_rows, (long long)n_elements);
    return D4GS_EINVAL;
  }
  if (bad_quantile(quantile)) {
    d4gs_set_error("%s: quantile=%g (finite and > 0)", who, (double)quantile);
    return D4GS_EINVAL;
  }
  return D4GS_OK;
}

}  // namespace

// host.h: the masked, normalized form over values that a caller's own kernel has left in the first n words of `scratch`
// (track_fit.hip's per-frame 2-D errors) - the control words are set here, the rest is trim_reduce
bool d4gs_bad_quantile(float q) { return bad_quantile(q); }
int d4gs_trim_masked_impl(void *scratch, const float *weights, int64_t n, float quantile, float *out, hipStream_t stream) {
  uint32_t *ctrl = (uint32_t *)scratch + trim_ctrl_offset(n, 1);
  double *partials = (double *)((uint32_t *)scratch + trim_partials_offset(n, 1));
  D4GS_LAUNCH("k_trim_init", k_trim_init, dim3(1), dim3(TB), 0, stream, ctrl, 1, (uint32_t)n);
  if (int rc = d4gs_check_launch("k_trim_init")) return rc;
  return trim_reduce((float *)scratch, weights, n, 1, quantile >= 1.f ? 0 : 1, 0, quantile, ctrl, partials, out, stream);
}

extern "C" {

int64_t d4gs_trimmed_scratch_words(int64_t n_max, int32_t terms) {
  if (n_max < 0 || n_max > INT32_MAX || terms < 1 || terms > 2) return 0;
  return trim_scratch_words(n_max, terms);
}

int d4gs_masked_l1_fwd(const float *pred, const float *gt, const float *mask, int64_t n, int32_t D, int32_t normalize, float quantile,
                       void *scratch, int64_t scratch_words, float *out, void *stream) {
  if (!mask) {
    d4gs_set_error("d4gs_masked_l1_fwd: NULL mask (the form without a mask is d4gs_trimmed_l1_fwd)");
    return D4GS_EINVAL;
  }
  return l1_fwd("d4gs_masked_l1_fwd", pred, gt, mask, n, D, quantile >= 1.f, normalize ? 0 : 1, quantile, scratch, scratch_words, out, stream);
}

int d4gs_masked_l1_bwd(const float *pred, const float *gt, const float *mask, const float *values, const float *out, const float *v_loss,
                       int64_t n, int32_t D, float quantile, float *v_pred, void *stream) {
  if (!mask || bad_quantile(quantile)) {
    d4gs_set_error("d4gs_masked_l1_bwd: NULL mask or quantile=%g (finite and > 0)", (double)quantile);
    return D4GS_EINVAL;
  }
  return l1_bwd("d4gs_masked_l1_bwd", pred, gt, mask, values, out, v_loss, n, D, quantile >= 1.f, v_pred, stream);
}

int d4gs_trimmed_l1_fwd(const float *pred, const float *gt, int64_t n, int32_t D, float quantile, void *scratch, int64_t scratch_words,
                        float *out, void *stream) {
  return l1_fwd("d4gs_trimmed_l1_fwd", pred, gt, nullptr, n, D, false, 1, quantile, scratch, scratch_words, out, stream);
}

int d4gs_trimmed_l1_bwd(const float *pred, const float *gt, const float *values, const float *out, const float *v_loss, int64_t n,
                        int32_t D, float *v_pred, void *stream) {
  return l1_bwd("d4gs_trimmed_l1_bwd", pred, gt, nullptr, values, out, v_loss, n, D, false, v_pred, stream);
}

int d4gs_gradient_loss_fwd(const float *pred, const float *gt, const float *mask, int32_t B, int32_t H, int32_t W, float quantile,
                           void *scratch, int64_t scratch_words, float *out, void *stream) {
  if (!pred || !gt || !mask || !scratch || !out) {
    d4gs_set_error("d4gs_gradient_loss_fwd: NULL argument");
    return D4GS_EINVAL;
  }
  const int64_t P = (int64_t)B * H * W;
  if (B < 0 || H < 0 || W < 0 || P > INT32_MAX) {
    d4gs_set_error("d4gs_gradient_loss_fwd: bad size B=%d H=%d W=%d (each >= 0, B H W <= 2^31 - 1)", B, H, W);
    return D4GS_EINVAL;
  }
  if (bad_quantile(quantile)) {
    d4gs_set_error("d4gs_gradient_loss_fwd: quantile=%g (finite and > 0)", (double)quantile);
    return D4GS_EINVAL;
  }
  if (scratch_words < trim_scratch_words(P, 2) || (uintptr_t)scratch % 8) {
    d4gs_set_error("d4gs_gradient_loss_fwd: scratch of %lld words (8-byte aligned) needed, %lld given at %p",
                   (long long)trim_scratch_words(P, 2), (long long)scratch_words, scratch);
    return D4GS_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  float *values = (float *)scratch;
  uint32_t *ctrl = (uint32_t *)scratch + trim_ctrl_offset(P, 2);
  double *partials = (double *)((uint32_t *)scratch + trim_partials_offset(P, 2));
  D4GS_LAUNCH("k_trim_init", k_trim_init, dim3(1), dim3(TB), 0, s, ctrl, 2, 0u);
  if (int rc = d4gs_check_launch("k_trim_init")) return rc;
  D4GS_LAUNCH("k_trim_grad_values", k_trim_grad_values, dim3((unsigned)trim_blocks(P)), dim3(TB), 0, s, pred, gt, mask, P, (int)H, (int)W,
              values, ctrl);
  if (int rc = d4gs_check_launch("k_trim_grad_values")) return rc;
  return trim_reduce(values, nullptr, P, 2, 2, 1, quantile, ctrl, partials, out, s);
}

int d4gs_gradient_loss_bwd(const float *pred, const float *gt, const float *mask, const float *values, const float *out,
                           const float *v_loss, int32_t B, int32_t H, int32_t W, float *v_pred, void *stream) {
  if (!pred || !gt || !mask || !values || !out || !v_loss || !v_pred) {
    d4gs_set_error("d4gs_gradient_loss_bwd: NULL argument");
    return D4GS_EINVAL;
  }
  const int64_t P = (int64_t)B * H * W;
  if (B < 0 || H < 0 || W < 0 || P > INT32_MAX) {
    d4gs_set_error("d4gs_gradient_loss_bwd: bad size B=%d H=%d W=%d (each >= 0, B H W <= 2^31 - 1)", B, H, W);
    return D4GS_EINVAL;
  }
  if (P == 0) return D4GS_OK;
  D4GS_LAUNCH("k_trim_grad_bwd", k_trim_grad_bwd, dim3((unsigned)trim_blocks(P)), dim3(TB), 0, (hipStream_t)stream, pred, gt, mask, values,
              out, v_loss, P, (int)H, (int)W, v_pred);
  return d4gs_check_launch("k_trim_grad_bwd");
}

int d4gs_track_losses_fwd(const float *tracks_3d, const int32_t *pix, const int32_t *rows, const uint8_t *visible, const float *weights,
                          const float *target_2d, const float *target_depth, const float *Ks, int64_t n_pixels, int32_t N, int32_t n_rows,
                          int64_t n_elements, float quantile, void *scratch, int64_t scratch_words, float *out, void *stream) {
  const void *ptrs[] = {tracks_3d, pix, rows, visible, weights, target_2d, target_depth, Ks, scratch, out};
  if (int rc = track_check("d4gs_track_losses_fwd", ptrs, 10, n_pixels, N, n_rows, n_elements, quantile)) return rc;
  const int64_t n = n_elements;
  if (scratch_words < trim_scratch_words(n, 2) || (uintptr_t)scratch % 8) {
    d4gs_set_error("d4gs_track_losses_fwd: scratch of %lld words (8-byte aligned) needed, %lld given at %p",
                   (long long)trim_scratch_words(n, 2), (long long)scratch_words, scratch);
    return D4GS_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  float *values = (float *)scratch;
  uint32_t *ctrl = (uint32_t *)scratch + trim_ctrl_offset(n, 2);
  double *partials = (double *)((uint32_t *)scratch + trim_partials_offset(n, 2));
  D4GS_LAUNCH("k_trim_init", k_trim_init, dim3(1), dim3(TB), 0, s, ctrl, 2, 0u);
  if (int rc = d4gs_check_launch("k_trim_init")) return rc;
  D4GS_LAUNCH("k_track_values", k_track_values, dim3((unsigned)trim_blocks(n)), dim3(TB), 0, s, tracks_3d, pix, rows, visible, target_2d,
              target_depth, Ks, n_pixels, (int)N, (int)n_rows, n, values, ctrl);
  if (int rc = d4gs_check_launch("k_track_values")) return rc;
  // the depth term (the reference's default quantile, 1) never selects; the 2-D term does unless its quantile says the same
  return trim_reduce(values, weights, n, 2, quantile >= 1.f ? 0 : 1, 2, quantile, ctrl, partials, out, s);
}

int d4gs_track_losses_bwd(const float *tracks_3d, const int32_t *pix, const int32_t *rows, const uint8_t *visible, const float *weights,
                          const float *target_2d, const float *target_depth, const float *Ks, const float *values, const float *out,
                          const float *v_losses, int64_t n_pixels, int32_t N, int32_t n_rows, int64_t n_elements, float quantile,
                          float *v_tracks_3d, void *stream) {
  const void *ptrs[] = {tracks_3d, pix, rows, visible, weights, target_2d, target_depth, Ks, values, out, v_losses, v_tracks_3d};
  if (int rc = track_check("d4gs_track_losses_bwd", ptrs, 12, n_pixels, N, n_rows, n_elements, quantile)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_floats = n_pixels * N * 3;
  // (a kernel, not a memset node: reduce.h)
  D4GS_LAUNCH("k_zero_f32", k_zero_f32<>, dim3((unsigned)trim_blocks(n_floats)), dim3(TB), 0, s, v_tracks_3d, n_floats);
  if (int rc = d4gs_check_launch("k_zero_f32")) return rc;
  D4GS_LAUNCH("k_track_bwd", k_track_bwd, dim3((unsigned)trim_blocks(n_elements)), dim3(TB), 0, s, tracks_3d, pix, rows, visible, weights,
              target_2d, target_depth, Ks, values, out, v_losses, n_pixels, (int)N, (int)n_rows, n_elements, (int)(quantile >= 1.f),
              v_tracks_3d);
  return d4gs_check_launch("k_track_bwd");
}

}  // extern "C"
