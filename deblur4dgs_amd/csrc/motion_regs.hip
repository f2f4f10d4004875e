// motion_regs.hip -- the four regularizers of Trainer.compute_dynamic_losses that never look at an image (flow3d/trainer.py:691-728,
// flow3d/loss_utils.py:118-157; include/d4gs.h, "Motion and scale regularizers"):
//   out[0] smooth_bases   w_rot mean_{k,tau} |2 rots[k,tau] - rots[k,tau-1] - rots[k,tau+1]| + w_transl (the same on transls)
//   out[1] smooth_tracks  0.5 mean_{g,b} |2 m1 - m0 - m2|      m_j[g,b] = the deformed mean of Gaussian g at clamp(ts_b, 1, T-2) + (j-1)
//   out[2] z_accel        mean ((m1 - m0).d)^2 + mean ((m2 - m1).d)^2,  d = normalize(m1 - camera centre_b)
//   out[3] scale_var      mean_g var(scales_g) (unbiased, over the three raw scales)
//
// The deformation and its adjoint are the pose kernels (k_poses_fwd / MODE_POSES of k_project_bwd, N = G, time-major, 3 B time slots):
// this file only forms the 3 B neighbour times and the B camera centres on the device (k_motion_prep), turns the neighbour means into
// the sums (k_motion_loss_fwd + k_motion_finish) and, backwards, into the gradient of the neighbour means and of the scales
// (k_motion_loss_bwd); the bases' own term is added to v_rots / v_transls behind the pose adjoint (k_motion_bases_bwd).
//
// No atomics: every sum is per wave (common.h), then per block in double, then added in block order by one block; every gradient
// address has one writer.  The same input gives the same bits on every run and every graph replay.
// The gradient of a norm at exactly zero is zero (torch's convention): tracks of a static basis set and straight basis rows get 0, not 0/0.
#include "common.h"
#include "reduce.h"

namespace {

constexpr int MB = REDUCE_NT;  // threads per block, all kernels: one lane per Gaussian / basis row
constexpr int PARTIAL_DOUBLES = 3;
constexpr float NORM_EPS = 1e-12f;  // F.normalize's clamp on the norm

// workspace layout (bytes; every part 16-byte aligned)
struct MotionWs {
  size_t times, centres, means_nb, partials, v_points, pose_partials, total;
  int gblocks, bblocks;
};
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

D4gsDims pose_dims(int G, int K, int T, int B) {
  D4gsDims d{};
  d.N = G, d.G = G, d.K = K, d.T = T, d.S = 3 * B, d.D = 1, d.width = 16, d.height = 16;
  d.flags = D4GS_RAW_PARAMS;  // motion_coefs are the raw leaf: softmax inside
  d.near_plane = 0.01f, d.far_plane = 1e10f, d.eps2d = 0.3f;
  return d;
}

MotionWs motion_ws(int G, int K, int T, int B) {
  MotionWs w;
  const size_t nb3 = (size_t)3 * B, pts = nb3 * (size_t)G * 3;
  w.gblocks = (G + MB - 1) / MB;
  w.bblocks = (K * (T - 2) + MB - 1) / MB;
  const D4gsDims d = pose_dims(G, K, T, B);
  size_t o = 0;
  w.times = o, o = align16(o + sizeof(float) * nb3);
  w.centres = o, o = align16(o + sizeof(float) * nb3);
  w.means_nb = o, o = align16(o + sizeof(float) * pts);
  w.partials = o, o = align16(o + sizeof(double) * PARTIAL_DOUBLES * ((size_t)w.gblocks + w.bblocks));
  w.v_points = o, o = align16(o + sizeof(float) * pts);
  w.pose_partials = o, o = align16(o + sizeof(float) * d4gs_poses_bwd_partials_bound(&d));
  w.total = o;
  return w;
}

// times_nb[j B + b] = clamp(ts_b, 1, T - 2) + (j - 1);  centre_b = -A^-1 t of w2c_b = [A t; 0 0 0 1] (cofactor inverse, A any invertible 3x3)
__global__ void __launch_bounds__(MB) k_motion_prep(const float *__restrict__ ts, const float *__restrict__ w2cs, int B, int T,
                                                    float *__restrict__ times_nb, float *__restrict__ centres) {
  const int i = blockIdx.x * MB + threadIdx.x;
  if (i < 3 * B) {
    const int j = i / B, b = i - j * B;
    times_nb[i] = fminf(fmaxf(ts[b], 1.f), (float)(T - 2)) + (float)(j - 1);
  }
  if (i < B) {
    const float *M = w2cs + (size_t)i * 16;
    const float a00 = M[0], a01 = M[1], a02 = M[2], a10 = M[4], a11 = M[5], a12 = M[6], a20 = M[8], a21 = M[9], a22 = M[10];
    const float t0 = M[3], t1 = M[7], t2 = M[11];
    const float c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;  // cofactors of row 0
    const float c10 = a02 * a21 - a01 * a22, c11 = a00 * a22 - a02 * a20, c12 = a01 * a20 - a00 * a21;
    const float c20 = a01 * a12 - a02 * a11, c21 = a02 * a10 - a00 * a12, c22 = a00 * a11 - a01 * a10;
    const float inv = 1.f / (a00 * c00 + a01 * c01 + a02 * c02);
    // A^-1 = cof^T / det
    centres[i * 3] = -(c00 * t0 + c10 * t1 + c20 * t2) * inv;
    centres[i * 3 + 1] = -(c01 * t0 + c11 * t1 + c21 * t2) * inv;
    centres[i * 3 + 2] = -(c02 * t0 + c12 * t1 + c22 * t2) * inv;
  }
}

struct Nb3 {
  float m0[3], m1[3], m2[3];
};
__device__ __forceinline__ Nb3 load_nb(const float *__restrict__ means_nb, int G, int B, int g, int b) {
  Nb3 n;
  const float *p0 = means_nb + ((size_t)b * G + g) * 3, *p1 = means_nb + ((size_t)(B + b) * G + g) * 3,
              *p2 = means_nb + ((size_t)(2 * B + b) * G + g) * 3;
#pragma unroll
  for (int i = 0; i < 3; i++) n.m0[i] = p0[i], n.m1[i] = p1[i], n.m2[i] = p2[i];
  return n;
}

// |2 x[tau] - x[tau-1] - x[tau+1]| of one basis row (D = 6 rots, 3 transls); the acceleration itself in `a`
template <int D>
__device__ __forceinline__ float accel_row(const float *__restrict__ x, int k, int T, int tau, float *a) {
  const float *p = x + ((size_t)k * T + tau) * D;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < D; i++) {
    a[i] = 2.f * p[i] - p[i - D] - p[i + D];
    s += a[i] * a[i];
  }
  return sqrtf(s);
}

// blocks [0, gblocks): one lane per Gaussian -> (sum_b |a|, sum_b p0^2 + p1^2, sum_i (s_i - mean)^2 / 2)
// blocks [gblocks, +bblocks): one lane per basis row (k, tau) -> (|accel rots|, |accel transls|, 0)
__global__ void __launch_bounds__(MB) k_motion_loss_fwd(const float *__restrict__ means_nb, const float *__restrict__ centres,
                                                        const float *__restrict__ scales, const float *__restrict__ rots,
                                                        const float *__restrict__ transls, int G, int K, int T, int B, int gblocks,
                                                        double *__restrict__ partials) {
  __shared__ float red[(MB / 64) * 4];  // per wave: 3 totals + the pad slot wave_sum_store wants
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float v[3] = {0.f, 0.f, 0.f};
  if ((int)blockIdx.x < gblocks) {
    const int g = blockIdx.x * MB + tid;
    if (g < G) {
      for (int b = 0; b < B; b++) {
        const Nb3 n = load_nb(means_nb, G, B, g, b);
        float aa = 0.f, rr = 0.f, e0r = 0.f, e1r = 0.f;
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const float a = 2.f * n.m1[i] - n.m0[i] - n.m2[i], r = n.m1[i] - centres[b * 3 + i];
          aa += a * a, rr += r * r, e0r += (n.m1[i] - n.m0[i]) * r, e1r += (n.m2[i] - n.m1[i]) * r;
        }
        const float inr = 1.f / fmaxf(sqrtf(rr), NORM_EPS), p0 = e0r * inr, p1 = e1r * inr;
        v[0] += sqrtf(aa);
        v[1] += p0 * p0 + p1 * p1;
      }
      const float s0 = scales[(size_t)g * 3], s1 = scales[(size_t)g * 3 + 1], s2 = scales[(size_t)g * 3 + 2];
      const float mean = (s0 + s1 + s2) * (1.f / 3.f), d0 = s0 - mean, d1 = s1 - mean, d2 = s2 - mean;
      v[2] = 0.5f * (d0 * d0 + d1 * d1 + d2 * d2);
    }
  } else {
    const int row = ((int)blockIdx.x - gblocks) * MB + tid;
    if (row < K * (T - 2)) {
      const int k = row / (T - 2), tau = 1 + row - k * (T - 2);
      float a[6];
      v[0] = accel_row<6>(rots, k, T, tau, a);
      v[1] = accel_row<3>(transls, k, T, tau, a);
    }
  }
  wave_sum_store(v, red, wave * 4, lane);
  __syncthreads();
  if (tid < 3) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < MB / 64; w++) s += (double)red[w * 4 + tid];
    partials[(size_t)blockIdx.x * PARTIAL_DOUBLES + tid] = s;
  }
}

// one block adds the block partials in block order (a fixed tree) and scales them into the four values
__global__ void __launch_bounds__(MB) k_motion_finish(const double *__restrict__ partials, int gblocks, int bblocks, int G, int K, int T,
                                                      int B, float w_rot, float w_transl, float *__restrict__ out) {
  double g[3], b[2];  // tracks, z, scale | bases rots, transls
  ordered_total(partials, gblocks, PARTIAL_DOUBLES, g);
  ordered_total(partials + (size_t)gblocks * PARTIAL_DOUBLES, bblocks, PARTIAL_DOUBLES, b);
  if (threadIdx.x == 0) {
    const double gb = (double)G * (double)B, rows = (double)K * (double)(T - 2);
    out[0] = (float)(((double)w_rot * b[0] + (double)w_transl * b[1]) / rows);
    out[1] = (float)(0.5 * g[0] / gb);
    out[2] = (float)(g[1] / gb);
    out[3] = (float)(g[2] / (double)G);
  }
}

// one lane per Gaussian: v_points [3B,G,3] (the gradient of the neighbour means) and v_scales [G,3]; every address has one writer
__global__ void __launch_bounds__(MB) k_motion_loss_bwd(const float *__restrict__ means_nb, const float *__restrict__ centres,
                                                        const float *__restrict__ scales, const float *__restrict__ v_out, int G, int B,
                                                        float *__restrict__ v_points, float *__restrict__ v_scales) {
  const int g = blockIdx.x * MB + threadIdx.x;
  if (g >= G) return;
  const float inv_gb = 1.f / ((float)G * (float)B);
  const float w_st = 0.5f * v_out[1] * inv_gb, w_z = 2.f * v_out[2] * inv_gb, w_sv = v_out[3] / (float)G;
  for (int b = 0; b < B; b++) {
    const Nb3 n = load_nb(means_nb, G, B, g, b);
    float a[3], r[3], e0[3], e1[3], aa = 0.f, rr = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      a[i] = 2.f * n.m1[i] - n.m0[i] - n.m2[i], r[i] = n.m1[i] - centres[b * 3 + i];
      e0[i] = n.m1[i] - n.m0[i], e1[i] = n.m2[i] - n.m1[i];
      aa += a[i] * a[i], rr += r[i] * r[i];
    }
    const float na = sqrtf(aa), nr = sqrtf(rr);
    const float ua = na > 0.f ? w_st / na : 0.f;  // the gradient of a norm at zero is zero
    const float inr = 1.f / fmaxf(nr, NORM_EPS);
    float d[3], p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] = r[i] * inr, p0 += e0[i] * d[i], p1 += e1[i] * d[i];
    const float g0 = w_z * p0, g1 = w_z * p1;  // dL/dp0, dL/dp1
    // d = r / max(|r|, eps): above the clamp v_r = (v_d - d (d.v_d)) / |r|, at or below it v_d / eps
    float vd[3], dvd = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) vd[i] = g0 * e0[i] + g1 * e1[i], dvd += d[i] * vd[i];
    if (!(nr >= NORM_EPS)) dvd = 0.f;
    float *q0 = v_points + ((size_t)b * G + g) * 3, *q1 = v_points + ((size_t)(B + b) * G + g) * 3,
          *q2 = v_points + ((size_t)(2 * B + b) * G + g) * 3;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const float vr = (vd[i] - d[i] * dvd) * inr, ta = ua * a[i];
      q0[i] = -ta - g0 * d[i];
      q1[i] = 2.f * ta + (g0 - g1) * d[i] + vr;
      q2[i] = -ta + g1 * d[i];
    }
  }
  const float s0 = scales[(size_t)g * 3], s1 = scales[(size_t)g * 3 + 1], s2 = scales[(size_t)g * 3 + 2];
  const float mean = (s0 + s1 + s2) * (1.f / 3.f);
  v_scales[(size_t)g * 3] = w_sv * (s0 - mean), v_scales[(size_t)g * 3 + 1] = w_sv * (s1 - mean), v_scales[(size_t)g * 3 + 2] = w_sv * (s2 - mean);
}

// u_tau = a_tau / |a_tau| (0 at zero norm and outside 1 .. T-2), scaled by s and added to acc
template <int D>
__device__ __forceinline__ void add_unit_accel(const float *__restrict__ x, int k, int T, int tau, float s, float *acc) {
  if (tau < 1 || tau > T - 2) return;
  float a[D];
  const float n = accel_row<D>(x, k, T, tau, a);
  if (!(n > 0.f)) return;
  const float f = s / n;
#pragma unroll
  for (int i = 0; i < D; i++) acc[i] += f * a[i];
}
// the bases' own gradient as a gather, one lane per (k, tau): v_x[k,tau] += c (2 u_tau - u_{tau-1} - u_{tau+1})
__global__ void __launch_bounds__(MB) k_motion_bases_bwd(const float *__restrict__ rots, const float *__restrict__ transls,
                                                         const float *__restrict__ v_out, int K, int T, float w_rot, float w_transl,
                                                         float *__restrict__ v_rots, float *__restrict__ v_transls) {
  const int i = blockIdx.x * MB + threadIdx.x;
  if (i >= K * T) return;
  const int k = i / T, tau = i - k * T;
  const float c = v_out[0] / ((float)K * (float)(T - 2));
  float gr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gt[3] = {0.f, 0.f, 0.f};
  add_unit_accel<6>(rots, k, T, tau, 2.f, gr), add_unit_accel<6>(rots, k, T, tau - 1, -1.f, gr), add_unit_accel<6>(rots, k, T, tau + 1, -1.f, gr);
  add_unit_accel<3>(transls, k, T, tau, 2.f, gt), add_unit_accel<3>(transls, k, T, tau - 1, -1.f, gt), add_unit_accel<3>(transls, k, T, tau + 1, -1.f, gt);
#pragma unroll
  for (int j = 0; j < 6; j++) v_rots[(size_t)i * 6 + j] += c * w_rot * gr[j];
#pragma unroll
  for (int j = 0; j < 3; j++) v_transls[(size_t)i * 3 + j] += c * w_transl * gt[j];
}

// sizes the entry points take: the index arithmetic of every kernel here and of the pose kernels stays inside 32 bits
bool motion_sizes_ok(int G, int K, int T, int B) {
  return G > 0 && B > 0 && K >= 1 && K <= D4GS_MAX_K && T >= 3 && (int64_t)9 * B * G <= INT32_MAX && (int64_t)9 * K * T <= INT32_MAX;
}

// host arithmetic only: no HIP call is made before every argument has passed.  Leaves the workspace layout in *ws.
int motion_check(const char *who, const void *const *ptrs, int n_ptrs, int G, int K, int T, int B, const void *workspace,
                 size_t workspace_bytes, MotionWs *ws) {
  for (int i = 0; i < n_ptrs; i++)
    if (!ptrs[i]) {
      d4gs_set_error("%s: NULL argument %d", who, i);
      return D4GS_EINVAL;
    }
  if (!motion_sizes_ok(G, K, T, B)) {
    d4gs_set_error("%s: bad size G=%d K=%d T=%d B=%d (G >= 1, 1 <= K <= %d, T >= 3: no interior frame otherwise, B >= 1, 9 B G and "
                   "9 K T <= 2^31 - 1)", who, G, K, T, B, D4GS_MAX_K);
    return D4GS_EINVAL;
  }
  *ws = motion_ws(G, K, T, B);
  const size_t need = ws->total;
  if (workspace_bytes < need || (uintptr_t)workspace % 16) {
    d4gs_set_error("%s: workspace of %zu bytes (16-byte aligned) needed, %zu given at %p", who, need, workspace_bytes, workspace);
    return D4GS_EINVAL;
  }
  return D4GS_OK;
}

D4gsProjIn pose_in(const float *means, const float *motion_coefs, const float *rots, const float *transls, const float *times) {
  D4gsProjIn in{};
  in.means = means, in.motion_coefs = motion_coefs, in.rots = rots, in.transls = transls, in.times = times;
  return in;
}

}  // namespace

extern "C" {

size_t d4gs_motion_regs_workspace_bytes(int32_t G, int32_t K, int32_t T, int32_t B) {
  if (!motion_sizes_ok(G, K, T, B)) return 0;
  return motion_ws(G, K, T, B).total;
}

int d4gs_motion_regs_fwd(const float *means, const float *motion_coefs, const float *scales, const float *rots, const float *transls,
                         const float *ts, const float *w2cs, int32_t G, int32_t K, int32_t T, int32_t B, float weight_rot,
                         float weight_transl, void *workspace, size_t workspace_bytes, float *out, void *stream) {
  const void *ptrs[] = {means, motion_coefs, scales, rots, transls, ts, w2cs, workspace, out};
  MotionWs w;
  if (int rc = motion_check("d4gs_motion_regs_fwd", ptrs, 9, G, K, T, B, workspace, workspace_bytes, &w)) return rc;
  char *base = (char *)workspace;
  float *times_nb = (float *)(base + w.times), *centres = (float *)(base + w.centres), *means_nb = (float *)(base + w.means_nb);
  double *partials = (double *)(base + w.partials);
  hipStream_t s = (hipStream_t)stream;
  D4GS_LAUNCH("k_motion_prep", k_motion_prep, dim3((3 * B + MB - 1) / MB), dim3(MB), 0, s, ts, w2cs, (int)B, (int)T, times_nb, centres);
  if (int rc = d4gs_check_launch("k_motion_prep")) return rc;
  const D4gsDims d = pose_dims(G, K, T, B);
  const D4gsProjIn in = pose_in(means, motion_coefs, rots, transls, times_nb);
  const D4gsPoses po = {means_nb, nullptr, nullptr, 0};
  if (int rc = d4gs_poses_fwd_impl(&d, &in, &po, s)) return rc;
  D4GS_LAUNCH("k_motion_loss_fwd", k_motion_loss_fwd, dim3(w.gblocks + w.bblocks), dim3(MB), 0, s, (const float *)means_nb,
              (const float *)centres, scales, rots, transls, (int)G, (int)K, (int)T, (int)B, w.gblocks, partials);
  if (int rc = d4gs_check_launch("k_motion_loss_fwd")) return rc;
  D4GS_LAUNCH("k_motion_finish", k_motion_finish, dim3(1), dim3(MB), 0, s, (const double *)partials, w.gblocks, w.bblocks, (int)G, (int)K,
              (int)T, (int)B, weight_rot, weight_transl, out);
  return d4gs_check_launch("k_motion_finish");
}

int d4gs_motion_regs_bwd(const float *means, const float *motion_coefs, const float *scales, const float *rots, const float *transls,
                         int32_t G, int32_t K, int32_t T, int32_t B, float weight_rot, float weight_transl, void *workspace,
                         size_t workspace_bytes, const float *v_out, const D4gsLeafGrads *grads, void *stream) {
  const void *ptrs[] = {means, motion_coefs, scales, rots, transls, workspace, v_out, grads,
                        grads ? grads->v_means : nullptr, grads ? grads->v_motion_coefs : nullptr, grads ? grads->v_scales : nullptr,
                        grads ? grads->v_rots : nullptr, grads ? grads->v_transls : nullptr};
  MotionWs w;
  if (int rc = motion_check("d4gs_motion_regs_bwd", ptrs, 13, G, K, T, B, workspace, workspace_bytes, &w)) return rc;
  char *base = (char *)workspace;
  const float *times_nb = (const float *)(base + w.times), *centres = (const float *)(base + w.centres),
              *means_nb = (const float *)(base + w.means_nb);
  float *v_points = (float *)(base + w.v_points);
  hipStream_t s = (hipStream_t)stream;
  D4GS_LAUNCH("k_motion_loss_bwd", k_motion_loss_bwd, dim3(w.gblocks), dim3(MB), 0, s, means_nb, centres, scales, v_out, (int)G, (int)B,
              v_points, grads->v_scales);
  if (int rc = d4gs_check_launch("k_motion_loss_bwd")) return rc;
  const D4gsDims d = pose_dims(G, K, T, B);
  const D4gsProjIn in = pose_in(means, motion_coefs, rots, transls, times_nb);
  const D4gsPoses vo = {v_points, nullptr, nullptr, 0};
  D4gsLeafGrads lg{};
  lg.v_means = grads->v_means, lg.v_motion_coefs = grads->v_motion_coefs, lg.v_rots = grads->v_rots, lg.v_transls = grads->v_transls;
  lg.partials = (float *)(base + w.pose_partials);
  if (int rc = d4gs_poses_bwd_impl(&d, &in, &vo, &lg, s)) return rc;  // overwrites v_rots / v_transls: the bases' own term comes behind it
  D4GS_LAUNCH("k_motion_bases_bwd", k_motion_bases_bwd, dim3((K * T + MB - 1) / MB), dim3(MB), 0, s, rots, transls, v_out, (int)K, (int)T,
              weight_rot, weight_transl, grads->v_rots, grads->v_transls);
  return d4gs_check_launch("k_motion_bases_bwd");
}

}  // extern "C"
