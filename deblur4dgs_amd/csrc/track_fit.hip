// track_fit.hip -- the warm-up fit of a tracked scene (flow3d/init_utils.py:273-402, run_initial_optim; include/d4gs.h, "Track
// fit"): the six terms of its loss from ONE deformation per (Gaussian, frame), their adjoint, and the schedule that
// moves four learning rates and the smoothness weight every iteration - all of it readable by a captured HIP graph.
//   out[1] track_3d       sum w3 mean_3 |p - xyz| / (sum w3 + 1e-8)                       p[g,tau] = the deformed mean at frame tau
//   out[2] track_2d       masked_l1_loss(proj(p), proj(xyz), w2, quantile) / Ks[0,0,0]    (trimmed.hip's selection over all G T errors)
//   out[3] coef_sparse    1 - mean_g sum_k softmax(motion_coefs_g)_k^2
//   out[4] smooth_bases   mean |2 rots[k,tau] - rots[k,tau-1] - rots[k,tau+1]| + 2 (the same on transls)
//   out[5] smooth_tracks  mean_{g, 1 <= tau <= T-2} |2 p_tau - p_{tau-1} - p_{tau+1}|
//   out[6] z_accel        compute_z_acc_loss over b = 0 .. T-1 at the neighbour frames clamp(b, 1, T-2) + {-1, 0, 1}, ray to camera b
//   out[0] sum_k weights[k] out[1 + k] with the weights the schedule step left in device memory
// The deformation and its adjoint are the pose kernels (k_poses_fwd / MODE_POSES of k_project_bwd: N = G, time-major, S = T, the
// times 0 .. T-1): the neighbour frames of the two acceleration terms ARE frames of the same table, so nothing is deformed twice.
//
// Mapping.  One lane per Gaussian, gridDim.y = ceil(T / FIT_CHUNK) chunks of frames: a block reads its chunk's frames and one (the
// adjoint: two) frame of halo on either side, every load coalesced over g.  G = 40 000, T = 24: 157 x 6 blocks = 3 768 waves.
// No atomics: every sum is per block (reduce.h), then added in block order by one block, in double; every gradient address has one
// writer - a frame GATHERS what its own terms and its neighbours' second differences send it.  The same input gives the same bits
// on every run and every graph replay.  The gradient of |x| at 0 and of a norm at exactly zero is zero (torch's convention).
#include <math.h>

#include "common.h"
#include "reduce.h"

namespace {

constexpr int FB = REDUCE_NT;     // threads per block, every kernel
constexpr int FIT_CHUNK = 4;      // frames per block
constexpr int PD = 6;             // per-block partial sums: 3-D, track accel, z accel, coef^2 | bases rots, bases transls
constexpr int CAM = 24;           // floats per frame of the camera table: A [9], t [3], Ks [9], centre [3]
constexpr float NORM_EPS = 1e-12f;  // F.normalize's clamp on the norm
constexpr float Z_MIN = 1e-5f;      // project_2d_tracks' clamp on the depth
enum { W_3D = 0, W_2D, W_COEF, W_BASES, W_TRACKS, W_Z, N_TERMS };

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// the prepared data (K does not enter) and the per-call workspace, in bytes; every part 16-byte aligned
struct FitData {
  size_t times, cams, consts, xyz, gt2d, w3, w2, w3_partials, total;
  int gblocks;
};
struct FitWs {
  size_t points, v_points, v_coefs, trim, trim_out, partials, pose_partials, total;
  int gblocks, bblocks, chunks;
};

bool data_sizes_ok(int G, int T) { return G >= 1 && T >= 3 && T <= 65535 && (int64_t)9 * T * G <= INT32_MAX; }
bool fit_sizes_ok(int G, int K, int T) {
  return data_sizes_ok(G, T) && K >= 1 && K <= D4GS_MAX_K && (int64_t)9 * K * T <= INT32_MAX && (int64_t)G * K <= INT32_MAX;
}

FitData fit_data(int G, int T) {
  FitData d;
  const size_t gt = (size_t)G * T;
  d.gblocks = (G + FB - 1) / FB;
  size_t o = 0;
  d.times = o, o = align16(o + sizeof(float) * T);
  d.cams = o, o = align16(o + sizeof(float) * CAM * T);
  d.consts = o, o = align16(o + sizeof(double) * 2);  // sum w3, 1 / fx
  d.xyz = o, o = align16(o + sizeof(float) * 3 * gt);
  d.gt2d = o, o = align16(o + sizeof(float) * 2 * gt);
  d.w3 = o, o = align16(o + sizeof(float) * gt);
  d.w2 = o, o = align16(o + sizeof(float) * gt);
  d.w3_partials = o, o = align16(o + sizeof(double) * (size_t)d.gblocks * T);
  d.total = o;
  return d;
}

D4gsDims pose_dims(int G, int K, int T) {
  D4gsDims d{};
  d.N = G, d.G = G, d.K = K, d.T = T, d.S = T, d.D = 1, d.width = 16, d.height = 16;
  d.flags = D4GS_RAW_PARAMS;  // motion_coefs are the raw leaf: softmax inside
  d.near_plane = 0.01f, d.far_plane = 1e10f, d.eps2d = 0.3f;
  return d;
}

FitWs fit_ws(int G, int K, int T) {
  FitWs w;
  const size_t gt = (size_t)G * T;
  w.gblocks = (G + FB - 1) / FB;
  w.bblocks = (K * (T - 2) + FB - 1) / FB;
  w.chunks = (T + FIT_CHUNK - 1) / FIT_CHUNK;
  const D4gsDims d = pose_dims(G, K, T);
  size_t o = 0;
  w.points = o, o = align16(o + sizeof(float) * 3 * gt);
  w.v_points = o, o = align16(o + sizeof(float) * 3 * gt);
  w.v_coefs = o, o = align16(o + sizeof(float) * (size_t)G * K);
  w.trim = o, o = align16(o + sizeof(uint32_t) * (size_t)d4gs_trimmed_scratch_words((int64_t)gt, 1));
  w.trim_out = o, o = align16(o + sizeof(float) * 8);
  w.partials = o, o = align16(o + sizeof(double) * PD * (size_t)(w.gblocks + w.bblocks) * w.chunks);
  w.pose_partials = o, o = align16(o + sizeof(float) * d4gs_poses_bwd_partials_bound(&d));
  w.total = o;
  return w;
}

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// proj(x, tau): c = A x + t; v = Ks c; uv = v.xy / max(v.z, 1e-5)
struct Proj {
  float u, v, z, vz;  // z the clamped depth, vz the depth before the clamp
};
__device__ __forceinline__ Proj project(const float *__restrict__ cam, const float *x) {
  float c[3], q[3];
#pragma unroll
  for (int r = 0; r < 3; r++) c[r] = cam[r * 3] * x[0] + cam[r * 3 + 1] * x[1] + cam[r * 3 + 2] * x[2] + cam[9 + r];
#pragma unroll
  for (int r = 0; r < 3; r++) q[r] = cam[12 + r * 3] * c[0] + cam[12 + r * 3 + 1] * c[1] + cam[12 + r * 3 + 2] * c[2];
  Proj p;
  p.vz = q[2], p.z = fmaxf(q[2], Z_MIN);
  p.u = q[0] / p.z, p.v = q[1] / p.z;
  return p;
}

// ---- prepare -----------------------------------------------------------------------------------------------------------------
// grid (gblocks, T): lane (g, tau) moves xyz and the two weights to the time-major planes, projects xyz and leaves its block's
// sum of w3 (double, reduce.h's block sum)
__global__ void __launch_bounds__(FB) k_fit_prepare(const float *__restrict__ xyz, const uint8_t *__restrict__ visibles,
                                                    const uint8_t *__restrict__ invisibles, const float *__restrict__ conf,
                                                    const float *__restrict__ Ks, const float *__restrict__ w2cs, int G, int T,
                                                    float *__restrict__ xyz_t, float *__restrict__ gt2d, float *__restrict__ w3,
                                                    float *__restrict__ w2, double *__restrict__ w3_partials) {
  __shared__ double red[4];
  const int tau = blockIdx.y, g = blockIdx.x * FB + threadIdx.x;
  double s[1] = {0.0};
  if (g < G) {
    float cam[21];
    const float *M = w2cs + (size_t)tau * 16, *Km = Ks + (size_t)tau * 9;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
      for (int c = 0; c < 3; c++) cam[r * 3 + c] = M[r * 4 + c], cam[12 + r * 3 + c] = Km[r * 3 + c];
      cam[9 + r] = M[r * 4 + 3];
    }
    const size_t in = (size_t)g * T + tau, o = (size_t)tau * G + g;
    const float x[3] = {xyz[in * 3], xyz[in * 3 + 1], xyz[in * 3 + 2]};
    const Proj p = project(cam, x);
    const float cf = conf[in], a = visibles[in] ? cf : 0.f, b = invisibles[in] ? cf : 0.f;
    xyz_t[o * 3] = x[0], xyz_t[o * 3 + 1] = x[1], xyz_t[o * 3 + 2] = x[2];
    gt2d[o * 2] = p.u, gt2d[o * 2 + 1] = p.v;
    w3[o] = a, w2[o] = b;
    s[0] = (double)a;
  }
  block_sum_store(s, red);
  __syncthreads();
  if (threadIdx.x == 0) w3_partials[(size_t)tau * gridDim.x + blockIdx.x] = block_sum_combine<1>(red, 0);
}

// one block: the frame times 0 .. T-1, the camera table (centre_b = -A^-1 t by the cofactor inverse, A any invertible 3x3), the
// ordered total of w3 and 1 / fx
__global__ void __launch_bounds__(FB) k_fit_prepare_finish(const float *__restrict__ Ks, const float *__restrict__ w2cs, int T,
                                                           const double *__restrict__ w3_partials, int n_partials,
                                                           float *__restrict__ times, float *__restrict__ cams, double *__restrict__ consts) {
  for (int i = threadIdx.x; i < T; i += FB) {
    const float *M = w2cs + (size_t)i * 16, *Km = Ks + (size_t)i * 9;
    float *cam = cams + (size_t)i * CAM;
    const float a00 = M[0], a01 = M[1], a02 = M[2], a10 = M[4], a11 = M[5], a12 = M[6], a20 = M[8], a21 = M[9], a22 = M[10];
    const float t0 = M[3], t1 = M[7], t2 = M[11];
    const float c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const float c10 = a02 * a21 - a01 * a22, c11 = a00 * a22 - a02 * a20, c12 = a01 * a20 - a00 * a21;
    const float c20 = a01 * a12 - a02 * a11, c21 = a02 * a10 - a00 * a12, c22 = a00 * a11 - a01 * a10;
    const float inv = 1.f / (a00 * c00 + a01 * c01 + a02 * c02);
    cam[0] = a00, cam[1] = a01, cam[2] = a02, cam[3] = a10, cam[4] = a11, cam[5] = a12, cam[6] = a20, cam[7] = a21, cam[8] = a22;
    cam[9] = t0, cam[10] = t1, cam[11] = t2;
#pragma unroll
    for (int j = 0; j < 9; j++) cam[12 + j] = Km[j];
    cam[21] = -(c00 * t0 + c10 * t1 + c20 * t2) * inv;
    cam[22] = -(c01 * t0 + c11 * t1 + c21 * t2) * inv;
    cam[23] = -(c02 * t0 + c12 * t1 + c22 * t2) * inv;
    times[i] = (float)i;
  }
  double tot[1];
  ordered_total(w3_partials, (int64_t)n_partials, (int64_t)1, tot);
  if (threadIdx.x == 0) consts[0] = tot[0], consts[1] = 1.0 / (double)Ks[0];
}

// ---- forward -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load3(const float *__restrict__ points, int G, int g, int tau, float *p) {
  const float *q = points + ((size_t)tau * G + g) * 3;
  p[0] = q[0], p[1] = q[1], p[2] = q[2];
}

// the two squared ray projections of compute_z_acc_loss for the neighbour frames (m0, m1, m2) and the centre c
__device__ __forceinline__ float z_pair(const float *m0, const float *m1, const float *m2, const float *c) {
  float rr = 0.f, e0r = 0.f, e1r = 0.f;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float r = m1[i] - c[i];
    rr += r * r, e0r += (m1[i] - m0[i]) * r, e1r += (m2[i] - m1[i]) * r;
  }
  const float inr = 1.f / fmaxf(sqrtf(rr), NORM_EPS), p0 = e0r * inr, p1 = e1r * inr;
  return p0 * p0 + p1 * p1;
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

// softmax(motion_coefs_g) as the pose kernels form it; -> sum_k s_k^2, and 1 / sum exp and the maximum for a second pass
__device__ __forceinline__ float coef_square_sum(const float *__restrict__ mc, int K, float &m, float &is) {
  m = -INFINITY;
  for (int k = 0; k < K; k++) m = fmaxf(m, mc[k]);
  float sum = 0.f;
  for (int k = 0; k < K; k++) sum += expf(mc[k] - m);
  is = 1.f / sum;
  float ss = 0.f;
  for (int k = 0; k < K; k++) {
    const float s = expf(mc[k] - m) * is;
    ss += s * s;
  }
  return ss;
}

// blocks x < gblocks: one lane per Gaussian over the frames of chunk y; blocks x >= gblocks (chunk 0 only): one lane per basis row.
// Every block writes its PD partials (zeros where it has nothing), so nothing is zeroed beforehand.
__global__ void __launch_bounds__(FB) k_fit_loss_fwd(const float *__restrict__ points, const float *__restrict__ xyz_t,
                                                     const float *__restrict__ gt2d, const float *__restrict__ w3,
                                                     const float *__restrict__ cams, const float *__restrict__ motion_coefs,
                                                     const float *__restrict__ rots, const float *__restrict__ transls, int G, int K,
                                                     int T, int gblocks, float *__restrict__ values, double *__restrict__ partials) {
  __shared__ float red[4 * PD];
  const int tid = threadIdx.x;
  float v[PD] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if ((int)blockIdx.x < gblocks) {
    const int g = blockIdx.x * FB + tid;
    if (g < G) {
      const int t0 = blockIdx.y * FIT_CHUNK, t1 = min(T, t0 + FIT_CHUNK);
      for (int tau = t0; tau < t1; tau++) {
        const size_t o = (size_t)tau * G + g;
        const float *cam = cams + (size_t)tau * CAM;
        float p1[3];
        load3(points, G, g, tau, p1);
        v[0] += w3[o] * ((fabsf(p1[0] - xyz_t[o * 3]) + fabsf(p1[1] - xyz_t[o * 3 + 1]) + fabsf(p1[2] - xyz_t[o * 3 + 2])) / 3.f);
        const Proj pr = project(cam, p1);
        values[o] = 0.5f * (fabsf(pr.u - gt2d[o * 2]) + fabsf(pr.v - gt2d[o * 2 + 1]));
        if (tau >= 1 && tau <= T - 2) {
          float p0[3], p2[3], aa = 0.f;
          load3(points, G, g, tau - 1, p0), load3(points, G, g, tau + 1, p2);
#pragma unroll
          for (int i = 0; i < 3; i++) {
            const float a = 2.f * p1[i] - p0[i] - p2[i];
            aa += a * a;
          }
          v[1] += sqrtf(aa);
          // the cameras b with clamp(b, 1, T-2) == tau: tau itself, 0 with frame 1, T-1 with frame T-2
          v[2] += z_pair(p0, p1, p2, cam + 21);
          if (tau == 1) v[2] += z_pair(p0, p1, p2, cams + 21);
          if (tau == T - 2) v[2] += z_pair(p0, p1, p2, cams + (size_t)(T - 1) * CAM + 21);
        }
      }
      if (blockIdx.y == 0) {
        float m, is;
        v[3] = coef_square_sum(motion_coefs + (size_t)g * K, K, m, is);
      }
    }
  } else if (blockIdx.y == 0) {
    const int row = ((int)blockIdx.x - gblocks) * FB + tid;
    if (row < K * (T - 2)) {
      const int k = row / (T - 2), tau = 1 + row - k * (T - 2);
      float a[6];
      v[4] = accel_row<6>(rots, k, T, tau, a);
      v[5] = accel_row<3>(transls, k, T, tau, a);
    }
  }
  block_sum_store(v, red);
  __syncthreads();
  if (tid < PD) partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * PD + tid] = (double)block_sum_combine<PD>(red, tid);
}

// one block: the ordered total of the block partials, the trimmed 2-D sum of trimmed.hip, the weights -> out[8] and the history row
__global__ void __launch_bounds__(FB) k_fit_finish(const double *__restrict__ partials, int n_partials, const float *__restrict__ trim_out,
                                                   const double *__restrict__ consts, const float *__restrict__ weights, int G, int K, int T,
                                                   float *__restrict__ out, const int32_t *__restrict__ iter, float *__restrict__ losses,
                                                   int num_iters) {
  double s[PD];
  ordered_total(partials, (int64_t)n_partials, (int64_t)PD, s);
  if (threadIdx.x == 0) {
    const double inner = (double)(T - 2);
    double term[N_TERMS];
    term[W_3D] = s[0] / (consts[0] + 1e-8);
    term[W_2D] = (double)trim_out[0] * consts[1];
    term[W_COEF] = 1.0 - s[3] / (double)G;
    term[W_BASES] = (s[4] + 2.0 * s[5]) / ((double)K * inner);
    term[W_TRACKS] = s[1] / ((double)G * inner);
    term[W_Z] = s[2] / ((double)G * (double)T);
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < N_TERMS; k++) {
      const float tk = (float)term[k];
      out[1 + k] = tk;
      total += (weights ? (double)weights[k] : 1.0) * (double)tk;
    }
    out[0] = (float)total;
    out[7] = trim_out[1];  // the 2-D term's threshold
    if (losses) {  // the history row of the iteration the schedule step has just counted: *iter is already its index + 1
      const int row = *iter - 1;
      if (row >= 0 && row < num_iters)
#pragma unroll
        for (int k = 0; k < 1 + N_TERMS; k++) losses[(size_t)row * (1 + N_TERMS) + k] = out[k];
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------
// u_j = a_j / |a_j| of the track acceleration at the interior frame j (0 at zero norm and outside 1 .. T-2), scaled by s, added
__device__ __forceinline__ void add_unit_track_accel(const float *__restrict__ points, int G, int g, int T, int j, float s, float *acc) {
  if (j < 1 || j > T - 2) return;
  float p0[3], p1[3], p2[3], a[3], aa = 0.f;
  load3(points, G, g, j - 1, p0), load3(points, G, g, j, p1), load3(points, G, g, j + 1, p2);
#pragma unroll
  for (int i = 0; i < 3; i++) a[i] = 2.f * p1[i] - p0[i] - p2[i], aa += a[i] * a[i];
  const float n = sqrtf(aa);
  if (!(n > 0.f)) return;
  const float f = s / n;
#pragma unroll
  for (int i = 0; i < 3; i++) acc[i] += f * a[i];
}

// what the z-acceleration pair of the interior frame j and the camera centre c sends to frame j + which (which = -1, 0, 1)
__device__ __forceinline__ void add_z_pair(const float *m0, const float *m1, const float *m2, const float *__restrict__ c, float w_z,
                                           int which, float *acc) {
  float r[3], e0[3], e1[3], rr = 0.f;
#pragma unroll
  for (int i = 0; i < 3; i++) r[i] = m1[i] - c[i], e0[i] = m1[i] - m0[i], e1[i] = m2[i] - m1[i], rr += r[i] * r[i];
  const float nr = sqrtf(rr), inr = 1.f / fmaxf(nr, NORM_EPS);
  float d[3], p0 = 0.f, p1 = 0.f;
#pragma unroll
  for (int i = 0; i < 3; i++) d[i] = r[i] * inr, p0 += e0[i] * d[i], p1 += e1[i] * d[i];
  const float g0 = w_z * p0, g1 = w_z * p1;
  if (which < 0) {
#pragma unroll
    for (int i = 0; i < 3; i++) acc[i] += -g0 * d[i];
  } else if (which > 0) {
#pragma unroll
    for (int i = 0; i < 3; i++) acc[i] += g1 * d[i];
  } else {
    // d = r / max(|r|, eps): above the clamp v_r = (v_d - d (d.v_d)) / |r|, at or below it v_d / eps
    float vd[3], dvd = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) vd[i] = g0 * e0[i] + g1 * e1[i], dvd += d[i] * vd[i];
    if (!(nr >= NORM_EPS)) dvd = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) acc[i] += (g0 - g1) * d[i] + (vd[i] - d[i] * dvd) * inr;
  }
}
// every camera of the interior frame j (tau itself, 0 with frame 1, T-1 with frame T-2), in the forward's order
__device__ __forceinline__ void add_z_frame(const float *__restrict__ points, const float *__restrict__ cams, int G, int g, int T, int j,
                                            float w_z, int which, float *acc) {
  if (j < 1 || j > T - 2) return;
  float m0[3], m1[3], m2[3];
  load3(points, G, g, j - 1, m0), load3(points, G, g, j, m1), load3(points, G, g, j + 1, m2);
  add_z_pair(m0, m1, m2, cams + (size_t)j * CAM + 21, w_z, which, acc);
  if (j == 1) add_z_pair(m0, m1, m2, cams + 21, w_z, which, acc);
  if (j == T - 2) add_z_pair(m0, m1, m2, cams + (size_t)(T - 1) * CAM + 21, w_z, which, acc);
}

// grid (gblocks, chunks): v_points [T,G,3], one writer per address; chunk 0 also writes the coefficient term's own v_coefs [G,K]
__global__ void __launch_bounds__(FB) k_fit_loss_bwd(const float *__restrict__ points, const float *__restrict__ xyz_t,
                                                     const float *__restrict__ gt2d, const float *__restrict__ w3, const float *__restrict__ w2,
                                                     const float *__restrict__ cams, const double *__restrict__ consts,
                                                     const float *__restrict__ values, const float *__restrict__ trim_out,
                                                     const float *__restrict__ motion_coefs, const float *__restrict__ v_out, int G, int K, int T,
                                                     int keep_all, float *__restrict__ v_points, float *__restrict__ v_coefs) {
  const int g = blockIdx.x * FB + threadIdx.x;
  if (g >= G) return;
  const float s3 = (float)((double)v_out[W_3D] / (consts[0] + 1e-8) / 3.0);
  const float s2 = (float)((double)v_out[W_2D] * consts[1] * (double)trim_out[2] * 0.5), thr = trim_out[1];
  const float c_st = v_out[W_TRACKS] / ((float)G * (float)(T - 2)), w_z = 2.f * v_out[W_Z] / ((float)G * (float)T);
  const int t0 = blockIdx.y * FIT_CHUNK, t1 = min(T, t0 + FIT_CHUNK);
  for (int tau = t0; tau < t1; tau++) {
    const size_t o = (size_t)tau * G + g;
    const float *cam = cams + (size_t)tau * CAM;
    float p[3], gx[3];
    load3(points, G, g, tau, p);
    const float a3 = s3 * w3[o];
#pragma unroll
    for (int i = 0; i < 3; i++) gx[i] = a3 * sgn(p[i] - xyz_t[o * 3 + i]);
    const float e = values[o];
    if (keep_all ? e == e : e < thr) {
      const Proj pr = project(cam, p);
      const float c = s2 * w2[o];
      const float gu = c * sgn(pr.u - gt2d[o * 2]), gv = c * sgn(pr.v - gt2d[o * 2 + 1]);
      // torch.clamp(min) passes the gradient where its input is >= the bound
      const float q[3] = {gu / pr.z, gv / pr.z, pr.vz >= Z_MIN ? -(gu * pr.u + gv * pr.v) / pr.z : 0.f};
      float vc[3];
#pragma unroll
      for (int j = 0; j < 3; j++) vc[j] = cam[12 + j] * q[0] + cam[15 + j] * q[1] + cam[18 + j] * q[2];  // Ks^T
#pragma unroll
      for (int j = 0; j < 3; j++) gx[j] += cam[j] * vc[0] + cam[3 + j] * vc[1] + cam[6 + j] * vc[2];  // A^T
    }
    add_unit_track_accel(points, G, g, T, tau, 2.f * c_st, gx);
    add_unit_track_accel(points, G, g, T, tau - 1, -c_st, gx);
    add_unit_track_accel(points, G, g, T, tau + 1, -c_st, gx);
    add_z_frame(points, cams, G, g, T, tau, w_z, 0, gx);
    add_z_frame(points, cams, G, g, T, tau + 1, w_z, -1, gx);  // tau is the frame before the interior frame tau + 1
    add_z_frame(points, cams, G, g, T, tau - 1, w_z, 1, gx);
    v_points[o * 3] = gx[0], v_points[o * 3 + 1] = gx[1], v_points[o * 3 + 2] = gx[2];
  }
  if (blockIdx.y == 0) {
    // d(1 - mean_g sum_k s_k^2) / d raw_j = -(2 / G) s_j (s_j - sum_k s_k^2)
    const float *mc = motion_coefs + (size_t)g * K;
    float m, is;
    const float ss = coef_square_sum(mc, K, m, is), c = -2.f * v_out[W_COEF] / (float)G;
    for (int k = 0; k < K; k++) {
      const float s = expf(mc[k] - m) * is;
      v_coefs[(size_t)g * K + k] = c * s * (s - ss);
    }
  }
}

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
// behind the pose adjoint (which overwrote the leaf gradients), ordered by the stream: the bases' own term as a gather, one lane per
// (k, tau), and the coefficient term, one lane per (g, k)
__global__ void __launch_bounds__(FB) k_fit_leaf_add(const float *__restrict__ rots, const float *__restrict__ transls,
                                                     const float *__restrict__ v_coefs, const float *__restrict__ v_out, int G, int K, int T,
                                                     float *__restrict__ v_rots, float *__restrict__ v_transls, float *__restrict__ v_motion_coefs) {
  const int i = blockIdx.x * FB + threadIdx.x;
  if (i < K * T) {
    const int k = i / T, tau = i - k * T;
    const float c = v_out[W_BASES] / ((float)K * (float)(T - 2));
    float gr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gt[3] = {0.f, 0.f, 0.f};
    add_unit_accel<6>(rots, k, T, tau, 2.f, gr), add_unit_accel<6>(rots, k, T, tau - 1, -1.f, gr), add_unit_accel<6>(rots, k, T, tau + 1, -1.f, gr);
    add_unit_accel<3>(transls, k, T, tau, 2.f, gt), add_unit_accel<3>(transls, k, T, tau - 1, -1.f, gt), add_unit_accel<3>(transls, k, T, tau + 1, -1.f, gt);
#pragma unroll
    for (int j = 0; j < 6; j++) v_rots[(size_t)i * 6 + j] += c * gr[j];
#pragma unroll
    for (int j = 0; j < 3; j++) v_transls[(size_t)i * 3 + j] += c * 2.f * gt[j];
  }
  if (i < G * K) v_motion_coefs[i] += v_coefs[i];
}

// ---- the schedule ------------------------------------------------------------------------------------------------------------
// iteration i of num_iters (kernel and CPU twin): ExponentialLR's closed form lr0 0.1^(i / num_iters) in double, and the six term
// weights with w_smooth_func(i, 0.01, 0.1, 400) evaluated in double in the reference's own order of operations
struct FitSchedule {
  double lr[4];
  float w[N_TERMS];
};
__host__ __device__ inline FitSchedule fit_schedule(int i, int num_iters, const double *lr0) {
#pragma clang fp contract(off)
  FitSchedule s;
  const double decay = pow(0.1, (double)i / (double)num_iters);
  for (int r = 0; r < 4; r++) s.lr[r] = lr0[r] * decay;
  const double min_v = 0.01, max_v = 0.1;
  // (num_iters <= 400 has no ramp: no iteration of it lies past 400, and a counter that has run past the end must not divide by <= 0)
  const double ws = i <= 400 || num_iters <= 400 ? min_v : (max_v - min_v) * (double)(i - 400) / (double)(num_iters - 400) + min_v;
  s.w[W_3D] = 1.f, s.w[W_2D] = 0.5f, s.w[W_COEF] = 0.01f, s.w[W_BASES] = (float)ws, s.w[W_TRACKS] = (float)(ws * 0.5), s.w[W_Z] = 0.1f;
  return s;
}

__global__ void __launch_bounds__(D4GS_WAVE) k_fit_schedule(int32_t *iter, int num_iters, D4gsAdamRec *table, double lr0, double lr1,
                                                            double lr2, double lr3, float *__restrict__ weights, float *__restrict__ lrs) {
  const int t = threadIdx.x, i = *iter;
  const double lr0s[4] = {lr0, lr1, lr2, lr3};
  const FitSchedule s = fit_schedule(i, num_iters, lr0s);
  __syncthreads();  // every lane has read *iter
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (t == r) {  // (selected, not indexed: the schedule stays in registers)
      table[r].lr = s.lr[r];
      if (lrs && i >= 0 && i < num_iters) lrs[(size_t)i * 4 + r] = (float)s.lr[r];
    }
#pragma unroll
  for (int k = 0; k < N_TERMS; k++)
    if (t == 8 + k) weights[k] = s.w[k];
  if (t == 63) *iter = i + 1;
}

int sched_check(const char *who, const int32_t *iter, int32_t num_iters, const D4gsAdamRec *table, const double *lr0, const float *weights,
                const float *lrs) {
  if (!iter || !table || !weights) {
    d4gs_set_error("%s: NULL argument (iter, table and weights are required)", who);
    return D4GS_EINVAL;
  }
  if ((uintptr_t)table % 8 || ((uintptr_t)iter | (uintptr_t)weights | (uintptr_t)lrs) % 4) {
    d4gs_set_error("%s: misaligned argument (table 8-byte, iter, weights and lrs 4-byte)", who);
    return D4GS_EINVAL;
  }
  if (num_iters < 1) {
    d4gs_set_error("%s: num_iters=%d (at least one iteration)", who, num_iters);
    return D4GS_EINVAL;
  }
  for (int r = 0; r < 4; r++)
    if (!(lr0[r] > 0.0) || !(lr0[r] < 1e300)) {
      d4gs_set_error("%s: lr0[%d]=%g (finite and > 0)", who, r, lr0[r]);
      return D4GS_EINVAL;
    }
  return D4GS_OK;
}

int fit_check(const char *who, const void *const *ptrs, int n_ptrs, int G, int K, int T, const void *targets, size_t targets_bytes,
              const void *workspace, size_t workspace_bytes, FitData *fd, FitWs *ws) {
  for (int i = 0; i < n_ptrs; i++)
    if (!ptrs[i]) {
      d4gs_set_error("%s: NULL argument %d", who, i);
      return D4GS_EINVAL;
    }
  if (!fit_sizes_ok(G, K, T)) {
    d4gs_set_error("%s: bad size G=%d K=%d T=%d (G >= 1, 1 <= K <= %d, 3 <= T <= 65535: no interior frame below 3, 9 G T, 9 K T and "
                   "G K <= 2^31 - 1)", who, G, K, T, D4GS_MAX_K);
    return D4GS_EINVAL;
  }
  *fd = fit_data(G, T);
  if (targets_bytes < fd->total || (uintptr_t)targets % 16) {
    d4gs_set_error("%s: targets of %zu bytes (16-byte aligned) needed, %zu given at %p", who, fd->total, targets_bytes, targets);
    return D4GS_EINVAL;
  }
  if (ws) {
    *ws = fit_ws(G, K, T);
    if (workspace_bytes < ws->total || (uintptr_t)workspace % 16) {
      d4gs_set_error("%s: workspace of %zu bytes (16-byte aligned) needed, %zu given at %p", who, ws->total, workspace_bytes, workspace);
      return D4GS_EINVAL;
    }
  }
  return D4GS_OK;
}

int quantile_check(const char *who, float quantile) {
  if (d4gs_bad_quantile(quantile)) {
    d4gs_set_error("%s: quantile=%g (finite and > 0)", who, (double)quantile);
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

size_t d4gs_track_fit_targets_bytes(int32_t G, int32_t T) { return data_sizes_ok(G, T) ? fit_data(G, T).total : 0; }

size_t d4gs_track_fit_workspace_bytes(int32_t G, int32_t K, int32_t T) { return fit_sizes_ok(G, K, T) ? fit_ws(G, K, T).total : 0; }

int d4gs_track_fit_prepare(const float *xyz, const uint8_t *visibles, const uint8_t *invisibles, const float *confidences, const float *Ks,
                           const float *w2cs, int32_t G, int32_t T, void *targets, size_t targets_bytes, void *stream) {
  const void *ptrs[] = {xyz, visibles, invisibles, confidences, Ks, w2cs, targets};
  FitData fd;
  if (int rc = fit_check("d4gs_track_fit_prepare", ptrs, 7, G, 1, T, targets, targets_bytes, nullptr, 0, &fd, nullptr)) return rc;
  char *base = (char *)targets;
  hipStream_t s = (hipStream_t)stream;
  double *w3p = (double *)(base + fd.w3_partials);
  D4GS_LAUNCH("k_fit_prepare", k_fit_prepare, dim3(fd.gblocks, T), dim3(FB), 0, s, xyz, visibles, invisibles, confidences, Ks, w2cs, (int)G,
              (int)T, (float *)(base + fd.xyz), (float *)(base + fd.gt2d), (float *)(base + fd.w3), (float *)(base + fd.w2), w3p);
  if (int rc = d4gs_check_launch("k_fit_prepare")) return rc;
  D4GS_LAUNCH("k_fit_prepare_finish", k_fit_prepare_finish, dim3(1), dim3(FB), 0, s, Ks, w2cs, (int)T, (const double *)w3p, fd.gblocks * T,
              (float *)(base + fd.times), (float *)(base + fd.cams), (double *)(base + fd.consts));
  return d4gs_check_launch("k_fit_prepare_finish");
}

int d4gs_track_fit_fwd(const float *means, const float *motion_coefs, const float *rots, const float *transls, int32_t G, int32_t K,
                       int32_t T, float quantile, const float *weights, const void *targets, size_t targets_bytes, void *workspace,
                       size_t workspace_bytes, float *out, const int32_t *iter, float *losses, int32_t num_iters, void *stream) {
  const void *ptrs[] = {means, motion_coefs, rots, transls, targets, workspace, out};
  FitData fd;
  FitWs w;
  if (int rc = fit_check("d4gs_track_fit_fwd", ptrs, 7, G, K, T, targets, targets_bytes, workspace, workspace_bytes, &fd, &w)) return rc;
  if (int rc = quantile_check("d4gs_track_fit_fwd", quantile)) return rc;
  if (losses && (!iter || num_iters < 1 || ((uintptr_t)iter | (uintptr_t)losses) % 4)) {
    d4gs_set_error("d4gs_track_fit_fwd: a loss history needs the device counter iter and num_iters >= 1 (4-byte aligned); got iter %p "
                   "num_iters=%d", (const void *)iter, num_iters);
    return D4GS_EINVAL;
  }
  const char *tb = (const char *)targets;
  char *base = (char *)workspace;
  float *points = (float *)(base + w.points), *values = (float *)(base + w.trim), *trim_out = (float *)(base + w.trim_out);
  double *partials = (double *)(base + w.partials);
  hipStream_t s = (hipStream_t)stream;
  const D4gsDims d = pose_dims(G, K, T);
  const D4gsProjIn in = pose_in(means, motion_coefs, rots, transls, (const float *)(tb + fd.times));
  const D4gsPoses po = {points, nullptr, nullptr, 0};
  if (int rc = d4gs_poses_fwd_impl(&d, &in, &po, s)) return rc;
  const int nx = w.gblocks + w.bblocks;
  D4GS_LAUNCH("k_fit_loss_fwd", k_fit_loss_fwd, dim3(nx, w.chunks), dim3(FB), 0, s, (const float *)points, (const float *)(tb + fd.xyz),
              (const float *)(tb + fd.gt2d), (const float *)(tb + fd.w3), (const float *)(tb + fd.cams), motion_coefs, rots, transls, (int)G,
              (int)K, (int)T, w.gblocks, values, partials);
  if (int rc = d4gs_check_launch("k_fit_loss_fwd")) return rc;
  if (int rc = d4gs_trim_masked_impl(values, (const float *)(tb + fd.w2), (int64_t)G * T, quantile, trim_out, s)) return rc;
  D4GS_LAUNCH("k_fit_finish", k_fit_finish, dim3(1), dim3(FB), 0, s, (const double *)partials, nx * w.chunks, (const float *)trim_out,
              (const double *)(tb + fd.consts), weights, (int)G, (int)K, (int)T, out, iter, losses, (int)num_iters);
  return d4gs_check_launch("k_fit_finish");
}

int d4gs_track_fit_bwd(const float *means, const float *motion_coefs, const float *rots, const float *transls, int32_t G, int32_t K,
                       int32_t T, float quantile, const void *targets, size_t targets_bytes, void *workspace, size_t workspace_bytes,
                       const float *v_out, const D4gsLeafGrads *grads, void *stream) {
  const void *ptrs[] = {means, motion_coefs, rots, transls, targets, workspace, v_out, grads,
                        grads ? grads->v_means : nullptr, grads ? grads->v_motion_coefs : nullptr, grads ? grads->v_rots : nullptr,
                        grads ? grads->v_transls : nullptr};
  FitData fd;
  FitWs w;
  if (int rc = fit_check("d4gs_track_fit_bwd", ptrs, 12, G, K, T, targets, targets_bytes, workspace, workspace_bytes, &fd, &w)) return rc;
  if (int rc = quantile_check("d4gs_track_fit_bwd", quantile)) return rc;
  const char *tb = (const char *)targets;
  char *base = (char *)workspace;
  const float *points = (const float *)(base + w.points), *values = (const float *)(base + w.trim), *trim_out = (const float *)(base + w.trim_out);
  float *v_points = (float *)(base + w.v_points), *v_coefs = (float *)(base + w.v_coefs);
  hipStream_t s = (hipStream_t)stream;
  D4GS_LAUNCH("k_fit_loss_bwd", k_fit_loss_bwd, dim3(w.gblocks, w.chunks), dim3(FB), 0, s, points, (const float *)(tb + fd.xyz),
              (const float *)(tb + fd.gt2d), (const float *)(tb + fd.w3), (const float *)(tb + fd.w2), (const float *)(tb + fd.cams),
              (const double *)(tb + fd.consts), values, trim_out, motion_coefs, v_out, (int)G, (int)K, (int)T, (int)(quantile >= 1.f), v_points,
              v_coefs);
  if (int rc = d4gs_check_launch("k_fit_loss_bwd")) return rc;
  const D4gsDims d = pose_dims(G, K, T);
  const D4gsProjIn in = pose_in(means, motion_coefs, rots, transls, (const float *)(tb + fd.times));
  const D4gsPoses vo = {v_points, nullptr, nullptr, 0};
  D4gsLeafGrads lg{};
  lg.v_means = grads->v_means, lg.v_motion_coefs = grads->v_motion_coefs, lg.v_rots = grads->v_rots, lg.v_transls = grads->v_transls;
  lg.partials = (float *)(base + w.pose_partials);
  if (int rc = d4gs_poses_bwd_impl(&d, &in, &vo, &lg, s)) return rc;  // overwrites the four leaf gradients: the own terms come behind it
  const int n = K * T > G * K ? K * T : G * K;
  D4GS_LAUNCH("k_fit_leaf_add", k_fit_leaf_add, dim3((n + FB - 1) / FB), dim3(FB), 0, s, rots, transls, (const float *)v_coefs, v_out, (int)G,
              (int)K, (int)T, grads->v_rots, grads->v_transls, grads->v_motion_coefs);
  return d4gs_check_launch("k_fit_leaf_add");
}

int d4gs_track_fit_schedule(int32_t *iter, int32_t num_iters, D4gsAdamRec *table, double lr0_rots, double lr0_transls, double lr0_coefs,
                            double lr0_means, float *weights, float *lrs, void *stream) {
  const double lr0[4] = {lr0_rots, lr0_transls, lr0_coefs, lr0_means};
  if (int rc = sched_check("d4gs_track_fit_schedule", iter, num_iters, table, lr0, weights, lrs)) return rc;
  D4GS_LAUNCH("k_fit_schedule", k_fit_schedule, dim3(1), dim3(D4GS_WAVE), 0, (hipStream_t)stream, iter, (int)num_iters, table, lr0_rots,
              lr0_transls, lr0_coefs, lr0_means, weights, lrs);
  return d4gs_check_launch("k_fit_schedule");
}

int d4gs_track_fit_schedule_cpu(int32_t *iter, int32_t num_iters, D4gsAdamRec *table, double lr0_rots, double lr0_transls,
                                double lr0_coefs, double lr0_means, float *weights, float *lrs) {
  const double lr0[4] = {lr0_rots, lr0_transls, lr0_coefs, lr0_means};
  if (int rc = sched_check("d4gs_track_fit_schedule_cpu", iter, num_iters, table, lr0, weights, lrs)) return rc;
  const int i = *iter;
  const FitSchedule s = fit_schedule(i, num_iters, lr0);
  for (int r = 0; r < 4; r++) {
    table[r].lr = s.lr[r];
    if (lrs && i >= 0 && i < num_iters) lrs[(size_t)i * 4 + r] = (float)s.lr[r];
  }
  for (int k = 0; k < N_TERMS; k++) weights[k] = s.w[k];
  *iter = i + 1;
  return D4GS_OK;
}

}  // extern "C"
