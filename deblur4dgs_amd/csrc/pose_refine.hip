// pose_refine.hip -- test-time pose refinement (include/d4gs.h, "Test-time pose refinement"): the camera-only
// adjoint of the projection stage and the fused scheduler + Adam + compose step of flow3d/validator.py:400-456, with its CPU twin.
//
// d4gs_pose_bwd.  The scene is frozen while a test view's pose is refined, so of everything k_project_bwd produces only the 12
// numbers of the view matrix and the 12 of each sub-sample's camera delta are read.  k_pose_bwd computes exactly those: one lane per
// (sub-sample, Gaussian), gridDim.y = S, the deformation recomputed from the leaves and the blended-bases table, the camera chain of
// k_project_bwd's phases 2 - 5 (same expressions; the reciprocal of the depth is the correctly rounded one here), no per-Gaussian
// output and no LDS beyond the block sum.  A lane's 24 values go through reduce.h: block sum -> partials [S][blocks][24], then ONE
// block (k_pose_finish) takes the ordered total of every sub-sample's blocks - in double - and adds the sub-samples' view-matrix
// totals in increasing s.  Every partial is written by its block (a culled or out-of-range lane adds zeros), so nothing is zeroed.
//
// d4gs_pose_step.  One wave: lanes 0 - 11 own one parameter each (gradient through the composition, learning rate of the cosine
// schedule at step + 1, Adam), lanes 0 - 15 then write the next composed matrix from the new parameters (handed over in LDS).
#include "adam_math.h"
#include "reduce.h"

namespace {

constexpr int NV = 24;  // per lane: dL/dRcw 9 (row-major), dL/dt 3, dL/dRT_s 12 (row-major [3,4])

struct PoseArgs {
  D4gsDims d;
  D4gsProjIn in;
  const int32_t *radii;
  const float *conics;
  const float *v_means2d, *v_conics, *v_depths;
  const float *btab;  // [S][K][16] time-blended bases (D4gsProjOut.blend_bases, or k_bases_table's behind the partials)
  float *partials;    // [S][gridDim.x][NV]
};

typedef const __attribute__((address_space(4))) float *pose_cfloat_p;  // wave-uniform rows of the bases table: scalar loads

__global__ void __launch_bounds__(REDUCE_NT) k_pose_bwd(const PoseArgs a) {
  __shared__ float red[4 * NV];
  const D4gsDims &d = a.d;
  const int N = d.N, G = d.G, K = d.K;
  const int s = blockIdx.y;
  const int g = blockIdx.x * REDUCE_NT + threadIdx.x;
  const bool raw = d.flags & D4GS_RAW_PARAMS;
  const Cam cam = load_cam(a.in.viewmat, a.in.Kmat, d.width, d.height);
  float out[NV];
#pragma unroll
  for (int c = 0; c < NV; c++) out[c] = 0.f;
  const size_t i = (size_t)s * N + (g < N ? g : 0);
  if (g < N && a.radii[i] > 0) {  // (the visibility decision is the forward's: near / far plane, radius_clip, the screen test)
    float mu[3], sc[3], qh[4];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      mu[c] = a.in.means[(size_t)g * 3 + c];
      const float v = a.in.scales[(size_t)g * 3 + c];
      sc[c] = raw ? expf(v) : v;
    }
    {
      const float *q = a.in.quats + (size_t)g * 4;
      const float inv_qn = 1.f / fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
#pragma unroll
      for (int c = 0; c < 4; c++) qh[c] = q[c] * inv_qn;
    }
    // ---- deformation forward (params.py:142-180): softmax(motion_coefs) . blended bases -> [Rd | transl] ----
    float Rm[9], mw0[3];
    quat_to_rotmat(qh[0], qh[1], qh[2], qh[3], Rm);
    if (g < G) {
      const float *mc = a.in.motion_coefs + (size_t)g * K;
      float m = -INFINITY, sum = 0.f;
      for (int k = 0; k < K; k++) m = fmaxf(m, mc[k]);
      for (int k = 0; k < K; k++) sum += expf(mc[k] - m);
      const float is = 1.f / sum;
      float v9[9];
#pragma unroll
      for (int j = 0; j < 9; j++) v9[j] = 0.f;
      for (int k = 0; k < K; k++) {
        const float c = expf(mc[k] - m) * is;
        pose_cfloat_p B = (pose_cfloat_p)(uintptr_t)a.btab + ((size_t)s * K + k) * 16;
#pragma unroll
        for (int j = 0; j < 9; j++) v9[j] += c * B[j];
      }
      GS6 gs;
      gram_schmidt(v9 + 3, gs);
      const float Rd[9] = {gs.x[0], gs.y[0], gs.z[0], gs.x[1], gs.y[1], gs.z[1], gs.x[2], gs.y[2], gs.z[2]};
#pragma unroll
      for (int r = 0; r < 3; r++) mw0[r] = Rd[r * 3] * mu[0] + Rd[r * 3 + 1] * mu[1] + Rd[r * 3 + 2] * mu[2] + v9[r];
      float Rq[9];
#pragma unroll
      for (int r = 0; r < 9; r++) Rq[r] = Rm[r];
      mat3_mul(Rd, Rq, Rm);
    } else {
#pragma unroll
      for (int r = 0; r < 3; r++) mw0[r] = mu[r];
    }
    // ---- camera forward (k_project_bwd phase 2): the delta moves the mean, not the rotation (scene_model.py:352-353) ----
    float mw[3] = {mw0[0], mw0[1], mw0[2]};
    if (a.in.RTs) {
      const float *RT = a.in.RTs + s * 12;
#pragma unroll
      for (int r = 0; r < 3; r++) mw[r] = RT[r * 4] * mw0[0] + RT[r * 4 + 1] * mw0[1] + RT[r * 4 + 2] * mw0[2] + RT[r * 4 + 3];
    }
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) pc[r] = cam.R[r * 3] * mw[0] + cam.R[r * 3 + 1] * mw[1] + cam.R[r * 3 + 2] * mw[2] + cam.t[r];
    float M[9];  // Rcw Rm diag(sc)
    {
      float Wm[9];
      mat3_mul(cam.R, Rm, Wm);
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[r * 3 + c] = Wm[r * 3 + c] * sc[c];
    }
    const float rz = 1.f / pc[2], rz2 = rz * rz, rz3 = rz2 * rz;
    const float xr = pc[0] * rz, yr = pc[1] * rz;
    const bool in_x = (xr <= cam.limx) && (xr >= -cam.limx), in_y = (yr <= cam.limy) && (yr >= -cam.limy);
    const float tx = pc[2] * fminf(cam.limx, fmaxf(-cam.limx, xr)), ty = pc[2] * fminf(cam.limy, fmaxf(-cam.limy, yr));
    const float J00 = cam.fx * rz, J11 = cam.fy * rz, J02 = -cam.fx * tx * rz2, J12 = -cam.fy * ty * rz2;
    // ---- adjoint of conic = inverse(cov2d + eps2d I), cov2d = J covc J^T (phase 3) ----
    float w00, w01, w11;
    {
      const float A = a.conics[i * 3], Bc = a.conics[i * 3 + 1], C = a.conics[i * 3 + 2];
      const float vA = a.v_conics[i * 3], vB = 0.5f * a.v_conics[i * 3 + 1], vC = a.v_conics[i * 3 + 2];
      const float t00 = A * vA + Bc * vB, t01 = A * vB + Bc * vC, t10 = Bc * vA + C * vB, t11 = Bc * vB + C * vC;
      w00 = -(t00 * A + t01 * Bc), w01 = -(t00 * Bc + t01 * C), w11 = -(t10 * Bc + t11 * C);
    }
    float vJ00, vJ02, vJ11, vJ12;
    {
      const float cxx = M[0] * M[0] + M[1] * M[1] + M[2] * M[2], cxy = M[0] * M[3] + M[1] * M[4] + M[2] * M[5];
      const float cxz = M[0] * M[6] + M[1] * M[7] + M[2] * M[8], cyy = M[3] * M[3] + M[4] * M[4] + M[5] * M[5];
      const float cyz = M[3] * M[6] + M[4] * M[7] + M[5] * M[8], czz = M[6] * M[6] + M[7] * M[7] + M[8] * M[8];
      const float js00 = J00 * cxx + J02 * cxz, js01 = J00 * cxy + J02 * cyz, js02 = J00 * cxz + J02 * czz;  // J covc (2x3)
      const float js10 = J11 * cxy + J12 * cxz, js11 = J11 * cyy + J12 * cyz, js12 = J11 * cyz + J12 * czz;
      vJ00 = 2.f * (w00 * js00 + w01 * js10), vJ02 = 2.f * (w00 * js02 + w01 * js12);
      vJ11 = 2.f * (w01 * js01 + w11 * js11), vJ12 = 2.f * (w01 * js02 + w11 * js12);
    }
    float v_pc[3];
    {
      const float vm0 = a.v_means2d[i * 2], vm1 = a.v_means2d[i * 2 + 1];
      v_pc[0] = cam.fx * rz * vm0;
      v_pc[1] = cam.fy * rz * vm1;
      v_pc[2] = -(cam.fx * pc[0] * vm0 + cam.fy * pc[1] * vm1) * rz2 + a.v_depths[i];
      // the clamped Jacobian: inside the 1.3 tan(fov / 2) window J02 / J12 follow x / y, outside they follow z alone
      if (in_x) v_pc[0] += -cam.fx * rz2 * vJ02; else v_pc[2] += -cam.fx * rz3 * vJ02 * tx;
      if (in_y) v_pc[1] += -cam.fy * rz2 * vJ12; else v_pc[2] += -cam.fy * rz3 * vJ12 * ty;
      v_pc[2] += -cam.fx * rz2 * vJ00 - cam.fy * rz2 * vJ11 + 2.f * cam.fx * tx * rz3 * vJ02 + 2.f * cam.fy * ty * rz3 * vJ12;
    }
    // ---- covc = M M^T: v_M = (v_covc + v_covc^T) M, v_covc = J^T w J; vW = v_M diag(sc) (phase 4) ----
    float vW[9];
    {
      const float a0 = w00 * J00, a1 = w01 * J11, a2 = w00 * J02 + w01 * J12;
      const float b0 = w01 * J00, b1 = w11 * J11, b2 = w01 * J02 + w11 * J12;
      const float s00 = 2.f * J00 * a0, s01 = J00 * a1 + J11 * b0, s02 = J00 * a2 + (J02 * a0 + J12 * b0);
      const float s11 = 2.f * J11 * b1, s12 = J11 * b2 + (J02 * a1 + J12 * b1), s22 = 2.f * (J02 * a2 + J12 * b2);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float m0 = M[c], m1 = M[3 + c], m2 = M[6 + c];
        vW[c] = (s00 * m0 + s01 * m1 + s02 * m2) * sc[c];
        vW[3 + c] = (s01 * m0 + s11 * m1 + s12 * m2) * sc[c];
        vW[6 + c] = (s02 * m0 + s12 * m1 + s22 * m2) * sc[c];
      }
    }
    // ---- dL/dRcw = vW Rm^T + v_pc mw^T, dL/dt = v_pc (phase 5); dL/dRT_s = (Rcw^T v_pc) [mw0; 1]^T ----
    {
      float tmp[9];
      mat3_mul_bt(vW, Rm, tmp);
#pragma unroll
      for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) out[r * 3 + c] = tmp[r * 3 + c] + v_pc[r] * mw[c];
        out[9 + r] = v_pc[r];
      }
    }
    if (a.in.RTs) {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const float v_mw = cam.R[r] * v_pc[0] + cam.R[3 + r] * v_pc[1] + cam.R[6 + r] * v_pc[2];
#pragma unroll
        for (int c = 0; c < 3; c++) out[12 + r * 4 + c] = v_mw * mw0[c];
        out[12 + r * 4 + 3] = v_mw;
      }
    }
  }
  block_sum_store<NV>(out, red);
  __syncthreads();
  if (threadIdx.x < NV) a.partials[((size_t)s * gridDim.x + blockIdx.x) * NV + threadIdx.x] = block_sum_combine<NV>(red, threadIdx.x);
}

// One block: the ordered total (reduce.h; 24 sums = 48 KB of LDS) of each sub-sample's block partials, in increasing s.
__global__ void __launch_bounds__(REDUCE_NT) k_pose_finish(const float *__restrict__ partials, int S, int nb, float *__restrict__ v_viewmat,
                                                           float *__restrict__ v_RTs) {
  double V[12];
#pragma unroll
  for (int c = 0; c < 12; c++) V[c] = 0.0;
  const int t = threadIdx.x;
  for (int s = 0; s < S; s++) {
    double tot[NV];
    ordered_total<NV>(partials + (size_t)s * nb * NV, (int64_t)nb, (int64_t)NV, tot);
#pragma unroll
    for (int c = 0; c < 12; c++) {
      V[c] += tot[c];
      if (v_RTs && t == c) v_RTs[(size_t)s * 12 + c] = (float)tot[12 + c];  // (selected, not indexed: the sums stay in registers)
    }
  }
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (t == r * 4 + c) v_viewmat[t] = (float)(c < 3 ? V[r * 3 + c] : V[9 + r]);
  }
  if (t >= 12 && t < 16) v_viewmat[t] = 0.f;
}

int pose_blocks(const D4gsDims *d) { return d->N > 0 ? (d->N + REDUCE_NT - 1) / REDUCE_NT : 1; }

// ---- the step ---------------------------------------------------------------------------------------------------------------
// CosineAnnealingLR's closed form at epoch k (torch.optim.lr_scheduler, _get_closed_form_lr), in double; k == t_max gives eta_min
__host__ __device__ inline double pose_lr(double lr0, double eta_min, int t_max, int k) {
  return eta_min + (lr0 - eta_min) * (1.0 + cos(3.14159265358979323846 * (double)k / (double)t_max)) / 2.0;
}

// THE update of parameter i < 12 (kernel and CPU twin): its gradient through W = [transR R0 | transT + t0] - row i / 3 of
// v_W[:3,:3] R0^T for transR, v_W[i - 9, 3] for transT - then adam.hip's per-element Adam.  Explicit FMAs, no contraction: the host
// and the device compiler round alike.
__host__ __device__ __forceinline__ void pose_step_update(const float *w2c, const float *v_W, int i, float &p, float &m, float &v,
                                                          const AdamCoef &c) {
#pragma clang fp contract(off)
  float g;
  if (i >= 9) {
    g = v_W[(i - 9) * 4 + 3];
  } else {
    const int r = i / 3, j = i - 3 * r;
    g = __builtin_fmaf(v_W[r * 4 + 2], w2c[j * 4 + 2], __builtin_fmaf(v_W[r * 4 + 1], w2c[j * 4 + 1], v_W[r * 4] * w2c[j * 4]));
  }
  adam_update(p, m, v, g, c);
}

// element e < 16 of the composed matrix [transR R0 | transT + t0; 0 0 0 1]
__host__ __device__ __forceinline__ float pose_compose(const float *w2c, const float *p, int e) {
#pragma clang fp contract(off)
  const int r = e >> 2, c = e & 3;
  if (r == 3) return c == 3 ? 1.f : 0.f;
  if (c == 3) return p[9 + r] + w2c[r * 4 + 3];
  return __builtin_fmaf(p[r * 3 + 2], w2c[8 + c], __builtin_fmaf(p[r * 3 + 1], w2c[4 + c], p[r * 3] * w2c[c]));
}

__global__ void __launch_bounds__(D4GS_WAVE) k_pose_step(const float *__restrict__ w2c, const float *__restrict__ v_W, float *p, float *m, float *v,
                                                         int32_t *step, double lr0, double eta_min, int t_max, double beta1, double beta2,
                                                         double eps, float *lr_out, float *W) {
  __shared__ float sp[12];
  const int t = threadIdx.x;
  const int k = *step + 1;
  const double lr = pose_lr(lr0, eta_min, t_max, k);
  if (t < 12) {
    const AdamCoef c = adam_coef(lr, beta1, beta2, eps, (float)k);
    float pi = p[t], mi = m[t], vi = v[t];
    pose_step_update(w2c, v_W, t, pi, mi, vi, c);
    p[t] = pi, m[t] = mi, v[t] = vi, sp[t] = pi;
  }
  __syncthreads();  // every lane has read *step; the new parameters are in LDS
  if (t < 16) W[t] = pose_compose(w2c, sp, t);
  if (t == 0) {
    *step = k;
    if (lr_out) *lr_out = (float)lr;
  }
}

int pose_step_check(const char *who, const float *w2c, const float *v_W, const float *p, const float *m, const float *v, const int32_t *step,
                    int32_t t_max, const float *lr_out, const float *W) {
  if (!w2c || !v_W || !p || !m || !v || !step || !W) {
    d4gs_set_error("%s: NULL argument (w2c, v_W, p, m, v, step and W are required)", who);
    return D4GS_EINVAL;
  }
  if (((uintptr_t)w2c | (uintptr_t)v_W | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)step | (uintptr_t)lr_out | (uintptr_t)W) % 4) {
    d4gs_set_error("%s: misaligned argument (4-byte words)", who);
    return D4GS_EINVAL;
  }
  if (t_max < 1) {
    d4gs_set_error("%s: t_max=%d (the cosine schedule needs t_max >= 1)", who, t_max);
    return D4GS_EINVAL;
  }
  return D4GS_OK;
}

}  // namespace

extern "C" {

size_t d4gs_pose_bwd_partials_elems(const D4gsDims *dims) {
  if (d4gs_check_dims(dims)) return 0;
  return (size_t)dims->S * pose_blocks(dims) * NV + (dims->G > 0 ? (size_t)dims->S * dims->K * 16 : 0);
}

int d4gs_pose_bwd(const D4gsDims *dims, const D4gsProjIn *in, const D4gsProjOut *proj, const float *v_means2d, const float *v_conics,
                  const float *v_depths, float *v_viewmat, float *v_RTs, float *partials, void *stream) {
  if (int rc = d4gs_check_dims(dims)) return rc;
  if (!in || !proj || !in->means || !in->quats || !in->scales || !in->viewmat || !in->Kmat || !proj->radii || !proj->conics || !v_means2d ||
      !v_conics || !v_depths || !v_viewmat) {
    d4gs_set_error("d4gs_pose_bwd: NULL required buffer");
    return D4GS_EINVAL;
  }
  if (!partials) {
    d4gs_set_error("d4gs_pose_bwd: NULL partials (d4gs_pose_bwd_partials_elems(dims) floats of scratch)");
    return D4GS_EINVAL;
  }
  if (dims->G > 0 && (!in->motion_coefs || !in->rots || !in->transls || !in->times)) {
    d4gs_set_error("d4gs_pose_bwd: G>0 needs motion_coefs/rots/transls/times");
    return D4GS_EINVAL;
  }
  if (v_RTs && !in->RTs) {
    d4gs_set_error("d4gs_pose_bwd: v_RTs given without in->RTs");
    return D4GS_EINVAL;
  }
  if (dims->S > 65535) {
    d4gs_set_error("d4gs_pose_bwd: S=%d overflows the grid (S <= 65535)", dims->S);
    return D4GS_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = pose_blocks(dims);
  PoseArgs a{};
  a.d = *dims, a.in = *in;
  a.radii = proj->radii, a.conics = proj->conics;
  a.v_means2d = v_means2d, a.v_conics = v_conics, a.v_depths = v_depths;
  a.partials = partials;
  a.btab = proj->blend_bases;
  if (dims->G > 0 && !a.btab) {  // a caller without the forward's table: built behind the partial sums
    float *btab = partials + (size_t)dims->S * nb * NV;
    a.btab = btab;
    if (int rc = d4gs_bases_table_launch(dims, in, btab, st)) return rc;
  }
  D4GS_LAUNCH("k_pose_bwd", k_pose_bwd, dim3(nb, dims->S), dim3(REDUCE_NT), 0, st, a);
  if (int rc = d4gs_check_launch("k_pose_bwd")) return rc;
  D4GS_LAUNCH("k_pose_finish", k_pose_finish, dim3(1), dim3(REDUCE_NT), 0, st, (const float *)partials, (int)dims->S, nb, v_viewmat, v_RTs);
  return d4gs_check_launch("k_pose_finish");
}

int d4gs_pose_step(const float *w2c, const float *v_W, float *p, float *m, float *v, int32_t *step, double lr0, double eta_min,
                   int32_t t_max, double beta1, double beta2, double eps, float *lr_out, float *W, void *stream) {
  if (int rc = pose_step_check("d4gs_pose_step", w2c, v_W, p, m, v, step, t_max, lr_out, W)) return rc;
  D4GS_LAUNCH("k_pose_step", k_pose_step, dim3(1), dim3(D4GS_WAVE), 0, (hipStream_t)stream, w2c, v_W, p, m, v, step, lr0, eta_min, (int)t_max,
              beta1, beta2, eps, lr_out, W);
  return d4gs_check_launch("k_pose_step");
}

int d4gs_pose_step_cpu(const float *w2c, const float *v_W, float *p, float *m, float *v, int32_t *step, double lr0, double eta_min,
                       int32_t t_max, double beta1, double beta2, double eps, float *lr_out, float *W) {
  if (int rc = pose_step_check("d4gs_pose_step_cpu", w2c, v_W, p, m, v, step, t_max, lr_out, W)) return rc;
  const int k = *step + 1;
  const double lr = pose_lr(lr0, eta_min, t_max, k);
  const AdamCoef c = adam_coef(lr, beta1, beta2, eps, (float)k);
  for (int i = 0; i < 12; i++) pose_step_update(w2c, v_W, i, p[i], m[i], v[i], c);
  float out[16];  // (W may alias nothing it is composed from, but compose first all the same)
  for (int e = 0; e < 16; e++) out[e] = pose_compose(w2c, p, e);
  for (int e = 0; e < 16; e++) W[e] = out[e];
  *step = k;
  if (lr_out) *lr_out = (float)lr;
  return D4GS_OK;
}

}  // extern "C"
