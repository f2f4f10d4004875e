// sh.hip -- real spherical-harmonic colours (degree 0..4), forward and backward: seam S1's `sh_degree`
// (gsplat 1.1.1 `rasterization(..., sh_degree=d)` / `spherical_harmonics`).
//
//   dir = p - origin (or p),  d = dir / |dir|,  raw[c] = sum_{k < (D+1)^2} Y_k(d) coeffs[n, k, c]
//   rgb = clamp ? max(raw + 0.5, 0) : raw
//
// One lane per Gaussian; the degree is a template parameter, so the basis and the coefficient loop unroll fully.  A
// masked Gaussian (mask[n] == 0) or one with |dir| == 0 has raw = 0 and zero gradients.  The backward recomputes the
// clamp decision from the coefficients (it reads them anyway for v_p) instead of saving raw in the forward; v_origin
// = -sum_n v_p[n] is a deterministic two-level sum (per-block partials in a fixed tree order, then one ordered block),
// like the photometric loss's.
#include "common.h"
#include "reduce.h"

namespace {

constexpr int SH_BLOCK = REDUCE_NT;

// forward-mode dual number: value and its partials w.r.t. the unit direction's (x, y, z); gives each basis polynomial's
// gradient from the same source as its value
struct D3 {
  float v, x, y, z;
  __device__ D3(float c = 0.f) : v(c), x(0.f), y(0.f), z(0.f) {}
  __device__ D3(float v_, float x_, float y_, float z_) : v(v_), x(x_), y(y_), z(z_) {}
};
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return D3(a.v + b.v, a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return D3(a.v - b.v, a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ D3 operator*(D3 a, D3 b) {
  return D3(a.v * b.v, a.x * b.v + a.v * b.x, a.y * b.v + a.v * b.y, a.z * b.v + a.v * b.z);
}
__device__ __forceinline__ D3 operator*(float s, D3 a) { return D3(s * a.v, s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ D3 operator+(D3 a, float s) { return D3(a.v + s, a.x, a.y, a.z); }
__device__ __forceinline__ D3 operator-(D3 a, float s) { return D3(a.v - s, a.x, a.y, a.z); }

// the real SH basis in the Inria / gsplat order and sign convention, on a unit vector (include/d4gs.h lists the table)
template <int DEG, class T>
__device__ __forceinline__ void sh_basis(T x, T y, T z, T *Y) {
  Y[0] = T(0.28209479177387814f);
  if constexpr (DEG >= 1) {
    Y[1] = -0.4886025119029199f * y;
    Y[2] = 0.4886025119029199f * z;
    Y[3] = -0.4886025119029199f * x;
  }
  if constexpr (DEG >= 2) {
    const T xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    Y[4] = 1.0925484305920792f * xy;
    Y[5] = -1.0925484305920792f * yz;
    Y[6] = 0.31539156525252005f * (2.f * zz - xx - yy);
    Y[7] = -1.0925484305920792f * xz;
    Y[8] = 0.5462742152960396f * (xx - yy);
    if constexpr (DEG >= 3) {
      const T t4 = 4.f * zz - xx - yy, x3y = xx - 3.f * yy, y3x = 3.f * xx - yy;
      Y[9] = -0.5900435899266435f * (y * y3x);
      Y[10] = 2.890611442640554f * (xy * z);
      Y[11] = -0.4570457994644658f * (y * t4);
      Y[12] = 0.3731763325901154f * (z * (2.f * zz - 3.f * xx - 3.f * yy));
      Y[13] = -0.4570457994644658f * (x * t4);
      Y[14] = 1.445305721320277f * (z * (xx - yy));
      Y[15] = -0.5900435899266435f * (x * x3y);
      if constexpr (DEG >= 4) {
        const T z71 = 7.f * zz - 1.f, z73 = 7.f * zz - 3.f;
        Y[16] = 2.5033429417967046f * (xy * (xx - yy));
        Y[17] = -1.7701307697799304f * (yz * y3x);
        Y[18] = 0.9461746957575601f * (xy * z71);
        Y[19] = -0.6690465435572892f * (yz * z73);
        Y[20] = 0.10578554691520431f * (zz * (35.f * zz - 30.f) + 3.f);
        Y[21] = -0.6690465435572892f * (xz * z73);
        Y[22] = 0.47308734787878004f * ((xx - yy) * z71);
        Y[23] = -1.7701307697799304f * (xz * x3y);
        Y[24] = 0.6258357354491761f * (xx * x3y - yy * y3x);
      }
    }
  }
}

struct ShArgs {
  const float *p, *origin, *coeffs;  // [N,3], [3] or null, [N,K,3]
  const uint8_t *mask;               // [N] or null
  int64_t N;
  int32_t K, clamp;
  float *rgb;                        // forward: [N,3]
  const float *v_rgb;                // backward: [N,3]
  float *v_coeffs, *v_p, *partials;  // [N,K,3] or null, [N,3] or null, [blocks,3] or null
};

// the unit direction of Gaussian n; false for a masked Gaussian or a zero-length direction
__device__ __forceinline__ bool sh_dir(const ShArgs &a, int64_t n, float &x, float &y, float &z, float &inv) {
  if (a.mask && !a.mask[n]) return false;
  float dx = a.p[3 * n], dy = a.p[3 * n + 1], dz = a.p[3 * n + 2];
  if (a.origin) dx -= a.origin[0], dy -= a.origin[1], dz -= a.origin[2];
  const float r2 = dx * dx + dy * dy + dz * dz;
  if (!(r2 > 0.f)) return false;
  inv = rsqrtf(r2);
  x = dx * inv, y = dy * inv, z = dz * inv;
  return true;
}

// the 3 (D+1)^2 coefficients of one Gaussian (row = its [K,3] block).  VEC: 16-byte loads (12 K % 16 == 0 and a 16-byte
// aligned base, so every row starts on a 16-byte boundary); the last word may run past 3 (D+1)^2 but never past 3 K.
template <int DEG, bool VEC>
constexpr int sh_nc() { return VEC ? ((3 * (DEG + 1) * (DEG + 1) + 3) / 4) * 4 : 3 * (DEG + 1) * (DEG + 1); }

template <int DEG, bool VEC>
__device__ __forceinline__ void load_coeffs(const float *row, float *c) {
  constexpr int NC = sh_nc<DEG, VEC>();
  if constexpr (VEC) {
    const float4 *r4 = reinterpret_cast<const float4 *>(row);
#pragma unroll
    for (int i = 0; i < NC / 4; i++) {
      const float4 v = r4[i];
      c[4 * i] = v.x, c[4 * i + 1] = v.y, c[4 * i + 2] = v.z, c[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NC; i++) c[i] = row[i];
  }
}

template <int DEG>
__device__ __forceinline__ void sh_dot(const float *Y, const float *c, float *raw) {
  constexpr int NB = (DEG + 1) * (DEG + 1);
  raw[0] = raw[1] = raw[2] = 0.f;
#pragma unroll
  for (int k = 0; k < NB; k++)
#pragma unroll
    for (int ch = 0; ch < 3; ch++) raw[ch] = fmaf(Y[k], c[3 * k + ch], raw[ch]);
}

template <int DEG, bool VEC>
__global__ void __launch_bounds__(SH_BLOCK) k_sh_fwd(const ShArgs a) {
  constexpr int NB = (DEG + 1) * (DEG + 1);
  const int64_t n = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  if (n >= a.N) return;
  float raw[3] = {0.f, 0.f, 0.f}, x, y, z, inv;
  if (sh_dir(a, n, x, y, z, inv)) {
    float Y[NB], c[sh_nc<DEG, VEC>()];
    sh_basis<DEG>(x, y, z, Y);
    load_coeffs<DEG, VEC>(a.coeffs + n * (3 * (int64_t)a.K), c);
    sh_dot<DEG>(Y, c, raw);
  }
#pragma unroll
  for (int ch = 0; ch < 3; ch++) a.rgb[3 * n + ch] = a.clamp ? fmaxf(raw[ch] + 0.5f, 0.f) : raw[ch];
}

template <int DEG, bool VEC>
__global__ void __launch_bounds__(SH_BLOCK) k_sh_bwd(const ShArgs a) {
  constexpr int NB = (DEG + 1) * (DEG + 1), NC = sh_nc<DEG, VEC>();
  __shared__ float red[3 * (SH_BLOCK / D4GS_WAVE)];
  const int64_t n = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  const bool need_p = a.v_p || a.partials;
  float vp[3] = {0.f, 0.f, 0.f};
  if (n < a.N) {
    float vr[3] = {a.v_rgb[3 * n], a.v_rgb[3 * n + 1], a.v_rgb[3 * n + 2]};
    float Y[NB], c[NC], x = 0.f, y = 0.f, z = 0.f, inv = 0.f;
    const bool ok = sh_dir(a, n, x, y, z, inv);
    if (ok) {
      sh_basis<DEG>(x, y, z, Y);
      if (a.clamp || need_p) load_coeffs<DEG, VEC>(a.coeffs + n * (3 * (int64_t)a.K), c);
      if (a.clamp) {  // the forward's decision, recomputed bit for bit (same basis, same fmaf chain): torch.clamp_min passes >= 0
        float raw[3];
        sh_dot<DEG>(Y, c, raw);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) vr[ch] = raw[ch] + 0.5f >= 0.f ? vr[ch] : 0.f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < NB; k++) Y[k] = 0.f;
      vr[0] = vr[1] = vr[2] = 0.f;
    }
    if (a.v_coeffs) {  // the whole [K,3] row: Y_k v_rgb below (D+1)^2, exact zeros above
      float *row = a.v_coeffs + n * (3 * (int64_t)a.K);
      const int nc = 3 * a.K;
      if constexpr (VEC) {
        float4 *r4 = reinterpret_cast<float4 *>(row);
#pragma unroll
        for (int i = 0; i < NC / 4; i++) {
          float w[4];
#pragma unroll
          for (int j = 0; j < 4; j++) w[j] = 4 * i + j < 3 * NB ? Y[(4 * i + j) / 3] * vr[(4 * i + j) % 3] : 0.f;
          r4[i] = make_float4(w[0], w[1], w[2], w[3]);
        }
        for (int i = NC / 4; i < nc / 4; i++) r4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
#pragma unroll
        for (int j = 0; j < 3 * NB; j++) row[j] = Y[j / 3] * vr[j % 3];
        for (int j = 3 * NB; j < nc; j++) row[j] = 0.f;
      }
    }
    if (ok && need_p) {
      // v_dhat = sum_k g_k grad Y_k,  g_k = <coeffs[k], v_rgb>;  v_dir = (I - d d^T) v_dhat / |dir|
      D3 Yd[NB];
      sh_basis<DEG>(D3(x, 1.f, 0.f, 0.f), D3(y, 0.f, 1.f, 0.f), D3(z, 0.f, 0.f, 1.f), Yd);
      float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
      for (int k = 1; k < NB; k++) {  // Y_0 is constant
        const float g = c[3 * k] * vr[0] + c[3 * k + 1] * vr[1] + c[3 * k + 2] * vr[2];
        gx = fmaf(g, Yd[k].x, gx), gy = fmaf(g, Yd[k].y, gy), gz = fmaf(g, Yd[k].z, gz);
      }
      const float dot = x * gx + y * gy + z * gz;
      vp[0] = (gx - x * dot) * inv, vp[1] = (gy - y * dot) * inv, vp[2] = (gz - z * dot) * inv;
    }
    if (a.v_p) {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) a.v_p[3 * n + ch] = vp[ch];
    }
  }
  if (!a.partials) return;  // uniform over the launch
  block_sum_store(vp, red);  // the block's sum of v_p
  __syncthreads();
  if (threadIdx.x < 3) a.partials[3 * (int64_t)blockIdx.x + threadIdx.x] = block_sum_combine<3>(red, threadIdx.x);
}

// v_origin = -sum of the block partials; one block
__global__ void __launch_bounds__(256) k_sh_finish(const float *partials, int64_t n_blocks, float *v_origin) {
  double t[3];
  ordered_total(partials, n_blocks, 3, t);
  if (threadIdx.x == 0)
#pragma unroll
    for (int ch = 0; ch < 3; ch++) v_origin[ch] = (float)-t[ch];
}

int64_t sh_blocks(int64_t N) { return (N + SH_BLOCK - 1) / SH_BLOCK; }

template <bool VEC>
int launch_fwd(int degree, const ShArgs &a, hipStream_t stream) {
  const dim3 grid((unsigned)sh_blocks(a.N));
  ProfScope ps("k_sh_fwd", stream);
  switch (degree) {
    case 0: k_sh_fwd<0, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
    case 1: k_sh_fwd<1, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
    case 2: k_sh_fwd<2, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
    case 3: k_sh_fwd<3, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
    default: k_sh_fwd<4, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
  }
  return d4gs_check_launch("k_sh_fwd");
}

template <bool VEC>
int launch_bwd(int degree, const ShArgs &a, hipStream_t stream) {
  const dim3 grid((unsigned)sh_blocks(a.N));
  ProfScope ps("k_sh_bwd", stream);
  switch (degree) {
    case 0: k_sh_bwd<0, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
    case 1: k_sh_bwd<1, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
    case 2: k_sh_bwd<2, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
    case 3: k_sh_bwd<3, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
    default: k_sh_bwd<4, VEC><<<grid, SH_BLOCK, 0, stream>>>(a); break;
  }
  return d4gs_check_launch("k_sh_bwd");
}

// 16-byte coefficient rows: 12 K % 16 == 0 and 16-byte aligned bases
bool sh_vec(int32_t K, const float *coeffs, const float *v_coeffs) {
  return (3 * K) % 4 == 0 && (uintptr_t)coeffs % 16 == 0 && (uintptr_t)v_coeffs % 16 == 0;
}

}  // namespace

extern "C" int64_t d4gs_sh_partials_elems(int64_t N) { return N > 0 ? 3 * sh_blocks(N) : 0; }

int d4gs_sh_fwd_impl(int64_t N, int32_t K, int32_t degree, const float *p, const float *origin, const float *coeffs,
                     const uint8_t *mask, int32_t clamp, float *rgb, hipStream_t stream) {
  if (N == 0) return D4GS_OK;
  ShArgs a = {};
  a.p = p, a.origin = origin, a.coeffs = coeffs, a.mask = mask, a.N = N, a.K = K, a.clamp = clamp != 0, a.rgb = rgb;
  return sh_vec(K, coeffs, nullptr) ? launch_fwd<true>(degree, a, stream) : launch_fwd<false>(degree, a, stream);
}

int d4gs_sh_bwd_impl(int64_t N, int32_t K, int32_t degree, const float *p, const float *origin, const float *coeffs,
                     const uint8_t *mask, int32_t clamp, const float *v_rgb, float *v_coeffs, float *v_p,
                     float *v_origin, float *partials, hipStream_t stream) {
  if (N == 0) return D4GS_OK;
  ShArgs a = {};
  a.p = p, a.origin = origin, a.coeffs = coeffs, a.mask = mask, a.N = N, a.K = K, a.clamp = clamp != 0;
  a.v_rgb = v_rgb, a.v_coeffs = v_coeffs, a.v_p = v_p, a.partials = v_origin ? partials : nullptr;
  int rc = sh_vec(K, coeffs, v_coeffs) ? launch_bwd<true>(degree, a, stream) : launch_bwd<false>(degree, a, stream);
  if (rc || !v_origin) return rc;
  ProfScope ps("k_sh_finish", stream);
  k_sh_finish<<<1, 256, 0, stream>>>(partials, sh_blocks(N), v_origin);
  return d4gs_check_launch("k_sh_finish");
}
