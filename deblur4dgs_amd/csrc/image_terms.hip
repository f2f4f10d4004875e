// image_terms.hip -- the image-sized terms of Trainer.compute_dynamic_losses / compute_static_losses that are plain torch ops in the
// reference: the dilated foreground mask (nn.MaxPool2d(9, 1, 4), flow3d/trainer.py:120,388,575,901), the sharp-keep loss
// (F.interpolate(scale_factor=0.25, mode="area") of prediction, mask and target, then F.l1_loss; trainer.py:736-760) and the
// coverage term F.mse_loss(acc, target) (trainer.py:621-631).  DESIGN.md section 22.
//
// Dilation: out = max over the (2r+1)^2 window clipped to the image, which is max-pool's -inf padding: cells outside the image hold
// -inf, so the identity is not 0.  The max is separable; one block stages a (16+2r) x (32+2r) patch in LDS, takes the row maxima
// into a second LDS array and the column maxima of those.  Values are copied, never computed: bit-exact (a NaN is taken and kept, as
// torch does; between +0 and -0, which compare equal, the first met stays, and the scan order here is not torch's).  r > 16 does not
// fit the static LDS and walks its clipped window in global memory.
//
// Sharp-keep: one thread per OUTPUT element (b, oy, ox, c), c fastest.  Window i of an axis of length L with Lo = L / factor outputs is
// [floor(i L / Lo), ceil((i + 1) L / Lo)) - torch's adaptive average pool.  The window sums of pred, target and mask are taken in
// double (the sum of at most 15 x 15 fp32 values is exact there), d = pbar mbar - tbar mbar is formed without fma contraction, so
// that pbar == tbar gives d == 0 exactly, and |d| goes through the block sum and the ordered total of reduce.h in double.  The
// forward saves g = sign(d) mbar / area per output element (1/factor^2 of the image); the backward reads nothing else: every
// input pixel gathers g from its at most 2 x 2 windows in a fixed order.
//
// Coverage: mean((a - t)^2), t == NULL: the constant 1.  Differences and squares in double, a fixed grid-stride partition, the same
// two-level sum.  No atomics anywhere, nothing is read on the host, every launch is on the caller's stream.
#include <cmath>

#include "common.h"
#include "reduce.h"

namespace {

constexpr int DT_Y = 16, DT_X = 32;  // the dilation's output tile: 256 threads, two outputs each
constexpr int D_RMAX = 16;           // the largest radius of the LDS form
constexpr int MSE_MAX_BLOCKS = 4096;

__device__ __forceinline__ float take_max(float m, float v) { return (v > m || v != v) ? v : m; }  // torch's max-pool update

struct DilateArgs {
  const float *mask;
  float *out, *comp;  // comp may be null
  int B, H, W, r;
};

__global__ void __launch_bounds__(256) k_dilate_tile(const DilateArgs a) {
  __shared__ float patch[(DT_Y + 2 * D_RMAX) * (DT_X + 2 * D_RMAX)];
  __shared__ float rows[(DT_Y + 2 * D_RMAX) * DT_X];
  const int tid = threadIdx.x, r = a.r;
  const int ph = DT_Y + 2 * r, pw = DT_X + 2 * r;
  const int ty0 = blockIdx.y * DT_Y, tx0 = blockIdx.x * DT_X;
  const size_t plane = (size_t)a.H * a.W;
  const float *mask = a.mask + (size_t)blockIdx.z * plane;
  for (int i = tid; i < ph * pw; i += 256) {
    const int cy = i / pw, cx = i - cy * pw;
    const int y = ty0 + cy - r, x = tx0 + cx - r;
    patch[i] = (y >= 0 && y < a.H && x >= 0 && x < a.W) ? mask[(size_t)y * a.W + x] : -INFINITY;
  }
  __syncthreads();
  for (int i = tid; i < ph * DT_X; i += 256) {  // row maxima: consecutive lanes read consecutive LDS words
    const int hy = i / DT_X, hx = i - hy * DT_X;
    const float *p = patch + hy * pw + hx;
    float m = p[0];
    for (int k = 1; k <= 2 * r; k++) m = take_max(m, p[k]);
    rows[i] = m;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int i = tid + j * 256;
    const int ly = i / DT_X, lx = i - ly * DT_X;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y < a.H && x < a.W) {
      float m = rows[ly * DT_X + lx];
      for (int k = 1; k <= 2 * r; k++) m = take_max(m, rows[(ly + k) * DT_X + lx]);
      const size_t q = (size_t)blockIdx.z * plane + (size_t)y * a.W + x;
      a.out[q] = m;
      if (a.comp) a.comp[q] = 1.f - m;
    }
  }
}

// r > D_RMAX: the same tiles, every output walks its own clipped window (row-major, torch's order)
__global__ void __launch_bounds__(256) k_dilate_direct(const DilateArgs a) {
  const size_t plane = (size_t)a.H * a.W;
  const float *mask = a.mask + (size_t)blockIdx.z * plane;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int i = threadIdx.x + j * 256;
    const int y = blockIdx.y * DT_Y + i / DT_X, x = blockIdx.x * DT_X + i % DT_X;
    if (y < a.H && x < a.W) {
      const int y0 = max(y - a.r, 0), y1 = min(y + a.r, a.H - 1), x0 = max(x - a.r, 0), x1 = min(x + a.r, a.W - 1);
      float m = -INFINITY;
      for (int yy = y0; yy <= y1; yy++)
        for (int xx = x0; xx <= x1; xx++) m = take_max(m, mask[(size_t)yy * a.W + xx]);
      const size_t q = (size_t)blockIdx.z * plane + (size_t)y * a.W + x;
      a.out[q] = m;
      if (a.comp) a.comp[q] = 1.f - m;
    }
  }
}

// window i of an axis of length L with Lo outputs: [win_lo, win_hi)
// (H, W <= 32768 and B H W C <= 2^31 - 1, checked on the host: every product below fits 32 bits)
__device__ __forceinline__ int win_lo(int i, int L, int Lo) { return (i * L) / Lo; }
__device__ __forceinline__ int win_hi(int i, int L, int Lo) { return ((i + 1) * L + Lo - 1) / Lo; }

struct KeepArgs {
  const float *pred, *mask, *target;
  int target_reduced;
  int B, H, W, C, Ho, Wo;
  uint32_t n_out;  // B Ho Wo C
  float *map;     // [B,Ho,Wo,C]: sign(d) mbar / area
  double *partials;
};

__global__ void __launch_bounds__(256) k_area_keep_fwd(const KeepArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  double v[1] = {0.0};
  if (e < a.n_out) {
    const int c = (int)(e % (uint32_t)a.C);
    uint32_t w = e / (uint32_t)a.C;
    const int ox = (int)(w % (uint32_t)a.Wo);
    w /= (uint32_t)a.Wo;
    const int oy = (int)(w % (uint32_t)a.Ho), b = (int)(w / (uint32_t)a.Ho);
    const int y0 = win_lo(oy, a.H, a.Ho), y1 = win_hi(oy, a.H, a.Ho), x0 = win_lo(ox, a.W, a.Wo), x1 = win_hi(ox, a.W, a.Wo);
    const bool full = !a.target_reduced;
    double sp = 0.0, st = 0.0, sm = 0.0;
    for (int y = y0; y < y1; y++) {
      const size_t row = ((size_t)b * a.H + y) * a.W;
      for (int x = x0; x < x1; x++) {
        const size_t q = row + x;
        sp += (double)a.pred[q * a.C + c];
        sm += (double)a.mask[q];
        if (full) st += (double)a.target[q * a.C + c];
      }
    }
    const double area = (double)(y1 - y0) * (double)(x1 - x0);
    const double pb = sp / area, mb = sm / area, tb = full ? st / area : (double)a.target[e];
    const double d = pb * mb - tb * mb;
    v[0] = fabs(d);
    const double s = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    a.map[e] = (float)(s * mb / area);
  }
  block_sum_store(v, red);
  __syncthreads();
  if (threadIdx.x == 0) a.partials[blockIdx.x] = block_sum_combine<1>(red, 0);
}

// out[0] = scale * the ordered total of the n block partials
__global__ void __launch_bounds__(256) k_image_terms_finish(const double *partials, int64_t n, double scale, float *out) {
  double t[1];
  ordered_total(partials, n, 1, t);
  if (threadIdx.x == 0) out[0] = (float)(t[0] * scale);
}

struct KeepBwdArgs {
  const float *map, *v_loss;
  int B, H, W, C, Ho, Wo;
  uint32_t n_in;  // B H W C
  float inv_n;   // 1 / (B Ho Wo C)
  float *v_pred;
};

// One thread per input element.  The windows that hold y are i = floor(y Lo / L) .. ceil((y + 1) Lo / L) - 1: one or two.
__global__ void __launch_bounds__(256) k_area_keep_bwd(const KeepBwdArgs a) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= a.n_in) return;
  const int c = (int)(e % (uint32_t)a.C);
  uint32_t w = e / (uint32_t)a.C;
  const int x = (int)(w % (uint32_t)a.W);
  w /= (uint32_t)a.W;
  const int y = (int)(w % (uint32_t)a.H), b = (int)(w / (uint32_t)a.H);
  const int oy0 = (y * a.Ho) / a.H, oy1 = ((y + 1) * a.Ho + a.H - 1) / a.H;
  const int ox0 = (x * a.Wo) / a.W, ox1 = ((x + 1) * a.Wo + a.W - 1) / a.W;
  float g = 0.f;
  for (int oy = oy0; oy < oy1; oy++)
    for (int ox = ox0; ox < ox1; ox++) g += a.map[(((size_t)b * a.Ho + oy) * a.Wo + ox) * a.C + c];
  a.v_pred[e] = a.v_loss[0] * a.inv_n * g;
}

__global__ void __launch_bounds__(256) k_mse_fwd(const float *__restrict__ x, const float *__restrict__ t, int64_t n, double *partials) {
  __shared__ double red[4];
  double v[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double d = (double)x[i] - (t ? (double)t[i] : 1.0);
    v[0] += d * d;
  }
  block_sum_store(v, red);
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = block_sum_combine<1>(red, 0);
}

__global__ void __launch_bounds__(256) k_mse_bwd(const float *__restrict__ x, const float *__restrict__ t, const float *v_loss, int64_t n,
                                                 float k, float *__restrict__ v_x) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v_x[i] = v_loss[0] * k * (x[i] - (t ? t[i] : 1.f));
}

struct PtrArg {
  const void *p;
  const char *name;
  unsigned align;
  bool required;
};

template <int N>
bool pointers_ok(const char *who, const PtrArg (&ptrs)[N]) {
  for (const auto &q : ptrs) {
    if (!q.p && q.required) {
      d4gs_set_error("%s: %s is NULL", who, q.name);
      return false;
    }
    if ((uintptr_t)q.p % q.align) {
      d4gs_set_error("%s: %s = %p is misaligned (%u-byte alignment needed)", who, q.name, q.p, q.align);
      return false;
    }
  }
  return true;
}

bool dilate_sizes_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && W >= 1 && B <= 65535 && ((int64_t)H + DT_Y - 1) / DT_Y <= 65535 && W <= (1 << 30);  // x + r stays an int
}

bool factor_ok(int f) { return f == 1 || f == 2 || f == 4 || f == 8; }

// the output elements B (H / factor) (W / factor) C of the keep loss, or 0: a size < 1, a bad factor, H or W < factor, or more than
// 2^31 - 1 input elements, or H or W above 32768
int64_t keep_out_elems(int B, int H, int W, int C, int factor) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || !factor_ok(factor) || H < factor || W < factor || H > 32768 || W > 32768) return 0;
  if ((double)B * H * W * C > (double)INT32_MAX) return 0;
  return (int64_t)B * (H / factor) * (W / factor) * C;
}

bool keep_sizes_ok(const char *who, int B, int H, int W, int C, int factor) {
  if (B < 1 || H < 1 || W < 1 || C < 1) {
    d4gs_set_error("%s: bad size B=%d H=%d W=%d C=%d (each must be >= 1)", who, B, H, W, C);
    return false;
  }
  if (!factor_ok(factor)) {
    d4gs_set_error("%s: factor=%d (must be 1, 2, 4 or 8)", who, factor);
    return false;
  }
  if (H < factor || W < factor) {
    d4gs_set_error("%s: H=%d W=%d below factor=%d: no output pixel", who, H, W, factor);
    return false;
  }
  if (!keep_out_elems(B, H, W, C, factor)) {
    d4gs_set_error("%s: size B=%d H=%d W=%d C=%d overflows the grid (H, W <= 32768, B H W C <= 2^31 - 1)", who, B, H, W, C);
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

int d4gs_dilate_mask(const float *mask, int32_t B, int32_t H, int32_t W, int32_t r, float *out, float *out_complement, void *stream) {
  const char *who = "d4gs_dilate_mask";
  const PtrArg ptrs[] = {{mask, "mask", 4, true}, {out, "out", 4, true}, {out_complement, "out_complement", 4, false}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (B < 1 || H < 1 || W < 1) {
    d4gs_set_error("%s: bad size B=%d H=%d W=%d (each must be >= 1)", who, B, H, W);
    return D4GS_EINVAL;
  }
  if (r < 0) {
    d4gs_set_error("%s: r=%d (must be >= 0)", who, r);
    return D4GS_EINVAL;
  }
  if (!dilate_sizes_ok(B, H, W)) {
    d4gs_set_error("%s: size B=%d H=%d W=%d overflows the grid (B and ceil(H / 16) <= 65535, W <= 2^30)", who, B, H, W);
    return D4GS_EINVAL;
  }
  DilateArgs a;
  a.mask = mask, a.out = out, a.comp = out_complement, a.B = B, a.H = H, a.W = W;
  a.r = r < (H > W ? H : W) ? r : (H > W ? H : W);  // a window beyond the image is the image
  const dim3 grid((W + DT_X - 1) / DT_X, (H + DT_Y - 1) / DT_Y, B);
  hipStream_t s = (hipStream_t)stream;
  if (a.r <= D_RMAX) {
    D4GS_LAUNCH("k_dilate_tile", k_dilate_tile, grid, dim3(256), 0, s, a);
    return d4gs_check_launch("k_dilate_tile");
  }
  D4GS_LAUNCH("k_dilate_direct", k_dilate_direct, grid, dim3(256), 0, s, a);
  return d4gs_check_launch("k_dilate_direct");
}

int64_t d4gs_area_keep_map_elems(int32_t B, int32_t H, int32_t W, int32_t C, int32_t factor) { return keep_out_elems(B, H, W, C, factor); }

int64_t d4gs_area_keep_blocks(int32_t B, int32_t H, int32_t W, int32_t C, int32_t factor) {
  return (keep_out_elems(B, H, W, C, factor) + 255) / 256;
}

int d4gs_area_keep_fwd(const float *pred, const float *mask, const float *target, int32_t target_reduced, int32_t B, int32_t H,
                       int32_t W, int32_t C, int32_t factor, float *map, double *partials, float *out, void *stream) {
  const char *who = "d4gs_area_keep_fwd";
  const PtrArg ptrs[] = {{pred, "pred", 4, true}, {mask, "mask", 4, true},         {target, "target", 4, true},
                         {map, "map", 4, true},   {partials, "partials", 8, true}, {out, "out", 4, true}};
  if (!pointers_ok(who, ptrs) || !keep_sizes_ok(who, B, H, W, C, factor)) return D4GS_EINVAL;
  KeepArgs a;
  a.pred = pred, a.mask = mask, a.target = target, a.target_reduced = target_reduced != 0;
  a.B = B, a.H = H, a.W = W, a.C = C, a.Ho = H / factor, a.Wo = W / factor;
  a.n_out = (uint32_t)keep_out_elems(B, H, W, C, factor);
  a.map = map, a.partials = partials;
  const int64_t blocks = ((int64_t)a.n_out + 255) / 256;
  hipStream_t s = (hipStream_t)stream;
  D4GS_LAUNCH("k_area_keep_fwd", k_area_keep_fwd, dim3((unsigned)blocks), dim3(256), 0, s, a);
  if (int rc = d4gs_check_launch("k_area_keep_fwd")) return rc;
  D4GS_LAUNCH("k_area_keep_finish", k_image_terms_finish, dim3(1), dim3(256), 0, s, (const double *)partials, blocks, 1.0 / (double)a.n_out,
              out);
  return d4gs_check_launch("k_area_keep_finish");
}

int d4gs_area_keep_bwd(const float *map, const float *v_loss, int32_t B, int32_t H, int32_t W, int32_t C, int32_t factor, float *v_pred,
                       void *stream) {
  const char *who = "d4gs_area_keep_bwd";
  const PtrArg ptrs[] = {{map, "map", 4, true}, {v_loss, "v_loss", 4, true}, {v_pred, "v_pred", 4, true}};
  if (!pointers_ok(who, ptrs) || !keep_sizes_ok(who, B, H, W, C, factor)) return D4GS_EINVAL;
  KeepBwdArgs a;
  a.map = map, a.v_loss = v_loss, a.B = B, a.H = H, a.W = W, a.C = C, a.Ho = H / factor, a.Wo = W / factor;
  a.n_in = (uint32_t)((int64_t)B * H * W * C);
  a.inv_n = (float)(1.0 / (double)keep_out_elems(B, H, W, C, factor));
  a.v_pred = v_pred;
  D4GS_LAUNCH("k_area_keep_bwd", k_area_keep_bwd, dim3((unsigned)(((int64_t)a.n_in + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return d4gs_check_launch("k_area_keep_bwd");
}

int64_t d4gs_mse_blocks(int64_t n) {
  if (n < 1 || n > INT32_MAX) return 0;
  const int64_t b = (n + 255) / 256;
  return b < MSE_MAX_BLOCKS ? b : MSE_MAX_BLOCKS;
}

int d4gs_mse_fwd(const float *a, const float *t, int64_t n, double *partials, float *out, void *stream) {
  const char *who = "d4gs_mse_fwd";
  const PtrArg ptrs[] = {{a, "a", 4, true}, {t, "t", 4, false}, {partials, "partials", 8, true}, {out, "out", 4, true}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  const int64_t blocks = d4gs_mse_blocks(n);
  if (!blocks) {
    d4gs_set_error("%s: bad size n=%lld (1 <= n <= 2^31 - 1)", who, (long long)n);
    return D4GS_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  D4GS_LAUNCH("k_mse_fwd", k_mse_fwd, dim3((unsigned)blocks), dim3(256), 0, s, a, t, n, partials);
  if (int rc = d4gs_check_launch("k_mse_fwd")) return rc;
  D4GS_LAUNCH("k_mse_finish", k_image_terms_finish, dim3(1), dim3(256), 0, s, (const double *)partials, blocks, 1.0 / (double)n, out);
  return d4gs_check_launch("k_mse_finish");
}

int d4gs_mse_bwd(const float *a, const float *t, const float *v_loss, int64_t n, float *v_a, void *stream) {
  const char *who = "d4gs_mse_bwd";
  const PtrArg ptrs[] = {{a, "a", 4, true}, {t, "t", 4, false}, {v_loss, "v_loss", 4, true}, {v_a, "v_a", 4, true}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (n < 1 || n > INT32_MAX) {
    d4gs_set_error("%s: bad size n=%lld (1 <= n <= 2^31 - 1)", who, (long long)n);
    return D4GS_EINVAL;
  }
  D4GS_LAUNCH("k_mse_bwd", k_mse_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, t, v_loss, n,
              (float)(2.0 / (double)n), v_a);
  return d4gs_check_launch("k_mse_bwd");
}

}  // extern "C"
