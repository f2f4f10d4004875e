// warp.hip -- PWC-Net's backward warp (flow3d/models/pwcnet.py: get_backwarp) and the aligned L1 of AlignedLoss.forward
// (flow3d/loss_utils.py) on top of it (include/d4gs.h, "Flow-aligned exposure consistency").
//
// One sampling function serves every kernel here: pixel (x, y) with flow (fx, fy) samples the input bilinearly, zeros outside, at
// (x + fx W / (W - 1), y + fy H / (H - 1)) - the reference divides the flow by (W - 1) / 2 on an align_corners=False grid, which
// leaves that factor.  The displacement is formed in double and split into its integer and fractional part BEFORE the pixel index
// is added, so the bilinear weights carry the displacement's precision and not the coordinate's.  The coverage is the sum of the
// in-bounds weights; mask = coverage > 0.999.  Gradients go to the sampled image only: a scatter with float atomics (the forward
// sums are ordered and reproducible, the scattered gradient is not bitwise so).
#include "common.h"
#include "reduce.h"

namespace {

constexpr int WB = REDUCE_NT;
constexpr int WARP_MAX_BLOCKS = 4096;
constexpr int AL1_MAX_BLOCKS = 128;  // per pair
constexpr int AL1_C = 3;

struct Taps {
  int x0, y0;
  float w[4];   // (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1); 0 for a tap outside the image
  float cover;  // their sum
};

// integer and fractional part of a displacement; anything that leaves the image from every pixel is clamped (NaN too)
__device__ __forceinline__ void warp_split(float f, int n, int &i0, float &t) {
  double d = (double)f * ((double)n / (double)(n - 1));
  d = fmin(fmax(d, -(double)(n + 1)), (double)(n + 1));
  const double fl = floor(d);
  i0 = (int)fl, t = (float)(d - fl);
}

__device__ __forceinline__ Taps warp_taps(float fx, float fy, int x, int y, int H, int W) {
  Taps s;
  float tx, ty;
  warp_split(fx, W, s.x0, tx);
  warp_split(fy, H, s.y0, ty);
  s.x0 += x, s.y0 += y;
  const float wx0 = s.x0 >= 0 && s.x0 < W ? 1.f - tx : 0.f, wx1 = s.x0 + 1 >= 0 && s.x0 + 1 < W ? tx : 0.f;
  const float wy0 = s.y0 >= 0 && s.y0 < H ? 1.f - ty : 0.f, wy1 = s.y0 + 1 >= 0 && s.y0 + 1 < H ? ty : 0.f;
  s.w[0] = wy0 * wx0, s.w[1] = wy0 * wx1, s.w[2] = wy1 * wx0, s.w[3] = wy1 * wx1;
  s.cover = (s.w[0] + s.w[1]) + (s.w[2] + s.w[3]);
  return s;
}

// offset of tap i from the image plane's base; only dereferenced where w[i] != 0 (the tap is inside)
__device__ __forceinline__ int64_t tap_at(const Taps &s, int i, int W) { return (int64_t)(s.y0 + (i >> 1)) * W + s.x0 + (i & 1); }

__device__ __forceinline__ float warp_sample(const float *__restrict__ img, const Taps &s, int W) {
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (s.w[i] != 0.f) v += s.w[i] * img[tap_at(s, i, W)];
  return v;
}

__device__ __forceinline__ void warp_scatter(float *__restrict__ img, const Taps &s, int W, float g) {
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (s.w[i] != 0.f) atomicAdd(&img[tap_at(s, i, W)], s.w[i] * g);
}

__global__ void __launch_bounds__(WB) k_backwarp_fwd(const float *__restrict__ input, const float *__restrict__ flow, int64_t n_pix, int C,
                                                     int H, int W, float *__restrict__ out, float *__restrict__ mask) {
  const int64_t plane = (int64_t)H * W, stride = (int64_t)gridDim.x * WB;
  for (int64_t p = (int64_t)blockIdx.x * WB + threadIdx.x; p < n_pix; p += stride) {
    const int64_t b = p / plane, r = p % plane;
    const int y = (int)(r / W), x = (int)(r % W);
    const Taps s = warp_taps(flow[b * 2 * plane + r], flow[(b * 2 + 1) * plane + r], x, y, H, W);
    const float m = s.cover > 0.999f ? 1.f : 0.f;
    mask[p] = m;
    for (int c = 0; c < C; c++) out[(b * C + c) * plane + r] = m != 0.f ? warp_sample(input + (b * C + c) * plane, s, W) : 0.f;
  }
}

__global__ void __launch_bounds__(WB) k_backwarp_bwd(const float *__restrict__ flow, const float *__restrict__ v_out, int64_t n_pix, int C,
                                                     int H, int W, float *__restrict__ v_input) {
  const int64_t plane = (int64_t)H * W, stride = (int64_t)gridDim.x * WB;
  for (int64_t p = (int64_t)blockIdx.x * WB + threadIdx.x; p < n_pix; p += stride) {
    const int64_t b = p / plane, r = p % plane;
    const int y = (int)(r / W), x = (int)(r % W);
    const Taps s = warp_taps(flow[b * 2 * plane + r], flow[(b * 2 + 1) * plane + r], x, y, H, W);
    if (!(s.cover > 0.999f)) continue;
    for (int c = 0; c < C; c++) warp_scatter(v_input + (b * C + c) * plane, s, W, v_out[(b * C + c) * plane + r]);
  }
}

// what one pixel of pair p contributes: a - b per channel with a = warp(pred) mm, b = target mm, mm = coverage mask * mask
struct Al1Pixel {
  Taps s;
  float mm;
};
__device__ __forceinline__ Al1Pixel al1_pixel(const float *__restrict__ flow, const float *__restrict__ mask, int64_t p, int64_t r, int H, int W) {
  const int64_t plane = (int64_t)H * W;
  const int y = (int)(r / W), x = (int)(r % W);
  Al1Pixel q;
  q.s = warp_taps(flow[p * 2 * plane + r], flow[(p * 2 + 1) * plane + r], x, y, H, W);
  q.mm = q.s.cover > 0.999f ? (mask ? mask[p * plane + r] : 1.f) : 0.f;
  return q;
}
__device__ __forceinline__ float al1_diff(const float *__restrict__ pred, const float *__restrict__ target, const Al1Pixel &q, int64_t chan,
                                          int64_t r, int H, int W) {
#pragma clang fp contract(off)
  const int64_t plane = (int64_t)H * W;
  if (q.mm == 0.f) return 0.f;
  return warp_sample(pred + chan * plane, q.s, W) * q.mm - target[chan * plane + r] * q.mm;
}

__global__ void __launch_bounds__(WB) k_al1_fwd(const float *__restrict__ pred, const float *__restrict__ flow, const float *__restrict__ target,
                                                const float *__restrict__ mask, int H, int W, double *__restrict__ partials) {
  __shared__ double red[WB / 64];
  const int64_t p = blockIdx.y, plane = (int64_t)H * W;
  double sum[1] = {0.0};
  for (int64_t r = (int64_t)blockIdx.x * WB + threadIdx.x; r < plane; r += (int64_t)gridDim.x * WB) {
    const Al1Pixel q = al1_pixel(flow, mask, p, r, H, W);
    for (int c = 0; c < AL1_C; c++) sum[0] += (double)fabsf(al1_diff(pred, target, q, p * AL1_C + c, r, H, W));
  }
  block_sum_store(sum, red);
  __syncthreads();
  if (threadIdx.x == 0) partials[p * gridDim.x + blockIdx.x] = block_sum_combine<1>(red, 0);
}

// one block per pair adds its partials in a fixed order
__global__ void __launch_bounds__(WB) k_al1_finish(const double *__restrict__ partials, int n_blocks, double inv_n, float *__restrict__ losses) {
  double t[1];
  ordered_total(partials + (int64_t)blockIdx.x * n_blocks, n_blocks, 1, t);
  if (threadIdx.x == 0) losses[blockIdx.x] = (float)(t[0] * inv_n);
}

__global__ void __launch_bounds__(WB) k_al1_bwd(const float *__restrict__ pred, const float *__restrict__ flow, const float *__restrict__ target,
                                                const float *__restrict__ mask, const float *__restrict__ v_loss, int H, int W, float inv_n,
                                                float *__restrict__ v_pred, float *__restrict__ v_target) {
  const int64_t p = blockIdx.y, plane = (int64_t)H * W;
  const float scale = v_loss[p] * inv_n;
  for (int64_t r = (int64_t)blockIdx.x * WB + threadIdx.x; r < plane; r += (int64_t)gridDim.x * WB) {
    const Al1Pixel q = al1_pixel(flow, mask, p, r, H, W);
    for (int c = 0; c < AL1_C; c++) {
      const float d = al1_diff(pred, target, q, p * AL1_C + c, r, H, W);
      const float g = d > 0.f ? scale * q.mm : (d < 0.f ? -scale * q.mm : 0.f);  // sign(0) = 0, as torch
      if (g != 0.f && v_pred) warp_scatter(v_pred + (p * AL1_C + c) * plane, q.s, W, g);
      if (v_target) v_target[(p * AL1_C + c) * plane + r] = -g;
    }
  }
}

int warp_check(const char *who, int32_t B, int32_t C, int32_t H, int32_t W) {
  if (B < 1 || C < 1) {
    d4gs_set_error("%s: bad size B=%d C=%d (each >= 1)", who, B, C);
    return D4GS_EINVAL;
  }
  if (H < 2 || W < 2) {
    d4gs_set_error("%s: H=%d W=%d (each >= 2: the flow is scaled by W / (W - 1) and H / (H - 1))", who, H, W);
    return D4GS_EINVAL;
  }
  if ((int64_t)B * C * H * W > ((int64_t)1 << 40) || B > 65535) {
    d4gs_set_error("%s: size B=%d C=%d H=%d W=%d is too large (B <= 65535, at most 2^40 elements)", who, B, C, H, W);
    return D4GS_EINVAL;
  }
  return D4GS_OK;
}

unsigned warp_blocks(int64_t n, int cap) {
  const int64_t b = (n + WB - 1) / WB;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// the scatter targets are zeroed by a kernel, not by a memset node (reduce.h)
int warp_zero(float *p, int64_t n, hipStream_t stream) {
  D4GS_LAUNCH("k_zero_f32", k_zero_f32<>, dim3(warp_blocks(n, WARP_MAX_BLOCKS)), dim3(WB), 0, stream, p, n);
  return d4gs_check_launch("k_zero_f32");
}

}  // namespace

extern "C" {

int d4gs_backwarp_fwd(const float *input, const float *flow, int32_t B, int32_t C, int32_t H, int32_t W, float *out, float *mask,
                      void *stream) {
  if (!input || !flow || !out || !mask) {
    d4gs_set_error("d4gs_backwarp_fwd: NULL argument");
    return D4GS_EINVAL;
  }
  if (int rc = warp_check("d4gs_backwarp_fwd", B, C, H, W)) return rc;
  const int64_t n_pix = (int64_t)B * H * W;
  D4GS_LAUNCH("k_backwarp_fwd", k_backwarp_fwd, dim3(warp_blocks(n_pix, WARP_MAX_BLOCKS)), dim3(WB), 0, (hipStream_t)stream, input, flow, n_pix,
              (int)C, (int)H, (int)W, out, mask);
  return d4gs_check_launch("k_backwarp_fwd");
}

int d4gs_backwarp_bwd(const float *flow, const float *v_out, int32_t B, int32_t C, int32_t H, int32_t W, float *v_input, void *stream) {
  if (!flow || !v_out || !v_input) {
    d4gs_set_error("d4gs_backwarp_bwd: NULL argument");
    return D4GS_EINVAL;
  }
  if (int rc = warp_check("d4gs_backwarp_bwd", B, C, H, W)) return rc;
  const int64_t n_pix = (int64_t)B * H * W;
  if (int rc = warp_zero(v_input, n_pix * C, (hipStream_t)stream)) return rc;
  D4GS_LAUNCH("k_backwarp_bwd", k_backwarp_bwd, dim3(warp_blocks(n_pix, WARP_MAX_BLOCKS)), dim3(WB), 0, (hipStream_t)stream, flow, v_out, n_pix,
              (int)C, (int)H, (int)W, v_input);
  return d4gs_check_launch("k_backwarp_bwd");
}

int64_t d4gs_aligned_l1_blocks(int32_t H, int32_t W) {
  if (H < 1 || W < 1) return 0;
  return warp_blocks((int64_t)H * W, AL1_MAX_BLOCKS);
}

int d4gs_aligned_l1_fwd(const float *pred, const float *flow, const float *target, const float *mask, int32_t P, int32_t H, int32_t W,
                        double *partials, float *losses, void *stream) {
  if (!pred || !flow || !target || !partials || !losses) {
    d4gs_set_error("d4gs_aligned_l1_fwd: NULL argument (only the mask is optional)");
    return D4GS_EINVAL;
  }
  if ((uintptr_t)partials % 8) {
    d4gs_set_error("d4gs_aligned_l1_fwd: partials at %p must be 8-byte aligned", (void *)partials);
    return D4GS_EINVAL;
  }
  if (int rc = warp_check("d4gs_aligned_l1_fwd", P, AL1_C, H, W)) return rc;
  const unsigned nb = warp_blocks((int64_t)H * W, AL1_MAX_BLOCKS);
  D4GS_LAUNCH("k_al1_fwd", k_al1_fwd, dim3(nb, P), dim3(WB), 0, (hipStream_t)stream, pred, flow, target, mask, (int)H, (int)W, partials);
  if (int rc = d4gs_check_launch("k_al1_fwd")) return rc;
  D4GS_LAUNCH("k_al1_finish", k_al1_finish, dim3(P), dim3(WB), 0, (hipStream_t)stream, (const double *)partials, (int)nb,
              1.0 / ((double)AL1_C * H * W), losses);
  return d4gs_check_launch("k_al1_finish");
}

int d4gs_aligned_l1_bwd(const float *pred, const float *flow, const float *target, const float *mask, const float *v_loss, int32_t P,
                        int32_t H, int32_t W, float *v_pred, float *v_target, void *stream) {
  if (!pred || !flow || !target || !v_loss || !v_pred) {
    d4gs_set_error("d4gs_aligned_l1_bwd: NULL argument (only the mask and v_target are optional)");
    return D4GS_EINVAL;
  }
  if (int rc = warp_check("d4gs_aligned_l1_bwd", P, AL1_C, H, W)) return rc;
  if (int rc = warp_zero(v_pred, (int64_t)P * AL1_C * H * W, (hipStream_t)stream)) return rc;
  const unsigned nb = warp_blocks((int64_t)H * W, AL1_MAX_BLOCKS);
  D4GS_LAUNCH("k_al1_bwd", k_al1_bwd, dim3(nb, P), dim3(WB), 0, (hipStream_t)stream, pred, flow, target, mask, v_loss, (int)H, (int)W,
              (float)(1.0 / ((double)AL1_C * H * W)), v_pred, v_target);
  return d4gs_check_launch("k_al1_bwd");
}

}  // extern "C"
