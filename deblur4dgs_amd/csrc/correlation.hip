// correlation.hip -- PWC-Net's 9x9 cost volume, forward and backward (include/d4gs.h, "Flow-aligned exposure consistency").
//
//   out[b, (dy+4)*9 + (dx+4), y, x] = lrelu( (1/C) * sum_c first[b,c,y,x] * second[b,c,y+dy,x+dx] ),  dx, dy in -4..4, zero outside
//
// A workgroup owns a 32 x 8 pixel tile of one batch item.  Per chunk of CORR_CH channels it stages the tile of the shifted operand
// plus its 4-pixel halo in LDS (zeros outside the image and beyond the last channel), straight from the NCHW input: no padded or
// channel-last copy is made.  A lane keeps the 81 values of its pixel in registers - the accumulators in the forward, the incoming
// gradients in the two backward gathers - and reads the 81 window positions at compile-time offsets from one LDS address.  A
// 32-lane half of a wave reads 32 consecutive dwords of one LDS row: no bank conflict.  The channel sum (forward) and the window sum
// (backward) run in a fixed order and nothing is atomic: the same input gives the same bits.
#include "common.h"

namespace {

constexpr int CORR_TX = 32, CORR_TY = 8, CORR_R = 4, CORR_D = 2 * CORR_R + 1, CORR_K = CORR_D * CORR_D;
constexpr int CORR_TB = CORR_TX * CORR_TY;
constexpr int CORR_CH = 8;  // channels staged per round: 8 x 16 x 40 floats = 20 KB
// waves per SIMD asked of the compiler: the forward fits its 81 accumulators and the window values in flight into 128 VGPRs; the backward
// gathers, whose prologue has 81 gradient and 81 saved-output loads in flight, spill at 128 and at 168 and get 256
constexpr int CORR_WAVES = 4, CORR_WAVES_BWD = 2;
constexpr int CORR_LW = CORR_TX + 2 * CORR_R, CORR_LH = CORR_TY + 2 * CORR_R, CORR_PLANE = CORR_LW * CORR_LH;

// channels [c0, c0 + CORR_CH) of src (one batch item, [C,H,W]) over the tile at (x0, y0) and its halo -> t
__device__ __forceinline__ void corr_stage(const float *__restrict__ src, int c0, int C, int H, int W, int x0, int y0, float *t) {
  for (int i = threadIdx.x; i < CORR_CH * CORR_PLANE; i += CORR_TB) {
    const int c = c0 + i / CORR_PLANE, r = i % CORR_PLANE;
    const int gy = y0 + r / CORR_LW - CORR_R, gx = x0 + r % CORR_LW - CORR_R;
    const bool in = c < C && gy >= 0 && gy < H && gx >= 0 && gx < W;
    t[i] = in ? src[((int64_t)c * H + gy) * W + gx] : 0.f;
  }
}

__global__ void __launch_bounds__(CORR_TB, CORR_WAVES) k_corr_fwd(const float *__restrict__ first, const float *__restrict__ second, int C, int H,
                                                                  int W, float inv_c, float slope, float *__restrict__ out) {
  __shared__ float t[CORR_CH * CORR_PLANE];
  __shared__ float tf[CORR_CH * CORR_TB];  // the lanes' own `first` values of the round (a register array indexed by the channel would spill)
  const int lx = threadIdx.x % CORR_TX, ly = threadIdx.x / CORR_TX;
  const int x0 = blockIdx.x * CORR_TX, y0 = blockIdx.y * CORR_TY, b = blockIdx.z;
  const int x = x0 + lx, y = y0 + ly;
  const bool live = x < W && y < H;
  const int64_t plane = (int64_t)H * W, pix = (int64_t)y * W + x;
  const float *fb = first + (int64_t)b * C * plane, *sb = second + (int64_t)b * C * plane;
  const float *mine = t + (ly + CORR_R) * CORR_LW + lx + CORR_R;
  float acc[CORR_K];
#pragma unroll
  for (int k = 0; k < CORR_K; k++) acc[k] = 0.f;
  for (int c0 = 0; c0 < C; c0 += CORR_CH) {
    __syncthreads();  // the previous round's reads are done
    corr_stage(sb, c0, C, H, W, x0, y0, t);
#pragma unroll
    for (int j = 0; j < CORR_CH; j++) tf[j * CORR_TB + threadIdx.x] = live && c0 + j < C ? fb[(int64_t)(c0 + j) * plane + pix] : 0.f;
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < CORR_CH; j++) {  // (a channel beyond C adds 0 * 0)
      const float f = tf[j * CORR_TB + threadIdx.x];
      const float *row = mine + j * CORR_PLANE;
#pragma unroll
      for (int dy = -CORR_R; dy <= CORR_R; dy++)
#pragma unroll
        for (int dx = -CORR_R; dx <= CORR_R; dx++) acc[(dy + CORR_R) * CORR_D + dx + CORR_R] += f * row[dy * CORR_LW + dx];
    }
  }
  if (!live) return;
  float *o = out + (int64_t)b * CORR_K * plane + pix;
#pragma unroll
  for (int k = 0; k < CORR_K; k++) {
    const float v = acc[k] * inv_c;
    o[(int64_t)k * plane] = v > 0.f ? v : v * slope;
  }
}

// v_out through the fused leaky ReLU: the slope applies where the saved output is not positive (torch's rule, 0 included)
__device__ __forceinline__ float corr_g(const float *__restrict__ v_out, const float *__restrict__ out, int64_t i, float slope) {
  const float v = v_out[i];
  return out && !(out[i] > 0.f) ? v * slope : v;
}

// SECOND == false: v_first[b,c,y,x]  = (1/C) sum_k g[b,k,y,x]       * second[b,c,y+dy,x+dx]   (src = second)
// SECOND == true:  v_second[b,c,y,x] = (1/C) sum_k g[b,k,y-dy,x-dx] * first[b,c,y-dy,x-dx]    (src = first)
// Either way a lane holds its pixel's 81 factors g in registers and gathers one output value per channel from the LDS tile.
template <bool SECOND>
__global__ void __launch_bounds__(CORR_TB, CORR_WAVES_BWD) k_corr_bwd(const float *__restrict__ src, const float *__restrict__ out,
                                                                  const float *__restrict__ v_out, int C, int H, int W, double inv_c, float slope,
                                                                  float *__restrict__ dst) {
  __shared__ float t[CORR_CH * CORR_PLANE];
  const int lx = threadIdx.x % CORR_TX, ly = threadIdx.x / CORR_TX;
  const int x0 = blockIdx.x * CORR_TX, y0 = blockIdx.y * CORR_TY, b = blockIdx.z;
  const int x = x0 + lx, y = y0 + ly;
  const bool live = x < W && y < H;
  const int64_t plane = (int64_t)H * W, pix = (int64_t)y * W + x;
  const float *sb = src + (int64_t)b * C * plane;
  const float *mine = t + (ly + CORR_R) * CORR_LW + lx + CORR_R;
  const int64_t vol = (int64_t)b * CORR_K * plane;
  constexpr int SGN = SECOND ? -1 : 1;
  float g[CORR_K];
#pragma unroll
  for (int dy = -CORR_R; dy <= CORR_R; dy++)
#pragma unroll
    for (int dx = -CORR_R; dx <= CORR_R; dx++) {
      const int k = (dy + CORR_R) * CORR_D + dx + CORR_R;
      const int gy = SECOND ? y - dy : y, gx = SECOND ? x - dx : x;  // the pixel whose window holds (y, x) at offset (dy, dx)
      const bool in = live && gy >= 0 && gy < H && gx >= 0 && gx < W;
      g[k] = in ? corr_g(v_out, out, vol + (int64_t)k * plane + (int64_t)gy * W + gx, slope) : 0.f;
    }
  for (int c0 = 0; c0 < C; c0 += CORR_CH) {
    __syncthreads();
    corr_stage(sb, c0, C, H, W, x0, y0, t);
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < CORR_CH; j++) {
      const float *row = mine + j * CORR_PLANE;
      // in double: a pixel near a corner of a small image has a handful of non-zero terms, and 81 2^-23 mean_k(|v| |x|) / C is then two
      // roundings of their sum - fp32 recursive summation spends one per term.  Here the one rounding is the store's.
      double s = 0.0;
#pragma unroll
      for (int dy = -CORR_R; dy <= CORR_R; dy++)
#pragma unroll
        for (int dx = -CORR_R; dx <= CORR_R; dx++)
          s += (double)g[(dy + CORR_R) * CORR_D + dx + CORR_R] * (double)row[SGN * (dy * CORR_LW + dx)];
      if (live && c0 + j < C) dst[(int64_t)b * C * plane + (int64_t)(c0 + j) * plane + pix] = (float)(s * inv_c);
    }
  }
}

int corr_check(const char *who, int32_t B, int32_t C, int32_t H, int32_t W) {
  if (B < 1 || C < 1 || H < 1 || W < 1) {
    d4gs_set_error("%s: bad size B=%d C=%d H=%d W=%d (each >= 1)", who, B, C, H, W);
    return D4GS_EINVAL;
  }
  if (B > 65535 || (H + CORR_TY - 1) / CORR_TY > 65535 || (int64_t)B * (C > CORR_K ? C : CORR_K) * H * W > ((int64_t)1 << 40)) {
    d4gs_set_error("%s: size B=%d C=%d H=%d W=%d is beyond the launch grid (B <= 65535, H <= 524280, at most 2^40 elements)", who, B, C, H, W);
    return D4GS_EINVAL;
  }
  return D4GS_OK;
}

dim3 corr_grid(int32_t B, int32_t H, int32_t W) { return dim3((W + CORR_TX - 1) / CORR_TX, (H + CORR_TY - 1) / CORR_TY, B); }

}  // namespace

extern "C" {

int d4gs_correlation_fwd(const float *first, const float *second, int32_t B, int32_t C, int32_t H, int32_t W, float negative_slope,
                         float *out, void *stream) {
  if (!first || !second || !out) {
    d4gs_set_error("d4gs_correlation_fwd: NULL argument (first, second and out are required)");
    return D4GS_EINVAL;
  }
  if (int rc = corr_check("d4gs_correlation_fwd", B, C, H, W)) return rc;
  D4GS_LAUNCH("k_corr_fwd", k_corr_fwd, corr_grid(B, H, W), dim3(CORR_TB), 0, (hipStream_t)stream, first, second, (int)C, (int)H, (int)W,
              1.f / (float)C, negative_slope, out);
  return d4gs_check_launch("k_corr_fwd");
}

int d4gs_correlation_bwd(const float *first, const float *second, const float *out, const float *v_out, int32_t B, int32_t C, int32_t H,
                         int32_t W, float negative_slope, float *v_first, float *v_second, void *stream) {
  if (!first || !second || !v_out) {
    d4gs_set_error("d4gs_correlation_bwd: NULL argument (first, second and v_out are required)");
    return D4GS_EINVAL;
  }
  if (!out && negative_slope != 1.f) {
    d4gs_set_error("d4gs_correlation_bwd: NULL out with negative_slope=%g (the saved output is needed unless the slope is 1)",
                   (double)negative_slope);
    return D4GS_EINVAL;
  }
  if (int rc = corr_check("d4gs_correlation_bwd", B, C, H, W)) return rc;
  const float *o = negative_slope == 1.f ? nullptr : out;
  const double inv_c = 1.0 / (double)C;
  if (v_first) {
    D4GS_LAUNCH("k_corr_bwd_first", k_corr_bwd<false>, corr_grid(B, H, W), dim3(CORR_TB), 0, (hipStream_t)stream, second, o, v_out, (int)C,
                (int)H, (int)W, inv_c, negative_slope, v_first);
    if (int rc = d4gs_check_launch("k_corr_bwd_first")) return rc;
  }
  if (v_second) {
    D4GS_LAUNCH("k_corr_bwd_second", k_corr_bwd<true>, corr_grid(B, H, W), dim3(CORR_TB), 0, (hipStream_t)stream, first, o, v_out, (int)C,
                (int)H, (int)W, inv_c, negative_slope, v_second);
    if (int rc = d4gs_check_launch("k_corr_bwd_second")) return rc;
  }
  return D4GS_OK;
}

}  // extern "C"
