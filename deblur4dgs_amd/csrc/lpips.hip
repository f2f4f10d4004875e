// lpips.hip -- everything of the validator's LPIPS metric that is not a convolution (models/networks_basic.py:PNetLin with the AlexNet
// trunk, version 0.1; flow3d/metrics.py:250-279), fused.  DESIGN.md section 29.  The trunk's five convolutions stay with MIOpen
// (deblur4dgs_amd/lpips.py); around them torch spends ~60 launches per image pair.  Here:
//
//   k_lpips_prepare   one launch: channel-last pred / target [B,H,W,3] and M masks -> the trunk's input [2,M,B,3,H,W],
//                     ((x * mask) * 2 - 1 - shift) / scale in the reference's fp32 operation order, bit for bit (no contraction, an
//                     IEEE division and not a multiplication by a reciprocal);
//   k_lpips_layer     one launch per layer: two feature tensors [n,C,h,w] and C head weights -> d [n,h,w],
//                     d = sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2 in the direct form: identical inputs give exactly 0;
//   k_lpips_score     one launch: the five maps upsampled to H x W (bilinear, align_corners=False), added in layer order, written as the
//                     score map and summed under each mask by block partials;  k_lpips_finish: the ordered total per (m, b);
//   k_lpips_mean      one launch: the mean over h x w of every layer map, added in layer order, per image pair.
//
// No atomics, nothing read on the host, every sum in the fixed order of reduce.h: bitwise reproducible.  Forward only.
//
// Numerics.  The layer kernel works in double from the fp32 features on: the norm is a sum of exact squares, g = f / (n + 1e-10) is a
// division (with one channel both g are 1 - 1e-10 / f, and their difference survives only if each is correctly rounded; a multiplication
// by a rounded reciprocal loses it), and the weighted squares are added in double; one rounding to fp32 at the end.  The score kernel takes
// source coordinates, interpolation and the five-layer sum in double as well (an fp32 source coordinate at x = 500 is off by ~1e-5 of a
// cell, which the interpolation weight passes on); the map is rounded to fp32 once, and the masked sum adds exactly those fp32 values.
#include "common.h"
#include "reduce.h"

namespace {

constexpr int LL = 5;                 // layers
constexpr int LP_MIN = 31;            // the smallest H, W that leaves every layer map at least 1 x 1
constexpr int LP_MAX_C = 4096;
constexpr int LP_WIDE_C = 128;        // from this many channels on, 16 pixels x 16 channel slices per block; below, 64 x 4
constexpr double LP_EPS = 1e-10;      // normalize_tensor's eps

struct PrepareArgs {
  const float *pred, *target;  // [B,H,W,3]
  const float *masks;          // [M,B,H,W] or null
  float *out;                  // [2,M,B,3,H,W]
  int M, B, normalize;
  int64_t plane;  // H * W
  int64_t total;  // 2 * M * B * plane
};

// one thread per (which, m, b, pixel): three channels in, three planes out
__global__ void __launch_bounds__(256) k_lpips_prepare(const PrepareArgs a) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int64_t q = i % a.plane, img = i / a.plane;  // img = (which * M + m) * B + b
  const int b = (int)(img % a.B), m = (int)((img / a.B) % a.M), which = (int)(img / ((int64_t)a.B * a.M));
  const float *src = (which ? a.target : a.pred) + ((int64_t)b * a.plane + q) * 3;
  const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
  float v[3] = {src[0], src[1], src[2]};
  if (a.masks) {
    const float mk = a.masks[((int64_t)m * a.B + b) * a.plane + q];
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = v[c] * mk;
  }
  float *dst = a.out + img * 3 * a.plane + q;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float x = v[c];
    if (a.normalize) x = x * 2.f - 1.f;
    dst[c * a.plane] = (x - shift[c]) / scale[c];
  }
}

struct LayerArgs {
  const float *f0, *f1;  // [n,C,h,w]
  const float *w;        // [C]
  float *out;            // [n,h,w]
  int C;
  int64_t plane;  // h * w
  int64_t total;  // n * plane
};

// PX pixels x S = 256 / PX channel slices per block: thread t has pixel t % PX of the block and the channels c = s, s + S, ... of slice
// s = t / PX, so neighbouring lanes read neighbouring addresses of one channel plane.  The S partial sums of a pixel are combined as
// reduce.h combines a block sum: the slices inside a wave by butterfly (o = 32, 16: PX = 16 only), then the four waves as
// (s_0 + s_1) + (s_2 + s_3) behind one barrier.  Two passes over the channels: the norms, then the weighted squares.
template <int PX>
__device__ __forceinline__ double slice_sum(double v, double *red) {
  constexpr int PER_WAVE = D4GS_WAVE / PX;  // slices inside one wave: 1 or 4
#pragma unroll
  for (int o = 32; o >= PX && PER_WAVE > 1; o >>= 1) v += __shfl_xor(v, o);
  const int wave = threadIdx.x / D4GS_WAVE, px = threadIdx.x % PX;
  __syncthreads();  // the previous use of red is over
  if ((threadIdx.x % D4GS_WAVE) < PX) red[wave * PX + px] = v;
  __syncthreads();
  return (red[px] + red[PX + px]) + (red[2 * PX + px] + red[3 * PX + px]);
}

template <int PX>
__global__ void __launch_bounds__(256) k_lpips_layer(const LayerArgs a) {
  constexpr int S = 256 / PX;
  __shared__ double red[4 * PX];
  const int px = threadIdx.x % PX, s = threadIdx.x / PX;
  const int64_t i = (int64_t)blockIdx.x * PX + px;  // pixel of [n, plane]
  const bool live = i < a.total;
  const int64_t img = live ? i / a.plane : 0, q = live ? i - img * a.plane : 0;
  const float *p0 = a.f0 + img * a.C * a.plane + q, *p1 = a.f1 + img * a.C * a.plane + q;
  double n0 = 0.0, n1 = 0.0;
  if (live)
    for (int c = s; c < a.C; c += S) {
      const double x0 = p0[c * a.plane], x1 = p1[c * a.plane];
      n0 += x0 * x0, n1 += x1 * x1;
    }
  n0 = slice_sum<PX>(n0, red), n1 = slice_sum<PX>(n1, red);
  const double m0 = sqrt(n0) + LP_EPS, m1 = sqrt(n1) + LP_EPS;
  double d = 0.0;
  if (live)
    for (int c = s; c < a.C; c += S) {
#pragma clang fp contract(off)
      const double g0 = (double)p0[c * a.plane] / m0, g1 = (double)p1[c * a.plane] / m1;
      const double e = g0 - g1;
      d += (double)a.w[c] * (e * e);
    }
  d = slice_sum<PX>(d, red);
  if (live && s == 0) a.out[i] = (float)d;
}

struct ScoreArgs {
  const float *layer[LL];  // [M*B, h_k, w_k]
  int h[LL], w[LL];
  double ry[LL], rx[LL];  // 1 / scale_factor, scale_factor = 1. * H / h as the reference passes it
  const float *masks;     // [M,B,H,W] or null (ones)
  float *map;             // [M,B,H,W] or null
  double *partials;       // [M*B, blocks per image, 2]
  int H, W;
};

// torch's source cell and weight of destination index `dst` (area_pixel_compute_source_index, align_corners=False)
__device__ __forceinline__ void source_of(int dst, double r, int size, int &i0, int &i1, double &l1) {
  const double s = fmax(r * (dst + 0.5) - 0.5, 0.0);
  i0 = min((int)s, size - 1);
  i1 = min(i0 + 1, size - 1);
  l1 = s - i0;
}

// one thread per output pixel, blockIdx.y = (m, b); partial j of a block: sum score * mask, sum mask
__global__ void __launch_bounds__(256) k_lpips_score(const ScoreArgs a) {
  __shared__ double red[2 * 4];
  const int mb = blockIdx.y;
  const int64_t plane = (int64_t)a.H * a.W, q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double v[2] = {0.0, 0.0};
  if (q < plane) {
#pragma clang fp contract(off)
    const int y = (int)(q / a.W), x = (int)(q - (int64_t)y * a.W);
    double score = 0.0;
#pragma unroll
    for (int k = 0; k < LL; k++) {
      int y0, y1, x0, x1;
      double ly, lx;
      source_of(y, a.ry[k], a.h[k], y0, y1, ly);
      source_of(x, a.rx[k], a.w[k], x0, x1, lx);
      const float *p = a.layer[k] + (int64_t)mb * a.h[k] * a.w[k];
      const double v00 = p[(int64_t)y0 * a.w[k] + x0], v01 = p[(int64_t)y0 * a.w[k] + x1];
      const double v10 = p[(int64_t)y1 * a.w[k] + x0], v11 = p[(int64_t)y1 * a.w[k] + x1];
      const double up = (1.0 - ly) * ((1.0 - lx) * v00 + lx * v01) + ly * ((1.0 - lx) * v10 + lx * v11);
      score = k ? score + up : up;
    }
    const float sf = (float)score;
    if (a.map) a.map[(int64_t)mb * plane + q] = sf;
    const double m = a.masks ? (double)a.masks[(int64_t)mb * plane + q] : 1.0;
    v[0] = (double)sf * m, v[1] = m;
  }
  block_sum_store(v, red);
  __syncthreads();
  if (threadIdx.x < 2) a.partials[((int64_t)mb * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = block_sum_combine<2>(red, threadIdx.x);
}

// one block per (m, b): out[mb] = sum score * mask, sum mask
__global__ void __launch_bounds__(256) k_lpips_finish(const double *partials, int blocks, double *out) {
  double t[2];
  ordered_total(partials + (int64_t)blockIdx.x * blocks * 2, blocks, 2, t);
  if (threadIdx.x < 2) out[(int64_t)blockIdx.x * 2 + threadIdx.x] = t[threadIdx.x];
}

struct MeanArgs {
  const float *layer[LL];  // [n, h_k, w_k]
  int64_t plane[LL];
  double *out;  // [n]
};

// one block per image pair: the five layer means, each an ordered total in double, added in layer order
__global__ void __launch_bounds__(256) k_lpips_mean(const MeanArgs a) {
  double sum = 0.0;
  for (int k = 0; k < LL; k++) {
    double t[1];
    ordered_total(a.layer[k] + (int64_t)blockIdx.x * a.plane[k], a.plane[k], 1, t);
    const double mean = t[0] / (double)a.plane[k];
    sum = k ? sum + mean : mean;
  }
  if (threadIdx.x == 0) a.out[blockIdx.x] = sum;
}

struct Ptr {
  const void *p;
  const char *name;
  unsigned align;
  bool required;
};

bool bad_pointers(const char *who, const Ptr *ptrs, int n) {
  for (int i = 0; i < n; i++) {
    const Ptr &q = ptrs[i];
    if (!q.p && q.required) {
      d4gs_set_error("%s: %s is NULL", who, q.name);
      return true;
    }
    if ((uintptr_t)q.p % q.align) {
      d4gs_set_error("%s: %s = %p is misaligned (%u-byte alignment needed)", who, q.name, q.p, q.align);
      return true;
    }
  }
  return false;
}

// blocks of k_lpips_score per (m, b), or 0: sizes the entry points refuse
int64_t score_blocks(int M, int B, int H, int W) {
  if (M <= 0 || B <= 0 || H < LP_MIN || W < LP_MIN) return 0;
  const int64_t blocks = ((int64_t)H * W + 255) / 256;
  if ((int64_t)M * B > 65535 || blocks * M * B > INT32_MAX) return 0;
  return blocks;
}

// the five map sizes of an H x W image must be positive and their planes addressable
bool bad_sizes(const char *who, const int32_t *sizes) {
  if (!sizes) {
    d4gs_set_error("%s: sizes is NULL", who);
    return true;
  }
  for (int k = 0; k < LL; k++)
    if (sizes[2 * k] < 1 || sizes[2 * k + 1] < 1) {
      d4gs_set_error("%s: bad size sizes[%d]=(%d, %d) (the h and w of every layer map must be >= 1)", who, k, sizes[2 * k], sizes[2 * k + 1]);
      return true;
    }
  return false;
}

}  // namespace

extern "C" {

int d4gs_lpips_prepare(const float *pred, const float *target, const float *masks, int32_t M, int32_t B, int32_t H, int32_t W,
                       int32_t normalize, float *out, void *stream) {
  const char *who = "d4gs_lpips_prepare";
  const Ptr ptrs[] = {{pred, "pred", 4, true}, {target, "target", 4, true}, {masks, "masks", 4, false}, {out, "out", 4, true}};
  if (bad_pointers(who, ptrs, 4)) return D4GS_EINVAL;
  if (M <= 0 || B <= 0 || H <= 0 || W <= 0) {
    d4gs_set_error("%s: bad size M=%d B=%d H=%d W=%d (each must be >= 1)", who, M, B, H, W);
    return D4GS_EINVAL;
  }
  if (H < LP_MIN || W < LP_MIN) {
    d4gs_set_error("%s: the trunk needs H and W >= %d, got H=%d W=%d", who, LP_MIN, H, W);
    return D4GS_EINVAL;
  }
  if (!masks && M != 1) {
    d4gs_set_error("%s: masks == NULL stands for one mask of ones: M must be 1, not %d", who, M);
    return D4GS_EINVAL;
  }
  PrepareArgs a;
  a.pred = pred, a.target = target, a.masks = masks, a.out = out, a.M = M, a.B = B, a.normalize = normalize != 0;
  a.plane = (int64_t)H * W;
  if (a.plane > INT32_MAX || (int64_t)M * B > INT32_MAX / 6 || 6 * (int64_t)M * B * a.plane > (int64_t)INT32_MAX * 256) {
    d4gs_set_error("%s: size M=%d B=%d H=%d W=%d overflows the grid (2 M B H W <= 256 (2^31 - 1) / 3)", who, M, B, H, W);
    return D4GS_EINVAL;
  }
  a.total = 2 * (int64_t)M * B * a.plane;
  D4GS_LAUNCH("k_lpips_prepare", k_lpips_prepare, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return d4gs_check_launch("k_lpips_prepare");
}

int d4gs_lpips_layer(const float *f0, const float *f1, const float *weights, int32_t n, int32_t C, int32_t h, int32_t w, float *out,
                     void *stream) {
  const char *who = "d4gs_lpips_layer";
  const Ptr ptrs[] = {{f0, "f0", 4, true}, {f1, "f1", 4, true}, {weights, "weights", 4, true}, {out, "out", 4, true}};
  if (bad_pointers(who, ptrs, 4)) return D4GS_EINVAL;
  if (n <= 0 || C <= 0 || h <= 0 || w <= 0) {
    d4gs_set_error("%s: bad size n=%d C=%d h=%d w=%d (each must be >= 1)", who, n, C, h, w);
    return D4GS_EINVAL;
  }
  if (C > LP_MAX_C) {
    d4gs_set_error("%s: C=%d is beyond the limit of %d channels", who, C, LP_MAX_C);
    return D4GS_EINVAL;
  }
  LayerArgs a;
  a.f0 = f0, a.f1 = f1, a.w = weights, a.out = out, a.C = C, a.plane = (int64_t)h * w, a.total = (int64_t)n * a.plane;
  if (a.total > INT32_MAX || a.total * C > ((int64_t)1 << 40)) {
    d4gs_set_error("%s: size n=%d C=%d h=%d w=%d overflows the grid (n h w <= 2^31 - 1, n C h w <= 2^40)", who, n, C, h, w);
    return D4GS_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  if (C >= LP_WIDE_C)
    D4GS_LAUNCH("k_lpips_layer_wide", k_lpips_layer<16>, dim3((unsigned)((a.total + 15) / 16)), dim3(256), 0, s, a);
  else
    D4GS_LAUNCH("k_lpips_layer", k_lpips_layer<64>, dim3((unsigned)((a.total + 63) / 64)), dim3(256), 0, s, a);
  return d4gs_check_launch("k_lpips_layer");
}

int64_t d4gs_lpips_score_blocks(int32_t M, int32_t B, int32_t H, int32_t W) { return (int64_t)M * B * score_blocks(M, B, H, W); }

int d4gs_lpips_score(const float *const *layers, const int32_t *sizes, const float *masks, int32_t M, int32_t B, int32_t H, int32_t W,
                     float *score_map, double *partials, double *out, void *stream) {
  const char *who = "d4gs_lpips_score";
  if (!layers) {
    d4gs_set_error("%s: layers is NULL", who);
    return D4GS_EINVAL;
  }
  if (bad_sizes(who, sizes)) return D4GS_EINVAL;
  const Ptr ptrs[] = {{layers[0], "layers[0]", 4, true}, {layers[1], "layers[1]", 4, true}, {layers[2], "layers[2]", 4, true},
                      {layers[3], "layers[3]", 4, true}, {layers[4], "layers[4]", 4, true}, {masks, "masks", 4, false},
                      {score_map, "score_map", 4, false}, {partials, "partials", 8, true}, {out, "out", 8, true}};
  if (bad_pointers(who, ptrs, 9)) return D4GS_EINVAL;
  if (M <= 0 || B <= 0 || H <= 0 || W <= 0) {
    d4gs_set_error("%s: bad size M=%d B=%d H=%d W=%d (each must be >= 1)", who, M, B, H, W);
    return D4GS_EINVAL;
  }
  if (H < LP_MIN || W < LP_MIN) {
    d4gs_set_error("%s: the trunk needs H and W >= %d, got H=%d W=%d", who, LP_MIN, H, W);
    return D4GS_EINVAL;
  }
  if (!masks && M != 1) {
    d4gs_set_error("%s: masks == NULL stands for one mask of ones: M must be 1, not %d", who, M);
    return D4GS_EINVAL;
  }
  const int64_t blocks = score_blocks(M, B, H, W);
  if (!blocks) {
    d4gs_set_error("%s: size M=%d B=%d H=%d W=%d overflows the grid (M * B <= 65535, blocks <= 2^31 - 1)", who, M, B, H, W);
    return D4GS_EINVAL;
  }
  ScoreArgs a;
  for (int k = 0; k < LL; k++) {
    a.layer[k] = layers[k], a.h[k] = sizes[2 * k], a.w[k] = sizes[2 * k + 1];
    a.ry[k] = 1.0 / (1.0 * H / a.h[k]), a.rx[k] = 1.0 / (1.0 * W / a.w[k]);
  }
  a.masks = masks, a.map = score_map, a.partials = partials, a.H = H, a.W = W;
  hipStream_t s = (hipStream_t)stream;
  D4GS_LAUNCH("k_lpips_score", k_lpips_score, dim3((unsigned)blocks, M * B), dim3(256), 0, s, a);
  if (int rc = d4gs_check_launch("k_lpips_score")) return rc;
  D4GS_LAUNCH("k_lpips_finish", k_lpips_finish, dim3(M * B), dim3(256), 0, s, (const double *)partials, (int)blocks, out);
  return d4gs_check_launch("k_lpips_finish");
}

int d4gs_lpips_mean(const float *const *layers, const int32_t *sizes, int32_t n, double *out, void *stream) {
  const char *who = "d4gs_lpips_mean";
  if (!layers) {
    d4gs_set_error("%s: layers is NULL", who);
    return D4GS_EINVAL;
  }
  if (bad_sizes(who, sizes)) return D4GS_EINVAL;
  const Ptr ptrs[] = {{layers[0], "layers[0]", 4, true}, {layers[1], "layers[1]", 4, true}, {layers[2], "layers[2]", 4, true},
                      {layers[3], "layers[3]", 4, true}, {layers[4], "layers[4]", 4, true}, {out, "out", 8, true}};
  if (bad_pointers(who, ptrs, 6)) return D4GS_EINVAL;
  if (n <= 0) {
    d4gs_set_error("%s: bad size n=%d (must be >= 1)", who, n);
    return D4GS_EINVAL;
  }
  MeanArgs a;
  for (int k = 0; k < LL; k++) a.layer[k] = layers[k], a.plane[k] = (int64_t)sizes[2 * k] * sizes[2 * k + 1];
  a.out = out;
  D4GS_LAUNCH("k_lpips_mean", k_lpips_mean, dim3(n), dim3(256), 0, (hipStream_t)stream, a);
  return d4gs_check_launch("k_lpips_mean");
}

}  // extern "C"
