// metrics.hip -- the validator's masked PSNR and SSIM (flow3d/metrics.py:99-124,142-217; flow3d/validator.py:460-499), fused.
//
// Per mask m and image b of one call:  sse = sum ((pred - target) * mask)^2,  mask_sum = sum mask,  and the mean of the dycheck
// masked SSIM map.  That SSIM is NOT the pytorch_msssim one of photometric.hip: each of the five moments p, t, p^2, t^2, p t goes
// through a separable "partial convolution" whose passes are normalised by the COUNT of the mask under the window,
//     cnt = sum_window mask,   out = cnt != 0 ? (sum_window f z mask) * 11 / cnt : 0,   mask' = (cnt != 0),
// first along x with the given mask, then along y on the result with mask'.  (The reference writes ones_like(f).sum() / (m_ * C) with
// f expanded to the three channels: 33 / (3 cnt).  The normaliser is the count and not sum f mask; that is the reference's
// behaviour and what its users publish.)  A position whose windows are all empty has every moment 0 and scores exactly 1.
// In eager PyTorch one evaluation is ~60 launches per mask; here one tile kernel handles all masks of all images, and a small
// ordered sum finishes: two launches, no atomics, nothing read on the host, bitwise reproducible.
//
// Numerics.  sigma = E[x^2] - mu^2 is a cancellation that is then divided by c2 = 9e-4, so every window sum
// and the whole SSIM algebra are in double: the products of two fp32 values are exact there, and the result is the fp64 evaluation
// of the reference's formula on the fp32 inputs to ~1e-13.  The tile-offset trick of photometric.hip does not apply: the
// count-normalised filter is not shift-invariant.  The algebra is compiled without fma contraction, so that pred == target gives
// numerator == denominator bit for bit and an SSIM of exactly 1.  Block partials carry sum (1 - ssim); the mean is 1 - sum / n.
#include "common.h"
#include "reduce.h"

namespace {

constexpr int MW = 11, MT = 16, MH = MT + MW - 1;  // window, tile, tile + halo (26)
constexpr int MC = 3;                              // channels
constexpr int MP = 3;                              // doubles per block partial and per (m, b) result: sse, mask sum, SSIM term
__constant__ double c_wind[MW] = D4GS_SSIM_WINDOW;
constexpr double SSIM_C1 = 1e-4, SSIM_C2 = 9e-4;  // (0.01 * data_range)^2, (0.03 * data_range)^2, data_range = 1

struct MetricsArgs {
  const float *pred, *target;  // [B,H,W,3]
  const float *masks;          // [M,B,H,W] or null (ones)
  int B, H, W, Ho, Wo;
  double *partials;  // [M*B*tiles_y*tiles_x, 3]
};

// 1 - ssim of one output pixel and channel from its five filtered moments (flow3d/metrics.py:189-211)
__device__ __forceinline__ double one_minus_ssim(double mu0, double mu1, double e00, double e11, double e01) {
#pragma clang fp contract(off)
  const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
  const double s00 = fmax(e00 - mu00, 0.0), s11 = fmax(e11 - mu11, 0.0), s = e01 - mu01;
  const double lim = fmin(sqrt(s00 * s11), fabs(s));
  const double s01 = s > 0.0 ? lim : (s < 0.0 ? -lim : 0.0);
  const double numer = (2.0 * mu01 + SSIM_C1) * (2.0 * s01 + SSIM_C2);
  const double denom = (mu00 + mu11 + SSIM_C1) * (s00 + s11 + SSIM_C2);
  return 1.0 - numer / denom;
}

// One 256-thread block per 16x16 tile of the INPUT grid and per (m, b): every input pixel's sse and mask-sum contribution is owned by
// exactly one thread of one block; output pixels of the SSIM map exist for oy < H - 10, ox < W - 10.  SSIM = false: the two sums only.
template <bool SSIM>
__global__ void __launch_bounds__(256) k_metrics(const MetricsArgs a) {
  constexpr int NS = SSIM ? MH * MH : 1, NH = SSIM ? MH * MT : 1;
  __shared__ float sp[NS * MC], st[NS * MC], sm[NS];  // the 26x26 patch: pred, target, mask (zero outside the image)
  __shared__ double hbuf[5 * NH];                     // one channel: the horizontal pass of p, t, pp, tt, pt
  __shared__ float hflag[NH];                         // mask' of the horizontal pass
  __shared__ double red[MP * 4];
  const int tid = threadIdx.x;
  const int mb = blockIdx.z, b = mb % a.B, ty0 = blockIdx.y * MT, tx0 = blockIdx.x * MT;
  const size_t plane = (size_t)a.H * a.W;
  const float *pred = a.pred + (size_t)b * plane * MC, *target = a.target + (size_t)b * plane * MC;
  const float *mask = a.masks ? a.masks + (size_t)mb * plane : nullptr;
  const int ly = tid / MT, lx = tid % MT;
  double sse = 0.0, msum = 0.0, osum = 0.0;
  if constexpr (!SSIM) {
    const int y = ty0 + ly, x = tx0 + lx;
    if (y < a.H && x < a.W) {
      const size_t q = (size_t)y * a.W + x;
      const double m = mask ? (double)mask[q] : 1.0;
      msum = m;
#pragma unroll
      for (int c = 0; c < MC; c++) {
        const double d = ((double)pred[q * MC + c] - (double)target[q * MC + c]) * m;
        sse += d * d;
      }
    }
  } else {
    // stage the patch.  Cells outside the image get mask 0; they are only ever read by windows of output pixels that do not exist.
    for (int i = tid; i < MH * MH; i += 256) {
      const int cy = i / MH, cx = i - cy * MH;
      const int y = ty0 + cy, x = tx0 + cx;
      float p[MC] = {0.f, 0.f, 0.f}, t[MC] = {0.f, 0.f, 0.f}, m = 0.f;
      if (y < a.H && x < a.W) {
        const size_t q = (size_t)y * a.W + x;
        m = mask ? mask[q] : 1.f;
#pragma unroll
        for (int c = 0; c < MC; c++) p[c] = pred[q * MC + c], t[c] = target[q * MC + c];
      }
      sm[i] = m;
#pragma unroll
      for (int c = 0; c < MC; c++) sp[i * MC + c] = p[c], st[i * MC + c] = t[c];
    }
    __syncthreads();
    {  // this thread's own pixel of the tile: the arithmetic of the SSIM = false form, so that the two forms' sums are the same bits
      const int j = ly * MH + lx;
      const double m = sm[j];
      msum = m;
#pragma unroll
      for (int c = 0; c < MC; c++) {
        const double d = ((double)sp[j * MC + c] - (double)st[j * MC + c]) * m;
        sse += d * d;
      }
    }
    // the horizontal pass has 26 rows x 16 columns = 416 items, two per thread at most and the same two for every channel: their
    // mask counts are taken once
    double cnt[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int i = tid + r * 256;
      if (i < MH * MT) {
        const int hy = i / MT, hx = i - hy * MT;
#pragma unroll
        for (int k = 0; k < MW; k++) cnt[r] += (double)sm[hy * MH + hx + k];
        hflag[i] = cnt[r] != 0.0 ? 1.f : 0.f;
      }
    }
    const int oy = ty0 + ly, ox = tx0 + lx;
    const bool live = oy < a.Ho && ox < a.Wo;
    double cnt2 = 0.0;
#pragma unroll
    for (int c = 0; c < MC; c++) {
      if (c) __syncthreads();  // the previous channel's vertical pass is done with hbuf
#pragma unroll
      for (int r = 0; r < 2; r++) {
        const int i = tid + r * 256;
        if (i < MH * MT) {
          const int hy = i / MT, hx = i - hy * MT;
          double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int k = 0; k < MW; k++) {
            const int j = hy * MH + hx + k;
            const double m = sm[j], pv = sp[j * MC + c], tv = st[j * MC + c];
            const double wm = c_wind[k] * m;
            h[0] += wm * pv, h[1] += wm * tv, h[2] += wm * (pv * pv), h[3] += wm * (tv * tv), h[4] += wm * (pv * tv);
          }
#pragma unroll
          for (int j = 0; j < 5; j++) hbuf[j * MH * MT + i] = cnt[r] != 0.0 ? h[j] * 11.0 / cnt[r] : 0.0;
        }
      }
      __syncthreads();
      // vertical pass, one thread per output pixel.  Where mask' is 0 the horizontal result is 0 already, so the masked sum is the
      // plain one.
      if (live) {
        if (c == 0) {
#pragma unroll
          for (int k = 0; k < MW; k++) cnt2 += (double)hflag[(ly + k) * MT + lx];
        }
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < MW; k++) {
          const double w = c_wind[k];
          const int i = (ly + k) * MT + lx;
#pragma unroll
          for (int j = 0; j < 5; j++) v[j] += w * hbuf[j * MH * MT + i];
        }
#pragma unroll
        for (int j = 0; j < 5; j++) v[j] = cnt2 != 0.0 ? v[j] * 11.0 / cnt2 : 0.0;
        osum += one_minus_ssim(v[0], v[1], v[2], v[3], v[4]);
      }
    }
  }
  double v[MP] = {sse, msum, osum};
  block_sum_store(v, red);
  __syncthreads();
  if (tid < MP) {
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.partials[blk * MP + tid] = block_sum_combine<MP>(red, tid);
  }
}

// One block per (m, b): its tiles' partials in a fixed order.  out[mb] = sse, mask sum, 1 - sum(1 - ssim) / n  (0 without SSIM).
__global__ void __launch_bounds__(256) k_metrics_finish(const double *partials, int tiles, double n_ssim, double *out) {
  double t[MP];
  ordered_total(partials + (size_t)blockIdx.x * tiles * MP, tiles, MP, t);
  if (threadIdx.x == 0) {
    double *o = out + (size_t)blockIdx.x * MP;
    o[0] = t[0], o[1] = t[1], o[2] = n_ssim > 0.0 ? 1.0 - t[2] / n_ssim : 0.0;
  }
}

// tiles per (m, b), or 0: sizes whose grid or whose block count leaves 32 bits
int64_t metrics_tiles(int M, int B, int H, int W) {
  if (M <= 0 || B <= 0 || H <= 0 || W <= 0) return 0;
  const int64_t tx = ((int64_t)W + MT - 1) / MT, ty = ((int64_t)H + MT - 1) / MT;
  if ((int64_t)M * B > 65535 || ty > 65535 || (int64_t)M * B * tx * ty > INT32_MAX) return 0;
  return tx * ty;
}

}  // namespace

extern "C" {

int64_t d4gs_metrics_blocks(int32_t M, int32_t B, int32_t H, int32_t W) { return (int64_t)M * B * metrics_tiles(M, B, H, W); }

int d4gs_masked_metrics(const float *pred, const float *target, const float *masks, int32_t M, int32_t B, int32_t H, int32_t W,
                        int32_t want_ssim, double *partials, double *out, void *stream) {
  const char *who = "d4gs_masked_metrics";
  const struct {
    const void *p;
    const char *name;
    unsigned align;
    bool required;
  } ptrs[] = {{pred, "pred", 4, true}, {target, "target", 4, true}, {masks, "masks", 4, false}, {partials, "partials", 8, true}, {out, "out", 8, true}};
  for (const auto &q : ptrs) {
    if (!q.p && q.required) {
      d4gs_set_error("%s: %s is NULL", who, q.name);
      return D4GS_EINVAL;
    }
    if ((uintptr_t)q.p % q.align) {
      d4gs_set_error("%s: %s = %p is misaligned (%u-byte alignment needed)", who, q.name, q.p, q.align);
      return D4GS_EINVAL;
    }
  }
  if (M <= 0 || B <= 0 || H <= 0 || W <= 0) {
    d4gs_set_error("%s: bad size M=%d B=%d H=%d W=%d (each must be >= 1)", who, M, B, H, W);
    return D4GS_EINVAL;
  }
  if (!masks && M != 1) {
    d4gs_set_error("%s: masks == NULL stands for one mask of ones: M must be 1, not %d", who, M);
    return D4GS_EINVAL;
  }
  if (want_ssim && (H < MW || W < MW)) {
    d4gs_set_error("%s: want_ssim needs H and W >= %d (the 11-tap window without padding), got H=%d W=%d", who, MW, H, W);
    return D4GS_EINVAL;
  }
  const int64_t tiles = metrics_tiles(M, B, H, W);
  if (!tiles) {
    d4gs_set_error("%s: size M=%d B=%d H=%d W=%d overflows the grid (M * B and ceil(H / 16) <= 65535, blocks <= 2^31 - 1)", who, M, B, H, W);
    return D4GS_EINVAL;
  }
  MetricsArgs a;
  a.pred = pred, a.target = target, a.masks = masks, a.B = B, a.H = H, a.W = W, a.Ho = H - (MW - 1), a.Wo = W - (MW - 1);
  a.partials = partials;
  const dim3 grid((W + MT - 1) / MT, (H + MT - 1) / MT, M * B);
  hipStream_t s = (hipStream_t)stream;
  if (want_ssim)
    D4GS_LAUNCH("k_metrics", k_metrics<true>, grid, dim3(256), 0, s, a);
  else
    D4GS_LAUNCH("k_metrics_psnr", k_metrics<false>, grid, dim3(256), 0, s, a);
  if (int rc = d4gs_check_launch("k_metrics")) return rc;
  const double n_ssim = want_ssim ? (double)MC * a.Ho * a.Wo : 0.0;
  D4GS_LAUNCH("k_metrics_finish", k_metrics_finish, dim3(M * B), dim3(256), 0, s, (const double *)partials, (int)tiles, n_ssim, out);
  return d4gs_check_launch("k_metrics_finish");
}

}  // extern "C"
