// sampling.h -- the one bilinear sampling rule of the data kernels (observations.hip: lifting; feed.hip: the batch).
#pragma once
#include "common.h"

// bilinear, coordinates clamped to the image (grid_sample's align_corners=True, padding_mode="border"); C interleaved channels
template <int C>
__device__ __forceinline__ void bilinear_border(const float *__restrict__ im, int H, int W, float x, float y, float (&o)[C]) {
  x = fminf(fmaxf(x, 0.f), (float)(W - 1));  // (a NaN becomes 0)
  y = fminf(fmaxf(y, 0.f), (float)(H - 1));
  const float fx0 = floorf(x), fy0 = floorf(y), ax = x - fx0, ay = y - fy0;
  const int ix0 = (int)fx0, iy0 = (int)fy0, ix1 = min(ix0 + 1, W - 1), iy1 = min(iy0 + 1, H - 1);  // (weight 0 where clamped)
  const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
#pragma unroll
  for (int c = 0; c < C; c++)
    o[c] = w00 * im[((size_t)iy0 * W + ix0) * C + c] + w01 * im[((size_t)iy0 * W + ix1) * C + c] + w10 * im[((size_t)iy1 * W + ix0) * C + c] +
           w11 * im[((size_t)iy1 * W + ix1) * C + c];
}
