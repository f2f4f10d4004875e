// composite.h -- the rules the composite kernels share, each stated once: raster_fwd.hip, raster_bwd.hip and their A/B references
// under variants/.  Like splat_sigma2 (common.h) they are used verbatim by the product kernels AND the reference variants: the
// "variants bit-identical" and "exact cull on == off" guarantees depend on every kernel computing them the same way.  What the
// variants exist to test - the mapping of pixels to lanes and which (pixel, splat) pairs are skipped - stays in each kernel.
#pragma once
#include "common.h"

// Block -> tile mapping, XCD-aware: block b runs on XCD b % 8, so consecutive logical tiles (same sub-sample, neighbouring tiles,
// shared splats) land on the same XCD and the gathered records hit that XCD's L2.  n_blocks is rounded up to a multiple of 8 by the
// launches; the caller drops t >= its tile count.
__device__ __forceinline__ int xcd_remap(int b, int n_blocks) {
  const int per = (n_blocks + 7) >> 3;
  return (b & 7) * per + (b >> 3);
}

// Half-extents (ex_, ey_), in pixels, of a staged splat's tight alpha >= 1/255 box from its threshold tau_ (D4GS_ALPHA_TAU of the
// opacity the composite sees) and its conic (a_, b_, c_): the ellipse sigma <= tau reaches sqrt(2 tau Sigma_xx), sqrt(2 tau Sigma_yy)
// from the centre, Sigma = conic^-1, plus 1e-3 px (tight_rect's margins, from the conic instead of the covariance).  Negative: the
// box is empty (opacity below 1/255, or no valid conic).  Every caller forms its own box from them - image coordinates as float4, or
// tile-local as 4 x f16 (d4gs_pack_box).  Declares ex_ and ey_.
// (A statement macro, expanded under the caller's `fp contract(off)`: every function form tried - reference, array or struct
// results, tau or the opacity as input - left the arithmetic alone but changed the register allocation or the schedule of forward
// kernels that no benchmark workload times, the D = 5 and D = 8 ones among them; profiles/refactor_composite_isa.txt.)
#define D4GS_TIGHT_EXTENTS(ex_, ey_, tau_, a_, b_, c_)                      \
  const float ex_##_det = (a_) * (c_) - (b_) * (b_);                        \
  const float ex_##_idet = 1.f / ex_##_det;                                 \
  float ex_ = -1.f, ey_ = -1.f;                                             \
  if ((tau_) > 0.f && ex_##_det > 0.f) {                                    \
    ex_ = sqrtf(2.f * tau_ * (c_) * ex_##_idet) + 1e-3f;                    \
    ey_ = sqrtf(2.f * tau_ * (a_) * ex_##_idet) + 1e-3f;                    \
  }
