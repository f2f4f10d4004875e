// adam_math.h -- torch's single-tensor Adam update for one element, stated ONCE for the kernels and the CPU twins that apply it:
// adam.hip (k_adam, d4gs_adam_step_cpu) and pose_refine.hip (k_pose_step, d4gs_pose_step_cpu).  Host and device code.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

struct AdamCoef {
  float w1, b2, w2;     // 1 - beta1, beta2, 1 - beta2
  float neg_step_size;  // -lr / (1 - beta1^t)
  float bc2_sqrt;       // sqrt(1 - beta2^t)
  float eps;
};

__host__ __device__ inline double adam_ipow(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

// t: the step count AFTER this update (>= 1), exact in fp32 like torch's `step` tensor
__host__ __device__ inline AdamCoef adam_coef(double lr, double beta1, double beta2, double eps, float t) {
  const int ti = (int)t;
  AdamCoef c;
  c.w1 = (float)(1.0 - beta1), c.b2 = (float)beta2, c.w2 = (float)(1.0 - beta2);
  c.neg_step_size = (float)(-(lr / (1.0 - adam_ipow(beta1, ti))));
  c.bc2_sqrt = (float)sqrt(1.0 - adam_ipow(beta2, ti));
  c.eps = (float)eps;
  return c;
}

// THE per-element update (device kernel and CPU twin), in the order of torch's single-tensor Adam: lerp_ (one FMA),
// mul_ + addcmul_ (value * g rounded, then one FMA), sqrt / bias_correction2_sqrt + eps, addcdiv_ ((value * m) / denom, then the
// add).  Written this way both moments come out bit-identical to torch's fp32 CPU path; sqrt and the divisions are the correctly
// rounded ones.  The FMAs are explicit and contraction is off, so the twin (host compiler) and the kernel (device compiler)
// cannot each pick their own.
__host__ __device__ __forceinline__ void adam_update(float &p, float &m, float &v, float g, const AdamCoef &c) {
#pragma clang fp contract(off)
  m = __builtin_fmaf(c.w1, g - m, m);
  v = __builtin_fmaf(c.w2 * g, g, v * c.b2);
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
  p = p + (c.neg_step_size * m) / denom;
}
