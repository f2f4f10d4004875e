// photometric.hip -- SURVEY 8f-2: the photometric term of the training loss, fused.
//
// Reference: flow3d/trainer.py:388-392,575-586
//     0.8 * F.l1_loss(pred * m, gt * m) + 0.2 * (1 - SSIM(pred * m, gt * m)),   SSIM = pytorch_msssim.SSIM(1.0, channel=3)
// (pytorch-msssim 1.0.0: 11-tap sigma-1.5 Gaussian, separable, no padding; see oracle/photometric.py).  In eager
// PyTorch one evaluation is ~25 launches forward and ~60 backward, three to four times per step; here it is one
// tile kernel forward (loss partials + five maps per output pixel and channel), a one-block ordered sum, and one tile
// kernel backward (transposed separable filter of the maps + the L1 sign term).  Images are read channel-last
// [B,H,W,C] exactly as the rasterizer writes them; the mask [B,H,W] multiplies both images.
//
// Numerics.  On flat, bright or converged images the variances are ~1e-6 beside means ~1 and are
// divided by C2 = 9e-4, so nothing here is ever formed from raw fp32 moments:
//   * every 16x16 tile has a per-channel offset (ox, oy): the masked pred / gt value at its centre pixel, recomputed from
//     the inputs wherever it is needed (identical bits in both passes, nothing stored);
//   * the forward stages u = pred*m - ox, v = gt*m - oy (product and difference in double, rounded once to fp32) and
//     takes the five window moments of (u, v) in double; s1 = E[uu] - E[u]^2 etc. and the whole per-pixel SSIM
//     algebra stay in double, the luminance term as 1 - (mu1 - mu2)^2 / (mu1^2 + mu2^2 + C1);
//   * maps hold, per output pixel p and channel, the fixed-sigma derivatives
//         a = dL/dmu1 * CS,   b = L * dCS/ds1 = -S / B2,   e = L * (dCS/ds12 + 2 dCS/ds1) = 2 L (1 - CS) / B2
//     and the means relative to the forward tile's offsets as E[u] - E[v] and E[v] (full relative precision in fp32;
//     the difference is stored because it multiplies b, which is ~1e3 on flat regions, while E[v] multiplies e ~ 0);
//   * dS(p)/dx(q) = w(p - q) [ a + 2 b ((x(q) - mu1(p)) - (y(q) - mu2(p))) + e (y(q) - mu2(p)) ]: the backward rewrites
//     the means about ITS tile's offset while staging, filters t = a - 2 b (m1 - m2) - e m2, b and e, and combines
//     Ft + 2 ((x - ox) - (y - oy)) Fb + (y - oy) Fe, the filter sums in double (where a tile holds a step between two flat
//     levels, t and 2 (x - y) b are each ~40 and cancel).  When pred == gt bitwise, a, e and t are exactly 0 and so is
//     the SSIM gradient;
//   * the block partials are sums of 1 - S (not S), so a loss of 1e-4 keeps its relative precision.
#include "common.h"
#include "reduce.h"

namespace {

constexpr int PW = 11, PT = 16, PH = PT + PW - 1;  // window, tile, tile + halo (26)
constexpr int PC = 3;                                      // channels (the reference's SSIM is built for 3)
constexpr int PM = 5;                                      // map floats per output pixel and channel: a, b, e, E[u] - E[v], E[v]
__constant__ double c_wind[PW] = D4GS_SSIM_WINDOW;  // (bitwise the oracle's window)
constexpr double SSIM_C1 = 1e-4, SSIM_C2 = 9e-4;

// the offset of 16x16 tile (ty, tx) of image b: the masked value at its centre pixel (clamped into the image)
__device__ __forceinline__ float tile_offset(const float *img, const float *mask, int b, int H, int W, int ty, int tx, int c) {
  const int y = min(ty * PT + PT / 2, H - 1), x = min(tx * PT + PT / 2, W - 1);
  const size_t p = ((size_t)b * H + y) * W + x;
  return (float)((double)img[p * PC + c] * (double)(mask ? mask[p] : 1.f));
}

struct PhotoArgs {
  const float *pred, *gt, *mask;  // [B,H,W,C], [B,H,W,C], [B,H,W] or null
  int B, H, W, Ho, Wo, tiles_x, tiles_y;
  float *maps;      // [B,Ho,Wo,C,PM]
  float *partials;  // [n_blocks,2]  {sum of 1 - ssim_map, sum of |x - y|}
};

__global__ void __launch_bounds__(256) k_photo_fwd(const PhotoArgs a) {
  __shared__ float su[PH * PH * PC], sv[PH * PH * PC];  // pred*m - ox, gt*m - oy
  __shared__ double hbuf[5 * PH * PT];                  // one channel: horizontally filtered u, v, uu, vv, uv
  __shared__ double red[4];
  __shared__ float redl[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.z, ty0 = blockIdx.y * PT, tx0 = blockIdx.x * PT;
  float offx[PC], offy[PC];
#pragma unroll
  for (int c = 0; c < PC; c++) {
    offx[c] = tile_offset(a.pred, a.mask, b, a.H, a.W, blockIdx.y, blockIdx.x, c);
    offy[c] = tile_offset(a.gt, a.mask, b, a.H, a.W, blockIdx.y, blockIdx.x, c);
  }
  // stage the 26x26 input patch (masked, centred).  Tiles cover the INPUT grid, so every input pixel's |x - y| is owned
  // by exactly one block (its 16x16 top-left cells); output pixels exist only for oy < H - 10, ox < W - 10.  Cells
  // outside the image are only ever read by windows of output pixels that do not exist.
  float l1[1] = {0.f};  // (arrays of one: the block sum takes R values)
  for (int i = tid; i < PH * PH; i += 256) {
    const int ly = i / PH, lx = i - ly * PH;
    const int y = ty0 + ly, x = tx0 + lx;
    float u[PC] = {0.f, 0.f, 0.f}, v[PC] = {0.f, 0.f, 0.f};
    if (y < a.H && x < a.W) {
      const size_t p = ((size_t)b * a.H + y) * a.W + x;
      const float m = a.mask ? a.mask[p] : 1.f;
#pragma unroll
      for (int c = 0; c < PC; c++) {
        const float pv = a.pred[p * PC + c], gv = a.gt[p * PC + c];
        u[c] = (float)((double)pv * (double)m - (double)offx[c]);
        v[c] = (float)((double)gv * (double)m - (double)offy[c]);
        if (ly < PT && lx < PT) l1[0] += fabsf(pv - gv) * fabsf(m);
      }
    }
#pragma unroll
    for (int c = 0; c < PC; c++) su[i * PC + c] = u[c], sv[i * PC + c] = v[c];
  }
  const int ly = tid / PT, lx = tid % PT;
  const int oy = ty0 + ly, ox = tx0 + lx;
  const bool live = oy < a.Ho && ox < a.Wo;
  double osum[1] = {0.0};  // sum of 1 - S
#pragma unroll
  for (int c = 0; c < PC; c++) {
    __syncthreads();  // staging done (c == 0) / the previous channel's vertical pass done with hbuf
    // horizontal pass: 26 rows x 16 columns
    for (int i = tid; i < PH * PT; i += 256) {
      const int hy = i / PT, hx = i - hy * PT;
      double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < PW; k++) {
        const double w = c_wind[k], uv = su[(hy * PH + hx + k) * PC + c], vv = sv[(hy * PH + hx + k) * PC + c];
        h[0] += w * uv, h[1] += w * vv, h[2] += w * (uv * uv), h[3] += w * (vv * vv), h[4] += w * (uv * vv);
      }
#pragma unroll
      for (int j = 0; j < 5; j++) hbuf[j * PH * PT + i] = h[j];
    }
    __syncthreads();
    // vertical pass + SSIM map + derivative maps: one thread per output pixel
    if (live) {
      double eu = 0.0, ev = 0.0, euu = 0.0, evv = 0.0, euv = 0.0;
#pragma unroll
      for (int k = 0; k < PW; k++) {
        const double w = c_wind[k];
        const int i = (ly + k) * PT + lx;
        eu += w * hbuf[i], ev += w * hbuf[PH * PT + i], euu += w * hbuf[2 * PH * PT + i];
        evv += w * hbuf[3 * PH * PT + i], euv += w * hbuf[4 * PH * PT + i];
      }
      const double mu1 = (double)offx[c] + eu, mu2 = (double)offy[c] + ev;
      const double d = ((double)offx[c] - (double)offy[c]) + (eu - ev);  // mu1 - mu2
      const double s1 = euu - eu * eu, s2 = evv - ev * ev, s12 = euv - eu * ev;
      const double iB1 = 1.0 / (mu1 * mu1 + mu2 * mu2 + SSIM_C1), iB2 = 1.0 / (s1 + s2 + SSIM_C2);
      const double L = 1.0 - d * d * iB1;
      const double ocs = (s1 + s2 - 2.0 * s12) * iB2;  // 1 - CS
      const double S = L * (1.0 - ocs);
      osum[0] += (d * d * iB1 + ocs) - d * d * iB1 * ocs;  // 1 - S
      float *mp = a.maps + ((((size_t)b * a.Ho + oy) * a.Wo + ox) * PC + c) * PM;
      mp[0] = (float)(-2.0 * d * (mu2 * (mu1 + mu2) + SSIM_C1) * iB1 * iB1 * (1.0 - ocs));
      mp[1] = (float)(-S * iB2);
      mp[2] = (float)(2.0 * L * ocs * iB2);
      mp[3] = (float)(eu - ev);
      mp[4] = (float)ev;
    }
  }
  block_sum_store(osum, red), block_sum_store(l1, redl);  // both block sums (reduce.h) behind one barrier
  __syncthreads();
  if (tid == 0) {
    const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.partials[blk * 2] = (float)block_sum_combine<1>(red, 0);
    a.partials[blk * 2 + 1] = block_sum_combine<1>(redl, 0);
  }
}

// loss[0] = w_l1 * l1 + w_ssim * (1 - ssim), loss[1] = l1, loss[2] = ssim; one block, ordered.  The partials carry
// 1 - ssim, and the loss is formed from it in double, so a small 1 - ssim is not rounded through an ssim near 1.
__global__ void __launch_bounds__(256) k_photo_finish(const float *partials, int n_blocks, double inv_nssim, double inv_nl1,
                                                      float w_l1, float w_ssim, float *loss) {
  double t[2];  // sum of 1 - ssim_map, sum of |x - y|
  ordered_total(partials, n_blocks, 2, t);
  if (threadIdx.x == 0) {
    const double dssim = t[0] * inv_nssim, l1 = t[1] * inv_nl1;
    loss[0] = (float)((double)w_l1 * l1 + (double)w_ssim * dssim), loss[1] = (float)l1, loss[2] = (float)(1.0 - dssim);
  }
}

struct PhotoBwdArgs {
  const float *pred, *gt, *mask, *maps, *v_loss;
  int B, H, W, Ho, Wo;
  float k_ssim, k_l1;  // -w_ssim / n_ssim, w_l1 / n_l1
  float *v_pred;
};

// dL/dpred(q) = m(q) * v * [ k_l1 sign(x - y) + k_ssim * sum_p w(p - q) dS(p)/dx(q) ]   (see the head of this file)
__global__ void __launch_bounds__(256) k_photo_bwd(const PhotoBwdArgs a) {
  __shared__ float sm[PH * PH * PC * 3];  // {t, b, e} of output pixels q - 10 .. q (zero outside the valid region)
  __shared__ double hb[PH * PT * 3];  // one channel at a time; double: t and b are large where they cancel (flat regions)
  __shared__ float so[2 * 2 * PC * 2];  // offsets of the forward tiles (by - 1 .. by) x (bx - 1 .. bx): [dy][dx][c][pred, gt]
  const int tid = threadIdx.x;
  const int b = blockIdx.z, ty0 = blockIdx.y * PT, tx0 = blockIdx.x * PT;
  if (tid < 2 * 2 * PC * 2) {
    const int k = tid & 1, c = (tid >> 1) % PC, t = tid / (2 * PC);
    const int ty = max((int)blockIdx.y - 1 + (t >> 1), 0), tx = max((int)blockIdx.x - 1 + (t & 1), 0);
    so[tid] = tile_offset(k ? a.gt : a.pred, a.mask, b, a.H, a.W, ty, tx, c);
  }
  __syncthreads();
  for (int i = tid; i < PH * PH; i += 256) {
    const int ly = i / PH, lx = i - ly * PH;
    const int oy = ty0 + ly - (PW - 1), ox = tx0 + lx - (PW - 1);
    const bool in = oy >= 0 && ox >= 0 && oy < a.Ho && ox < a.Wo;
    if (in) {
      const float *mp = a.maps + (((size_t)b * a.Ho + oy) * a.Wo + ox) * PC * PM;
      const int t = ((oy / PT) - ((int)blockIdx.y - 1)) * 2 + ((ox / PT) - ((int)blockIdx.x - 1));  // the tile that wrote p
#pragma unroll
      for (int c = 0; c < PC; c++) {
        const float ma = mp[c * PM], mb = mp[c * PM + 1], me = mp[c * PM + 2];
        // about this block's offsets: mu1 - mu2 (from the stored difference, so that it keeps its precision where the forward
        // tile's offset is far from the local level) and mu2: (forward tile's offset - ours) + stored mean
        const double ox1 = so[(t * PC + c) * 2], oy1 = so[(t * PC + c) * 2 + 1];
        const double ox0 = so[(3 * PC + c) * 2], oy0 = so[(3 * PC + c) * 2 + 1];
        const double m12 = ((ox1 - oy1) - (ox0 - oy0)) + (double)mp[c * PM + 3];
        const double m2 = (oy1 - oy0) + (double)mp[c * PM + 4];
        sm[(i * PC + c) * 3] = (float)((double)ma - 2.0 * (double)mb * m12 - (double)me * m2);
        sm[(i * PC + c) * 3 + 1] = mb, sm[(i * PC + c) * 3 + 2] = me;
      }
    } else {
#pragma unroll
      for (int j = 0; j < PC * 3; j++) sm[i * PC * 3 + j] = 0.f;
    }
  }
  __syncthreads();
  const int ly = tid / PT, lx = tid % PT;
  const int y = ty0 + ly, x = tx0 + lx;
  const bool live = y < a.H && x < a.W;
  const size_t p = ((size_t)b * a.H + (live ? y : 0)) * a.W + (live ? x : 0);
  const float m = a.mask ? a.mask[p] : 1.f;
  const float v = a.v_loss[0];
#pragma unroll
  for (int c = 0; c < PC; c++) {
    // horizontal (transposed): input column x gathers output columns x - 10 .. x with weight w[x - ox]
    for (int i = tid; i < PH * PT * 3; i += 256) {
      const int j = i % 3, hx = (i / 3) % PT, hy = i / (3 * PT);
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < PW; k++) acc += c_wind[PW - 1 - k] * (double)sm[((hy * PH + hx + k) * PC + c) * 3 + j];
      hb[i] = acc;
    }
    __syncthreads();
    if (live) {
      double ft = 0.0, fb = 0.0, fe = 0.0;
#pragma unroll
      for (int k = 0; k < PW; k++) {
        const double w = c_wind[PW - 1 - k];
        const double *h = hb + ((ly + k) * PT + lx) * 3;
        ft += w * h[0], fb += w * h[1], fe += w * h[2];
      }
      const float pv = a.pred[p * PC + c], gv = a.gt[p * PC + c];
      const double dx = (double)pv * (double)m - (double)so[(3 * PC + c) * 2];
      const double dy = (double)gv * (double)m - (double)so[(3 * PC + c) * 2 + 1];
      const float dl = (pv - gv) * m;  // sign(x - y) with x = pred m, y = gt m
      const float sgn = dl > 0.f ? 1.f : (dl < 0.f ? -1.f : 0.f);
      const float gs = (float)(ft + 2.0 * (dx - dy) * fb + dy * fe);
      a.v_pred[p * PC + c] = m * v * (a.k_l1 * sgn + a.k_ssim * gs);
    }
    __syncthreads();  // hb is rewritten for the next channel
  }
}

}  // namespace

int d4gs_photometric_fwd_impl(const float *pred, const float *gt, const float *mask, int32_t B, int32_t H, int32_t W,
                              float w_l1, float w_ssim, float *maps, float *partials, float *loss, hipStream_t stream) {
  PhotoArgs a;
  a.pred = pred, a.gt = gt, a.mask = mask, a.B = B, a.H = H, a.W = W, a.Ho = H - (PW - 1), a.Wo = W - (PW - 1);
  a.maps = maps, a.partials = partials;
  a.tiles_x = (W + PT - 1) / PT, a.tiles_y = (H + PT - 1) / PT;
  const dim3 grid(a.tiles_x, a.tiles_y, B);
  {
    ProfScope ps("k_photo_fwd", stream);
    k_photo_fwd<<<grid, 256, 0, stream>>>(a);
  }
  int rc = d4gs_check_launch("k_photo_fwd");
  if (rc) return rc;
  const int nb = a.tiles_x * a.tiles_y * B;
  ProfScope ps("k_photo_finish", stream);
  k_photo_finish<<<1, 256, 0, stream>>>(partials, nb, 1.0 / ((double)B * PC * a.Ho * a.Wo), 1.0 / ((double)B * PC * H * W), w_l1,
                                        w_ssim, loss);
  return d4gs_check_launch("k_photo_finish");
}

int d4gs_photometric_bwd_impl(const float *pred, const float *gt, const float *mask, const float *maps,
                              const float *v_loss, int32_t B, int32_t H, int32_t W, float w_l1, float w_ssim,
                              float *v_pred, hipStream_t stream) {
  PhotoBwdArgs a;
  a.pred = pred, a.gt = gt, a.mask = mask, a.maps = maps, a.v_loss = v_loss, a.B = B, a.H = H, a.W = W;
  a.Ho = H - (PW - 1), a.Wo = W - (PW - 1);
  a.k_ssim = -w_ssim / ((float)B * PC * a.Ho * a.Wo), a.k_l1 = w_l1 / ((float)B * PC * H * W);
  a.v_pred = v_pred;
  const dim3 grid((W + PT - 1) / PT, (H + PT - 1) / PT, B);
  ProfScope ps("k_photo_bwd", stream);
  k_photo_bwd<<<grid, 256, 0, stream>>>(a);
  return d4gs_check_launch("k_photo_bwd");
}

extern "C" int64_t d4gs_photometric_blocks(int32_t B, int32_t H, int32_t W) {
  return (int64_t)B * ((W + PT - 1) / PT) * ((H + PT - 1) / PT);
}

extern "C" int64_t d4gs_photometric_maps_elems(int32_t B, int32_t H, int32_t W) {
  return H < PW || W < PW ? 0 : (int64_t)B * (H - (PW - 1)) * (W - (PW - 1)) * PC * PM;
}
