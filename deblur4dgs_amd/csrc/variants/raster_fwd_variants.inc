// Non-default forward composites, compiled only with -DD4GS_VARIANTS (tests/libd4gs_variants.so): kept as A/B references -
// `test_forward_variants_bitwise_equal` checks them bit for bit against the shipped k_raster_fwd_r.  Included inside
// raster_fwd.hip's anonymous namespace.
// ---- what variants A and B share: the per-pair arithmetic and the pixel write-out, in the product kernel's operation order (so the
// three stay bit-identical).  How pixels map to lanes and which pairs are looked at is each variant's own.  The product kernel
// (raster_fwd_r_body) keeps its own statement of these in its two loops: every shared form tried changed the code of instantiations
// that no benchmark workload times (profiles/refactor_composite_isa.txt). ----
// alpha of staged splat (g0 = centre, opacity, depth; g1 = stage_conic) at pixel centre (pxf, pyf) and the transmittance behind it.
// The pair counts iff sigma >= 0 and alpha >= 1/255; it saturates the pixel (and is NOT composited) iff nT <= 1e-4.
__device__ __forceinline__ void fwd_pair(const float4 g0, const float4 g1, float pxf, float pyf, float T, float &sigma, float &alpha, float &nT) {
#pragma clang fp contract(off)
  const float dx = g0.x - pxf, dy = g0.y - pyf;
  sigma = splat_sigma2(g1, dx, dy);  // sigma * log2(e)
  alpha = fminf(0.999f, g0.z * __builtin_amdgcn_exp2f(-sigma));
  nT = T * (1.f - alpha);
}
// A pair's effect on its pixel once `valid` is decided (it counts, the pixel was not saturated and does not saturate with it):
// acc[c] = fma(colour[c], vis, acc[c]) over the D channels of the staged colour record `rec` ((D + 3) / 4 float4) and the depth
// channel, vis = alpha T (0 for an invalid pair), the new transmittance, and `at` as the pixel's last contributor.
template <int D, bool DEPTH>
__device__ __forceinline__ void fwd_commit(bool valid, float alpha, float nT, const float4 *rec, float depth, int at, float &T, int &last, float *acc) {
#pragma clang fp contract(off)
  const float vis = valid ? alpha * T : 0.f;
#pragma unroll
  for (int v = 0; v < (D + 3) / 4; v++) {
    const float4 c4 = rec[v];
    if (v * 4 < D) acc[v * 4] = __builtin_fmaf(c4.x, vis, acc[v * 4]);
    if (v * 4 + 1 < D) acc[v * 4 + 1] = __builtin_fmaf(c4.y, vis, acc[v * 4 + 1]);
    if (v * 4 + 2 < D) acc[v * 4 + 2] = __builtin_fmaf(c4.z, vis, acc[v * 4 + 2]);
    if (v * 4 + 3 < D) acc[v * 4 + 3] = __builtin_fmaf(c4.w, vis, acc[v * 4 + 3]);
  }
  if (DEPTH) acc[D] = __builtin_fmaf(depth, vis, acc[D]);
  T = valid ? nT : T;
  last = valid ? at : last;
}
// The pixel's outputs: alpha, final transmittance, last contributor (list index), the channels over the background, and the depth
// channel - divided by max(alpha, 1e-10) for the expected depth (a.ed).
template <int D, bool DEPTH>
__device__ __forceinline__ void fwd_write_pixel(const RasterFwdArgs &a, int s, int x, int y, float T, int last, const float *acc) {
#pragma clang fp contract(off)
  const size_t pix = ((size_t)s * a.height + y) * a.width + x;
  const float al = 1.f - T;
  a.alphas[pix] = al;
  a.final_T[pix] = T;
  a.last_ids[pix] = last;
  float *o = a.out + pix * (D + (DEPTH ? 1 : 0));
#pragma unroll
  for (int c = 0; c < D; c++) o[c] = acc[c] + (a.background ? T * a.background[c] : 0.f);
  if (DEPTH) o[D] = a.ed ? acc[D] / fmaxf(al, 1e-10f) : acc[D];
}

// Variant A: one wave64 per 16x16 tile, 2x2 pixels per lane.
template <int D, bool DEPTH>
__global__ void __launch_bounds__(64) k_raster_fwd(const RasterFwdArgs a) {
#pragma clang fp contract(off)
  constexpr int NCH = D + (DEPTH ? 1 : 0);
  constexpr int DP = (D + 3) & ~3;
  constexpr int DV = DP / 4;
  __shared__ float4 sg0[64];
  __shared__ float4 sg1[64];
  __shared__ float4 scol[64 * DV];

  if (lists_overflowed(a.n_dev, a.cap, a.max_hint)) return;
  const int n_tiles_s = a.tw * a.th;
  const int n_tiles = a.S * n_tiles_s;
  const int t = xcd_remap(blockIdx.x, n_tiles);
  if (t >= n_tiles) return;
  const int s = t / n_tiles_s, tl = t - s * n_tiles_s;
  const int ty = tl / a.tw, tx = tl - ty * a.tw;
  const int lane = threadIdx.x;
  const int x0 = tx * D4GS_TILE + 2 * (lane & 7), y0 = ty * D4GS_TILE + 2 * (lane >> 3);

  float pxf[4], pyf[4], T[4], acc[4][NCH];
  int last[4];
  bool done[4];
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int x = x0 + (p & 1), y = y0 + (p >> 1);
    pxf[p] = (float)x + 0.5f;
    pyf[p] = (float)y + 0.5f;
    T[p] = 1.f;
    last[p] = 0;
    done[p] = !(x < a.width && y < a.height);
#pragma unroll
    for (int c = 0; c < NCH; c++) acc[p][c] = 0.f;
  }

  const int start = a.tile_offsets[t], end = a.tile_offsets[t + 1];
  const size_t inst_base = (size_t)s * a.N;
  for (int b = start; b < end; b += 64) {
    if (__all(done[0] && done[1] && done[2] && done[3])) break;
    __syncthreads();
    const int idx = b + lane;
    if (idx < end) {
      const int gid = a.sorted_gid[idx];
      const float4 *gp = reinterpret_cast<const float4 *>(a.geom + (inst_base + gid) * D4GS_GEOM_STRIDE);
      const float4 q1 = gp[1];
      sg0[lane] = gp[0];
      sg1[lane] = stage_conic(q1.x, q1.y, q1.z, 0.f);  // exp2 argument (same as the bwd)
      const float4 *cp = reinterpret_cast<const float4 *>(a.ctab + (size_t)gid * DP);
#pragma unroll
      for (int v = 0; v < DV; v++) scol[lane * DV + v] = cp[v];
    }
    __syncthreads();
    const int nb = min(64, end - b);
    for (int j = 0; j < nb; j++) {
      if ((j & 15) == 0 && j && __all(done[0] && done[1] && done[2] && done[3])) break;
      const float4 g0 = sg0[j], g1 = sg1[j];
#pragma unroll
      for (int p = 0; p < 4; p++) {
        float sigma, alpha, nT;
        fwd_pair(g0, g1, pxf[p], pyf[p], T[p], sigma, alpha, nT);
        bool valid = !done[p] && (sigma >= 0.f) && (alpha >= (1.f / 255.f));
        const bool stop = valid && (nT <= 1e-4f);
        done[p] = done[p] || stop;
        valid = valid && !stop;
        fwd_commit<D, DEPTH>(valid, alpha, nT, scol + j * DV, g0.w, b + j, T[p], last[p], acc[p]);
      }
    }
  }

#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int x = x0 + (p & 1), y = y0 + (p >> 1);
    if (x < a.width && y < a.height) fwd_write_pixel<D, DEPTH>(a, s, x, y, T[p], last[p], acc[p]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Variant B (default): one 256-lane workgroup per tile = 4 waves, each wave owns an 8x8 QUADRANT (1 pixel / lane).
// Batches of 256 splats are staged once per tile; at staging every lane also computes its splat's tight
// alpha >= 1/255 bounding box (same margins as D4GS_EXACT_CULL).  Each wave then ballots "does splat j touch MY
// quadrant" (4 x 64-bit masks per batch) and walks only the set bits, so a splat that covers one corner of the tile
// costs one wave ~30 instructions instead of the whole tile 126.  Arithmetic per (splat, pixel) is identical to
// variant A, and skipped pairs would have failed the alpha test: the two variants are bitwise identical.
// ---------------------------------------------------------------------------------------------------------------
template <int D, bool DEPTH>
__global__ void __launch_bounds__(256) k_raster_fwd_q(const RasterFwdArgs a) {
#pragma clang fp contract(off)
  constexpr int NCH = D + (DEPTH ? 1 : 0);
  constexpr int DP = (D + 3) & ~3;
  constexpr int DV = DP / 4;
  constexpr int FB = 256;  // splats per batch (forward)
  __shared__ float4 sg0[FB];
  __shared__ float4 sg1[FB];
  __shared__ float4 sbox[FB];
  __shared__ float4 scol[FB * DV];

  if (lists_overflowed(a.n_dev, a.cap, a.max_hint)) return;
  const int n_tiles_s = a.tw * a.th;
  const int n_tiles = a.S * n_tiles_s;
  const int t = xcd_remap(blockIdx.x, n_tiles);
  if (t >= n_tiles) return;
  const int s = t / n_tiles_s, tl = t - s * n_tiles_s;
  const int ty = tl / a.tw, tx = tl - ty * a.tw;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int qx0 = tx * D4GS_TILE + (wv & 1) * 8, qy0 = ty * D4GS_TILE + (wv >> 1) * 8;
  const int x = qx0 + (lane & 7), y = qy0 + (lane >> 3);
  const bool inside = x < a.width && y < a.height;
  const float pxf = (float)x + 0.5f, pyf = (float)y + 0.5f;
  // pixel-centre extent of this wave's quadrant
  const float qlx = (float)qx0 + 0.5f, qhx = (float)qx0 + 7.5f, qly = (float)qy0 + 0.5f, qhy = (float)qy0 + 7.5f;

  float T = 1.f, acc[NCH];
  int last = 0;
  bool done = !inside;
#pragma unroll
  for (int c = 0; c < NCH; c++) acc[c] = 0.f;

  const int start = a.tile_offsets[t], end = a.tile_offsets[t + 1];
  const size_t inst_base = (size_t)s * a.N;
  for (int b = start; b < end; b += FB) {
    if (__syncthreads_and(done)) break;  // also orders the previous batch's LDS reads before restaging
    const int idx = b + tid;
    if (tid < FB && idx < end) {
      const int gid = a.sorted_gid[idx];
      const float4 *gp = reinterpret_cast<const float4 *>(a.geom + (inst_base + gid) * D4GS_GEOM_STRIDE);
      const float4 q0 = gp[0], q1 = gp[1];
      sg0[tid] = q0;
      sg1[tid] = stage_conic(q1.x, q1.y, q1.z, 0.f);
      const float tau = D4GS_ALPHA_TAU(q0.z);
      D4GS_TIGHT_EXTENTS(ex, ey, tau, q1.x, q1.y, q1.z)
      sbox[tid] = ex < 0.f ? make_float4(1e30f, -1e30f, 1e30f, -1e30f) : make_float4(q0.x - ex, q0.x + ex, q0.y - ey, q0.y + ey);
      const float4 *cp = reinterpret_cast<const float4 *>(a.ctab + (size_t)gid * DP);
#pragma unroll
      for (int v = 0; v < DV; v++) scol[tid * DV + v] = cp[v];
    }
    __syncthreads();
    const int nb = min(FB, end - b);
    unsigned long long mask[FB / 64];
#pragma unroll
    for (int k = 0; k < FB / 64; k++) {
      const int j = k * 64 + lane;
      bool hit = false;
      if (j < nb) {
        const float4 bx = sbox[j];
        hit = (bx.x <= qhx) && (bx.y >= qlx) && (bx.z <= qhy) && (bx.w >= qly);
      }
      mask[k] = __ballot(hit);
    }
    bool wdone = false;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < FB / 64; k++) {
      unsigned long long m = wdone ? 0ull : mask[k];
      while (m) {
        const int j = k * 64 + (__ffsll((long long)m) - 1);
        m &= m - 1;
        const float4 g0 = sg0[j], g1 = sg1[j];
        float sigma, alpha, nT;
        fwd_pair(g0, g1, pxf, pyf, T, sigma, alpha, nT);
        bool valid = !done && (sigma >= 0.f) && (alpha >= (1.f / 255.f));
        const bool stop = valid && (nT <= 1e-4f);
        done = done || stop;
        valid = valid && !stop;
        fwd_commit<D, DEPTH>(valid, alpha, nT, scol + j * DV, g0.w, b + j, T, last, acc);
        if ((++cnt & 15) == 0 && __all(done)) {
          m = 0;
          wdone = true;
        }
      }
    }
  }

  if (inside) fwd_write_pixel<D, DEPTH>(a, s, x, y, T, last, acc);
}
