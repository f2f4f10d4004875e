// observations.hip -- the device side of deblur4dgs_amd/observations.py: what the reference's flow3d/data/utils.py and the
// get_tracks_3d / get_bkgd_points bodies of its datasets do to raw arrays (aligned depths, masks, TAPIR 2-D tracks, Ks, w2cs)
// before scene initialisation starts.  Contracts: include/d4gs.h, "Observations"; rules, layout and times: DESIGN.md section 26.
//
// Masked median: five launches on the stream, nothing read on the host.
//   k_mm_count   16 x 16 pixel tiles; the tile's validity (mask == 1, inside the image) with its (k - 1) / 2 halo goes to LDS as
//                bytes, every lane counts its window and leaves the parity of its INVALID count (k k is odd: 1 ^ parity of the
//                valid count) in par[pixel]; the tile's min / max of the image go to a partials table.
//   k_mm_chunk   the parity of every chunk of MM_CHUNK consecutive pixels (row-major; chunks restart at every image).
//   k_mm_carry   one block: the exclusive prefix parity over the chunks in order (per image with per_image), and lo = min(min, 0),
//                hi = max(max, 0) from the partials (the zero padding belongs to the reference's min / max for every k >= 3).
//   k_mm_prefix  second look: bit 1 of par[pixel] becomes the parity of all invalid entries BEFORE the pixel.
//   k_mm_select  the tile and its halo go to LDS once as order-preserving integer keys, invalid entries as the key 0xFFFFFFFF (the
//                image of a NaN: finite inputs never produce it).  A lane knows n_lo (its invalid entries sent to lo) from its two
//                parity bits and its valid count, so the lower median is lo, hi, or the (rank - n_lo)-th smallest valid key, found
//                by a bit-by-bit descent: for bit 31 ... 0, count the window's keys that agree with the prefix above the bit and
//                have a 0 there; step past them or stay.  The invalid key has a 1 in every bit and is never counted.  32 x k k LDS
//                reads per pixel, no sort, no registers beyond a handful.  LDS pitch 48 words: the two rows of a 32-lane half fall
//                on disjoint banks.
// Lifting: k_lift_samples (one lane per (track, frame)) and k_lift_tracks (one lane per track: the visible count, its histogram
// bin by an integer atomic, the colour).  Background points: k_bkgd, one lane per pixel, and k_bkgd_compact, one block per frame.
#include <cmath>

#include "args.h"
#include "common.h"
#include "sampling.h"

namespace {

constexpr int MM_TILE = 16, MM_NT = MM_TILE * MM_TILE;
constexpr int MM_MAX_K = 15, MM_MAX_HALO = MM_TILE + MM_MAX_K - 1;  // 30
constexpr int MM_PITCH = 48;                                         // words per staged row of keys
constexpr int MM_VPITCH = 32;                                        // bytes per staged row of validity
constexpr int MM_CHUNK = 1024, MM_PER_LANE = MM_CHUNK / MM_NT;       // pixels per chunk of the parity scan
constexpr uint32_t MM_INVALID = 0xFFFFFFFFu;
static_assert(MM_MAX_HALO <= MM_VPITCH && MM_MAX_HALO <= MM_PITCH && MM_PITCH % 32 == 16, "staging pitches");
static_assert(MM_NT == 4 * D4GS_WAVE, "four waves per block");

__device__ __forceinline__ uint32_t float_key(float v) {  // a < b  <=>  key(a) < key(b) for finite a, b (-0 below +0)
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// the parity of the lanes of this wave that hold `bit`, below this lane (exclusive) and over the whole wave
__device__ __forceinline__ void wave_parity(bool bit, int &below, int &all) {
  const unsigned long long b = __ballot(bit);
  const int lane = threadIdx.x & (D4GS_WAVE - 1);
  below = __popcll(b & ((1ull << lane) - 1ull)) & 1;
  all = __popcll(b) & 1;
}

__global__ void __launch_bounds__(MM_NT) k_mm_count(const float *__restrict__ image, const float *__restrict__ mask, int H, int W, int k,
                                                    int tw, int tiles, uint8_t *__restrict__ par, float *__restrict__ partials) {
  __shared__ uint8_t v[MM_MAX_HALO * MM_VPITCH];
  __shared__ float red[2][4];
  const int img = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int y0 = (tile / tw) * MM_TILE, x0 = (tile % tw) * MM_TILE, r = k >> 1, hw = MM_TILE + 2 * r;
  const size_t base = (size_t)img * H * W;
  for (int i = threadIdx.x; i < hw * hw; i += MM_NT) {
    const int hy = i / hw, hx = i - hy * hw, gy = y0 + hy - r, gx = x0 + hx - r;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    v[hy * MM_VPITCH + hx] = in && mask[base + (size_t)gy * W + gx] == 1.0f;
  }
  __syncthreads();
  const int ty = threadIdx.x / MM_TILE, tx = threadIdx.x % MM_TILE, y = y0 + ty, x = x0 + tx;
  const bool mine = y < H && x < W;
  float mn = INFINITY, mx = -INFINITY;
  if (mine) {
    int cnt = 0;
    for (int ky = 0; ky < k; ky++)
      for (int kx = 0; kx < k; kx++) cnt += v[(ty + ky) * MM_VPITCH + tx + kx];
    par[base + (size_t)y * W + x] = (uint8_t)((k * k - cnt) & 1);
    mn = mx = image[base + (size_t)y * W + x];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o)), mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & (D4GS_WAVE - 1)) == 0) red[0][threadIdx.x / D4GS_WAVE] = mn, red[1][threadIdx.x / D4GS_WAVE] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * (size_t)blockIdx.x] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    partials[2 * (size_t)blockIdx.x + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

// pass 0: chunk[b] = the parity of the chunk.  pass 1: par[pixel] |= 2 x (the parity of everything before the pixel).
template <int PASS>
__global__ void __launch_bounds__(MM_NT) k_mm_chunk(uint8_t *__restrict__ par, int64_t HW, int cpi, uint8_t *__restrict__ chunk) {
  __shared__ int wave_all[4];
  const int img = blockIdx.x / cpi, c = blockIdx.x % cpi;
  const int64_t first = (int64_t)c * MM_CHUNK + (int64_t)threadIdx.x * MM_PER_LANE;
  uint8_t *p = par + (size_t)img * HW;
  int bits[MM_PER_LANE], x = 0;
#pragma unroll
  for (int i = 0; i < MM_PER_LANE; i++) {
    bits[i] = first + i < HW ? (p[first + i] & 1) : 0;
    x ^= bits[i];
  }
  int below, all;
  wave_parity(x != 0, below, all);
  if ((threadIdx.x & (D4GS_WAVE - 1)) == 0) wave_all[threadIdx.x / D4GS_WAVE] = all;
  __syncthreads();
  if (PASS == 0) {
    if (threadIdx.x == 0) chunk[blockIdx.x] = (uint8_t)(wave_all[0] ^ wave_all[1] ^ wave_all[2] ^ wave_all[3]);
  } else {
    int before = chunk[blockIdx.x] ^ below;
    for (int w = 0; w < (int)(threadIdx.x / D4GS_WAVE); w++) before ^= wave_all[w];
#pragma unroll
    for (int i = 0; i < MM_PER_LANE; i++) {
      if (first + i < HW) p[first + i] = (uint8_t)(bits[i] | (before << 1));
      before ^= bits[i];
    }
  }
}

// block b: the images [b, b + 1) with per_image, else all of them
__global__ void __launch_bounds__(MM_NT) k_mm_carry(uint8_t *__restrict__ chunk, const float *__restrict__ partials, int n_img, int cpi,
                                                    int tiles, int per_image, float *__restrict__ lohi) {
  __shared__ float red[2][4];
  __shared__ int wave_all[4];
  const int i0 = per_image ? blockIdx.x : 0, i1 = per_image ? blockIdx.x + 1 : n_img;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)i0 * tiles + threadIdx.x; i < (int64_t)i1 * tiles; i += MM_NT)
    mn = fminf(mn, partials[2 * i]), mx = fmaxf(mx, partials[2 * i + 1]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o)), mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & (D4GS_WAVE - 1)) == 0) red[0][threadIdx.x / D4GS_WAVE] = mn, red[1][threadIdx.x / D4GS_WAVE] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    lohi[2 * blockIdx.x] = fminf(fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3])), 0.f);
    lohi[2 * blockIdx.x + 1] = fmaxf(fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3])), 0.f);
  }
  int carry = 0;
  for (int64_t b = (int64_t)i0 * cpi; b < (int64_t)i1 * cpi; b += MM_NT) {  // (uniform trip count: the barriers are met by all)
    const int64_t i = b + threadIdx.x;
    const bool in = i < (int64_t)i1 * cpi;
    const int bit = in ? chunk[i] : 0;
    int below, all;
    wave_parity(bit != 0, below, all);
    __syncthreads();  // the previous turn's wave_all has been read
    if ((threadIdx.x & (D4GS_WAVE - 1)) == 0) wave_all[threadIdx.x / D4GS_WAVE] = all;
    __syncthreads();
    int before = carry ^ below;
    for (int w = 0; w < (int)(threadIdx.x / D4GS_WAVE); w++) before ^= wave_all[w];
    if (in) chunk[i] = (uint8_t)before;
    carry ^= wave_all[0] ^ wave_all[1] ^ wave_all[2] ^ wave_all[3];
  }
}

__global__ void __launch_bounds__(MM_NT) k_mm_select(const float *__restrict__ image, const float *__restrict__ mask,
                                                     const float *__restrict__ blend, const uint8_t *__restrict__ par,
                                                     const float *__restrict__ lohi, int H, int W, int k, int tw, int tiles, int per_image,
                                                     float *__restrict__ out) {
  __shared__ uint32_t keys[MM_MAX_HALO * MM_PITCH];
  const int img = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int y0 = (tile / tw) * MM_TILE, x0 = (tile % tw) * MM_TILE, r = k >> 1, hw = MM_TILE + 2 * r;
  const size_t base = (size_t)img * H * W;
  for (int i = threadIdx.x; i < hw * hw; i += MM_NT) {
    const int hy = i / hw, hx = i - hy * hw, gy = y0 + hy - r, gx = x0 + hx - r;
    uint32_t key = MM_INVALID;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t g = base + (size_t)gy * W + gx;
      if (mask[g] == 1.0f) key = float_key(image[g]);
    }
    keys[hy * MM_PITCH + hx] = key;
  }
  __syncthreads();
  const int ty = threadIdx.x / MM_TILE, tx = threadIdx.x % MM_TILE, y = y0 + ty, x = x0 + tx;
  if (y >= H || x >= W) return;  // (no barrier below)
  const size_t g = base + (size_t)y * W + x;
  const float old = image[g], b = blend ? blend[g] : 1.f;
  // blend == 0 leaves `old` whatever the median is - except for old = -0.0, where the sum's sign is the median's: that one is computed
  if (blend && b == 0.f && __float_as_uint(old) != 0x80000000u) {
    out[g] = old;
    return;
  }
  const uint32_t *win = keys + ty * MM_PITCH + tx;
  int n_valid = 0;
  for (int ky = 0; ky < k; ky++)
    for (int kx = 0; kx < k; kx++) n_valid += win[ky * MM_PITCH + kx] != MM_INVALID;
  const int kk = k * k, rank = (kk - 1) >> 1, n_inv = kk - n_valid, start = (par[g] >> 1) & 1;
  const int n_lo = start ? n_inv >> 1 : (n_inv + 1) >> 1;  // the invalid entries alternate lo, hi, ... from lo (start 0) or hi (1)
  const float lo = lohi[per_image ? 2 * img : 0], hi = lohi[per_image ? 2 * img + 1 : 1];
  float med;
  int j = rank - n_lo;
  if (j < 0) {
    med = lo;
  } else if (j >= n_valid) {
    med = hi;
  } else {
    uint32_t prefix = 0;
    for (int bit = 31; bit >= 0; bit--) {
      const uint32_t want = prefix >> bit;  // the bits above `bit` as chosen, a 0 at `bit`
      int c = 0;
      for (int ky = 0; ky < k; ky++)
        for (int kx = 0; kx < k; kx++) c += (win[ky * MM_PITCH + kx] >> bit) == want;
      if (j >= c) j -= c, prefix |= 1u << bit;
    }
    med = key_float(prefix);
  }
  // the dataset's blend, rounded product by product as torch evaluates depth * mask + old * (1 - mask)
  out[g] = blend ? __fadd_rn(__fmul_rn(med, b), __fmul_rn(old, __fsub_rn(1.f, b))) : med;
}

// ---- lifting ----------------------------------------------------------------------------------------------------------------
struct Cam {
  float ik[9], c2w[12];
};
__device__ __forceinline__ Cam load_cam(const float *__restrict__ inv_Ks, const float *__restrict__ c2ws, int t) {
  Cam c;
#pragma unroll
  for (int i = 0; i < 9; i++) c.ik[i] = inv_Ks[(size_t)t * 9 + i];
#pragma unroll
  for (int i = 0; i < 12; i++) c.c2w[i] = c2ws[(size_t)t * 16 + i];
  return c;
}
// c2w (inv_K (x, y, 1) d)
__device__ __forceinline__ void unproject(const Cam &c, float x, float y, float d, float (&w)[3]) {
  const float cx = (c.ik[0] * x + c.ik[1] * y + c.ik[2]) * d, cy = (c.ik[3] * x + c.ik[4] * y + c.ik[5]) * d,
              cz = (c.ik[6] * x + c.ik[7] * y + c.ik[8]) * d;
#pragma unroll
  for (int i = 0; i < 3; i++) w[i] = c.c2w[4 * i] * cx + c.c2w[4 * i + 1] * cy + c.c2w[4 * i + 2] * cz + c.c2w[4 * i + 3];
}

// every bilinear corner of (x, y) with a non-zero weight lies in the image and has mask == 1.  Stated in pixel coordinates: the
// corner floor(x) always weighs, floor(x) + 1 weighs iff x is no integer (x - floor(x) is exact), and the same in y.
__device__ __forceinline__ bool corners_in_mask(const float *__restrict__ m, int H, int W, float x, float y) {
  if (!(fabsf(x) < 1e9f) || !(fabsf(y) < 1e9f)) return false;  // NaN, inf, and nothing that far is in an image
  const float fx0 = floorf(x), fy0 = floorf(y);
  const int nx = x != fx0 ? 2 : 1, ny = y != fy0 ? 2 : 1;
  if (fx0 < 0.f || fy0 < 0.f || fx0 + (float)(nx - 1) > (float)(W - 1) || fy0 + (float)(ny - 1) > (float)(H - 1)) return false;
  const int ix = (int)fx0, iy = (int)fy0;
  for (int b = 0; b < ny; b++)
    for (int a = 0; a < nx; a++)
      if (m[(size_t)(iy + b) * W + ix + a] != 1.0f) return false;
  return true;
}

struct LiftArgs {
  const float *tracks, *depths, *masks, *query_img, *inv_Ks, *c2ws;
  int N, T, H, W, query;
  float *xyz, *conf, *colors;
  uint8_t *vis, *invis, *in_mask;
  int32_t *count, *hist;
};

__global__ void __launch_bounds__(256) k_lift_samples(const LiftArgs a) {
  const int64_t total = (int64_t)a.N * a.T, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t h = i; h <= a.T; h += (int64_t)gridDim.x * 256) a.hist[h] = 0;  // k_lift_tracks, behind this launch, fills it
  if (i >= total) return;
  const int t = (int)(i % a.T);
  const float x = a.tracks[4 * i], y = a.tracks[4 * i + 1], occ = a.tracks[4 * i + 2], dist = a.tracks[4 * i + 3];
  const float vis = 1.f - 1.f / (1.f + expf(-occ)), conf = 1.f - 1.f / (1.f + expf(-dist));
  const bool visible = vis * conf > 0.5f, invisible = (1.f - vis) * conf > 0.5f;
  const size_t frame = (size_t)t * a.H * a.W;
  const bool in = corners_in_mask(a.masks + frame, a.H, a.W, x, y);
  float d[1], w[3];
  bilinear_border<1>(a.depths + frame, a.H, a.W, x, y, d);
  unproject(load_cam(a.inv_Ks, a.c2ws, t), x, y, d[0], w);
  a.xyz[3 * i] = w[0], a.xyz[3 * i + 1] = w[1], a.xyz[3 * i + 2] = w[2];
  a.vis[i] = visible && in, a.invis[i] = invisible && in, a.in_mask[i] = in;
  a.conf[i] = (visible || invisible) && in ? conf : 0.f;
}

__global__ void __launch_bounds__(256) k_lift_tracks(const LiftArgs a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.N) return;
  int c = 0;
  for (int t = 0; t < a.T; t++) c += a.vis[(size_t)n * a.T + t];
  a.count[n] = c;
  atomicAdd(&a.hist[c], 1);  // an integer count: the same bins whatever the order
  const size_t q = ((size_t)n * a.T + a.query) * 4;
  float rgb[3];
  bilinear_border<3>(a.query_img, a.H, a.W, a.tracks[q], a.tracks[q + 1], rgb);
  a.colors[3 * (size_t)n] = rgb[0], a.colors[3 * (size_t)n + 1] = rgb[1], a.colors[3 * (size_t)n + 2] = rgb[2];
}

// ---- background points --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bkgd(const float *__restrict__ depths, const float *__restrict__ masks,
                                              const float *__restrict__ valid_masks, const float *__restrict__ inv_Ks,
                                              const float *__restrict__ c2ws, int64_t total, int H, int W, float *__restrict__ points,
                                              float *__restrict__ normals, uint8_t *__restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t HW = (int64_t)H * W;
  const int t = (int)(i / HW), y = (int)((i % HW) / W), x = (int)(i % W);
  const float *D = depths + (size_t)t * HW;
  const Cam cam = load_cam(inv_Ks, c2ws, t);
  const float d = D[(size_t)y * W + x];
  float p[3];
  unproject(cam, (float)x, (float)y, d, p);
  points[3 * i] = p[0], points[3 * i + 1] = p[1], points[3 * i + 2] = p[2];
  float n[3] = {0.f, 0.f, 0.f};
  if (x > 0 && x < W - 1 && y > 0 && y < H - 1) {  // the one-pixel border keeps the zero the reference pads with
    float r[3], l[3], u[3], b[3];
    unproject(cam, (float)(x + 1), (float)y, D[(size_t)y * W + x + 1], r);
    unproject(cam, (float)(x - 1), (float)y, D[(size_t)y * W + x - 1], l);
    unproject(cam, (float)x, (float)(y - 1), D[(size_t)(y - 1) * W + x], u);
    unproject(cam, (float)x, (float)(y + 1), D[(size_t)(y + 1) * W + x], b);
    const float e[3] = {r[0] - l[0], r[1] - l[1], r[2] - l[2]}, f[3] = {u[0] - b[0], u[1] - b[1], u[2] - b[2]};  // left to right, bottom to top
    n[0] = e[1] * f[2] - e[2] * f[1], n[1] = e[2] * f[0] - e[0] * f[2], n[2] = e[0] * f[1] - e[1] * f[0];
    const float inv = 1.f / fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-12f);
    n[0] *= inv, n[1] *= inv, n[2] *= inv;
  }
  normals[3 * i] = n[0], normals[3 * i + 1] = n[1], normals[3 * i + 2] = n[2];
  keep[i] = __fmul_rn(__fmul_rn(__fsub_rn(1.f, masks[i]), valid_masks[i]), d > 0.f ? 1.f : 0.f) != 0.f;
}

// Ordered compaction of one frame's keep flags: block t walks frame t in turns of BK_NT pixels; a kept pixel's place is the running
// count plus the kept pixels before it in the turn (ballot inside the wave, the waves' totals through LDS).  index[t, 0 .. counts[t])
// = the kept pixels' offsets in the frame, ascending: the order of boolean indexing.
constexpr int BK_NT = 1024, BK_WAVES = BK_NT / D4GS_WAVE;
__global__ void __launch_bounds__(BK_NT) k_bkgd_compact(const uint8_t *__restrict__ keep, int64_t HW, int32_t *__restrict__ index,
                                                        int32_t *__restrict__ counts) {
  __shared__ int wave_total[BK_WAVES];
  const uint8_t *K = keep + (size_t)blockIdx.x * HW;
  int32_t *I = index + (size_t)blockIdx.x * HW;
  const int wave = threadIdx.x / D4GS_WAVE, lane = threadIdx.x & (D4GS_WAVE - 1);
  int base = 0;
  for (int64_t first = 0; first < HW; first += BK_NT) {  // (uniform trip count: the barriers are met by all)
    const int64_t i = first + threadIdx.x;
    const bool flag = i < HW && K[i];
    const unsigned long long b = __ballot(flag);
    __syncthreads();  // the previous turn's totals have been read
    if (lane == 0) wave_total[wave] = __popcll(b);
    __syncthreads();
    int before = base + __popcll(b & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < BK_WAVES; w++) {
      before += w < wave ? wave_total[w] : 0;
      total += wave_total[w];
    }
    if (flag) I[before] = (int32_t)i;
    base += total;
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = base;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
inline int64_t up16(int64_t n) { return (n + 15) & ~(int64_t)15; }

struct MedianPlan {
  int tw, tiles, cpi;  // tiles across, tiles and chunks per image
  int64_t par, chunk, partials, lohi, bytes;  // byte offsets into the workspace, and its size
};
// false: a size < 1 or n_img H W > 2^31 - 1
bool median_plan(int64_t n_img, int64_t H, int64_t W, MedianPlan *p) {
  if (n_img < 1 || H < 1 || W < 1 || (double)n_img * (double)H * (double)W > (double)INT32_MAX) return false;
  const int64_t tw = (W + MM_TILE - 1) / MM_TILE, th = (H + MM_TILE - 1) / MM_TILE, cpi = (H * W + MM_CHUNK - 1) / MM_CHUNK;
  p->tw = (int)tw, p->tiles = (int)(tw * th), p->cpi = (int)cpi;
  p->par = 0;
  p->chunk = up16(n_img * H * W);
  p->partials = p->chunk + up16(n_img * cpi);
  p->lohi = p->partials + up16(n_img * tw * th * 8);
  p->bytes = p->lohi + up16(n_img * 8);
  return true;
}

}  // namespace

extern "C" {

int64_t d4gs_masked_median_ws_bytes(int64_t n_img, int64_t H, int64_t W) {
  MedianPlan p;
  return median_plan(n_img, H, W, &p) ? p.bytes : 0;
}

int d4gs_masked_median_blur(const float *image, const float *mask, const float *blend, int32_t n_img, int32_t H, int32_t W,
                            int32_t kernel_size, int32_t per_image, float *out, void *workspace, void *stream) {
  const char *who = "d4gs_masked_median_blur";
  const Ptr ptrs[] = {{image, "image", 4, true}, {mask, "mask", 4, true}, {blend, "blend", 4, false}, {out, "out", 4, true},
                      {workspace, "workspace", 16, true}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (n_img < 1 || H < 1 || W < 1) {
    d4gs_set_error("%s: bad size n_img=%d H=%d W=%d (each must be >= 1)", who, n_img, H, W);
    return D4GS_EINVAL;
  }
  if (kernel_size < 3 || kernel_size > MM_MAX_K || kernel_size % 2 == 0) {
    d4gs_set_error("%s: kernel_size=%d (odd, 3 <= kernel_size <= %d)", who, kernel_size, MM_MAX_K);
    return D4GS_EINVAL;
  }
  MedianPlan p;
  if (!median_plan(n_img, H, W, &p)) {
    d4gs_set_error("%s: size n_img=%d H=%d W=%d overflows (n_img H W <= 2^31 - 1)", who, n_img, H, W);
    return D4GS_EINVAL;
  }
  if (out == image) {
    d4gs_set_error("%s: out aliases image (the windows of later tiles read the input)", who);
    return D4GS_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  char *ws = (char *)workspace;
  uint8_t *par = (uint8_t *)(ws + p.par), *chunk = (uint8_t *)(ws + p.chunk);
  float *partials = (float *)(ws + p.partials), *lohi = (float *)(ws + p.lohi);
  const int k = kernel_size, pi = per_image != 0;
  const int64_t HW = (int64_t)H * W;
  const dim3 tile_grid((unsigned)(n_img * p.tiles)), chunk_grid((unsigned)(n_img * p.cpi));
  D4GS_LAUNCH("k_mm_count", k_mm_count, tile_grid, dim3(MM_NT), 0, s, image, mask, (int)H, (int)W, k, p.tw, p.tiles, par, partials);
  if (int rc = d4gs_check_launch("k_mm_count")) return rc;
  D4GS_LAUNCH("k_mm_chunk", k_mm_chunk<0>, chunk_grid, dim3(MM_NT), 0, s, par, HW, p.cpi, chunk);
  if (int rc = d4gs_check_launch("k_mm_chunk")) return rc;
  D4GS_LAUNCH("k_mm_carry", k_mm_carry, dim3(pi ? n_img : 1), dim3(MM_NT), 0, s, chunk, (const float *)partials, (int)n_img, p.cpi, p.tiles,
              pi, lohi);
  if (int rc = d4gs_check_launch("k_mm_carry")) return rc;
  D4GS_LAUNCH("k_mm_prefix", k_mm_chunk<1>, chunk_grid, dim3(MM_NT), 0, s, par, HW, p.cpi, chunk);
  if (int rc = d4gs_check_launch("k_mm_prefix")) return rc;
  D4GS_LAUNCH("k_mm_select", k_mm_select, tile_grid, dim3(MM_NT), 0, s, image, mask, blend, (const uint8_t *)par, (const float *)lohi,
              (int)H, (int)W, k, p.tw, p.tiles, pi, out);
  return d4gs_check_launch("k_mm_select");
}

int d4gs_lift_tracks(const float *tracks_2d, const float *depths, const float *masks, const float *query_img, const float *inv_Ks,
                     const float *c2ws, int32_t N, int32_t T, int32_t H, int32_t W, int32_t query, float *xyz, uint8_t *visibles,
                     uint8_t *invisibles, float *confidences, uint8_t *in_mask, float *colors, int32_t *visible_count, int32_t *hist,
                     void *stream) {
  const char *who = "d4gs_lift_tracks";
  const Ptr ptrs[] = {{tracks_2d, "tracks_2d", 4, true},     {depths, "depths", 4, true},
                      {masks, "masks", 4, true},             {query_img, "query_img", 4, true},
                      {inv_Ks, "inv_Ks", 4, true},           {c2ws, "c2ws", 4, true},
                      {xyz, "xyz", 4, true},                 {visibles, "visibles", 1, true},
                      {invisibles, "invisibles", 1, true},   {confidences, "confidences", 4, true},
                      {in_mask, "in_mask", 1, true},         {colors, "colors", 4, true},
                      {visible_count, "visible_count", 4, true}, {hist, "hist", 4, true}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (N < 1 || T < 1 || H < 1 || W < 1) {
    d4gs_set_error("%s: bad size N=%d T=%d H=%d W=%d (each must be >= 1)", who, N, T, H, W);
    return D4GS_EINVAL;
  }
  if (query < 0 || query >= T) {
    d4gs_set_error("%s: query=%d outside 0..T-1 (T=%d)", who, query, T);
    return D4GS_EINVAL;
  }
  if ((double)N * T * 4 > (double)INT32_MAX || (double)T * H * W > (double)INT32_MAX || (double)H * W * 3 > (double)INT32_MAX) {
    d4gs_set_error("%s: size N=%d T=%d H=%d W=%d overflows (N T 4, T H W, H W 3 <= 2^31 - 1)", who, N, T, H, W);
    return D4GS_EINVAL;
  }
  LiftArgs a;
  a.tracks = tracks_2d, a.depths = depths, a.masks = masks, a.query_img = query_img, a.inv_Ks = inv_Ks, a.c2ws = c2ws;
  a.N = N, a.T = T, a.H = H, a.W = W, a.query = query;
  a.xyz = xyz, a.conf = confidences, a.colors = colors, a.vis = visibles, a.invis = invisibles, a.in_mask = in_mask;
  a.count = visible_count, a.hist = hist;
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)N * T;
  D4GS_LAUNCH("k_lift_samples", k_lift_samples, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
  if (int rc = d4gs_check_launch("k_lift_samples")) return rc;
  D4GS_LAUNCH("k_lift_tracks", k_lift_tracks, dim3((N + 255) / 256), dim3(256), 0, s, a);
  return d4gs_check_launch("k_lift_tracks");
}

int d4gs_bkgd_points(const float *depths, const float *masks, const float *valid_masks, const float *inv_Ks, const float *c2ws, int32_t T,
                     int32_t H, int32_t W, float *points, float *normals, uint8_t *keep, int32_t *index, int32_t *counts, void *stream) {
  const char *who = "d4gs_bkgd_points";
  const Ptr ptrs[] = {{depths, "depths", 4, true}, {masks, "masks", 4, true},   {valid_masks, "valid_masks", 4, true}, {inv_Ks, "inv_Ks", 4, true},
                      {c2ws, "c2ws", 4, true},     {points, "points", 4, true}, {normals, "normals", 4, true},         {keep, "keep", 1, true},
                      {index, "index", 4, false},  {counts, "counts", 4, false}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (T < 1 || H < 1 || W < 1) {
    d4gs_set_error("%s: bad size T=%d H=%d W=%d (each must be >= 1)", who, T, H, W);
    return D4GS_EINVAL;
  }
  if (!index != !counts) {
    d4gs_set_error("%s: index and counts come together (index=%p counts=%p)", who, (void *)index, (void *)counts);
    return D4GS_EINVAL;
  }
  if ((double)T * H * W * 3 > (double)INT32_MAX) {
    d4gs_set_error("%s: size T=%d H=%d W=%d overflows (T H W 3 <= 2^31 - 1)", who, T, H, W);
    return D4GS_EINVAL;
  }
  const int64_t total = (int64_t)T * H * W;
  D4GS_LAUNCH("k_bkgd", k_bkgd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depths, masks, valid_masks, inv_Ks,
              c2ws, total, (int)H, (int)W, points, normals, keep);
  if (int rc = d4gs_check_launch("k_bkgd")) return rc;
  if (!index) return D4GS_OK;
  D4GS_LAUNCH("k_bkgd_compact", k_bkgd_compact, dim3(T), dim3(BK_NT), 0, (hipStream_t)stream, (const uint8_t *)keep, (int64_t)H * W, index,
              counts);
  return d4gs_check_launch("k_bkgd_compact");
}

}  // extern "C"
