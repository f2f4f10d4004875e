// scene_init.hip -- the device side of deblur4dgs_amd/scene_init.py: what the reference's flow3d/init_utils.py takes from cupy
// (batched_interp_masked), cuML (KMeans), sklearn (NearestNeighbors) and a Python loop over torch.linalg.svd.  Contracts:
// include/d4gs.h, "Scene initialisation"; kernels, resources and measured times: DESIGN.md section 24.
//
// Track features: one lane per track walks its row once.  Between two visible frames p < n the value at t is a + (b - a) (t - p) /
// (n - p) in double, rounded once; visible frames are copied.  The velocity direction uses the double values.
//
// kNN: a block holds 512 queries, two per lane, each with its running k best (squared distance, index) in registers, sorted
// ascending.  Candidates pass through LDS D4GS_KNN_TILE at a time as (x, y, z, -) quads; every lane reads the same quad, which the
// LDS broadcasts, and one read serves both of the lane's queries.  Four candidates are measured per turn and their minimum is held
// against the worse of the two current k-th distances, so the insertion (a bubble of k - 1 compare-exchanges) is rarely entered
// once the lists have warmed up.  Strict comparisons everywhere: among equal distances the candidate met first - the lower index -
// stays ahead.  A tile that overlaps the block's own queries runs the variant that skips j == q.  blockIdx.y splits the candidate
// tiles; each split leaves its sorted lists in the workspace and k_knn_merge folds them in split order (still lower index first).
//
// k-means: k_kmeans_assign (centres in LDS, one row per lane per turn), k_kmeans_accum (per block and cluster the sums of the D
// columns and the count, four columns at a time through the block sum of reduce.h), k_kmeans_finish (ordered total over the blocks,
// the division, the changed count).  The three use the same partition of the rows over blocks.
//
// Procrustes moments: one block per (frame, cluster), 16 running doubles per lane, the block sum of reduce.h.
#include <cmath>

#include "common.h"
#include "reduce.h"

namespace {

constexpr int KNN_NT = 256, KNN_QPL = 2, KNN_QB = KNN_NT * KNN_QPL;  // threads, queries per lane, queries per block
constexpr int KNN_TILE = D4GS_KNN_TILE;
constexpr int KNN_TARGET_BLOCKS = 1024;  // four 256-thread blocks per CU
constexpr int KNN_MAX_SPLITS = 64;
constexpr int64_t KNN_MAX_N = 1 << 24;
constexpr int KM_MAX_BLOCKS = 256;
constexpr int KM_MAX_LDS_FLOATS = 12288;  // K D floats of centres: 48 KiB
static_assert(KNN_TILE % 4 == 0, "four candidates per turn");

// ---- track features -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_track_features(const float *__restrict__ xyz, const uint8_t *__restrict__ visible, int G, int T,
                                                        float *__restrict__ interp, float *__restrict__ vel) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const float *X = xyz + (size_t)g * T * 3;
  const uint8_t *vis = visible + (size_t)g * T;
  float *I = interp ? interp + (size_t)g * T * 3 : nullptr;
  float *V = vel ? vel + (size_t)g * (T - 1) * 3 : nullptr;
  int n = 0;  // the next visible frame at or after t (T: none)
  while (n < T && !vis[n]) n++;
  const bool none = n == T;  // no visible frame: the row is kept as it is
  int p = -1;                // the last visible frame before t (-1: none yet)
  double prev[3] = {0.0, 0.0, 0.0};
  for (int t = 0; t < T; t++) {
    double cur[3];
    bool copy = none;
    if (!none && t == n) {
      copy = true;
      p = n;
      n = t + 1;
      while (n < T && !vis[n]) n++;
    }
    if (copy) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float x = X[t * 3 + c];
        cur[c] = (double)x;
        if (I) I[t * 3 + c] = x;
      }
    } else {
      const int a = p < 0 ? n : p, b = n == T ? p : n;  // before the first: both the first; after the last: both the last
      const double w = (p < 0 || n == T) ? 0.0 : (double)(t - p) / (double)(n - p);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double va = (double)X[a * 3 + c], vb = (double)X[b * 3 + c];
        cur[c] = va + (vb - va) * w;
        if (I) I[t * 3 + c] = (float)cur[c];
      }
    }
    if (V && t > 0) {
      const double v0 = cur[0] - prev[0], v1 = cur[1] - prev[1], v2 = cur[2] - prev[2];
      const double inv = 1.0 / (sqrt(v0 * v0 + v1 * v1 + v2 * v2) + 1e-5);
      V[(t - 1) * 3 + 0] = (float)(v0 * inv), V[(t - 1) * 3 + 1] = (float)(v1 * inv), V[(t - 1) * 3 + 2] = (float)(v2 * inv);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) prev[c] = cur[c];
  }
}

// ---- kNN ------------------------------------------------------------------------------------------------------------------
template <int K>
struct Best {
  float d[K];
  int i[K];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int s = 0; s < K; s++) d[s] = INFINITY, i[s] = -1;
  }
  // dist < d[K - 1] is known: the candidate takes the last slot and rises while it is strictly nearer than the slot above
  __device__ __forceinline__ void insert(float dist, int idx) {
    d[K - 1] = dist, i[K - 1] = idx;
#pragma unroll
    for (int s = K - 1; s > 0; s--) {
      const bool up = d[s] < d[s - 1];
      const float lo = up ? d[s] : d[s - 1], hi = up ? d[s - 1] : d[s];
      const int ilo = up ? i[s] : i[s - 1], ihi = up ? i[s - 1] : i[s];
      d[s - 1] = lo, d[s] = hi, i[s - 1] = ilo, i[s] = ihi;
    }
  }
};

__device__ __forceinline__ float sqdist(const float4 c, float x, float y, float z) {
  const float dx = c.x - x, dy = c.y - y, dz = c.z - z;
  return dx * dx + dy * dy + dz * dz;
}

// one staged tile against the lane's two queries; cnt is a multiple of 4 (the tile's tail holds +inf coordinates: never nearer)
template <int K, bool SELF>
__device__ __forceinline__ void knn_scan(const float4 *tile, int cnt, int base, const int (&q)[KNN_QPL], const float (&qp)[KNN_QPL][3],
                                         Best<K> (&best)[KNN_QPL]) {
  for (int j = 0; j < cnt; j += 4) {
    float d[KNN_QPL][4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const float4 c = tile[j + u];
#pragma unroll
      for (int a = 0; a < KNN_QPL; a++) {
        d[a][u] = sqdist(c, qp[a][0], qp[a][1], qp[a][2]);
        if (SELF && base + j + u == q[a]) d[a][u] = INFINITY;
      }
    }
#pragma unroll
    for (int a = 0; a < KNN_QPL; a++) {
      const float m = fminf(fminf(d[a][0], d[a][1]), fminf(d[a][2], d[a][3]));
      if (m < best[a].d[K - 1]) {
#pragma unroll
        for (int u = 0; u < 4; u++)
          if (d[a][u] < best[a].d[K - 1]) best[a].insert(d[a][u], base + j + u);
      }
    }
  }
}

struct KnnArgs {
  const float *points;
  int N, splits, tiles_per_split;
  float *dists;    // [N,K]
  int32_t *idx;    // [N,K] or null
  float *ws_d;     // [splits,N,K] squared distances (splits > 1)
  int32_t *ws_i;   // [splits,N,K]
};

template <int K>
__global__ void __launch_bounds__(KNN_NT) k_knn(const KnnArgs a) {
  __shared__ float4 tile[KNN_TILE];
  const int tid = threadIdx.x, q0 = blockIdx.x * KNN_QB;
  int q[KNN_QPL];
  float qp[KNN_QPL][3];
  Best<K> best[KNN_QPL];
#pragma unroll
  for (int u = 0; u < KNN_QPL; u++) {
    q[u] = q0 + u * KNN_NT + tid;
    const int qq = q[u] < a.N ? q[u] : a.N - 1;  // a lane past the end measures the last point and writes nothing
#pragma unroll
    for (int c = 0; c < 3; c++) qp[u][c] = a.points[(size_t)qq * 3 + c];
    best[u].init();
  }
  const int ntiles = (a.N + KNN_TILE - 1) / KNN_TILE;
  const int t0 = blockIdx.y * a.tiles_per_split, t1 = min(t0 + a.tiles_per_split, ntiles);
  for (int t = t0; t < t1; t++) {
    const int base = t * KNN_TILE, cnt = min(KNN_TILE, a.N - base), cnt4 = (cnt + 3) & ~3;
    __syncthreads();  // the previous tile has been read by every lane
    for (int i = tid; i < cnt4; i += KNN_NT) {
      float4 c = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
      if (i < cnt) {
        const float *p = a.points + (size_t)(base + i) * 3;
        c.x = p[0], c.y = p[1], c.z = p[2];
      }
      tile[i] = c;
    }
    __syncthreads();
    if (base < q0 + KNN_QB && base + cnt > q0)  // block-uniform: the tile holds some of the block's own queries
      knn_scan<K, true>(tile, cnt4, base, q, qp, best);
    else
      knn_scan<K, false>(tile, cnt4, base, q, qp, best);
  }
#pragma unroll
  for (int u = 0; u < KNN_QPL; u++) {
    if (q[u] >= a.N) continue;
    if (a.splits == 1) {
#pragma unroll
      for (int s = 0; s < K; s++) {
        a.dists[(size_t)q[u] * K + s] = sqrtf(best[u].d[s]);
        if (a.idx) a.idx[(size_t)q[u] * K + s] = best[u].i[s];
      }
    } else {
      const size_t o = ((size_t)blockIdx.y * a.N + q[u]) * K;
#pragma unroll
      for (int s = 0; s < K; s++) a.ws_d[o + s] = best[u].d[s], a.ws_i[o + s] = best[u].i[s];
    }
  }
}

template <int K>
__global__ void __launch_bounds__(256) k_knn_merge(const KnnArgs a) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= a.N) return;
  Best<K> best;
  best.init();
  for (int sp = 0; sp < a.splits; sp++) {
    const size_t o = ((size_t)sp * a.N + q) * K;
#pragma unroll
    for (int s = 0; s < K; s++) {
      const float d = a.ws_d[o + s];
      if (d < best.d[K - 1]) best.insert(d, a.ws_i[o + s]);
    }
  }
#pragma unroll
  for (int s = 0; s < K; s++) {
    a.dists[(size_t)q * K + s] = sqrtf(best.d[s]);
    if (a.idx) a.idx[(size_t)q * K + s] = best.i[s];
  }
}

// the split of the candidate tiles over blockIdx.y; false: illegal N
bool knn_plan(int64_t N, int *splits, int *tiles_per_split) {
  if (N < 2 || N > KNN_MAX_N) return false;
  const int ntiles = (int)((N + KNN_TILE - 1) / KNN_TILE), qblocks = (int)((N + KNN_QB - 1) / KNN_QB);
  int s = 1;
  if (N > D4GS_KNN_SPLIT_MIN) {
    s = (KNN_TARGET_BLOCKS + qblocks - 1) / qblocks;
    s = s < 1 ? 1 : (s > KNN_MAX_SPLITS ? KNN_MAX_SPLITS : s);
    s = s > ntiles ? ntiles : s;
  }
  const int per = (ntiles + s - 1) / s;
  *tiles_per_split = per;
  *splits = (ntiles + per - 1) / per;  // no empty split
  return true;
}

template <int K>
int knn_launch(const KnnArgs &a, hipStream_t s) {
  const dim3 grid((a.N + KNN_QB - 1) / KNN_QB, a.splits);
  D4GS_LAUNCH("k_knn", k_knn<K>, grid, dim3(KNN_NT), 0, s, a);
  if (int rc = d4gs_check_launch("k_knn")) return rc;
  if (a.splits == 1) return D4GS_OK;
  D4GS_LAUNCH("k_knn_merge", k_knn_merge<K>, dim3((a.N + 255) / 256), dim3(256), 0, s, a);
  return d4gs_check_launch("k_knn_merge");
}

// ---- k-means --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_kmeans_assign(const float *__restrict__ x, int G, int D, int K, const float *__restrict__ centres,
                                                       int32_t *__restrict__ labels, int32_t *__restrict__ changed_partials) {
  extern __shared__ float cen[];  // [K,D]
  __shared__ int wave_changed[4];
  const int tid = threadIdx.x;
  for (int i = tid; i < K * D; i += 256) cen[i] = centres[i];
  __syncthreads();
  int nchg = 0;
  for (int g = blockIdx.x * 256 + tid; g < G; g += gridDim.x * 256) {
    const float *xr = x + (size_t)g * D;
    float bestd = INFINITY;
    int bestk = 0;
    for (int k = 0; k < K; k++) {
      const float *c = cen + k * D;
      float s = 0.f;
      for (int d = 0; d < D; d++) {
        const float t = xr[d] - c[d];
        s = fmaf(t, t, s);
      }
      if (s < bestd) bestd = s, bestk = k;  // strict: a tie keeps the lower index
    }
    nchg += labels[g] != bestk;
    labels[g] = bestk;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nchg += __shfl_xor(nchg, o);
  if ((tid & (D4GS_WAVE - 1)) == 0) wave_changed[tid / D4GS_WAVE] = nchg;
  __syncthreads();
  if (tid == 0) changed_partials[blockIdx.x] = wave_changed[0] + wave_changed[1] + wave_changed[2] + wave_changed[3];
}

// partials [gridDim.x][K][Dp]: columns 0..D-1 the sums of the cluster's rows, column D its count, the rest (Dp = D + 1 rounded up to
// a multiple of 4) zero
__global__ void __launch_bounds__(256) k_kmeans_accum(const float *__restrict__ x, int G, int D, int Dp, int K,
                                                      const int32_t *__restrict__ labels, double *__restrict__ partials) {
  __shared__ double red[4 * 4];
  const int tid = threadIdx.x, k = blockIdx.y;
  for (int d0 = 0; d0 < Dp; d0 += 4) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = blockIdx.x * 256 + tid; g < G; g += gridDim.x * 256) {
      if (labels[g] != k) continue;
      const float *xr = x + (size_t)g * D;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int col = d0 + r;
        v[r] += col < D ? (double)xr[col] : (col == D ? 1.0 : 0.0);
      }
    }
    block_sum_store(v, red);
    __syncthreads();
    if (tid < 4) partials[((size_t)blockIdx.x * K + k) * Dp + d0 + tid] = block_sum_combine<4>(red, tid);
    __syncthreads();  // red is written again in the next turn
  }
}

__global__ void __launch_bounds__(256) k_kmeans_finish(const double *__restrict__ partials, int nb, int D, int Dp, int K,
                                                       float *__restrict__ centres, const int32_t *__restrict__ changed_partials,
                                                       int32_t *__restrict__ changed) {
  const int tid = threadIdx.x, k = blockIdx.x;
  const double *base = partials + (size_t)k * Dp;
  const int64_t stride = (int64_t)K * Dp;
  double cnt[1];
  ordered_total(base + D, (int64_t)nb, stride, cnt);
  for (int d0 = 0; d0 < Dp; d0 += 4) {
    double t[4];
    ordered_total(base + d0, (int64_t)nb, stride, t);
    if (cnt[0] > 0.0) {  // an empty cluster keeps its centre
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (tid == r && d0 + r < D) centres[(size_t)k * D + d0 + r] = (float)(t[r] / cnt[0]);
    }
  }
  if (k == 0 && tid == 0) {
    int s = 0;
    for (int i = 0; i < nb; i++) s += changed_partials[i];
    changed[0] = s;
  }
}

int64_t kmeans_blocks(int64_t G) {
  if (G < 1 || G > INT32_MAX) return 0;
  const int64_t b = (G + 255) / 256;
  return b < KM_MAX_BLOCKS ? b : KM_MAX_BLOCKS;
}

bool kmeans_sizes_ok(int64_t G, int32_t D, int32_t K) {
  return G >= 1 && D >= 1 && K >= 1 && K <= D4GS_KMEANS_MAX_K && (int64_t)K * D <= KM_MAX_LDS_FLOATS && (double)G * D <= (double)INT32_MAX;
}

int kmeans_dp(int D) { return (D + 1 + 3) & ~3; }

// ---- Procrustes moments ---------------------------------------------------------------------------------------------------
struct MomentArgs {
  const float *xyz, *w, *conf;
  const int32_t *order, *seg;
  int G, T, K, cano;
  double *out;
};

__global__ void __launch_bounds__(256) k_procrustes_moments(const MomentArgs a) {
  __shared__ double red[4 * 16];
  const int tid = threadIdx.x, t = blockIdx.x, k = blockIdx.y;
  const int lo = min(max(a.seg[k], 0), a.G), hi = min(max(a.seg[k + 1], 0), a.G);
  double v[16];
#pragma unroll
  for (int r = 0; r < 16; r++) v[r] = 0.0;
  for (int i = lo + tid; i < hi; i += 256) {
    const int p = a.order[i];
    if ((unsigned)p >= (unsigned)a.G) continue;
    const size_t rc = (size_t)p * a.T + a.cano, rt = (size_t)p * a.T + t;
    const double u = (((double)a.w[rc] * (double)a.w[rt]) * ((double)a.conf[rc] + (double)a.conf[rt])) / 2.0;
    double s[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; c++) s[c] = (double)a.xyz[rc * 3 + c], d[c] = (double)a.xyz[rt * 3 + c];
    v[0] += u;
#pragma unroll
    for (int c = 0; c < 3; c++) v[1 + c] += u * s[c], v[4 + c] += u * d[c];
#pragma unroll
    for (int i2 = 0; i2 < 3; i2++)
#pragma unroll
      for (int j = 0; j < 3; j++) v[7 + 3 * i2 + j] += (u * d[i2]) * s[j];
  }
  block_sum_store(v, red);
  __syncthreads();
  if (tid < 16) a.out[((size_t)k * a.T + t) * 16 + tid] = block_sum_combine<16>(red, tid);
}

// ---- argument checks ------------------------------------------------------------------------------------------------------
struct Ptr {
  const void *p;
  const char *name;
  unsigned align;
  bool required;
};

template <int N>
bool pointers_ok(const char *who, const Ptr (&ptrs)[N]) {
  for (const auto &q : ptrs) {
    if (!q.p && q.required) {
      d4gs_set_error("%s: %s is NULL", who, q.name);
      return false;
    }
    if ((uintptr_t)q.p % q.align) {
      d4gs_set_error("%s: %s = %p is misaligned (%u-byte alignment needed)", who, q.name, q.p, q.align);
      return false;
    }
  }
  return true;
}

}  // namespace

extern "C" {

int d4gs_track_features(const float *xyz, const uint8_t *visible, int32_t G, int32_t T, float *xyz_interp, float *vel_dirs, void *stream) {
  const char *who = "d4gs_track_features";
  const Ptr ptrs[] = {{xyz, "xyz", 4, true}, {visible, "visible", 1, true}, {xyz_interp, "xyz_interp", 4, false}, {vel_dirs, "vel_dirs", 4, false}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (G < 1 || T < 1) {
    d4gs_set_error("%s: bad size G=%d T=%d (each must be >= 1)", who, G, T);
    return D4GS_EINVAL;
  }
  if (vel_dirs && T < 2) {
    d4gs_set_error("%s: vel_dirs needs T >= 2 (T=%d)", who, T);
    return D4GS_EINVAL;
  }
  if ((double)G * T * 3 > (double)INT32_MAX) {
    d4gs_set_error("%s: size G=%d T=%d overflows (G T 3 <= 2^31 - 1)", who, G, T);
    return D4GS_EINVAL;
  }
  if (!xyz_interp && !vel_dirs) return D4GS_OK;
  D4GS_LAUNCH("k_track_features", k_track_features, dim3((G + 255) / 256), dim3(256), 0, (hipStream_t)stream, xyz, visible, (int)G, (int)T,
              xyz_interp, vel_dirs);
  return d4gs_check_launch("k_track_features");
}

int32_t d4gs_knn_splits(int64_t N) {
  int s, per;
  return knn_plan(N, &s, &per) ? s : 0;
}

int64_t d4gs_knn_workspace_bytes(int64_t N, int32_t k) {
  int s, per;
  if (k < 1 || k > D4GS_KNN_MAX_K || N < (int64_t)k + 1 || !knn_plan(N, &s, &per)) return 0;
  const int64_t b = s > 1 ? (int64_t)s * N * k * 8 : 0;
  return b > 16 ? b : 16;
}

int d4gs_knn(const float *points, int32_t N, int32_t k, float *dists, int32_t *idx, void *workspace, void *stream) {
  const char *who = "d4gs_knn";
  const Ptr ptrs[] = {{points, "points", 4, true}, {dists, "dists", 4, true}, {idx, "idx", 4, false}, {workspace, "workspace", 16, true}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (N < 1) {
    d4gs_set_error("%s: bad size N=%d (must be >= 1)", who, N);
    return D4GS_EINVAL;
  }
  if (k < 1 || k > D4GS_KNN_MAX_K) {
    d4gs_set_error("%s: k=%d (1 <= k <= %d)", who, k, D4GS_KNN_MAX_K);
    return D4GS_EINVAL;
  }
  if (N < k + 1) {
    d4gs_set_error("%s: N=%d points have no k=%d neighbours each (N >= k + 1)", who, N, k);
    return D4GS_EINVAL;
  }
  KnnArgs a;
  if (!knn_plan(N, &a.splits, &a.tiles_per_split)) {
    d4gs_set_error("%s: size N=%d overflows (N <= 2^24)", who, N);
    return D4GS_EINVAL;
  }
  a.points = points, a.N = N, a.dists = dists, a.idx = idx;
  a.ws_d = (float *)workspace;
  a.ws_i = (int32_t *)((char *)workspace + (size_t)a.splits * N * k * 4);
  hipStream_t s = (hipStream_t)stream;
  switch (k) {
    case 1: return knn_launch<1>(a, s);
    case 2: return knn_launch<2>(a, s);
    case 3: return knn_launch<3>(a, s);
    case 4: return knn_launch<4>(a, s);
    case 5: return knn_launch<5>(a, s);
    case 6: return knn_launch<6>(a, s);
    case 7: return knn_launch<7>(a, s);
    default: return knn_launch<8>(a, s);
  }
}

int64_t d4gs_kmeans_blocks(int64_t G) { return kmeans_blocks(G); }

int64_t d4gs_kmeans_scratch_bytes(int64_t G, int32_t D, int32_t K) {
  if (!kmeans_sizes_ok(G, D, K)) return 0;
  const int64_t nb = kmeans_blocks(G);
  return nb * K * kmeans_dp(D) * 8 + ((nb * 4 + 7) & ~(int64_t)7);
}

int d4gs_kmeans_step(const float *x, int32_t G, int32_t D, int32_t K, int32_t iters, float *centres, int32_t *labels, int32_t *changed,
                     void *scratch, void *stream) {
  const char *who = "d4gs_kmeans_step";
  const Ptr ptrs[] = {{x, "x", 4, true},           {centres, "centres", 4, true}, {labels, "labels", 4, true},
                      {changed, "changed", 4, true}, {scratch, "scratch", 8, true}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (G < 1 || D < 1 || K < 1 || iters < 1) {
    d4gs_set_error("%s: bad size G=%d D=%d K=%d iters=%d (each must be >= 1)", who, G, D, K, iters);
    return D4GS_EINVAL;
  }
  if (K > D4GS_KMEANS_MAX_K) {
    d4gs_set_error("%s: K=%d (K <= %d)", who, K, D4GS_KMEANS_MAX_K);
    return D4GS_EINVAL;
  }
  if (!kmeans_sizes_ok(G, D, K)) {
    d4gs_set_error("%s: size G=%d D=%d K=%d overflows (K D <= %d, G D <= 2^31 - 1)", who, G, D, K, KM_MAX_LDS_FLOATS);
    return D4GS_EINVAL;
  }
  const int nb = (int)kmeans_blocks(G), Dp = kmeans_dp(D);
  double *partials = (double *)scratch;
  int32_t *chg = (int32_t *)((char *)scratch + (size_t)nb * K * Dp * 8);
  hipStream_t s = (hipStream_t)stream;
  for (int it = 0; it < iters; it++) {
    D4GS_LAUNCH("k_kmeans_assign", k_kmeans_assign, dim3(nb), dim3(256), (size_t)K * D * sizeof(float), s, x, (int)G, (int)D, (int)K,
                (const float *)centres, labels, chg);
    if (int rc = d4gs_check_launch("k_kmeans_assign")) return rc;
    D4GS_LAUNCH("k_kmeans_accum", k_kmeans_accum, dim3(nb, K), dim3(256), 0, s, x, (int)G, (int)D, Dp, (int)K, (const int32_t *)labels,
                partials);
    if (int rc = d4gs_check_launch("k_kmeans_accum")) return rc;
    D4GS_LAUNCH("k_kmeans_finish", k_kmeans_finish, dim3(K), dim3(256), 0, s, (const double *)partials, nb, (int)D, Dp, (int)K, centres,
                (const int32_t *)chg, changed);
    if (int rc = d4gs_check_launch("k_kmeans_finish")) return rc;
  }
  return D4GS_OK;
}

int d4gs_procrustes_moments(const float *xyz, const float *weights, const float *conf, const int32_t *order, const int32_t *seg, int32_t G,
                            int32_t T, int32_t K, int32_t cano_t, double *out, void *stream) {
  const char *who = "d4gs_procrustes_moments";
  const Ptr ptrs[] = {{xyz, "xyz", 4, true},     {weights, "weights", 4, true}, {conf, "conf", 4, true},
                      {order, "order", 4, true}, {seg, "seg", 4, true},         {out, "out", 8, true}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (G < 1 || T < 1 || K < 1) {
    d4gs_set_error("%s: bad size G=%d T=%d K=%d (each must be >= 1)", who, G, T, K);
    return D4GS_EINVAL;
  }
  if (cano_t < 0 || cano_t >= T) {
    d4gs_set_error("%s: cano_t=%d outside 0..T-1 (T=%d)", who, cano_t, T);
    return D4GS_EINVAL;
  }
  if (K > 65535 || (double)G * T * 3 > (double)INT32_MAX) {
    d4gs_set_error("%s: size G=%d T=%d K=%d overflows the grid (K <= 65535, G T 3 <= 2^31 - 1)", who, G, T, K);
    return D4GS_EINVAL;
  }
  MomentArgs a;
  a.xyz = xyz, a.w = weights, a.conf = conf, a.order = order, a.seg = seg, a.G = G, a.T = T, a.K = K, a.cano = cano_t, a.out = out;
  D4GS_LAUNCH("k_procrustes_moments", k_procrustes_moments, dim3(T, K), dim3(256), 0, (hipStream_t)stream, a);
  return d4gs_check_launch("k_procrustes_moments");
}

}  // extern "C"
