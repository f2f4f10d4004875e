// feed.hip -- the device side of deblur4dgs_amd/feed.py: what StereoLowDataset.__getitem__ (flow3d/data/stereo_low_dataset.py:574-666),
// train_collate_fn and the trainer's shaping of the track supervision (trainer.py:549-565, 646-659) do per training step, from a clip
// that lives in device memory.  Contracts: include/d4gs.h, "Feed"; layout, rules and times: DESIGN.md section 28.
//
// k_feed_draw   one wave: num_targets distinct frames of [start, end) from an integer hash of (seed, *counter), then *counter += 1.
//               Floyd's sampling: pick k is t = rand_k mod (R - n + k + 1), or R - n + k where an earlier pick already holds t; lane k
//               keeps pick k, "already holds" is a ballot.  feed_rand is compiled for the host too: d4gs_feed_draw_cpu is the twin.
// k_feed_batch  one launch, three kinds of block in one grid (FB lanes each):
//   track blocks   N x ceil(P / FB): block (n, c) takes the queries p = c FB ... of target n, so the selection (query frame, target
//                  frame, their time ids, the query frame's slice of the track table) is block-uniform - scalar loads, SGPRs.  A lane
//                  loads its 16-byte track row (consecutive lanes, consecutive rows) and the query row, forms the flags, samples the
//                  target frame's depth and image, and writes the batch tensors and the track-loss tables.
//   plane blocks   the query frame's image, valid mask, mask and depth, PLANE_CHUNK floats per block: 16-byte words where source and
//                  destination share their offset in a 16-byte line, dwords for the head, the tail and every other case.
//   the last block the small tensors: ts, K, w2c, the targets' ts / Ks / w2cs, n_queries, status.
// No atomics, one writer per address: bitwise reproducible.  A selection that is out of range never forms an address: every block
// evaluates the same test and writes padding instead.
#include "args.h"
#include "common.h"
#include "sampling.h"

namespace {

constexpr int FB = 256;                 // lanes per block
constexpr int PLANE_CHUNK = FB * 16;    // floats of a plane per block: four 16-byte words per lane
constexpr int FEED_MAX_TARGETS = 64;    // one wave holds a draw
enum { ST_INDEX = 1, ST_TARGET = 2, ST_TIME = 4, ST_TABLE = 8 };

__host__ __device__ inline uint64_t feed_mix(uint64_t z) {  // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the k-th 32-bit word of step `step` under `seed`: counter-based, no state
__host__ __device__ inline uint32_t feed_rand(uint64_t seed, int64_t step, int k) {
  const uint64_t key = feed_mix(seed ^ feed_mix((uint64_t)step + 0x9E3779B97F4A7C15ull));
  return (uint32_t)(feed_mix(key + 0x9E3779B97F4A7C15ull * (uint64_t)(k + 1)) >> 32);
}
// Floyd's candidate of pick k of n out of R: uniform in 0 ... R - n + k (multiply-shift: the bias is below 2^-32 R)
__host__ __device__ inline int feed_candidate(uint64_t seed, int64_t step, int k, int n, int R) {
  return (int)(((uint64_t)feed_rand(seed, step, k) * (uint64_t)(R - n + k + 1)) >> 32);
}

__global__ void __launch_bounds__(D4GS_WAVE) k_feed_draw(int64_t *counter, uint64_t seed, int start, int end, int n, int32_t *__restrict__ targets) {
  const int lane = threadIdx.x, R = end - start;
  const int64_t step = *counter;
  __syncthreads();  // every lane has read the counter
  int mine = -1;
  for (int k = 0; k < n; k++) {
    const int t = feed_candidate(seed, step, k, n, R);
    const bool taken = __ballot(lane < k && mine == t) != 0ull;
    if (lane == k) mine = taken ? R - n + k : t;
  }
  if (lane < n) targets[lane] = start + mine;
  if (lane == 0) *counter = step + 1;
}

struct FeedArgs {
  const float *imgs, *depths, *masks, *valid_masks, *Ks, *w2cs, *tracks;
  const int64_t *time_ids, *offsets;
  const int32_t *index, *targets;
  int64_t n_rows;
  int F, H, W, N, P, num_frames;
  int track_blocks, per_target, plane_blocks, img_blocks, map_blocks;
  int64_t *ts, *target_ts;
  float *w2c, *K, *img, *valid_mask, *mask, *depth, *query, *target_w2cs, *target_Ks, *target_tracks, *conf, *tdepth, *timg, *weights;
  uint8_t *visibles, *invisibles, *vis;
  int32_t *pix, *rows, *n_queries, *status;
};

// What every block reads first, from block-uniform addresses: the query frame, its queries and where their rows start, or status != 0
// and Pq = 0.  Nothing is addressed through a value that failed its test.
struct Selection {
  int q, Pq, status;
  int64_t base;
};
__device__ __forceinline__ Selection feed_select(const FeedArgs &a) {
  Selection s{a.index[0], 0, 0, 0};
  if (s.q < 0 || s.q >= a.F) s.status |= ST_INDEX;
  for (int n = 0; n < a.N; n++) {
    const int t = a.targets[n];
    if (t < 0 || t >= a.F) {
      s.status |= ST_TARGET;
    } else {
      const int64_t tt = a.time_ids[t];
      if (tt < 0 || tt >= a.F) s.status |= ST_TIME;  // (the reference takes target_w2cs and target_Ks at the TIME id)
    }
  }
  if (!(s.status & ST_INDEX)) {
    const int64_t o0 = a.offsets[s.q], o1 = a.offsets[s.q + 1];
    if (o0 < 0 || o1 < o0 || o1 > a.n_rows || (o1 - o0) % a.F != 0 || (o1 - o0) / a.F > (int64_t)INT32_MAX)
      s.status |= ST_TABLE;
    else
      s.base = o0, s.Pq = (int)((o1 - o0) / a.F);
  }
  if (s.status) s.Pq = 0;
  return s;
}

__device__ __forceinline__ void feed_tracks(const FeedArgs &a, const Selection &s, int block) {
  const int n = block / a.per_target, p = (block - n * a.per_target) * FB + (int)threadIdx.x;
  if (p >= a.P) return;
  float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
  float qx = -1.f, qy = -1.f, conf = 0.f, d[1] = {0.f}, rgb[3] = {0.f, 0.f, 0.f}, w = 0.f;
  bool visible = false, invisible = false;
  int pix = -1;
  if (p < s.Pq) {
    const int t = a.targets[n];  // (in range: s.status == 0)
    const float4 *T = reinterpret_cast<const float4 *>(a.tracks);
    row = T[s.base + (int64_t)t * s.Pq + p];
    const float4 qr = T[s.base + (int64_t)s.q * s.Pq + p];
    qx = qr.x, qy = qr.y;
    const float vis = 1.f - 1.f / (1.f + expf(-row.z)), c = 1.f - 1.f / (1.f + expf(-row.w));  // utils.py:60-65
    visible = vis * c > 0.5f, invisible = (1.f - vis) * c > 0.5f;
    conf = visible || invisible ? c : 0.f;
    const size_t frame = (size_t)t * a.H * a.W;
    bilinear_border<1>(a.depths + frame, a.H, a.W, row.x, row.y, d);
    bilinear_border<3>(a.imgs + frame * 3, a.H, a.W, row.x, row.y, rgb);
    // trainer.py:549,646-647 and the trailing-axis sum of track_losses: conf sum_n' exp(-2 |ts - target_ts[n']| / num_frames)
    const int64_t ts = a.time_ids[s.q];
    float sum = 0.f;
    for (int m = 0; m < a.N; m++) {
      const int64_t dt = ts - a.time_ids[a.targets[m]];
      sum += expf(-2.f * (float)(dt < 0 ? -dt : dt) / (float)a.num_frames);
    }
    // the query's pixel, truncated as the trainer's query_pixels; outside the image: no pixel, not visible, no weight
    if (fabsf(qx) < 1e9f && fabsf(qy) < 1e9f) {
      const int xi = (int)qx, yi = (int)qy;
      if (xi >= 0 && xi < a.W && yi >= 0 && yi < a.H) pix = yi * a.W + xi, w = conf * sum;
    }
  }
  const int64_t o = (int64_t)n * a.P + p;
  if (n == 0) reinterpret_cast<float2 *>(a.query)[p] = make_float2(qx, qy);
  reinterpret_cast<float2 *>(a.target_tracks)[o] = make_float2(row.x, row.y);
  a.visibles[o] = visible, a.invisibles[o] = invisible, a.conf[o] = conf, a.tdepth[o] = d[0];
#pragma unroll
  for (int c = 0; c < 3; c++) a.timg[((int64_t)n * 3 + c) * a.P + p] = rgb[c];
  a.pix[o] = pix, a.rows[o] = n, a.vis[o] = visible && pix >= 0, a.weights[o] = w;
}

// dst[0 .. len) = src[0 .. len), or zeros without a source; the block's lanes share the work
__device__ __forceinline__ void feed_copy(float *__restrict__ dst, const float *__restrict__ src, int len) {
  const int tid = threadIdx.x;
  if (!src) {
    for (int i = tid; i < len; i += FB) dst[i] = 0.f;
    return;
  }
  if ((((uintptr_t)src ^ (uintptr_t)dst) & 15u) != 0) {  // the two never meet on a 16-byte line
    for (int i = tid; i < len; i += FB) dst[i] = src[i];
    return;
  }
  const int head = min(len, (int)(((16u - ((uintptr_t)src & 15u)) & 15u) >> 2)), words = (len - head) >> 2, tail = head + 4 * words;
  if (tid < head) dst[tid] = src[tid];
  const float4 *s4 = reinterpret_cast<const float4 *>(src + head);
  float4 *d4 = reinterpret_cast<float4 *>(dst + head);
  for (int i = tid; i < words; i += FB) d4[i] = s4[i];
  if (tail + tid < len) dst[tail + tid] = src[tail + tid];
}

__device__ __forceinline__ void feed_planes(const FeedArgs &a, const Selection &s, int block) {
  const int64_t HW = (int64_t)a.H * a.W;
  const float *src;
  float *dst;
  int64_t len;
  if (block < a.img_blocks) {
    src = a.imgs, dst = a.img, len = 3 * HW;
  } else {
    block -= a.img_blocks;
    const int which = block / a.map_blocks;
    block -= which * a.map_blocks;
    src = which == 0 ? a.valid_masks : which == 1 ? a.masks : a.depths;
    dst = which == 0 ? a.valid_mask : which == 1 ? a.mask : a.depth;
    len = HW;
  }
  const int64_t first = (int64_t)block * PLANE_CHUNK;
  const int count = (int)min((int64_t)PLANE_CHUNK, len - first);
  feed_copy(dst + first, s.status ? nullptr : src + (int64_t)s.q * len + first, count);
}

__device__ __forceinline__ void feed_small(const FeedArgs &a, const Selection &s) {
  const int tid = threadIdx.x;
  const bool ok = s.status == 0;
  if (tid < 16) a.w2c[tid] = ok ? a.w2cs[(size_t)s.q * 16 + tid] : 0.f;
  if (tid < 9) a.K[tid] = ok ? a.Ks[(size_t)s.q * 9 + tid] : 0.f;
  for (int i = tid; i < a.N * 16; i += FB) {
    const int n = i >> 4;
    a.target_w2cs[i] = ok ? a.w2cs[(size_t)a.time_ids[a.targets[n]] * 16 + (i & 15)] : 0.f;
  }
  for (int i = tid; i < a.N * 9; i += FB) {
    const int n = i / 9;
    a.target_Ks[i] = ok ? a.Ks[(size_t)a.time_ids[a.targets[n]] * 9 + (i - 9 * n)] : 0.f;
  }
  for (int n = tid; n < a.N; n += FB) a.target_ts[n] = ok ? a.time_ids[a.targets[n]] : 0;
  if (tid == 0) {
    a.ts[0] = ok ? a.time_ids[s.q] : 0;
    a.n_queries[0] = s.Pq;
    a.status[0] |= s.status;  // (one writer: no atomic; sticky until the caller clears it)
  }
}

__global__ void __launch_bounds__(FB) k_feed_batch(const FeedArgs a) {
  const Selection s = feed_select(a);
  const int b = blockIdx.x;
  if (b < a.track_blocks)
    feed_tracks(a, s, b);
  else if (b < a.track_blocks + a.plane_blocks)
    feed_planes(a, s, b - a.track_blocks);
  else
    feed_small(a, s);
}

int draw_check(const char *who, const int64_t *counter, int32_t start, int32_t end, int32_t n, const int32_t *targets) {
  const Ptr ptrs[] = {{counter, "counter", 8, true}, {targets, "targets", 4, true}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (start < 0 || end <= start) {
    d4gs_set_error("%s: bad range start=%d end=%d (0 <= start < end)", who, start, end);
    return D4GS_EINVAL;
  }
  if (n < 1 || n > FEED_MAX_TARGETS || n > end - start) {
    d4gs_set_error("%s: n=%d distinct frames of %d (1 <= n <= min(end - start, %d))", who, n, end - start, FEED_MAX_TARGETS);
    return D4GS_EINVAL;
  }
  return D4GS_OK;
}

}  // namespace

extern "C" {

int d4gs_feed_draw(int64_t *counter, uint64_t seed, int32_t start, int32_t end, int32_t n, int32_t *targets, void *stream) {
  if (int rc = draw_check("d4gs_feed_draw", counter, start, end, n, targets)) return rc;
  D4GS_LAUNCH("k_feed_draw", k_feed_draw, dim3(1), dim3(D4GS_WAVE), 0, (hipStream_t)stream, counter, seed, (int)start, (int)end, (int)n, targets);
  return d4gs_check_launch("k_feed_draw");
}

int d4gs_feed_draw_cpu(int64_t *counter, uint64_t seed, int32_t start, int32_t end, int32_t n, int32_t *targets) {
  if (int rc = draw_check("d4gs_feed_draw_cpu", counter, start, end, n, targets)) return rc;
  const int R = end - start;
  const int64_t step = *counter;
  for (int k = 0; k < n; k++) {
    const int t = feed_candidate(seed, step, k, n, R);
    bool taken = false;
    for (int j = 0; j < k; j++) taken |= targets[j] == start + t;
    targets[k] = start + (taken ? R - n + k : t);
  }
  *counter = step + 1;
  return D4GS_OK;
}

int d4gs_feed_batch(const float *imgs, const float *depths, const float *masks, const float *valid_masks, const float *Ks, const float *w2cs,
                    const int64_t *time_ids, const float *tracks, const int64_t *offsets, int64_t n_rows, const int32_t *index,
                    const int32_t *targets, int32_t F, int32_t H, int32_t W, int32_t N, int32_t P, int32_t num_frames, int64_t *ts,
                    float *w2c, float *K, float *img, float *valid_mask, float *mask, float *depth, float *query_tracks_2d,
                    int64_t *target_ts, float *target_w2cs, float *target_Ks, float *target_tracks_2d, uint8_t *target_visibles,
                    uint8_t *target_invisibles, float *target_confidences, float *target_track_depths, float *target_track_imgs,
                    int32_t *pix, int32_t *rows, uint8_t *vis, float *weights, int32_t *n_queries, int32_t *status, void *stream) {
  const char *who = "d4gs_feed_batch";
  const Ptr ptrs[] = {{imgs, "imgs", 4, true},
                      {depths, "depths", 4, true},
                      {masks, "masks", 4, true},
                      {valid_masks, "valid_masks", 4, true},
                      {Ks, "Ks", 4, true},
                      {w2cs, "w2cs", 4, true},
                      {time_ids, "time_ids", 8, true},
                      {tracks, "tracks", 16, true},
                      {offsets, "offsets", 8, true},
                      {index, "index", 4, true},
                      {targets, "targets", 4, true},
                      {ts, "ts", 8, true},
                      {w2c, "w2c", 4, true},
                      {K, "K", 4, true},
                      {img, "img", 4, false},
                      {valid_mask, "valid_mask", 4, false},
                      {mask, "mask", 4, false},
                      {depth, "depth", 4, false},
                      {query_tracks_2d, "query_tracks_2d", 8, true},
                      {target_ts, "target_ts", 8, true},
                      {target_w2cs, "target_w2cs", 4, true},
                      {target_Ks, "target_Ks", 4, true},
                      {target_tracks_2d, "target_tracks_2d", 8, true},
                      {target_visibles, "target_visibles", 1, true},
                      {target_invisibles, "target_invisibles", 1, true},
                      {target_confidences, "target_confidences", 4, true},
                      {target_track_depths, "target_track_depths", 4, true},
                      {target_track_imgs, "target_track_imgs", 4, true},
                      {pix, "pix", 4, true},
                      {rows, "rows", 4, true},
                      {vis, "vis", 1, true},
                      {weights, "weights", 4, true},
                      {n_queries, "n_queries", 4, true},
                      {status, "status", 4, true}};
  if (!pointers_ok(who, ptrs)) return D4GS_EINVAL;
  if (F < 1 || H < 1 || W < 1 || N < 1 || P < 1 || num_frames < 1 || n_rows < 1) {
    d4gs_set_error("%s: bad size F=%d H=%d W=%d N=%d P=%d num_frames=%d n_rows=%lld (each must be >= 1)", who, F, H, W, N, P, num_frames,
                   (long long)n_rows);
    return D4GS_EINVAL;
  }
  if (N > FEED_MAX_TARGETS) {
    d4gs_set_error("%s: N=%d target frames (N <= %d)", who, N, FEED_MAX_TARGETS);
    return D4GS_EINVAL;
  }
  const int planes = (img != nullptr) + (valid_mask != nullptr) + (mask != nullptr) + (depth != nullptr);
  if (planes != 0 && planes != 4) {
    d4gs_set_error("%s: img, valid_mask, mask and depth come together (img=%p valid_mask=%p mask=%p depth=%p)", who, (void *)img,
                   (void *)valid_mask, (void *)mask, (void *)depth);
    return D4GS_EINVAL;
  }
  if ((double)F * H * W * 3 > (double)INT32_MAX || (double)N * P * 3 > (double)INT32_MAX) {
    d4gs_set_error("%s: size F=%d H=%d W=%d N=%d P=%d overflows (F H W 3, N P 3 <= 2^31 - 1)", who, F, H, W, N, P);
    return D4GS_EINVAL;
  }
  FeedArgs a;
  a.imgs = imgs, a.depths = depths, a.masks = masks, a.valid_masks = valid_masks, a.Ks = Ks, a.w2cs = w2cs, a.tracks = tracks;
  a.time_ids = time_ids, a.offsets = offsets, a.index = index, a.targets = targets, a.n_rows = n_rows;
  a.F = F, a.H = H, a.W = W, a.N = N, a.P = P, a.num_frames = num_frames;
  const int64_t HW = (int64_t)H * W;
  a.per_target = (P + FB - 1) / FB, a.track_blocks = N * a.per_target;
  a.img_blocks = planes ? (int)((3 * HW + PLANE_CHUNK - 1) / PLANE_CHUNK) : 0;
  a.map_blocks = planes ? (int)((HW + PLANE_CHUNK - 1) / PLANE_CHUNK) : 0;
  a.plane_blocks = a.img_blocks + 3 * a.map_blocks;
  a.ts = ts, a.target_ts = target_ts, a.w2c = w2c, a.K = K, a.img = img, a.valid_mask = valid_mask, a.mask = mask, a.depth = depth;
  a.query = query_tracks_2d, a.target_w2cs = target_w2cs, a.target_Ks = target_Ks, a.target_tracks = target_tracks_2d;
  a.conf = target_confidences, a.tdepth = target_track_depths, a.timg = target_track_imgs, a.weights = weights;
  a.visibles = target_visibles, a.invisibles = target_invisibles, a.vis = vis;
  a.pix = pix, a.rows = rows, a.n_queries = n_queries, a.status = status;
  D4GS_LAUNCH("k_feed_batch", k_feed_batch, dim3((unsigned)(a.track_blocks + a.plane_blocks + 1)), dim3(FB), 0, (hipStream_t)stream, a);
  return d4gs_check_launch("k_feed_batch");
}

}  // extern "C"
