// host.h -- every host function of libd4gs.so that one translation unit defines and another calls, declared ONCE.
//
// No device code and nothing that needs one: cpu_twin.hip includes this file alone, every other source gets it through common.h.
// The extern "C" entry points themselves are declared in include/d4gs.h.  Default arguments are written here and nowhere else.
//
// Every defining file sees its own declaration, so a definition that drifts from it collides at compile time wherever a default
// argument or a call in the same file is involved.  Where it does not (C++ takes the drifted definition for a new overload), the
// declared function stays undefined in libd4gs.so (a shared library links with undefined symbols) and ctypes loads the library
// with RTLD_NOW: the first test that loads it fails with "undefined symbol".  That load is the check.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/d4gs.h"

// ---- error plumbing and argument checks (capi.hip) ------------------------------------------------------------------------
void d4gs_set_error(const char *fmt, ...);  // the thread's d4gs_last_error() message
int d4gs_check_launch(const char *what);    // hipGetLastError() -> D4GS_OK / D4GS_ELAUNCH (+ message)
int d4gs_check_dims(const D4gsDims *d);     // the dims every render entry point accepts -> D4GS_OK / D4GS_EINVAL (+ message)
// D4GS_ABSGRAD and its buffers come together; so do D4GS_ANTIALIASED and D4gsProjOut.compensations
int d4gs_check_absgrad(const char *who, const D4gsDims *d, const float *v_means2d_abs, int32_t stats_absgrad);
int d4gs_check_antialiased(const char *who, const D4gsDims *d, const float *compensations);
int d4gs_copy_counts_impl(const int64_t *n_isect, int64_t *host_pinned, hipStream_t stream);

// ---- projection, poses (project_fwd.hip, project_bwd.hip) -----------------------------------------------------------------
int d4gs_project_fwd_impl(const D4gsDims *dims, const D4gsProjIn *in, const D4gsProjOut *out, hipStream_t stream);
int d4gs_project_bwd_impl(const D4gsDims *dims, const D4gsProjIn *in, const D4gsProjOut *proj, const float *v_means2d,
                          const float *v_conics, const float *v_depths, const float *v_opac_act, const float *v_ctab,
                          const D4gsLeafGrads *grads, hipStream_t stream);
int d4gs_poses_fwd_impl(const D4gsDims *dims, const D4gsProjIn *in, const D4gsPoses *out, hipStream_t stream);
int d4gs_poses_bwd_impl(const D4gsDims *dims, const D4gsProjIn *in, const D4gsPoses *v_out, const D4gsLeafGrads *grads,
                        hipStream_t stream);
size_t d4gs_poses_bwd_partials_bound(const D4gsDims *d);  // host arithmetic only: no device is asked
// [S][K][16] time-blended bases (project_bwd.hip: k_bases_table), for callers of d4gs_project_bwd without D4gsProjOut.blend_bases
int d4gs_bases_table_launch(const D4gsDims *dims, const D4gsProjIn *in, float *btab, hipStream_t stream);
// tiles across `pixels` of width or height; colour channels + the depth channel of a render
inline int d4gs_tiles_across(int pixels) { return (pixels + D4GS_TILE - 1) / D4GS_TILE; }
inline int d4gs_nch(const D4gsDims *d) { return d->D + (d->depth_mode != D4GS_DEPTH_NONE ? 1 : 0); }

// ---- the list front end's launch rules, stated once (project_fwd.hip) -----------------------------------------------------
// Projection, tile counting, the scans, k_emit, the tile sorts and the composites all launch over the same tile grid, and
// k_count_tiles / k_emit over the same chunks of instances: every entry point computes this plan once and reads it.
constexpr int D4GS_CHUNK_THREADS = 1024;  // lanes of a k_count_tiles / k_emit block: one constant, so their chunks cannot drift apart
static_assert(D4GS_CHUNK_THREADS % 64 == 0 && D4GS_CHUNK_THREADS <= 1024, "whole waves, one workgroup");
struct FrontPlan {
  int tw, th, tiles;  // the tile grid of one sub-sample
  int n_tiles;        // x S
  bool hist_in_lds;   // one sub-sample's tile histogram (an int per tile) fits in 64 KB of LDS: k_emit bins there, and ...
  bool count_apart;   // ... k_count_tiles counts there (unless N = 0 or D4GS_COUNT_IN_PROJECT, the tests' hook for the fallback,
                      // k_project_fwd's global atomics, that bigger grids take)
  // Chunks: a block takes per_block = D4GS_CHUNK_THREADS * pt consecutive instances of one sub-sample.  pt, the instances per lane,
  // is 1 when 4 would leave fewer blocks than CUs (S = 1, N = 300 k gave 74 blocks for 256 CUs), else the fewest of 2 ... 6 that
  // makes the launch one round of the chip's 512 block slots, else 4 (always 4 for D4GS_LAZY_SORT): d4gs_front_plan.
  int pt, per_block, nchunks /* per sub-sample */, blocks /* nchunks * S */;
  int fused_chunks;  // nchunks: the fused scan is in effect (k_count_tiles leaves chunk sums, k_emit writes isect_offsets); 0: the
                     // two-pass scan (D4GS_NO_FUSED_SCAN, the tests' hook; !count_apart; a scan_ws too small for the chunk sums)
};
FrontPlan d4gs_front_plan(const D4gsDims *d);

// ---- binning, D4GS_LAZY_SORT (binning.hip, project_fwd.hip) ---------------------------------------------------------------
int d4gs_bin_sort_impl(const D4gsDims *dims, const D4gsProjOut *proj, const D4gsIsect *isect, hipStream_t stream);
bool d4gs_lazy_on(const D4gsDims *d, const D4gsProjOut *out, const FrontPlan &fp);
int d4gs_lazy_pivot_launch(const D4gsDims *d, const D4gsProjOut *out, const FrontPlan &fp, int64_t near_target, hipStream_t stream);
int d4gs_lazy_far_sort(const D4gsDims *dims, const D4gsProjOut *proj, const D4gsIsect *isect, hipStream_t stream);

// ---- composites (raster_fwd.hip, raster_bwd.hip) --------------------------------------------------------------------------
// The exposure blend's adjoint (blend.hip k_blend_bwd) folded into the composite backward's prologue by the one-call path (frame.hip):
// a pixel of sub-sample s takes v_blended / S on the mean channels, the whole of it on a max / min channel iff s is the first
// sub-sample (of the first S - 1) whose value equals the blended one (k_blend_fwd leaves that index), and v_acc / S on alpha - k_blend_bwd's expressions, bit for bit.
struct BlendAdj {
  const float *v_blended;  // [H,W,channels] or NULL
  const float *v_acc;      // [H,W] or NULL
  const int8_t *win;       // [H,W,channels] max / min channels: the sub-sample the gradient goes to, -1 = the mean (k_blend_fwd)
  uint64_t non_mean;       // bit c: channel c is a max / min channel
};
int d4gs_raster_fwd_impl(const D4gsDims *dims, const D4gsProjOut *proj, const D4gsIsect *isect, const D4gsRaster *r,
                         hipStream_t stream);
int d4gs_raster_bwd_impl(const D4gsDims *dims, const D4gsProjOut *proj, const D4gsIsect *isect, const D4gsRaster *r,
                         const D4gsRasterGrads *g, const BlendAdj *blend, hipStream_t stream);
// floats of D4gsRaster.seg_state for one configuration (0: segments are not used for it; common.h, "depth segments")
int64_t d4gs_seg_state_elems(const D4gsDims *d);
// do the composite kernels of this launch use segments?  (the forward writes the boundary states, the backward replays by segment)
bool d4gs_seg_on(const D4gsDims *d, const D4gsIsect *isect, const D4gsRaster *r);

// ---- exposure blend (blend.hip) -------------------------------------------------------------------------------------------
int d4gs_blend_fwd_impl(int32_t S, int64_t P, int32_t C, const int32_t *policy, const float *renders, const float *alphas,
                        float *out, float *acc, int8_t *win, hipStream_t stream, const int64_t *n_isect = nullptr,
                        int64_t *counts_pinned = nullptr);
int d4gs_blend_bwd_impl(int32_t S, int64_t P, int32_t C, const int32_t *policy, const float *renders, const float *out,
                        const float *v_out, const float *v_acc, float *v_renders, float *v_alphas, hipStream_t stream);
int d4gs_blend_bwd_add_impl(int32_t S, int64_t P, int32_t C, const int32_t *policy, const float *renders, const float *out,
                            const float *v_out, const float *v_acc, float *v_renders, float *v_alphas, const float *add_r,
                            const float *add_a, hipStream_t stream, const int8_t *win = nullptr);
int d4gs_blend_shard_impl(int what, const D4gsShardBlend *b, const void *p0, const void *p1, const void *p2, void *o0, void *o1,
                          hipStream_t stream);

// ---- control steps (control.hip) ------------------------------------------------------------------------------------------
int d4gs_control_stats_impl(int32_t S, int32_t N, const float *xys_grad, const int32_t *radii, int32_t width, int32_t height,
                            int32_t batch_size, float *grad_norm_acc, int64_t *vis_count, float *max_radii,
                            int32_t update_max_radii, hipStream_t stream);
int d4gs_control_plan_impl(int32_t N, const uint8_t *split_or_cull, const uint8_t *dup, int32_t *src_map, int32_t *counts,
                           hipStream_t stream);
int d4gs_gather_rows_impl(const int32_t *src_map, int64_t n_out, int32_t row_floats, const float *in, float *out,
                          int64_t zero_from, int64_t add_from, float add, hipStream_t stream);

// ---- camera path, MoveModel (camera.hip) ----------------------------------------------------------------------------------
int d4gs_pose_encode_impl(const float *R, int32_t r_stride, const float *T, int32_t t_stride, float *enc, hipStream_t stream);
int d4gs_pose_encode_bwd_impl(const float *R, int32_t r_stride, const float *T, int32_t t_stride, const float *v_enc, float *v_R,
                              float *v_T, hipStream_t stream);
int d4gs_camera_path_fwd_impl(const float *delta0, const float *delta1, int32_t S, const float *time_params, int32_t index,
                              float t, int32_t moving, float *RTs, float *jac, float *times, float *dtimes, float *deltaT,
                              hipStream_t stream);
int d4gs_camera_path_bwd_impl(const float *jac, const float *dtimes, const float *deltaT, const float *v_RTs,
                              const float *v_times, const float *v_deltaT, int32_t S, int32_t index, int32_t n_time_params,
                              float *v_delta0, float *v_delta1, float *v_time_params, hipStream_t stream);
int d4gs_move_model_fwd_impl(const float *R, int32_t r_stride, const float *T, int32_t t_stride, const float *const *w,
                             const float *const *b, int32_t S, const float *time_params, int32_t index, float t, int32_t moving,
                             float *enc, float *acts, float *delta, float *RTs, float *jac, float *times, float *dtimes,
                             float *deltaT, hipStream_t stream);
int d4gs_move_model_bwd_impl(const float *jac, const float *dtimes, const float *deltaT, const float *acts, const float *const *w,
                             const float *const *b, const float *v_RTs, const float *v_times, const float *v_deltaT, int32_t S,
                             int32_t index, int32_t n_time_params, float *v_delta, float *const *v_w, float *const *v_b,
                             float *v_time_params, float *v_enc, hipStream_t stream);

// ---- quantile selection over a caller's own values (trimmed.hip; track_fit.hip calls it) ----------------------------------
// values: the first n words of `scratch` (d4gs_trimmed_scratch_words(n, 1) words, 8-byte aligned), written on `stream` before this
// call.  masked_l1_loss(normalize=True): out[0] = sum_{v < thr} v w / (sum_{v < thr} w + 1e-8), out[1] = thr, out[2] = 1 / denominator;
// quantile >= 1 keeps every element.  No second radix select anywhere: this is trim_reduce.
bool d4gs_bad_quantile(float q);  // NaN, <= 0, inf
int d4gs_trim_masked_impl(void *scratch, const float *weights, int64_t n, float quantile, float *out, hipStream_t stream);

// ---- photometric loss (photometric.hip), spherical harmonics (sh.hip) -----------------------------------------------------
int d4gs_photometric_fwd_impl(const float *pred, const float *gt, const float *mask, int32_t B, int32_t H, int32_t W, float w_l1,
                              float w_ssim, float *maps, float *partials, float *loss, hipStream_t stream);
int d4gs_photometric_bwd_impl(const float *pred, const float *gt, const float *mask, const float *maps, const float *v_loss,
                              int32_t B, int32_t H, int32_t W, float w_l1, float w_ssim, float *v_pred, hipStream_t stream);
int d4gs_sh_fwd_impl(int64_t N, int32_t K, int32_t degree, const float *p, const float *origin, const float *coeffs,
                     const uint8_t *mask, int32_t clamp, float *rgb, hipStream_t stream);
int d4gs_sh_bwd_impl(int64_t N, int32_t K, int32_t degree, const float *p, const float *origin, const float *coeffs,
                     const uint8_t *mask, int32_t clamp, const float *v_rgb, float *v_coeffs, float *v_p, float *v_origin,
                     float *partials, hipStream_t stream);
