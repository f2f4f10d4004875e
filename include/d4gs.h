/* d4gs.h -- C ABI of libd4gs.so: MI355X-native (gfx950) 4D-Gaussian exposure rasterizer.
 *
 * Drop-in boundary for ONE path of ZcsrenlongZ/Deblur4DGS: everything `SceneModel.render`
 * (reference flow3d/scene_model.py:162-487) does on the device for one blurry frame --
 *   per-Gaussian activations            flow3d/params.py:39-43,70-84
 *   motion-basis deformation            flow3d/params.py:142-180, flow3d/transforms.py:41-53
 *   pose compose + camera delta         flow3d/scene_model.py:67-120,352-353
 *   gsplat.rendering.rasterization      flow3d/scene_model.py:360-373  (gsplat==1.1.1, packed=False)
 *   exposure blend                      flow3d/scene_model.py:386-397
 * forward and backward.  The reference reaches that code through Python (torch autograd + the gsplat
 * CUDA extension); there is no C interface in the reference to copy, so the entry points below are what a
 * ctypes / pybind binding of this path binds (see INTEGRATION.md for the stub).
 *
 * Conventions
 *  - plain C, no torch types.  A descriptor struct (`const D4gsDims *dims`, `D4gsSizes *sizes`, ...) is passed as a HOST pointer,
 *    unless its parameter is marked [device].  Every other pointer, parameter or struct field, is a DEVICE pointer unless it is
 *    marked [host] (the CPU twins say so of all of theirs in their own paragraph).  The marks are read by machine: this header is
 *    the one statement of the ABI, and deblur4dgs_amd/_lib.py derives the ctypes binding from it.  A mark
 *    counts where it stands in the inline comment of its own declaration - after a parameter and before its comma, or after a
 *    field's semicolon on the same line; block comments above a declaration are prose.
 *  - the library never allocates, frees or synchronises: outputs and scratch are caller-provided,
 *    every call only enqueues work on `stream` (a hipStream_t passed as void*).
 *  - return 0 on success, negative D4GS_E* on error; message via d4gs_last_error() (thread-local).
 *  - all floating point is fp32; matrices are row-major; quaternions are wxyz.
 *  - instance index i = s*N + g (sub-sample s, Gaussian g); the first G Gaussians are dynamic.
 */
#ifndef D4GS_H
#define D4GS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libd4gs.so is built with -fvisibility=hidden: the entry points below are its whole dynamic symbol table. */
#define D4GS_API __attribute__((visibility("default")))

#define D4GS_VERSION 305
#define D4GS_TILE 16
#define D4GS_GEOM_STRIDE 8 /* floats per instance record: x, y, opacity, depth, conic a, b, c, pad */

enum {
  D4GS_OK = 0,
  D4GS_EINVAL = -1,     /* bad argument / unsupported shape */
  D4GS_ELAUNCH = -2,    /* hipLaunch / runtime error (message holds hipGetErrorString) */
  D4GS_ECAPACITY = -3   /* caller-provided buffer too small */
};

enum { /* D4gsDims.flags */
  D4GS_RAW_PARAMS = 1,  /* quats/scales/opacities/motion_coefs are raw leaves: apply normalize/exp/sigmoid/softmax
                           (params.py:39-43).  When clear, scales/opacities are used as given (gsplat seam). */
  D4GS_RAW_COLORS = 2,  /* the first `n_sigmoid` colour channels are raw: apply sigmoid (params.py:40) */
  D4GS_LAZY_SORT = 8,   /* occluded / large-footprint scenes (most of every tile list lies behind the tile's last contributor):
                           every list is split into a NEAR part (the nearest depth buckets, about D4gsIsect.near_target keys)
                           and the rest; near parts are emitted, sorted and composited first, the far part of a list is
                           emitted and sorted - and the tile composited again over its whole list - only if the tile did not
                           saturate within the near part (d4gs_raster_fwd does that between its two passes).  Same lists where they matter, same image and gradients bit for bit;
                           needs D4gsProjOut.lazy_ws. */
  D4GS_EXACT_TILES = 16, /* (v305) on top of D4GS_EXACT_CULL: inside the tight rectangle, bin a splat only into the tiles its alpha >= 1/255
                           ellipse actually reaches (the corner tiles of a 2 x 2 ... 8 x 8 rectangle usually are not reached: 15 - 40 % shorter
                           lists at 720p).  The per-tile test runs in d4gs_project_fwd, the pairs of a wave's 64 instances spread over its
                           lanes, and leaves a 64-bit tile mask per instance (D4gsProjOut.tile_masks, required with the flag).  Same images
                           and gradients bit for bit; tiles_touched / the lists get shorter.  Pays from ~3 tiles per instance on.
                           The flag must be THE SAME in the dims passed to d4gs_project_fwd, d4gs_bin_sort, d4gs_raster_fwd and
                           d4gs_raster_bwd of one render (the counts and offsets are built from the masks; the binning walks them):
                           with the flag and no tile_masks those calls return D4GS_EINVAL. */
  D4GS_ABSGRAD = 32,    /* (v305) absgrad (gsplat's `absgrad=True`, the AbsGS grow criterion): d4gs_raster_bwd / d4gs_backward also
                           return v_means2d_abs [S,N,2] = sum over pixels p of (|dL_p/dx|, |dL_p/dy|) per instance - each pixel's own
                           contribution to v_means2d, every channel, the depth channel, v_alphas and the background included, made
                           absolute before the sum.  Rows of isect_grad grow by two floats (D4gsSizes.isect_grad_row = 8 + D'), the
                           frame workspace with them.  Needs D4gsRasterGrads / D4gsFrameGrads.v_means2d_abs (and v_means2d_abs
                           needs the flag); renders of more than 16 colour channels (several channel chunks) cannot be assembled from
                           per-chunk sums.  The CPU twins do not implement it (D4GS_EINVAL). */
  D4GS_ANTIALIASED = 64, /* (v305) gsplat's rasterize_mode="antialiased" (the Mip-Splatting 2-D filter): d4gs_project_fwd computes per
                           instance compensation = sqrt(max(0, det(cov2d) / det(cov2d + eps2d I))) (0 for culled instances), writes it to
                           D4gsProjOut.compensations and composites - and culls, under D4GS_EXACT_CULL / D4GS_EXACT_TILES - with opacity *
                           compensation.  means2d, conics, depths, radii and the tile rectangles keep their classic definitions.
                           d4gs_raster_bwd / d4gs_backward fold the compensation's adjoint into v_conics and return v_opac_act = sum over s
                           of compensation * (gradient of the effective opacity).  Needs D4gsProjOut.compensations (and it needs the flag)
                           in d4gs_project_fwd and d4gs_raster_bwd; the one-call frame carves it from the workspace.  The CPU twins do
                           not implement it (D4GS_EINVAL). */
  D4GS_EXACT_CULL = 4   /* bin a splat only into tiles that hold a pixel with alpha >= 1/255 (tight ellipse
                           sigma <= ln(255*opacity), intersected with gsplat's 3-sigma tile rectangle).  Pixels in
                           the dropped tiles would fail gsplat's alpha test anyway, so images and gradients are
                           unchanged; only the intersection lists (tiles_touched / flatten ids) get shorter. */
};

enum { D4GS_DEPTH_NONE = 0, D4GS_DEPTH_ED = 1, D4GS_DEPTH_D = 2 }; /* render_mode RGB / RGB+ED / RGB+D */
/* Depth-only renders (v305): D4gsDims.D == 0 with depth_mode D4GS_DEPTH_D or D4GS_DEPTH_ED is gsplat's render_mode "D" / "ED" - one
 * channel, the composited depth (ED: divided by max(alpha, 1e-10)), no background.  d4gs_query_sizes (ctab 0, isect_grad_row 7, or 9
 * with D4GS_ABSGRAD), d4gs_project_fwd (no colour table is written: in->colors and out->ctab may be NULL), d4gs_bin_sort,
 * d4gs_raster_fwd, d4gs_raster_bwd (v_ctab may be NULL) and d4gs_project_bwd (colors, ctab, v_ctab and v_colors may be NULL) take it.
 * D == 0 with D4GS_DEPTH_NONE, and D == 0 passed to d4gs_forward / d4gs_backward / d4gs_frame_workspace_bytes(_fwd), are D4GS_EINVAL
 * (the workspace queries return 0). */
/* D4gsRasterGrads.row_mode.  DENSE: every row of isect_grad is written (rows behind a tile's last contributor zero-filled);
 * SPARSE: only replayed rows are written and flagged in isect_live (large-footprint / occluded scenes).  Same gradients, bitwise. */
enum { D4GS_ROWS_AUTO = 0, D4GS_ROWS_DENSE = 1, D4GS_ROWS_SPARSE = 2 };

typedef struct D4gsDims {
  int32_t N;          /* Gaussians */
  int32_t G;          /* dynamic Gaussians (deformed by the motion bases); 0 = static scene */
  int32_t K;          /* motion bases */
  int32_t T;          /* frames per basis */
  int32_t S;          /* exposure sub-samples in this call */
  int32_t D;          /* colour channels supplied by the caller (without the depth channel); 0: a depth-only render (see above) */
  int32_t width, height;
  int32_t depth_mode; /* D4GS_DEPTH_* ; channels rendered = D + (depth_mode != 0) */
  int32_t flags;      /* D4GS_RAW_* */
  int32_t n_sigmoid;  /* with D4GS_RAW_COLORS: channels [0,n_sigmoid) get sigmoid */
  float near_plane, far_plane, eps2d, radius_clip; /* gsplat defaults 0.01, 1e10, 0.3, 0 */
} D4gsDims;

/* leaf inputs of the deform+project stage */
typedef struct D4gsProjIn {
  const float *means;        /* [N,3] */
  const float *quats;        /* [N,4] wxyz */
  const float *scales;       /* [N,3] */
  const float *opacities;    /* [N]   */
  const float *colors;       /* [N,D] row-major, or NULL if every channel is generated (mask) */
  const float *motion_coefs; /* [G,K] or NULL */
  const float *rots;         /* [K,T,6] or NULL */
  const float *transls;      /* [K,T,3] or NULL */
  const float *times;        /* [S] exposure times (frame units); ignored when G == 0 */
  const float *RTs;          /* [S,3,4] camera deltas, or NULL = identity */
  const float *viewmat;      /* [4,4] world->camera */
  const float *Kmat;         /* [3,3] intrinsics */
} D4gsProjIn;

/* per-instance outputs + binning counters produced by d4gs_project_fwd */
typedef struct D4gsProjOut {
  float *means2d;          /* [S,N,2] pixel units */
  float *depths;           /* [S,N]   */
  float *conics;           /* [S,N,3] */
  int32_t *radii;          /* [S,N]  >0 <=> visible */
  float *opac_act;         /* [N]    activated opacity */
  float *ctab;             /* [N,DP] activated colour table, DP = 4*ceil(D/4); 16-byte aligned (rows are stored / read as 16-byte words:
                              d4gs_project_fwd / d4gs_project_bwd return D4GS_EINVAL otherwise) */
  float *geom;             /* [S*N,8] packed raster record */
  int32_t *tile_rects;     /* [S*N,2] packed tile rectangle: x0 | x1<<16 , y0 | y1<<16 (min incl., max excl.) */
  int32_t *tiles_touched;  /* [S*N] */
  int32_t *isect_offsets;  /* [S*N] exclusive scan of tiles_touched (emission index base of every instance); complete after
                              d4gs_bin_sort: for small tile grids the binning stage finishes the scan itself */
  int32_t *lazy_ws;        /* [D4gsSizes.lazy_ws] scratch of D4GS_LAZY_SORT (per (tile, depth bucket) counts, near counts, pivots,
                              slot cursors, tile flags, depth range); NULL without the flag.  (Until v302 this slot was the
                              unused `tile_ranks`.) */
  int32_t *tile_counts;    /* [2*S*tiles]: [0,T) splats per tile, [T,2T) per-tile slot cursors - zeroed by
                              d4gs_project_fwd and consumed by d4gs_bin_sort, which therefore runs once per projection
                              (a launch refused by the capacity check does not touch them); T = S*tiles */
  int32_t *tile_offsets;   /* [S*tiles+1] exclusive scan of tile_counts */
  int64_t *n_isect;        /* [4] {total intersections, longest tile list, sampled entries, sampled live entries}: [0], [1]
                              are read back by the host to size the next stage and to pick the sort size classes.  [2], [3]
                              (zeroed by d4gs_project_fwd, accumulated by d4gs_raster_fwd over a fixed sample of <= 128 tiles -
                              device-scope atomics queue up memory-side, one per tile would cost the composite 5 - 30 %): list
                              entries of the sampled tiles, and how many of them lie at or in front of their tile's last
                              contributor, i.e. the rows the backward will replay.  [3] / [2] estimates the live fraction a
                              caller can choose D4gsRasterGrads.row_mode from (deblur4dgs_amd/engine.py does, one render late) */
  int32_t *scan_ws;        /* [d4gs_scan_ws_elems(S*N)] scratch */
  float *blend_bases;      /* [S,K,16] or NULL (v305, appended): the time-blended motion bases of the S sub-samples (row k: transl 3,
                              6-D rotation 6, 7 pad floats), written by d4gs_project_fwd when G > 0 and read by d4gs_project_bwd with
                              scalar loads.  NULL: d4gs_project_bwd builds the table itself (one small launch more). */
  uint64_t *tile_masks;    /* [S*N] (v305, appended; needed with D4GS_EXACT_TILES only): bit (ty - y0) * 8 + (tx - x0) = tile (tx, ty) of the
                              instance's packed rectangle is binned; 0 = no mask, the whole rectangle is (rectangles wider or taller
                              than 8 tiles, single tiles, flag off) */
  float *compensations;    /* [S,N] (v305, appended) out with D4GS_ANTIALIASED (required then, NULL otherwise): the antialiasing
                              compensation of every instance, 0 where radii == 0 */
} D4gsProjOut;

typedef struct D4gsIsect {
  int64_t n_isect;         /* [host] CAPACITY of the four lists below (elements), >= D4gsProjOut.n_isect[0].  The host
                            * may size them from a guess: every kernel of d4gs_bin_sort / d4gs_raster_fwd compares the
                            * device-side count with this value and returns at once (outputs untouched) when it does
                            * not fit, so the caller reads D4gsProjOut.n_isect AFTER launching and re-launches with
                            * exact sizes in that case - no host sync sits between the projection and the rasterizer.
                            * d4gs_raster_bwd needs the exact count. */
  int64_t max_tile_count;  /* [host] upper bound of D4gsProjOut.n_isect[1], checked on the device like n_isect
                            * (<= 0: unknown, launch every sort class) */
  int64_t near_target;     /* [host] D4GS_LAZY_SORT: keys per tile list to aim the near part at (<= 0: 1024).  About twice the
                            * entries a tile is expected to consume before it saturates. */
  uint64_t *keys;          /* [n_isect] scratch: (depth bits << 32 | emission index) per tile slot */
  int32_t *gid_of_emit;    /* [n_isect] Gaussian id of each emission index */
  int32_t *sorted_gid;     /* [n_isect] per-tile depth-sorted Gaussian ids (flatten_ids) */
  int32_t *sorted_emit;    /* [n_isect] emission index of each sorted slot */
} D4gsIsect;

typedef struct D4gsRaster {
  const float *background; /* [D] or NULL (depth channel's background is 0) */
  float *render_colors;    /* [S,H,W,D+depth] */
  float *render_alphas;    /* [S,H,W] */
  int32_t *last_ids;       /* [S,H,W] index (into sorted_gid) of the last composited splat */
  float *final_T;          /* [S,H,W] transmittance left behind the last splat.  The backward starts from this instead
                              of 1 - render_alphas (as gsplat does): for nearly opaque pixels (T ~ 1e-4) the fp32
                              subtraction loses ~3 digits, which shows up as a ~5e-4 relative bias of the gradients. */
  float *seg_state;        /* [D4gsSizes.seg_state] scratch or NULL.  Few-tile launches (S * tiles <= 1280: one or two exposure
                              sub-samples of a 288x512 frame, i.e. a rank of BASELINE config 4) cannot fill 256 CUs with one
                              workgroup per tile; given this buffer, d4gs_raster_fwd also stores every pixel's transmittance and
                              accumulated channels at up to 7 depth-segment boundaries of its tile list (+ the final ones) and
                              d4gs_raster_bwd replays the segments in parallel workgroups, each starting from the stored state.
                              Same image bit for bit; gradients equal to the unsegmented replay up to fp32 rounding of the
                              hand-off (deterministic).  NULL, or a configuration whose seg_state size is 0: one workgroup per
                              tile as before.  The SAME value must be passed to the forward and its backward. */
} D4gsRaster;

/* gradients w.r.t. the raster stage's per-instance inputs */
typedef struct D4gsRasterGrads {
  const float *v_render_colors; /* [S,H,W,D+depth] */
  const float *v_render_alphas; /* [S,H,W] or NULL */
  float *isect_grad;            /* [n_isect, 6+D+depth] scratch, 16-byte aligned: the row of every intersection that was
                                   replayed (at or before its tile's last contributor); the other rows are NOT written */
  uint8_t *isect_live;          /* [n_isect rounded up to a multiple of 4] scratch, 4-byte aligned: 1 = the row above was
                                   written by this call, 0 = skip it */
  float *v_means2d;             /* [S,N,2]  (= means2d.grad contract, trainer.py:975) */
  float *v_conics;              /* [S,N,3] */
  float *v_depths;              /* [S,N]   (zeros when depth_mode == 0) */
  float *v_opac_act;            /* [N]     summed over S */
  float *v_ctab;                /* [N,DP]  summed over S; 16-byte aligned (d4gs_project_bwd reads it as 16-byte words) */
  /* SURVEY 8f-1, fused: when stats_grad_norm_acc != NULL the gather epilogue also does the accumulation loop of
   * Trainer._prepare_control_step (flow3d/trainer.py:967-989) for this render - per visible instance (radii > 0), in
   * sub-sample order: grad_norm_acc[g] += |v_means2d * (W/2, H/2) * stats_batch_size * S|, vis_count[g] += 1, and, only
   * if stats_update_max_radii (the reference's index_put result is discarded, so upstream never updates it),
   * max_radii[g] = max(max_radii[g], radius / max(W, H)).  Same arithmetic and order as d4gs_control_stats. */
  float *stats_grad_norm_acc;   /* [N] or NULL */
  int64_t *stats_vis_count;     /* [N] */
  float *stats_max_radii;       /* [N] */
  int32_t stats_batch_size;
  int32_t stats_update_max_radii;
  int32_t row_mode;             /* D4GS_ROWS_*: AUTO picks dense / sparse rows from the list capacity per instance */
  float *v_means2d_abs;         /* [S,N,2] (v305, appended) out with D4GS_ABSGRAD (required then, NULL otherwise): the absgrad contract */
  int32_t stats_absgrad;        /* (v305, appended) with D4GS_ABSGRAD only: the fused statistics accumulate |v_means2d_abs * (W/2, H/2) *
                                   stats_batch_size * S| instead (same arithmetic and order) */
} D4gsRasterGrads;

/* leaf gradients produced by d4gs_project_bwd (all overwritten, not accumulated) */
typedef struct D4gsLeafGrads {
  float *v_means, *v_quats, *v_scales, *v_opacities, *v_colors; /* [N,3] [N,4] [N,3] [N] [N,D] */
  float *v_motion_coefs; /* [G,K] or NULL */
  float *v_rots;         /* [K,T,6] or NULL */
  float *v_transls;      /* [K,T,3] or NULL */
  float *v_times;        /* [S] or NULL */
  float *v_RTs;          /* [S,3,4] or NULL */
  float *v_viewmat;      /* [4,4] or NULL (test-time pose optimisation, validator.py:437-452) */
  float *partials;       /* [d4gs_bwd_partials_elems(dims)] scratch for the deterministic 2-level reduction */
} D4gsLeafGrads;

D4GS_API int d4gs_version(void);
/* optional per-kernel HIP-event timing (bench.py's roofline object): enable, run, then collect
 * "kernel_name launches total_ms" lines.  on = 1 times every kernel (two stream events per launch: ~0.12 ms per
 * cfg2 frame), on = 2 only the rasterization kernels (k_raster*), on = 3 only the composite backward (k_raster_bwd*: what bench.py's
 * roofline object needs from its timed region), 0 = off (default; no
 * events are created). */
D4GS_API void d4gs_profile_enable(int on);
D4GS_API int d4gs_profile_collect(char *buf /* [host] */, size_t cap);
D4GS_API const char *d4gs_last_error(void);
/* The two MEASURED device ceilings bench.py quotes its roofline fractions against: a device-to-device stream copy over
 * `scratch` (first half -> second half, best of 8) and an FMA issue loop at 8 waves per SIMD.  out[0] = copy GB/s (read + write),
 * out[1] = fp32 TFLOP/s with v_pk_fma_f32, out[2] = fp32 TFLOP/s with v_fma_f32 (what the composite kernels issue), out[3] = bytes
 * copied per launch.  Diagnostic: creates its own HIP events and WAITS for them - not for timed regions or stream captures. */
D4GS_API int d4gs_measure_peaks(void *scratch /* device, >= 64 MiB */, size_t scratch_bytes, double *out /* [host] [4] */, void *stream);
/* D4gsProjOut.n_isect -> PINNED (device-addressable: hipHostMalloc / torch pin_memory) host memory, by a one-wave kernel on `stream`
 * that stores the four counts there (a kernel node when the stream is being captured - how a step replayed from a HIP graph keeps
 * reporting its list sizes: engine.GraphWatch; a device-to-host copy node would hold up the kernels behind it).  Read the buffer after
 * an event recorded behind this call has completed.  (Pageable memory is accepted too: it gets an ordinary device-to-host copy.) */
D4GS_API int d4gs_copy_counts(const int64_t *n_isect /* device [4] */, int64_t *host_pinned /* [4] */, void *stream);
D4GS_API size_t d4gs_scan_ws_elems(int64_t n_instances);
D4GS_API size_t d4gs_bwd_partials_elems(const D4gsDims *dims);

/* Element counts of every caller-allocated buffer for one configuration (the "workspace query" of SURVEY 8b): the
 * per-instance / per-tile buffers of D4gsProjOut, the image buffers of D4gsRaster, and - per intersection, to be
 * multiplied by the list capacity the caller chooses (see D4gsIsect.n_isect) - the rows of D4gsIsect and of
 * D4gsRasterGrads.isect_grad.  Element types are the ones of the struct fields. */
typedef struct {
  int64_t means2d, depths, conics, radii, opac_act, ctab, geom, tile_rects, tiles_touched, isect_offsets;
  int64_t tile_counts, tile_offsets, n_isect, scan_ws;          /* D4gsProjOut */
  int64_t render_colors, render_alphas, last_ids, final_T;       /* D4gsRaster (seg_state: last field of this struct) */
  int64_t isect_grad_row;                                        /* floats per intersection in isect_grad (isect_live: 1 byte) */
  int64_t bwd_partials;                                          /* D4gsLeafGrads.partials */
  int64_t seg_state;                                             /* D4gsRaster.seg_state; 0 = this configuration does not use depth segments */
  int64_t lazy_ws;                                               /* D4gsProjOut.lazy_ws (int32 elements; needed with D4GS_LAZY_SORT only) */
  int32_t tiles_x, tiles_y, channels;                            /* tile grid; D + depth channel */
  int64_t blend_bases;                                           /* D4gsProjOut.blend_bases (v305, appended; 0 when G == 0) */
  int64_t tile_masks;                                            /* D4gsProjOut.tile_masks (uint64 elements; needed with D4GS_EXACT_TILES) */
  int64_t compensations;                                         /* D4gsProjOut.compensations (v305, appended): S*N with D4GS_ANTIALIASED, else 0 */
} D4gsSizes;
D4GS_API int d4gs_query_sizes(const D4gsDims *dims, D4gsSizes *sizes);

/* a1-a6 + projection + tile counting + scans.  Replaces params.py:39-43,142-180, transforms.py:41-53,
 * scene_model.py:67-120,352-353 and gsplat fully_fused_projection_fwd + isect_tiles pass 1 for all S. */
D4GS_API int d4gs_project_fwd(const D4gsDims *dims, const D4gsProjIn *in, const D4gsProjOut *out, void *stream);

/* isect_tiles pass 2 + per-tile depth sort (replaces gsplat isect_tiles / radix sort / isect_offset_encode). */
D4GS_API int d4gs_bin_sort(const D4gsDims *dims, const D4gsProjOut *proj, const D4gsIsect *isect, void *stream);

/* rasterize_to_pixels_fwd for all S sub-samples (+ expected-depth normalisation when depth_mode == ED). */
D4GS_API int d4gs_raster_fwd(const D4gsDims *dims, const D4gsProjOut *proj, const D4gsIsect *isect, const D4gsRaster *r,
                    void *stream);

/* rasterize_to_pixels_bwd + per-instance gather of the per-intersection gradients (deterministic, no float atomics). */
D4GS_API int d4gs_raster_bwd(const D4gsDims *dims, const D4gsProjOut *proj, const D4gsIsect *isect, const D4gsRaster *r,
                    const D4gsRasterGrads *g, void *stream);

/* fully_fused_projection_bwd + deformation / activation adjoints for all S, reduced to leaf gradients. */
D4GS_API int d4gs_project_bwd(const D4gsDims *dims, const D4gsProjIn *in, const D4gsProjOut *proj,
                     const float *v_means2d, const float *v_conics, const float *v_depths, const float *v_opac_act,
                     const float *v_ctab, const D4gsLeafGrads *grads, void *stream);

/* a11 track channels (scene_model.py:258-289): camera-space position of every Gaussian at S target times,
 * points[s,g] = RTs[s] * deform(g, times[s]) (then viewmat, normally identity).  Uses dims N/G/K/T/S and
 * in->means, motion_coefs, rots, transls, times (= target_ts), RTs (= target_w2cs[:, :3, :], may be NULL), viewmat,
 * Kmat; every other input may be NULL.  The backward fills v_means, v_motion_coefs, v_rots, v_transls, v_times,
 * v_RTs, v_viewmat of D4gsLeafGrads (the other leaf pointers are not touched). */
D4GS_API int d4gs_points_fwd(const D4gsDims *dims, const D4gsProjIn *in, float *points /* [S,N,3] */, void *stream);
D4GS_API int d4gs_points_bwd(const D4gsDims *dims, const D4gsProjIn *in, const float *v_points /* [S,N,3] */,
                    const D4gsLeafGrads *grads, void *stream);

/* a4/a5 pose API of the S2 seam (flow3d/scene_model.py:58-120; called by the reference's Trainer at
 * flow3d/trainer.py:303,478,485,701,818 and its Renderer at flow3d/renderer.py:37): for the S = B times in in->times
 *   transforms[g,b] = [cont_6d_to_rmat(r6) | transl] of the time-blended, coefficient-weighted bases   (G dynamic rows)
 *   means[g,b]      = R means_g + transl                          (static rows g >= G: means_g)
 *   quats[g,b]      = normalize( wxyz( rotmat_to_unitquat(R)_xyzw (x) xyzw(normalize(quats_g)) ) )   (static: normalize)
 * Uses dims N/G/K/T/S and in->means, quats (only when `quats` is requested), motion_coefs, rots, transls, times; in->RTs
 * [S,3,4] and in->viewmat (both optional, NULL = identity) are applied to the MEANS only - that is d4gs_points_fwd, the
 * a11 track channels.  Any of the three outputs may be NULL.  g_major selects the layout: 0 = time-major [S,N,...]
 * ([S,G,3,4] for transforms), 1 = the reference's Gaussian-major (G,B,...) tensors.
 * d4gs_poses_bwd takes the three gradients in the same struct (NULL = zero) and fills v_means, v_quats (if quats'
 * gradient was given and v_quats != NULL), v_motion_coefs, v_rots, v_transls, v_times, v_RTs of D4gsLeafGrads. */
typedef struct D4gsPoses {
  float *means;       /* [S,N,3] | [N,S,3] */
  float *quats;       /* [S,N,4] | [N,S,4]  wxyz, unit */
  float *transforms;  /* [S,G,3,4] | [G,S,3,4] */
  int32_t g_major;
} D4gsPoses;
D4GS_API int d4gs_poses_fwd(const D4gsDims *dims, const D4gsProjIn *in, const D4gsPoses *out, void *stream);
D4GS_API int d4gs_poses_bwd(const D4gsDims *dims, const D4gsProjIn *in, const D4gsPoses *v_out, const D4gsLeafGrads *grads,
                   void *stream);

/* Densification statistics, Trainer._prepare_control_step (flow3d/trainer.py:953-990) for one render of
 * S sub-samples: for every visible instance (radii > 0)
 *   grad_norm_acc[g] += || xys_grad[s,g] * (W/2, H/2) * batch_size * S ||,  vis_count[g] += 1,
 *   max_radii[g] = max(max_radii[g], radii[s,g] / max(W, H))  -- ONLY when update_max_radii != 0: the reference
 *   computes this maximum and then drops it (out-of-place `index_put`, trainer.py:987-989), so its `max_radii`
 *   stays at its initial value; 0 reproduces that.   Running stats are updated in place. */
D4GS_API int d4gs_control_stats(int32_t S, int32_t N, const float *xys_grad /* [S,N,2] */, const int32_t *radii /* [S,N] */,
                       int32_t width, int32_t height, int32_t batch_size, float *grad_norm_acc /* [N] */,
                       int64_t *vis_count /* [N] */, float *max_radii /* [N] */, int32_t update_max_radii,
                       void *stream);

/* SURVEY 8f-1, control steps: the row surgery of GaussianParams.densify_params / cull_params (flow3d/params.py:86-118)
 * and of dup_in_optim / remove_from_optim (flow3d/trainer.py:1199-1236) as stream compaction.
 * d4gs_control_plan: flags [N] (uint8) -> src_map (capacity 3N for a densify plan, N for a cull plan) in the reference's
 * row order - rows with split == 0, then rows with dup != 0, then the rows with split != 0 TWICE (x[split].repeat(2));
 * with dup == NULL the first flag array is a cull mask and the plan keeps the rows whose flag is 0.
 * counts [4] (device) = {n_keep, n_dup, n_split, n_out}.  d4gs_gather_rows: out[i,:] = in[src_map[i],:] for one tensor
 * of `row_floats` 32-bit words per row; rows >= zero_from are zero-filled (new Adam moments: zero_from = n_keep), rows
 * >= add_from get `add` added (split halves of `scales`: add_from = n_keep + n_dup, add = -log 1.6); pass INT64_MAX
 * to disable either. */
D4GS_API int d4gs_control_plan(int32_t N, const uint8_t *split_or_cull, const uint8_t *dup, int32_t *src_map, int32_t *counts,
                      void *stream);
D4GS_API int d4gs_gather_rows(const int32_t *src_map, int64_t n_out, int32_t row_floats, const float *in, float *out,
                     int64_t zero_from, int64_t add_from, float add, void *stream);

/* a12 camera path: the generator of `RTs [S,3,4]` / `times [S]` that feed d4gs_project_fwd.
 * Replaces the eager chain of MoveModel.forward_start_end_mid (flow3d/models/move_model.py:138-166):
 *   pypose se3.Exp(delta0/1) -> linear_interpolation (flow3d/models/utils/spline_utils.py:371-408) -> SE3.Log ->
 *   se3_to_SE3 (spline_utils.py:197-215, with the [tau,phi]-read-as-[w,u] convention of move_model.py:146-147), and
 *   the exposure-time lerp of move_model.py:118-135,151-158 (half-width clamp(relu(time_params[index]),0.1,0.9) on
 *   interior frames 0 < index < n_time_params-1, else 0; pass time_params = NULL for stage "first").
 * delta0/delta1 [6] are the two MLP head outputs.  jac [S,12,12] = d RTs[s,i] / d (delta0|delta1)[j] (NULL to skip),
 * dtimes [S] = d times / d time_params[index], deltaT [2] = {|half-width|, its derivative}.  The backward is the
 * mat-vec v_delta = v_RTs . jac plus the time_params row (v_* inputs may be NULL = zero). */
D4GS_API int d4gs_camera_path_fwd(const float *delta0, const float *delta1, int32_t S, const float *time_params,
                         int32_t n_time_params, int32_t index, float t, float *RTs /* [S,3,4] */,
                         float *jac /* [S,12,12] */, float *times /* [S] */, float *dtimes /* [S] */,
                         float *deltaT /* [2] */, void *stream);
D4GS_API int d4gs_camera_path_bwd(const float *jac, const float *dtimes, const float *deltaT, const float *v_RTs,
                         const float *v_times, const float *v_deltaT, int32_t S, int32_t index,
                         int32_t n_time_params, float *v_delta0 /* [6] */, float *v_delta1 /* [6] */,
                         float *v_time_params /* [n_time_params] */, void *stream);
/* MoveModel.preprocessPose + positional embedding (move_model.py:12-63,104-110; spline_utils.py:177-195):
 * R [3,3] with row stride r_stride (4 for the top-left block of a [4,4] w2c), T [3] with element stride t_stride
 * -> enc [66] = [x, sin(x f), cos(x f)]_{f=1,2,4,8,16}, x = SE3_to_se3([R|T]). */
D4GS_API int d4gs_pose_encode(const float *R, int32_t r_stride, const float *T, int32_t t_stride, float *enc /* [66] */,
                     void *stream);
/* Its input gradient (test-time pose refinement differentiates the render w.r.t. w2c, which also feeds the
 * MoveModel: flow3d/validator.py:442-448 -> flow3d/scene_model.py:249-256): v_enc [66] -> v_R [3,3] dense, v_T [3]. */
D4GS_API int d4gs_pose_encode_bwd(const float *R, int32_t r_stride, const float *T, int32_t t_stride, const float *v_enc,
                         float *v_R /* [9] */, float *v_T /* [3] */, void *stream);

/* The whole MoveModel (move_model.py:66-166) for one pose, one call each way: d4gs_pose_encode -> the 9-layer MLP
 * (66 -> 64 x4 LeakyReLU(0.01) -> 64, heads 64 -> 64 -> 6; ~30 GEMV launches per render in eager PyTorch) ->
 * d4gs_camera_path_fwd.  Layer order in w[] / b[]: RT_main.0, .2, .4, .6, .8, RT_head0.0, .2, RT_head1.0, .2;
 * weights are [out,in] row-major as nn.Linear stores them. */
typedef struct {
  const float *w[9];
  const float *b[9];
  const float *time_params; /* [n_time_params] or NULL */
  int32_t n_time_params;
} D4gsMoveModelParams;
typedef struct {
  float *enc;    /* [66]  scratch */
  float *acts;   /* [514] saved layer inputs (backward) */
  float *delta;  /* [12]  the two head outputs */
  float *RTs;    /* [S,3,4] */
  float *jac;    /* [S,12,12] */
  float *times;  /* [S] */
  float *dtimes; /* [S] */
  float *deltaT; /* [2] */
} D4gsMoveModelOut;
typedef struct {
  float *v_w[9];
  float *v_b[9];
  float *v_time_params; /* [n_time_params] */
  float *v_delta;       /* [12] scratch */
  float *v_enc;         /* [66] gradient of the pose encoding (input of d4gs_pose_encode_bwd), or NULL to skip */
} D4gsMoveModelGrads;
D4GS_API int d4gs_move_model_fwd(const float *R, int32_t r_stride, const float *T, int32_t t_stride, const D4gsMoveModelParams *p,
                        int32_t S, int32_t index, float t, int32_t stage_first, const D4gsMoveModelOut *out, void *stream);
D4GS_API int d4gs_move_model_bwd(const D4gsMoveModelParams *p, const D4gsMoveModelOut *out, const float *v_RTs,
                        const float *v_times, const float *v_deltaT, int32_t S, int32_t index,
                        const D4gsMoveModelGrads *grads, void *stream);

/* the photometric loss term, fused (flow3d/trainer.py:388-392,575-586):
 *   loss = w_l1 * mean|pred*m - gt*m| + w_ssim * (1 - SSIM(pred*m, gt*m)),
 * SSIM = pytorch_msssim.SSIM(data_range=1, size_average=True, channel=3) [11-tap sigma-1.5 window, no padding].
 * pred, gt [B,H,W,3] channel-last; mask [B,H,W] or NULL.  Forward: loss[3] = {loss, l1, ssim} (device), plus what the
 * backward needs: maps [d4gs_photometric_maps_elems(B,H,W)] floats (five per output pixel and channel, [B,H-10,W-10,3,5]: it was
 * three before the variances were taken about a local offset; callers size it with the query, never by hand) and partials
 * [d4gs_photometric_blocks(B,H,W), 2] scratch.  Backward: v_pred [B,H,W,3] = dL/dpred * v_loss[0] (v_loss is a device scalar). */
D4GS_API int64_t d4gs_photometric_blocks(int32_t B, int32_t H, int32_t W);
D4GS_API int64_t d4gs_photometric_maps_elems(int32_t B, int32_t H, int32_t W); /* 0 if H or W < 11 */
D4GS_API int d4gs_photometric_fwd(const float *pred, const float *gt, const float *mask, int32_t B, int32_t H, int32_t W, int32_t C,
                         float w_l1, float w_ssim, float *maps, float *partials, float *loss, void *stream);
D4GS_API int d4gs_photometric_bwd(const float *pred, const float *gt, const float *mask, const float *maps, const float *v_loss,
                         int32_t B, int32_t H, int32_t W, int32_t C, float w_l1, float w_ssim, float *v_pred,
                         void *stream);

/* Spherical-harmonic colours (seam S1's `sh_degree`, gsplat 1.1.1 `spherical_harmonics` + its `rasterization` epilogue).
 * Per Gaussian n, with dir = p[n] - origin (dir = p[n] when origin is NULL) and d = dir / |dir|:
 *   raw[c] = sum_{k < (degree+1)^2} Y_k(d) coeffs[n,k,c],   rgb[n,c] = clamp ? max(raw[c] + 0.5, 0) : raw[c].
 * Y_k is the real SH basis (degree 0..4) in the Inria / gsplat order and sign convention, e.g. Y_0 = 0.2820948,
 * Y_1 = -0.4886025 y, Y_2 = 0.4886025 z, Y_3 = -0.4886025 x, ... (the full table: csrc/sh.hip).
 * p [N,3], origin [3] or NULL, coeffs [N,K,3] with K >= (degree+1)^2 (coefficients k >= (degree+1)^2 are ignored),
 * mask [N] (uint8 / bool, 0 = masked) or NULL, rgb [N,3].
 * A masked Gaussian, and one with |dir| == 0 (on the camera centre: the near plane culls it), has raw = 0 and zero
 * gradients (gsplat would produce NaN for the latter).
 * Backward, from v_rgb [N,3] (the clamp's pass-through, raw + 0.5 >= 0, is recomputed from coeffs):
 *   v_coeffs [N,K,3] or NULL: Y_k(d) v_rgb[n,:] below (degree+1)^2, exact zeros above and for masked Gaussians;
 *   v_p [N,3] or NULL: dL/dp;  v_origin [3] or NULL: -sum_n dL/dp[n], summed in a fixed order (bitwise reproducible)
 *   through partials [d4gs_sh_partials_elems(N)] scratch; needs origin.
 * N == 0 launches nothing.  D4GS_EINVAL for N < 0, degree outside 0..4, K < (degree+1)^2 or a NULL required buffer. */
D4GS_API int64_t d4gs_sh_partials_elems(int64_t N);
D4GS_API int d4gs_sh_fwd(int64_t N, int32_t K, int32_t degree, const float *p, const float *origin, const float *coeffs,
                         const uint8_t *mask, int32_t clamp, float *rgb, void *stream);
D4GS_API int d4gs_sh_bwd(int64_t N, int32_t K, int32_t degree, const float *p, const float *origin, const float *coeffs,
                         const uint8_t *mask, int32_t clamp, const float *v_rgb, float *v_coeffs, float *v_p,
                         float *v_origin, float *partials, void *stream);

/* a9 exposure blend (scene_model.py:386-397): out = mean_S; policy[c] 1 -> max over {raw_0..raw_{S-2}, mean},
 * 2 -> min over the same set (the reference's in-place quirk); acc = mean_S alphas. */
D4GS_API int d4gs_blend_fwd(int32_t S, int64_t n_pixels, int32_t C, const int32_t *policy /* [host] [C] */,
                   const float *renders /* [S,P,C] */, const float *alphas /* [S,P] */, float *out /* [P,C] */,
                   float *acc /* [P] */, void *stream);
D4GS_API int d4gs_blend_bwd(int32_t S, int64_t n_pixels, int32_t C, const int32_t *policy /* [host] */, const float *renders,
                   const float *out, const float *v_out, const float *v_acc, float *v_renders /* [S,P,C] */,
                   float *v_alphas /* [S,P] */, void *stream);

/* One call each way: d4gs_forward = d4gs_project_fwd + d4gs_bin_sort + d4gs_raster_fwd (+ d4gs_blend_fwd when
 * io->blended != NULL), d4gs_backward = (d4gs_blend_bwd +) d4gs_raster_bwd + d4gs_project_bwd.  Same kernels, same order:
 * bit-identical to the staged calls.  Every buffer that only lives between / inside the two calls sits in ONE caller-provided
 * workspace (256-byte aligned, d4gs_frame_workspace_bytes(dims, isect_capacity) bytes; the forward's part of it must reach the
 * backward untouched); what the caller reads is in D4gsFrameIO.  `isect_capacity` / `max_tile_hint` are D4gsIsect.n_isect /
 * .max_tile_count: a guess the kernels check on the device - read io->n_isect afterwards and call again if it did not fit.
 * The backward takes any of v_blended, v_acc, v_renders, v_alphas when io->blended was given (losses on the blurry frame and
 * on the per-sub-sample images, flow3d/trainer.py:575-618), else v_renders [+ v_alphas]; a caller that needs `means2d` as an
 * autograd intermediate or renders more than 16 colour channels uses the staged entry points. */
#define D4GS_FRAME_BLEND_MAX_S 129
typedef struct D4gsFrameIO {
  float *blended;          /* [H,W,D+depth] or NULL: no blend.  With it, S <= D4GS_FRAME_BLEND_MAX_S (else D4GS_EINVAL): the one-call path
                              keeps the max / min channels' winning sub-sample as one signed byte per pixel and channel (0 .. 127; -1 =
                              the mean), and the candidates are the sub-samples 0 .. S - 2.  More sub-samples: the staged entry points
                              (d4gs_blend_bwd searches the renders for the winner and has no such limit). */
  float *acc;              /* [H,W] (with blended) */
  float *renders;          /* [S,H,W,D+depth] */
  float *alphas;           /* [S,H,W] */
  float *means2d;          /* [S,N,2] */
  int32_t *radii;          /* [S,N] */
  int64_t *n_isect;        /* [4] device: {intersections, longest tile list, sampled entries, sampled live entries} (D4gsProjOut.n_isect) */
  const float *background; /* [D] or NULL */
  const int32_t *policy;   /* [host] [D+depth] blend policy per channel (0 mean, 1 max, 2 min) or NULL = all mean */
  int64_t near_target;     /* [host] D4GS_LAZY_SORT: D4gsIsect.near_target of the frame (<= 0: 1024) */
  int64_t *counts_pinned;  /* [PINNED host memory, device-addressable] [4] or NULL (v305, appended): d4gs_forward also leaves the four
                              counts of n_isect there - stored by its LAST kernel (the blend, when io->blended is given: no extra
                              launch; otherwise one one-wave kernel), i.e. what d4gs_copy_counts would do in a launch of its own.
                              Read it after an event recorded behind d4gs_forward has completed. */
} D4gsFrameIO;
typedef struct D4gsFrameGrads {
  const float *v_blended, *v_acc;     /* [H,W,D+depth], [H,W] or NULL */
  const float *v_renders, *v_alphas;  /* [S,H,W,D+depth], [S,H,W] or NULL */
  float *v_means2d;                   /* [S,N,2] out: the means2d.grad contract (trainer.py:975) */
  float *stats_grad_norm_acc;         /* fused densification statistics, as in D4gsRasterGrads; NULL = off */
  int64_t *stats_vis_count;
  float *stats_max_radii;
  int32_t stats_batch_size, stats_update_max_radii, row_mode;
  float *v_means2d_abs;               /* [S,N,2] out (v305, appended): as in D4gsRasterGrads, with D4GS_ABSGRAD */
  int32_t stats_absgrad;              /* (v305, appended) as in D4gsRasterGrads */
} D4gsFrameGrads;
D4GS_API size_t d4gs_frame_workspace_bytes(const D4gsDims *dims, int64_t isect_capacity);
/* The prefix of that workspace d4gs_forward alone touches (everything but the backward's scratch: image-gradient stack, per-
 * intersection gradient rows, per-instance gradients, block partials - roughly half): a forward that will never be followed by
 * d4gs_backward (validation, viewer) may pass a workspace of this size. */
D4GS_API size_t d4gs_frame_workspace_bytes_fwd(const D4gsDims *dims, int64_t isect_capacity);
D4GS_API int d4gs_forward(const D4gsDims *dims, const D4gsProjIn *in, const D4gsFrameIO *io, void *workspace, size_t ws_bytes,
                 int64_t isect_capacity, int64_t max_tile_hint, void *stream);
D4GS_API int d4gs_backward(const D4gsDims *dims, const D4gsProjIn *in, const D4gsFrameIO *io, const D4gsFrameGrads *g,
                  const D4gsLeafGrads *leaf /* .partials is ignored: it lives in the workspace */, void *workspace,
                  size_t ws_bytes, int64_t isect_capacity, int64_t max_tile_hint, void *stream);

/* CPU twins of the two calls above (BASELINE config 1, the CPU-runnable plumbing case): the same arithmetic rules
 * and the same structs with every pointer a HOST pointer; no stream, no workspace (scratch is allocated and freed inside; the
 * backward re-runs the forward), io->n_isect [4] host.  Scalar fp32, one thread - a separate entry point for hosts without a
 * GPU, never a fallback: d4gs_forward and the Python seams still refuse CPU tensors.  csrc/cpu_twin.hip. */
D4GS_API int d4gs_forward_cpu(const D4gsDims *dims, const D4gsProjIn *in, const D4gsFrameIO *io);
D4GS_API int d4gs_backward_cpu(const D4gsDims *dims, const D4gsProjIn *in, const D4gsFrameIO *io, const D4gsFrameGrads *g,
                      const D4gsLeafGrads *leaf);

/* Exposure sharding (one process per GPU): the same blend when this process holds only the sub-samples
 * s_first + j * s_stride, j < S_local, of the S_total.  Collectives stay with the caller (RCCL through torch.distributed):
 *   forward : partial_fwd -> all-reduce SUM of part [P,C+1] (colours + alpha) and MAX of cand [P,npol] (the max / min
 *             policy channels in ascending channel order, min packed as -x; -inf where this rank has no candidate) -> finish_fwd;
 *   backward: winner (lowest own s <= S_total-2 whose raw value equals the blended one, else S_total) -> all-reduce MIN ->
 *             bwd.  The mean channels need no collective backward (the loss is evaluated on every rank).
 * Equals d4gs_blend_fwd/bwd on the full stack up to the order of the S-term sums. */
typedef struct D4gsShardBlend {
  int32_t S_total, S_local, s_first, s_stride, C;
  int64_t n_pixels;
  const int32_t *policy; /* [host] [C] */
} D4gsShardBlend;
D4GS_API int d4gs_blend_shard_partial_fwd(const D4gsShardBlend *b, const float *renders /* [S_local,P,C] */,
                                 const float *alphas /* [S_local,P] */, float *part /* [P,C+1] */, float *cand /* [P,npol] */,
                                 void *stream);
D4GS_API int d4gs_blend_shard_finish_fwd(const D4gsShardBlend *b, const float *part, const float *cand, float *out /* [P,C] */,
                                float *acc /* [P] */, void *stream);
D4GS_API int d4gs_blend_shard_winner(const D4gsShardBlend *b, const float *renders, const float *out, int32_t *win /* [P,npol] */,
                            void *stream);
D4GS_API int d4gs_blend_shard_bwd(const D4gsShardBlend *b, const float *v_out, const float *v_acc /* or NULL */, const int32_t *win,
                         float *v_renders /* [S_local,P,C] */, float *v_alphas /* [S_local,P] */, void *stream);

/* Multi-tensor Adam (appended; D4GS_VERSION unchanged): ONE launch updates every tensor of a table that lives in DEVICE memory,
 * so a launch captured in a HIP graph stays valid when the host refreshes an lr (or any other field) in the table between replays.
 * torch.optim.Adam with default flags (no amsgrad, no weight decay, no maximize), fp32 tensors, per record with t = step + 1:
 *   m += (g - m) (1 - beta1);  v = beta2 v + (1 - beta2) g g;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * The four scalars are doubles, as torch holds them: 1 - beta1, 1 - beta2 and the two bias corrections are formed in fp64 (on the
 * device, once per workgroup) and rounded to fp32 once; every per-element operation is one correctly rounded fp32 operation, with
 * no contraction, in the order torch's single-tensor path applies them.
 * A record whose `grad` is NULL is skipped: nothing of it is written and its step does not advance (torch skips `grad is None`).
 * Workgroup b of the launch serves chunk (b - block_prefix[r]) - D4GS_ADAM_CHUNK elements - of the record r with
 * block_prefix[r] <= b < block_prefix[r + 1]; a record has d4gs_adam_blocks(n) = max(1, ceil(n / D4GS_ADAM_CHUNK)) workgroups,
 * so block_prefix [n_records + 1] is the running sum of those counts and n_blocks = block_prefix[n_records].  16-byte loads and
 * stores when the four bases of a record are 16-byte aligned (the n % 4 tail as dwords), dwords otherwise.  No atomics and no
 * cross-workgroup traffic: bitwise reproducible.  That is also why the step count is kept once per WORKGROUP: block_steps
 * [n_blocks] (float, like torch's `step`) holds each workgroup's own copy of its record's count - it reads, increments and
 * writes back only that word, and chunk 0 also stores the new count to `*step` for the host to see.  Whoever builds the table
 * seeds block_steps[b] with the `*step` of b's record (and seeds it again after changing `*step` from outside). */
#define D4GS_ADAM_CHUNK 2048
typedef struct D4gsAdamRec {
  float *param;              /* [n] */
  const float *grad;         /* [n] or NULL: the record is skipped */
  float *exp_avg;            /* [n] m */
  float *exp_avg_sq;         /* [n] v */
  float *step;               /* [1] the step count torch keeps in state["step"] (fp32) */
  int64_t n;
  double lr, beta1, beta2, eps;
} D4gsAdamRec;
D4GS_API int64_t d4gs_adam_blocks(int64_t n);
/* table [n_records], block_prefix [n_records + 1] and block_steps [n_blocks]: device memory (table 8-byte, the others 4-byte
 * aligned).  n_records == 0 launches nothing.  D4GS_EINVAL for a NULL or misaligned argument or a negative count; what the
 * records hold cannot be checked from the host - the kernel itself never touches an element at or beyond `n`. */
D4GS_API int d4gs_adam_step(const D4gsAdamRec *table /* [device] */, int32_t n_records, const int32_t *block_prefix,
                            int32_t n_blocks, float *block_steps, void *stream);
/* table[r].grad = grads[r] for r < n_records, by kernels that carry the pointers as ARGUMENTS (64 per launch): the one way to
 * point a device table at gradient tensors that were born inside a stream capture - a captured copy from host memory would be
 * read again at every replay.  grads [host] [n_records]. */
D4GS_API int d4gs_adam_set_grads(D4gsAdamRec *table /* [device] */, int32_t n_records, const float *const *grads /* [host] */,
                                 void *stream);
/* CPU twin: the same per-element function on HOST pointers (table and everything it points to), one thread, no stream, no block
 * tables (t = *step + 1).  Never a fallback.  Validates every record: D4GS_EINVAL for a NULL param / exp_avg / exp_avg_sq /
 * step, a pointer that is not 4-byte aligned, or n < 0. */
D4GS_API int d4gs_adam_step_cpu(const D4gsAdamRec *table, int32_t n_records);

/* Trimmed losses (appended; D4GS_VERSION unchanged): the reference's masked_l1_loss, trimmed_l1_loss and compute_gradient_loss
 * (flow3d/loss_utils.py:26-42,64-68,71-90) without a sort and without a host read, so a step that holds them can be captured in a
 * HIP graph.  Elements: v_i = mean over the last axis of |pred - gt|, i < n.  Threshold: t = torch.quantile(v, quantile) over all n
 * elements with linear interpolation, rank r = quantile * (n - 1) evaluated in fp32, t = lerp(v_(floor r), v_(ceil r), frac r); the
 * two order statistics are found exactly by a most-significant-digit radix select (4 histogram passes of 8 bits over the bit
 * patterns of v).  An element is kept when v_i < t (strictly: a tie group at t is dropped whole).
 *   masked (mask [n], any float weights): quantile >= 1 keeps every element and selects nothing;
 *       normalize != 0: sum_kept v_i m_i / (sum_kept m_i + 1e-8),  normalize == 0: sum_kept v_i m_i / #kept
 *   trimmed (no mask): sum_kept v_i / #kept; always selects (quantile >= 1 gives t = max v, as torch.quantile(v, 1) does)
 *   gradient (pred, gt, mask [B,H,W]): x term over |dx pred - dx gt| at horizontally adjacent pixels whose mask values are both
 *       non-zero, y term the same vertically; each term is `trimmed` over its own elements, whose COUNT is data: it is counted
 *       on the device and the rank is formed there.  loss = x term + y term.
 * An empty kept set is 0 / 0 = NaN for the mean forms (also a gradient term without a valid pair, where the reference raises: that
 * cannot be done without a host wait) and 0 for normalize != 0.  Non-finite inputs are out of scope (no out-of-bounds access).
 * pred, gt [n, D] (D >= 1) fp32 contiguous; 0 <= n, B H W <= 2^31 - 1.  scratch: d4gs_trimmed_scratch_words(n, 1) 32-bit words
 * (gradient: (B H W, 2)), 8-byte aligned; the forward leaves the elements in its first n (gradient: 2 B H W) words - the `values`
 * the backward wants - and writes out [8]: out[0] the loss, out[1] / out[3] the thresholds, out[2] / out[4] 1 / denominator per term
 * (and out[5] / out[6] each term's own loss).
 * Backward: v_pred = v_loss[0] * dL/dpred (v_loss: device scalar), sign(pred - gt) / D * m_i / denominator on kept elements and
 * zero elsewhere; the gradient form gathers per pixel from its at most four pairs (no atomics).  Nothing flows to gt or the mask.
 * Every sum has a fixed order and the histograms are integer: bitwise reproducible.  D4GS_EINVAL before any GPU call for a NULL
 * pointer, a negative or too large size, a quantile that is not finite or <= 0, or undersized / misaligned scratch. */
D4GS_API int64_t d4gs_trimmed_scratch_words(int64_t n_max, int32_t terms); /* terms: 1, or 2 for the gradient and track forms; 0: bad argument */
D4GS_API int d4gs_masked_l1_fwd(const float *pred, const float *gt, const float *mask, int64_t n, int32_t D, int32_t normalize,
                                float quantile, void *scratch, int64_t scratch_words, float *out, void *stream);
D4GS_API int d4gs_masked_l1_bwd(const float *pred, const float *gt, const float *mask, const float *values, const float *out,
                                const float *v_loss, int64_t n, int32_t D, float quantile, float *v_pred, void *stream);
D4GS_API int d4gs_trimmed_l1_fwd(const float *pred, const float *gt, int64_t n, int32_t D, float quantile, void *scratch,
                                 int64_t scratch_words, float *out, void *stream);
D4GS_API int d4gs_trimmed_l1_bwd(const float *pred, const float *gt, const float *values, const float *out, const float *v_loss,
                                 int64_t n, int32_t D, float *v_pred, void *stream);
D4GS_API int d4gs_gradient_loss_fwd(const float *pred, const float *gt, const float *mask, int32_t B, int32_t H, int32_t W,
                                    float quantile, void *scratch, int64_t scratch_words, float *out, void *stream);
D4GS_API int d4gs_gradient_loss_bwd(const float *pred, const float *gt, const float *mask, const float *values, const float *out,
                                    const float *v_loss, int32_t B, int32_t H, int32_t W, float *v_pred, void *stream);
/* The 2-D track loss and the mapped (track) depth loss of Trainer.compute_dynamic_losses (flow3d/trainer.py:633-667,681-689) in one
 * pass over n_elements elements e = (row r = b N + n over batch x target frames, query p), ordered as the reference concatenates
 * its targets.  Per element: pix[e] the query's flat pixel in [B,H,W] (n_pixels = B H W), rows[e] = r, visible[e] one byte, weights[e],
 * target_2d[e] = (u, v), target_depth[e] = d; Ks [n_rows,3,3] row-major.  A live element (visible != 0, 0 <= pix < n_pixels,
 * 0 <= rows < n_rows; nothing is read through an index outside these ranges) takes X = tracks_3d[pix, rows % N, 0:3] from the
 * channel-last [n_pixels, N, 3] image, P = K[r] X, z = max(P_z, 1e-6), (x, y) = P_xy / z, and gives
 *   term 0: 0.5 (|x - u| + |y - v|), kept when strictly below torch.quantile of the live term-0 elements (quantile >= 1: all kept)
 *   term 1: |1 / (z + 1e-5) - 1 / (d + 1e-5)|, always kept (the reference's default quantile of 1)
 * each term = sum_kept v w / (sum_kept w + 1e-8).  The live count is formed on the device.  No live element: term 0 is NaN when it
 * selects (the reference raises), term 1 is 0.  scratch: d4gs_trimmed_scratch_words(n_elements, 2); its first 2 n_elements words are
 * the `values` of the backward.  out [8]: out[1] / out[3] thresholds, out[2] / out[4] 1 / denominator, out[5] term 0, out[6] term 1
 * (out[0] their plain sum).  Backward: v_losses [2] (device) the two upstream gradients; v_tracks_3d [n_pixels, N, 3] is zeroed on
 * the stream, then every live element adds K^T dL/dP to its point with a float atomicAdd - queries of one row may share a pixel.
 * With distinct pixels per row every address receives one add onto zero: bitwise reproducible.  No gradient reaches P_z where the
 * clamp is active (x and y still divide by 1e-6 there).  D4GS_EINVAL before any GPU call for a NULL pointer, N < 1, n_rows not a
 * positive multiple of N, n_elements < 1, n_pixels < 1 (or either above 2^31 - 1), a bad quantile, undersized / misaligned scratch. */
D4GS_API int d4gs_track_losses_fwd(const float *tracks_3d, const int32_t *pix, const int32_t *rows, const uint8_t *visible,
                                   const float *weights, const float *target_2d, const float *target_depth, const float *Ks,
                                   int64_t n_pixels, int32_t N, int32_t n_rows, int64_t n_elements, float quantile, void *scratch,
                                   int64_t scratch_words, float *out, void *stream);
D4GS_API int d4gs_track_losses_bwd(const float *tracks_3d, const int32_t *pix, const int32_t *rows, const uint8_t *visible,
                                   const float *weights, const float *target_2d, const float *target_depth, const float *Ks,
                                   const float *values, const float *out, const float *v_losses, int64_t n_pixels, int32_t N,
                                   int32_t n_rows, int64_t n_elements, float quantile, float *v_tracks_3d, void *stream);

/* Motion and scale regularizers (appended; D4GS_VERSION unchanged): the four terms of Trainer.compute_dynamic_losses that look at no
 * image (flow3d/trainer.py:691-728, flow3d/loss_utils.py:118-157), one call forward and one backward.  Inputs, fp32 contiguous:
 * the foreground means [G,3], raw motion_coefs [G,K] (softmax is applied), raw scales [G,3] (penalised before exp, as the reference
 * does), rots [K,T,6], transls [K,T,3], ts [B] (frame units, any float), w2cs [B,4,4] = [A t; 0 0 0 1] with A any invertible 3x3.
 * With tc_b = clamp(ts_b, 1, T-2) and m_j[g,b] (j = 0, 1, 2) the deformed mean of Gaussian g at tc_b + (j - 1) (the deformation of
 * d4gs_poses_fwd), c_b = -A_b^-1 t_b the camera centre and d = (m_1 - c_b) / max(|m_1 - c_b|, 1e-12), out [4] (device) receives
 *   out[0] smooth_bases  = weight_rot * mean_{k, 1 <= tau <= T-2} |2 rots[k,tau] - rots[k,tau-1] - rots[k,tau+1]| + weight_transl * (the
 *                          same on transls)                                                   (the reference's weights: 1, 2)
 *   out[1] smooth_tracks = 0.5 * mean_{g,b} |2 m_1 - m_0 - m_2|
 *   out[2] z_accel       = mean_{g,b} ((m_1 - m_0) . d)^2 + mean_{g,b} ((m_2 - m_1) . d)^2
 *   out[3] scale_var     = mean_g sum_i (s_gi - mean_i s_gi)^2 / 2
 * The neighbour times and the camera centres are formed on the device: nothing is read on the host.  workspace:
 * d4gs_motion_regs_workspace_bytes(G, K, T, B) bytes (0: bad sizes), 16-byte aligned; the forward leaves the neighbour times, the
 * centres and the neighbour means [3B,G,3] in it, and the backward must be given the same, unmodified workspace.
 * Backward: v_out [4] (device) the four upstream gradients; fills v_means [G,3], v_motion_coefs [G,K], v_scales [G,3], v_rots [K,T,6]
 * and v_transls [K,T,3] of `grads` (overwritten; all five required, the other fields - .partials too - are ignored).  Nothing flows
 * to ts or w2cs.  The gradient of a norm that is exactly zero is zero (torch's convention): a static set of bases, or a basis row
 * that is the exact midpoint of its neighbours, gives 0 and not 0 / 0.  Every sum has a fixed order and every gradient address one
 * writer: forward and backward are bitwise reproducible.  A NaN in ts is not propagated: the clamp takes it to frame 1 (torch.clamp
 * would return NaN); non-finite inputs are otherwise out of scope (no out-of-bounds access follows from them).  D4GS_EINVAL, by host
 * arithmetic alone and before any HIP call, for a NULL pointer, G < 1, K outside 1..32, T < 3 (no interior frame: the reference's
 * mean over nothing is NaN), B < 1, 9 B G or 9 K T > 2^31 - 1, or an undersized or misaligned workspace.  The workspace size depends
 * on the four sizes only, not on the device. */
D4GS_API size_t d4gs_motion_regs_workspace_bytes(int32_t G, int32_t K, int32_t T, int32_t B);
D4GS_API int d4gs_motion_regs_fwd(const float *means, const float *motion_coefs, const float *scales, const float *rots,
                                  const float *transls, const float *ts, const float *w2cs, int32_t G, int32_t K, int32_t T, int32_t B,
                                  float weight_rot, float weight_transl, void *workspace, size_t workspace_bytes, float *out,
                                  void *stream);
D4GS_API int d4gs_motion_regs_bwd(const float *means, const float *motion_coefs, const float *scales, const float *rots,
                                  const float *transls, int32_t G, int32_t K, int32_t T, int32_t B, float weight_rot,
                                  float weight_transl, void *workspace, size_t workspace_bytes, const float *v_out,
                                  const D4gsLeafGrads *grads, void *stream);

/* Flow-aligned exposure consistency (appended; D4GS_VERSION unchanged): the pieces of the reference's AlignedLoss (flow3d/loss_utils.py,
 * flow3d/models/pwcnet.py) that are not convolutions.  Every tensor is fp32, contiguous, NCHW.
 *
 * Cost volume: out[b, (dy+4)*9 + (dx+4), y, x] = lrelu((1/C) * sum_c first[b,c,y,x] * second[b,c,y+dy,x+dx]), dx, dy in -4..4, second
 * zero outside the image; first, second [B,C,H,W], out [B,81,H,W].  lrelu(v) = v > 0 ? v : negative_slope * v is the leaky ReLU the
 * network always applies to the volume (negative_slope = 1: none).  The channel sum runs in a fixed order.
 * Backward: with g = v_out where the saved `out` is positive and negative_slope * v_out elsewhere (`out` may be NULL when the slope
 * is 1), both gradients are gathers without atomics, each optional (NULL: not computed):
 *   v_first[b,c,y,x]  = (1/C) * sum_k g[b,k,y,x]       * second[b,c,y+dy,x+dx]
 *   v_second[b,c,y,x] = (1/C) * sum_k g[b,k,y-dy,x-dx] * first[b,c,y-dy,x-dx]
 * Forward and backward are bitwise reproducible.  D4GS_EINVAL before any GPU call for a NULL required pointer or a dimension < 1
 * (also B > 65535, H > 524280 or more than 2^40 elements). */
D4GS_API int d4gs_correlation_fwd(const float *first, const float *second, int32_t B, int32_t C, int32_t H, int32_t W,
                                  float negative_slope, float *out, void *stream);
D4GS_API int d4gs_correlation_bwd(const float *first, const float *second, const float *out, const float *v_out, int32_t B, int32_t C,
                                  int32_t H, int32_t W, float negative_slope, float *v_first, float *v_second, void *stream);
/* Backward warp (pwcnet.py get_backwarp): input [B,C,H,W], flow [B,2,H,W] (x first, in pixels).  Pixel (x, y) samples the input
 * bilinearly, zeros outside, at (x + fx W / (W - 1), y + fy H / (H - 1)) - the factor is what the reference's normalisation by
 * (W - 1) / 2 leaves on its align_corners=False grid; H < 2 or W < 2 is D4GS_EINVAL.  coverage = the sum of the in-bounds bilinear
 * weights, mask [B,1,H,W] = coverage > 0.999 ? 1 : 0, out [B,C,H,W] = sample * mask.  Backward: v_input (zeroed here, then
 * scattered into with float atomics: not bitwise reproducible) = the adjoint of the sampling under the mask; nothing flows to the
 * flow or through the mask. */
D4GS_API int d4gs_backwarp_fwd(const float *input, const float *flow, int32_t B, int32_t C, int32_t H, int32_t W, float *out, float *mask,
                               void *stream);
D4GS_API int d4gs_backwarp_bwd(const float *flow, const float *v_out, int32_t B, int32_t C, int32_t H, int32_t W, float *v_input,
                               void *stream);
/* Aligned L1 (AlignedLoss.forward without the flow network) for P pairs at once, with the same sampling:
 *   losses[p] = mean over 3 H W of | warp(pred_p, flow_p) m_p mask_p - target_p m_p mask_p |
 * pred, target [P,3,H,W], flow [P,2,H,W], m_p the coverage mask, mask [P,H,W] or NULL (ones).  partials: d4gs_aligned_l1_blocks(H, W)
 * doubles per pair, 8-byte aligned; block partials are accumulated in double and added in a fixed order (the forward is bitwise
 * reproducible).  Backward: v_loss [P] (device), v_pred [P,3,H,W] (zeroed here, then scattered into with float atomics) and, when
 * not NULL, v_target [P,3,H,W] (written directly); sign(0) = 0.  Nothing flows to the flow or the masks. */
D4GS_API int64_t d4gs_aligned_l1_blocks(int32_t H, int32_t W); /* 0: bad argument */
D4GS_API int d4gs_aligned_l1_fwd(const float *pred, const float *flow, const float *target, const float *mask, int32_t P, int32_t H,
                                 int32_t W, double *partials, float *losses, void *stream);
D4GS_API int d4gs_aligned_l1_bwd(const float *pred, const float *flow, const float *target, const float *mask, const float *v_loss,
                                 int32_t P, int32_t H, int32_t W, float *v_pred, float *v_target, void *stream);

/* Masked image metrics (appended; D4GS_VERSION unchanged): what the reference's mPSNR and mSSIM accumulate (flow3d/metrics.py:99-124,
 * 142-217), for M masks of B images in one call.  pred, target [B,H,W,3] fp32 channel-last as the rasterizer writes them; masks
 * [M,B,H,W] fp32, any values (the reference's are binary), or NULL = one mask of ones (M must be 1).  out [M,B,3] doubles (device):
 *   out[m,b,0] = sum over pixels and channels of ((pred - target) * mask)^2
 *   out[m,b,1] = sum of the mask
 *   out[m,b,2] = the mean over the [H-10,W-10,3] map of the dycheck masked SSIM (want_ssim != 0; otherwise 0 and H, W may be < 11):
 *                the moments p, t, p^2, t^2, p t each pass a count-normalised 11-tap sigma-1.5 filter along x, then along y,
 *                  cnt = sum_window mask, out = cnt != 0 ? (sum_window f z mask) * 11 / cnt : 0, mask' = (cnt != 0),
 *                the y pass on the x pass's result under its mask'; variances clipped at 0, the covariance to the geometric mean;
 *                c1 = 1e-4, c2 = 9e-4.  A position whose windows are empty scores 1, as in the reference.
 * Every sum is in double and has a fixed order (no atomics): bitwise reproducible, and each (m, b) does not depend on M.  partials:
 * [d4gs_metrics_blocks(M,B,H,W), 3] doubles of scratch, 8-byte aligned.  Nothing is read on the host.  D4GS_EINVAL, by host
 * arithmetic alone and before any HIP call, for a NULL pred / target / partials / out, a misaligned pointer, M, B, H or W < 1,
 * masks == NULL with M != 1, want_ssim with H < 11 or W < 11, or sizes beyond the grid (M * B or ceil(H / 16) > 65535, more than
 * 2^31 - 1 blocks). */
D4GS_API int64_t d4gs_metrics_blocks(int32_t M, int32_t B, int32_t H, int32_t W); /* 0: illegal sizes */
D4GS_API int d4gs_masked_metrics(const float *pred, const float *target, const float *masks, int32_t M, int32_t B, int32_t H,
                                 int32_t W, int32_t want_ssim, double *partials, double *out, void *stream);

/* Image terms (appended; D4GS_VERSION unchanged): the passes of Trainer.compute_dynamic_losses / compute_static_losses that the
 * reference writes as plain torch ops.  Every tensor is fp32, contiguous, channel-last; nothing is read on the host, no atomics, every
 * sum has a fixed order (bitwise reproducible), every launch is on `stream`.  D4GS_EINVAL, by host arithmetic alone and before any
 * HIP call, for a NULL required pointer, a misaligned pointer, a size < 1 or beyond the grid, and what each entry names below.
 *
 * Dilation (nn.MaxPool2d(2r+1, stride 1, padding r); the reference's r is 4): mask, out [B,H,W];
 *   out[b,y,x] = max of mask[b,y',x'] over |y' - y| <= r, |x' - x| <= r clipped to the image
 * - max-pool's -inf padding, so a mask of all -1 dilates to -1.  Values are copied: bit-exact (NaN propagates as in torch; which of
 * +0 and -0 a tie keeps is not specified).  out_complement, when not NULL, receives 1 - out in the same pass.  r >= 0 (r < 0:
 * D4GS_EINVAL); B and ceil(H / 16) <= 65535, W <= 2^30.  No gradient: masks are data.
 *
 * Sharp-keep loss (flow3d/trainer.py:736-760: F.interpolate(scale_factor=1/factor, mode="area") of prediction, mask and target, then
 * F.l1_loss): pred [B,H,W,C], mask [B,H,W], target [B,H,W,C] (target_reduced == 0) or already reduced [B,Ho,Wo,C] (!= 0), factor one
 * of 1, 2, 4, 8, Ho = H / factor and Wo = W / factor rounded down.  Output window i along an axis of length L with Lo outputs covers
 * [floor(i L / Lo), ceil((i + 1) L / Lo)) (torch's adaptive average pool: when factor does not divide L, windows differ in size and
 * neighbours overlap by at most one row or column).  With abar the window mean of a (tbar = t for a reduced target):
 *   out[0] = sum |pbar mbar - tbar mbar| / (B Ho Wo C)
 * Window sums, the products and the total are in double.  map [d4gs_area_keep_map_elems] receives sign(pbar mbar - tbar mbar) * mbar /
 * area(window) per output element, sign(0) = 0: all the backward reads.  partials: d4gs_area_keep_blocks doubles of scratch, 8-byte
 * aligned.  Both queries return 0 for sizes the entry points refuse: a size < 1, a factor outside the set, H < factor or W < factor
 * (torch returns an empty tensor and a NaN loss there), H or W > 32768, B H W C > 2^31 - 1.
 * Backward: v_pred[b,y,x,c] = v_loss[0] * sum over the at most 2 x 2 windows that hold (y, x) of map / (B Ho Wo C) (v_loss: device
 * scalar), a gather per input pixel.  Nothing flows to mask or target.
 *
 * Coverage (F.mse_loss): out[0] = mean over n elements of (a - t)^2, t == NULL: the constant 1; differences, squares and sums in
 * double.  partials: d4gs_mse_blocks(n) doubles, 8-byte aligned (0: n < 1 or n > 2^31 - 1).  Backward: v_a = v_loss[0] * 2 (a - t) / n,
 * exactly 0 where a == t. */
D4GS_API int d4gs_dilate_mask(const float *mask, int32_t B, int32_t H, int32_t W, int32_t r, float *out, float *out_complement,
                              void *stream);
D4GS_API int64_t d4gs_area_keep_map_elems(int32_t B, int32_t H, int32_t W, int32_t C, int32_t factor); /* 0: illegal sizes */
D4GS_API int64_t d4gs_area_keep_blocks(int32_t B, int32_t H, int32_t W, int32_t C, int32_t factor);    /* 0: illegal sizes */
D4GS_API int d4gs_area_keep_fwd(const float *pred, const float *mask, const float *target, int32_t target_reduced, int32_t B, int32_t H,
                                int32_t W, int32_t C, int32_t factor, float *map, double *partials, float *out, void *stream);
D4GS_API int d4gs_area_keep_bwd(const float *map, const float *v_loss, int32_t B, int32_t H, int32_t W, int32_t C, int32_t factor,
                                float *v_pred, void *stream);
D4GS_API int64_t d4gs_mse_blocks(int64_t n); /* 0: illegal size */
D4GS_API int d4gs_mse_fwd(const float *a, const float *t, int64_t n, double *partials, float *out, void *stream);
D4GS_API int d4gs_mse_bwd(const float *a, const float *t, const float *v_loss, int64_t n, float *v_a, void *stream);

/* Scene initialisation (appended; D4GS_VERSION unchanged): what flow3d/init_utils.py needs from cupy, cuML and sklearn to turn 3-D
 * tracks and static points into a first scene.  The block is declared under a macro of its own: D4GS_API stays the table of the
 * frame, its losses and its metrics (the binding keeps it as EXPORTS), D4GS_INIT_API is the one-off preprocessing
 * (INIT_PROTOTYPES); both are exported, parsed by the same strict rules and bound by the same call.  Every pointer below is DEVICE
 * memory; tensors are contiguous; nothing is read on the host, no atomics, every launch is on `stream`, and every result is bitwise
 * reproducible from run to run.  D4GS_EINVAL, by host arithmetic alone and before any HIP call, for a NULL required pointer, a
 * misaligned pointer, a size < 1 or beyond the limits each entry names.
 *
 * Track features (batched_interp_masked, init_utils.py:594-654, and the velocity directions of :571-574): xyz [G,T,3] fp32, visible
 * [G,T] uint8 (non-zero = visible).  xyz_interp [G,T,3] (may be NULL): per track and coordinate np.interp over the visible frames -
 * linear between neighbouring visible frames, constant before the first and after the last - evaluated in double and rounded once; a
 * visible frame's value is copied bit for bit.  Two deviations from the reference: a track WITHOUT a visible frame keeps its input
 * row (the reference's concatenation interpolates it across the neighbouring tracks in memory; its callers filter such tracks out
 * first), and the whole row is one interpolation for any T (the reference restarts at every 64-frame chunk, an artefact of its
 * batching).  vel_dirs [G,3(T-1)] (may be NULL; T >= 2 then, else D4GS_EINVAL): vel_dirs[g, 3t + c] = v_c / (|v| + 1e-5) with
 * v = xyz_interp[g,t+1] - xyz_interp[g,t] taken from the double values before they are rounded.  G T 3 <= 2^31 - 1.
 *
 * k nearest neighbours (loss_utils.py:93-99, sklearn's brute force; exact): points [N,3] fp32, 1 <= k <= D4GS_KNN_MAX_K, N >= k + 1
 * (sklearn raises below that) and N <= 2^24.  dists [N,k] fp32 ascending, idx [N,k] int32 (may be NULL): the k nearest OTHER points.
 * Self is excluded by index, so an exact duplicate of the query is a neighbour at distance 0 - the distances of the reference's "drop
 * column 0".  The squared distance is the sum of the three squared coordinate differences (never |a|^2 + |b|^2 - 2 a.b), its root
 * is taken once at the end; among equal distances the lower index comes first.  Candidates are staged in LDS D4GS_KNN_TILE at a time;
 * above N = D4GS_KNN_SPLIT_MIN the candidate range is split over d4gs_knn_splits(N) blocks per query block and a second pass merges
 * their lists.  workspace: d4gs_knn_workspace_bytes(N, k) bytes, 16-byte aligned (0: illegal N or k; never 0 for a legal pair).
 * Non-finite coordinates: unspecified neighbours, no fault.
 *
 * k-means (Lloyd iterations; cuML's KMeans in the reference, :577-582): x [G,D] fp32, centres [K,D] fp32 and labels [G] int32 are
 * read AND written, 1 <= K <= D4GS_KMEANS_MAX_K, K D <= 12288 (the centres live in LDS), G D <= 2^31 - 1.  One iteration: every row
 * takes the label of its nearest centre by the fp32 sum of squared differences (ties: the lowest index, as argmin), then every centre
 * becomes the mean of its rows - sums in double in the fixed order of csrc/reduce.h (thread t of block b adds rows 256 b + t +
 * 256 d4gs_kmeans_blocks(G) i in increasing i, block sum, ordered total over the blocks); a centre without rows keeps its value.
 * `iters` >= 1 iterations run back to back on the stream.  changed [1] int32: how many labels the LAST iteration changed (the first
 * one compares with the labels passed in).  scratch: d4gs_kmeans_scratch_bytes(G, D, K) bytes, 8-byte aligned (0: illegal sizes).
 * The initial centres are the caller's: the package seeds them by k-means++, so its labels are a Lloyd fixed point of that seed and
 * NOT cuML's labels (cuML's random initialisation cannot be matched and is no contract).
 *
 * Procrustes moments (the sums under solve_procrustes for every (basis, frame) pair of init_motion_params_with_procrustes, :188-240,
 * in one launch): xyz [G,T,3], weights [G,T], conf [G,T] fp32; order [G] int32 = the track indices sorted by cluster, seg [K+1] int32
 * = where each cluster starts in order (entries outside 0..G - 1 / 0..G are skipped / clamped, never followed).  For cluster n and
 * frame t, over the tracks p of the cluster, with u = ((w[p,cano_t] w[p,t]) (conf[p,cano_t] + conf[p,t])) / 2, src = xyz[p,cano_t],
 * dst = xyz[p,t]:   out[n,t,0] = sum u, [1..3] = sum u src, [4..6] = sum u dst, [7 + 3 i + j] = sum u dst_i src_j
 * out [K,T,16] doubles, 8-byte aligned; every product and sum in double, one block per pair in the block-sum order of reduce.h (thread
 * t adds members t, t + 256, ... in increasing order).  0 <= cano_t < T, K <= 65535, G T 3 <= 2^31 - 1.  The reference's logged
 * err / err_before are not computed. */
#define D4GS_INIT_API __attribute__((visibility("default")))
#define D4GS_KNN_MAX_K 8
#define D4GS_KNN_TILE 1024
#define D4GS_KNN_SPLIT_MIN 4096
#define D4GS_KMEANS_MAX_K 64
D4GS_INIT_API int d4gs_track_features(const float *xyz, const uint8_t *visible, int32_t G, int32_t T, float *xyz_interp, float *vel_dirs,
                                      void *stream);
D4GS_INIT_API int32_t d4gs_knn_splits(int64_t N);                    /* 0: illegal N */
D4GS_INIT_API int64_t d4gs_knn_workspace_bytes(int64_t N, int32_t k); /* 0: illegal N or k */
D4GS_INIT_API int d4gs_knn(const float *points, int32_t N, int32_t k, float *dists, int32_t *idx, void *workspace, void *stream);
D4GS_INIT_API int64_t d4gs_kmeans_blocks(int64_t G);                                     /* 0: illegal G */
D4GS_INIT_API int64_t d4gs_kmeans_scratch_bytes(int64_t G, int32_t D, int32_t K); /* 0: illegal sizes */
D4GS_INIT_API int d4gs_kmeans_step(const float *x, int32_t G, int32_t D, int32_t K, int32_t iters, float *centres, int32_t *labels,
                                   int32_t *changed, void *scratch, void *stream);
D4GS_INIT_API int d4gs_procrustes_moments(const float *xyz, const float *weights, const float *conf, const int32_t *order,
                                          const int32_t *seg, int32_t G, int32_t T, int32_t K, int32_t cano_t, double *out, void *stream);

/* Test-time pose refinement (appended; D4GS_VERSION unchanged): what Validator.validate_imgs_with_optimization (flow3d/validator.py:
 * 400-456) runs per validation frame - 500 iterations of render, L1, backward into a free 3x3 transR and a 3x1 transT composed into
 * w2c, CosineAnnealingLR.step(), Adam.step() - needs beyond the render.  The block is declared under a macro of its own, like the
 * scene initialisation: D4GS_EVAL_API is the evaluation-time block (the binding's EVAL_PROTOTYPES); exported, parsed by the same
 * strict rules and bound by the same call.  csrc/pose_refine.hip; DESIGN.md section 25.
 *
 * d4gs_pose_bwd: the camera-only adjoint of d4gs_project_fwd.  From the three cotangents v_means2d [S,N,2], v_conics [S,N,3] and
 * v_depths [S,N] (v_opac_act and v_ctab do not reach the camera; with D4GS_ANTIALIASED the compensation's adjoint arrives folded
 * into v_conics) it writes what d4gs_project_bwd leaves in D4gsLeafGrads.v_viewmat / .v_RTs - the same mathematics, summed in
 * another order - and NO per-Gaussian gradient: nothing of size N is allocated, computed or written.  v_viewmat [4,4]: rows 0-2 the
 * gradient, row 3 exact zeros.  v_RTs [S,3,4] or NULL (not wanted; with in->RTs == NULL it must be NULL).  Reads in->means, quats,
 * scales, viewmat, Kmat, RTs and, for G > 0, motion_coefs, rots, transls, times (the deformation is recomputed from the leaves and
 * proj->blend_bases; without that table it is built behind the partial sums, one small launch more); proj->radii and proj->conics
 * (an instance with radii == 0 contributes nothing: near / far plane, radius_clip and the screen test are the forward's decisions).
 * Honours D4GS_RAW_PARAMS and the 1.3 tan(fov / 2) clamp of the Jacobian; opacities, colours and their tables are not read.
 * One lane per (sub-sample, Gaussian), gridDim.y = S; the 24 values of a lane (12 of the view matrix, 12 of its sub-sample's camera
 * delta) are summed per block and then over the blocks in the fixed order of csrc/reduce.h - no atomics, nothing to zero: bitwise
 * reproducible from run to run and graph replay to graph replay.  partials: d4gs_pose_bwd_partials_elems(dims) floats of scratch
 * (host arithmetic only; 0 for dims the entry point refuses).  D4GS_EINVAL, before any HIP call, for bad dims (G > N among them),
 * a NULL required pointer, a NULL partials, or v_RTs without in->RTs.
 *
 * d4gs_pose_step: one one-wave launch that ends an iteration and prepares the next.  w2c [4,4] the base matrix [R0 t0; .], v_W [4,4]
 * the gradient of the composed matrix, p [12] the parameters (transR row-major, then transT), m, v [12] Adam's moments, step [1]
 * int32 the number of updates made - all in device memory, so a captured launch stays valid while the learning rate moves.
 *   g[0:9] = v_W[:3,:3] R0^T,  g[9:12] = v_W[:3,3]
 *   k = step + 1;  lr = eta_min + (lr0 - eta_min) (1 + cos(pi k / t_max)) / 2 in double: the reference calls scheduler.step() BEFORE
 *   optimizer.step(), so update i (from 0) runs at lr(i + 1) and update t_max - 1 at eta_min
 *   torch.optim.Adam on (p, m, v) with gradient g, learning rate lr and t = k: d4gs_adam_step's per-element update
 *   step <- k;  lr_out[0] <- (float)lr (may be NULL);  W [4,4] <- [transR R0 | transT + t0; 0 0 0 1]
 * W may be the buffer v_W was taken with respect to, not w2c.  The reference leaves ZEROS in the bottom row of its composed matrix
 * (torch.zeros_like(w2c), validator.py:442); nothing reads that row - the projection, the MoveModel's pose encoding and both
 * adjoints use rows 0-2 - so (0, 0, 0, 1) is written, and every other matrix of the package stays a rigid transform.
 * D4GS_EINVAL, before any HIP call, for a NULL (lr_out excepted) or misaligned pointer or t_max < 1.
 * d4gs_pose_step_cpu: the same inline function on HOST pointers, one thread, no stream.  Never a fallback. */
#define D4GS_EVAL_API __attribute__((visibility("default")))
D4GS_EVAL_API size_t d4gs_pose_bwd_partials_elems(const D4gsDims *dims);
D4GS_EVAL_API int d4gs_pose_bwd(const D4gsDims *dims, const D4gsProjIn *in, const D4gsProjOut *proj, const float *v_means2d,
                                const float *v_conics, const float *v_depths, float *v_viewmat, float *v_RTs, float *partials,
                                void *stream);
D4GS_EVAL_API int d4gs_pose_step(const float *w2c, const float *v_W, float *p, float *m, float *v, int32_t *step, double lr0,
                                 double eta_min, int32_t t_max, double beta1, double beta2, double eps, float *lr_out, float *W,
                                 void *stream);
D4GS_EVAL_API int d4gs_pose_step_cpu(const float *w2c /* [host] */, const float *v_W /* [host] */, float *p /* [host] */,
                                     float *m /* [host] */, float *v /* [host] */, int32_t *step /* [host] */, double lr0,
                                     double eta_min, int32_t t_max, double beta1, double beta2, double eps,
                                     float *lr_out /* [host] */, float *W /* [host] */);

/* Observations (appended; D4GS_VERSION unchanged): what the reference's flow3d/data/utils.py and the get_tracks_3d / get_bkgd_points
 * bodies of its datasets do to a dataset's raw arrays - aligned depth maps, foreground masks, TAPIR 2-D tracks, Ks, w2cs - before
 * the scene initialisation takes over.  The block is declared under a macro of its own, like the two before it: D4GS_DATA_API is
 * the data-preparation block (the binding's DATA_PROTOTYPES); exported, parsed by the same strict rules and bound by the same call.
 * csrc/observations.hip; DESIGN.md section 26.  Every pointer is DEVICE memory, tensors are contiguous fp32 unless stated, every
 * launch is on `stream`, nothing is read on the host, and every result is bitwise reproducible from run to run.  D4GS_EINVAL, by
 * host arithmetic alone and before any HIP call, for a NULL required pointer, a misaligned pointer, a size < 1, a product of sizes
 * beyond 2^31 - 1 as each entry names it, or an illegal kernel_size / query.
 *
 * d4gs_masked_median_blur: masked_median_blur (utils.py:207-250), exactly.  image, mask, out [n_img,H,W] (n_img = B C), kernel_size
 * k odd in 3..15, n_img H W <= 2^31 - 1.  The window is k x k and zero-padded: a position outside the image has value 0 and mask 0.
 * An entry is VALID iff its mask value equals 1.0f; every other entry, out-of-image positions included, is invalid.
 * lo = min(min(image), 0), hi = max(max(image), 0).  Enumerate the invalid entries in (image, h, w, window index ky k + kx) order:
 * the even-numbered ones count as lo, the odd-numbered ones as hi - so a pixel's own invalid entries alternate, starting with lo
 * iff an even number of invalid entries precedes the pixel.  out = the LOWER median of the pixel's k k entries, rank (k k - 1) / 2:
 * with n_lo entries sent to lo, it is lo if rank < n_lo, else the (rank - n_lo)-th smallest valid value if there is one, else hi.
 * The output is one of the inputs' bit patterns (or lo / hi).  Inputs must be finite; -0.0 orders below +0.0.
 * per_image != 0: lo, hi and the enumeration restart at every image, so n_img images give what n_img calls with one image give
 * (the dataset blurs frame by frame).  blend (may be NULL) [n_img,H,W]: out = median * blend + image * (1 - blend), each product and
 * the sum rounded to fp32 on its own (the dataset's depth * mask + old * (1 - mask), stereo_low_dataset.py:239-241).  out must not be
 * image.  workspace: d4gs_masked_median_ws_bytes(n_img, H, W) bytes, 16-byte aligned (0: a size < 1 or past the limit; never 0
 * for legal sizes).  Tiles of 16 x 16 pixels, staged with their (k - 1) / 2 halo in LDS.
 *
 * d4gs_lift_tracks: get_tracks_3d_for_query_frame (utils.py:69-152) before its filter.  tracks_2d [N,T,4] = x, y, occlusion logit,
 * expected-distance logit; depths, masks [T,H,W]; query_img [H,W,3]; inv_Ks [T,3,3]; c2ws [T,4,4]; 0 <= query < T.  Per sample:
 * vis = 1 - sigmoid(occ), conf = 1 - sigmoid(dist), visible = vis conf > 0.5, invisible = (1 - vis) conf > 0.5, confidence = conf
 * where either holds, else 0; depth = bilinear sample of depths[t] at (x, y) with the coordinates clamped to the image;
 * xyz = c2ws[t] (inv_Ks[t] (x, y, 1) depth) with the unclamped x, y.  in_mask = every one of the four bilinear corners of (x, y)
 * that has a non-zero weight lies inside the image and has mask == 1.0f; the corner floor(x) always weighs, floor(x) + 1 weighs iff
 * x is no integer, the same in y.  (The reference's grid_sample(...) == 1 also rejects ~1.5 % of samples whose corners are all 1,
 * where the rounded weights do not sum to 1: rounding, not intent.)  visibles, invisibles [N,T] uint8 and confidences [N,T] are
 * multiplied by in_mask [N,T] uint8.  colors [N,3]: query_img sampled like the depth at the track's position in frame `query`.
 * visible_count [N] int32 = the row sums of visibles; hist [T + 1] int32 = how many tracks have each count (zeroed by the call;
 * integer atomics).  N T 4, T H W and H W 3 <= 2^31 - 1.  Non-finite coordinates: not in the mask, depth from a clamped position.
 *
 * d4gs_bkgd_points: the per-pixel part of get_bkgd_points (stereo_low_dataset.py:512-547) and normal_from_depth_image (utils.py:
 * 337-360) for T frames.  depths, masks, valid_masks [T,H,W]; inv_Ks [T,3,3]; c2ws [T,4,4].  points [T,H,W,3] = c2ws[t] (inv_Ks[t]
 * (x, y, 1) depth).  normals [T,H,W,3] = n / max(|n|, 1e-12), n = cross(right - left, top - bottom) of the four neighbours' world
 * points (top = y - 1); exact zeros on the one-pixel border.  keep [T,H,W] uint8 = ((1 - mask) valid_mask (depth > 0)) != 0.
 * index [T,H,W] int32 and counts [T] int32 (both or neither): index[t, 0 .. counts[t]) = the offsets y W + x of frame t's kept pixels
 * in ascending order - the order boolean indexing gives, so a caller's selections mean what they mean in the reference; the rest of
 * index[t] is not written.  One block per frame walks it with a ballot scan (the single-block plan of d4gs_control_plan, T frames
 * side by side); counts is the one thing a caller reads on the host.  T H W 3 <= 2^31 - 1. */
#define D4GS_DATA_API __attribute__((visibility("default")))
D4GS_DATA_API int64_t d4gs_masked_median_ws_bytes(int64_t n_img, int64_t H, int64_t W); /* 0: illegal sizes */
D4GS_DATA_API int d4gs_masked_median_blur(const float *image, const float *mask, const float *blend, int32_t n_img, int32_t H, int32_t W,
                                          int32_t kernel_size, int32_t per_image, float *out, void *workspace, void *stream);
D4GS_DATA_API int d4gs_lift_tracks(const float *tracks_2d, const float *depths, const float *masks, const float *query_img,
                                   const float *inv_Ks, const float *c2ws, int32_t N, int32_t T, int32_t H, int32_t W, int32_t query,
                                   float *xyz, uint8_t *visibles, uint8_t *invisibles, float *confidences, uint8_t *in_mask,
                                   float *colors, int32_t *visible_count, int32_t *hist, void *stream);
D4GS_DATA_API int d4gs_bkgd_points(const float *depths, const float *masks, const float *valid_masks, const float *inv_Ks,
                                   const float *c2ws, int32_t T, int32_t H, int32_t W, float *points, float *normals, uint8_t *keep,
                                   int32_t *index, int32_t *counts, void *stream);

/* Track fit (appended; D4GS_VERSION unchanged): the warm-up of flow3d/init_utils.py:273-402 (run_initial_optim) - an Adam fit of the
 * motion bases, the raw motion coefficients and the canonical means to the 3-D tracks, before training starts.  The block is declared
 * under a macro of its own, like the three before it: D4GS_FIT_API is the binding's FIT_PROTOTYPES; exported, parsed by the same
 * strict rules and bound by the same call.  csrc/track_fit.hip; DESIGN.md section 27.  Every pointer is DEVICE memory unless marked,
 * tensors are contiguous fp32 unless stated, every launch is on `stream`, nothing is read on the host, no atomics on floats, and every
 * result is bitwise reproducible from run to run and graph replay to graph replay.
 *
 * Leaves: means [G,3], raw motion_coefs [G,K], rots [K,T,6], transls [K,T,3].  Data: xyz [G,T,3], visibles / invisibles [G,T] uint8
 * (non-zero = set), confidences [G,T], Ks [T,3,3] (any 3x3), w2cs [T,4,4] = [A t; 0 0 0 1] (A any invertible 3x3).
 *   p[g,tau] = the deformation of means_g at the integer frame tau (softmax coefficients, Gram-Schmidt)   tau = 0 .. T-1
 *   w3 = visibles conf,  w2 = invisibles conf;  proj(x,tau): c = A x + t, v = Ks c, uv = v.xy / max(v.z, 1e-5)
 *   out[1] track_3d      = sum w3 mean_3 |p - xyz| / (sum w3 + 1e-8)
 *   out[2] track_2d      = masked_l1_loss(proj(p), proj(xyz), w2, quantile) / Ks[0,0,0]: e = mean_2 |.|, thr = torch.quantile of e over
 *                          ALL G T elements (linear interpolation; quantile >= 1: every element kept), sum_{e < thr} w2 e / (sum_{e < thr}
 *                          w2 + 1e-8); the selection is d4gs_masked_l1_fwd's
 *   out[3] coef_sparse   = 1 - mean_g sum_k softmax(motion_coefs_g)_k^2
 *   out[4] smooth_bases  = mean_{k, 1 <= tau <= T-2} |2 rots - rots[tau-1] - rots[tau+1]| + 2 (the same on transls)
 *   out[5] smooth_tracks = mean_{g, 1 <= tau <= T-2} |2 p_tau - p_{tau-1} - p_{tau+1}|      (no factor 0.5: not d4gs_motion_regs')
 *   out[6] z_accel       = mean_{g,b} ((m1 - m0).d)^2 + mean_{g,b} ((m2 - m1).d)^2, b = 0 .. T-1, m_j = p[g, clamp(b,1,T-2) + j - 1],
 *                          d = normalize(m1 - centre_b, eps 1e-12), centre_b = -A_b^-1 t_b (cofactor inverse): the centre of frame b,
 *                          so frames 1 and T-2 enter twice (T = 3: frame 1 three times)
 *   out[0] = sum_k weights[k] out[1 + k] (weights [6] in device memory, what d4gs_track_fit_schedule left there; NULL: all 1);
 *   out[7] = thr.  out [8].  losses (may be NULL) [num_iters,7]: out[0..6] also go to row *iter - 1 when that row exists - iter the
 *   device counter as d4gs_track_fit_schedule has just left it (the iteration's index + 1) - so a loop keeps its history
 *   without a launch of its own.
 * The gradient of |x| at 0 and of a norm at exactly 0 is 0; the depth clamp passes the gradient where v.z >= 1e-5; none flows
 * through thr.
 *
 * d4gs_track_fit_prepare, once per run: the time-major planes of xyz, proj(xyz), w3 and w2, sum w3 (double, the fixed order of
 * csrc/reduce.h), the T camera tables with their centres and 1 / Ks[0,0,0] -> targets, d4gs_track_fit_targets_bytes(G, T) bytes,
 * 16-byte aligned; K does not enter.  d4gs_track_fit_fwd: ONE deformation per (g, frame) by the pose kernels (time-major, S = T),
 * then one loss launch - one lane per Gaussian, the frames split over gridDim.y in chunks of 4 with one-frame halos, the basis rows
 * in extra blocks - the selection, one finish block.  workspace: d4gs_track_fit_workspace_bytes(G, K, T) bytes, 16-byte aligned; the
 * forward leaves the positions, the errors e and thr there and d4gs_track_fit_bwd reads them.  The backward takes v_out [6], the
 * cotangents of out[1..6], and OVERWRITES grads->v_means, v_motion_coefs, v_rots, v_transls (the other fields are not read): a
 * gather over the frames (one writer per address), the pose adjoint, then the bases' and the coefficients' own terms.
 * Both size functions are host arithmetic alone and return 0 for sizes the entry points refuse.  D4GS_EINVAL with a message, before
 * any HIP call: a NULL required pointer, G < 1, K outside 1 .. D4GS_MAX_K (32), T < 3 (no interior frame: the reference's mean over
 * nothing is NaN) or T > 65535, 9 G T, 9 K T or G K beyond 2^31 - 1, targets or workspace too small or not 16-byte aligned, a
 * quantile that is NaN, <= 0 or infinite, a loss history without the counter or with num_iters < 1.
 *
 * d4gs_track_fit_schedule: one one-wave launch at the head of iteration i = *iter (int32, device).  table: FOUR D4gsAdamRec in
 * device memory in the order rots, transls, motion_coefs, means (the reference's param groups).
 *   lr_r = lr0_r 0.1^(i / num_iters) in double (ExponentialLR's closed form) -> table[r].lr and, for 0 <= i < num_iters, lrs[i,r]
 *     (fp32 history [num_iters,4], may be NULL)
 *   w = 0.01 for i <= 400 or num_iters <= 400, else (0.1 - 0.01) (i - 400) / (num_iters - 400) + 0.01 in double (never divides by
 *     <= 0, also for a counter that has run past the end)
 *   weights [6] = 1, 0.5, 0.01, w, 0.5 w, 0.1 rounded to fp32 (track_3d, track_2d, coef_sparse, smooth_bases, smooth_tracks, z_accel)
 *   *iter = i + 1
 * A captured launch therefore stays valid while four learning rates and the smoothness weight move; d4gs_adam_step reads the table
 * as it is.  D4GS_EINVAL for a NULL iter / table / weights, a misaligned pointer, num_iters < 1 or an lr0 that is not finite and > 0.
 * d4gs_track_fit_schedule_cpu: the same inline function on HOST pointers, one thread, no stream.  Never a fallback. */
#define D4GS_FIT_API __attribute__((visibility("default")))
D4GS_FIT_API size_t d4gs_track_fit_targets_bytes(int32_t G, int32_t T);              /* 0: illegal sizes */
D4GS_FIT_API size_t d4gs_track_fit_workspace_bytes(int32_t G, int32_t K, int32_t T); /* 0: illegal sizes */
D4GS_FIT_API int d4gs_track_fit_prepare(const float *xyz, const uint8_t *visibles, const uint8_t *invisibles, const float *confidences,
                                        const float *Ks, const float *w2cs, int32_t G, int32_t T, void *targets, size_t targets_bytes,
                                        void *stream);
D4GS_FIT_API int d4gs_track_fit_fwd(const float *means, const float *motion_coefs, const float *rots, const float *transls, int32_t G,
                                    int32_t K, int32_t T, float quantile, const float *weights, const void *targets, size_t targets_bytes,
                                    void *workspace, size_t workspace_bytes, float *out, const int32_t *iter, float *losses,
                                    int32_t num_iters, void *stream);
D4GS_FIT_API int d4gs_track_fit_bwd(const float *means, const float *motion_coefs, const float *rots, const float *transls, int32_t G,
                                    int32_t K, int32_t T, float quantile, const void *targets, size_t targets_bytes, void *workspace,
                                    size_t workspace_bytes, const float *v_out, const D4gsLeafGrads *grads, void *stream);
D4GS_FIT_API int d4gs_track_fit_schedule(int32_t *iter, int32_t num_iters, D4gsAdamRec *table /* [device] */, double lr0_rots,
                                         double lr0_transls, double lr0_coefs, double lr0_means, float *weights, float *lrs, void *stream);
D4GS_FIT_API int d4gs_track_fit_schedule_cpu(int32_t *iter /* [host] */, int32_t num_iters, D4gsAdamRec *table, double lr0_rots,
                                             double lr0_transls, double lr0_coefs, double lr0_means, float *weights /* [host] */,
                                             float *lrs /* [host] */);

/* Feed (appended; D4GS_VERSION unchanged): one training batch per step from a clip that lives in device memory - what
 * StereoLowDataset.__getitem__ (flow3d/data/stereo_low_dataset.py:574-666), train_collate_fn and the trainer's shaping of the track
 * supervision (trainer.py:549-565, 646-659) do on the host, written into buffers of fixed address so that a captured step reads new
 * data on every replay.  The block is declared under a macro of its own, like the four before it: D4GS_FEED_API is the binding's
 * FEED_PROTOTYPES; exported, parsed by the same strict rules and bound by the same call.  csrc/feed.hip; DESIGN.md section 28.  Every
 * pointer is DEVICE memory unless marked, tensors are contiguous fp32 unless stated, every launch is on `stream`, nothing is read on the
 * host, no atomics, and every result is bitwise reproducible.  D4GS_EINVAL with a message that names the argument, by host arithmetic
 * alone and before any HIP call: a NULL required pointer, a misaligned pointer, a size < 1 or beyond its limit.
 *
 * d4gs_feed_draw: one wave.  step = *counter (int64); targets [n] int32 = n DISTINCT frames of [start, end), start + Floyd's sampling
 * over R = end - start: pick k = 0 .. n-1 is t = (r_k (R - n + k + 1)) >> 32, or R - n + k if an earlier pick equals t, with r_k the
 * 32-bit word k of a counter-based integer hash (splitmix64's finaliser) of (seed, step); then *counter = step + 1.  Every subset is
 * equally likely up to the multiply-shift's bias (< 2^-32 R).  1 <= n <= min(R, 64), 0 <= start < end.  It is no stream of numpy's.
 * d4gs_feed_draw_cpu: the same inline functions on HOST pointers, one thread, no stream: the exact twin.  Never a fallback.
 *
 * d4gs_feed_batch: ONE launch.  The clip: imgs [F,H,W,3], depths, masks, valid_masks [F,H,W], Ks [F,3,3], w2cs [F,4,4], time_ids [F]
 * int64, tracks [n_rows,4] (16-byte aligned; rows x, y, occlusion logit, expected-distance logit), offsets [F + 1] int64: the rows of
 * query frame q are offsets[q] .. offsets[q+1], P_q = (offsets[q+1] - offsets[q]) / F of them per target frame, target-frame-major
 * (row offsets[q] + t P_q + p; 64-bit).  The selection is read from device memory: index [1] int32 = q, targets [N] int32 (N <= 64).
 * P is the row stride of every per-query output: lanes p >= P_q are PADDING (coordinates, depth, image sample, confidence, weight 0,
 * flags 0, pix -1, query (-1, -1)); n_queries [1] int32 = P_q.  With t = targets[n], tt = time_ids[t] and row = the track row (q, t, p):
 *   ts [1] int64 = time_ids[q]; w2c [16], K [9] of frame q; img [H,W,3], valid_mask, mask, depth [H,W] = frame q's planes (all four or
 *   none: NULL skips the copy; 16-byte words where source and destination share their offset in a 16-byte line, dwords otherwise)
 *   query_tracks_2d [P,2] = x, y of row (q, q, p)            target_ts [N] int64 = tt
 *   target_w2cs [N,16] = w2cs[tt], target_Ks [N,9] = Ks[tt]  (at the TIME id, as the reference indexes them)
 *   target_tracks_2d [N,P,2] = row.xy   (8-byte aligned, as query_tracks_2d)
 *   vis = 1 - sigmoid(row.z), conf = 1 - sigmoid(row.w); target_visibles = vis conf > 0.5, target_invisibles = (1 - vis) conf > 0.5
 *   (uint8), target_confidences = conf where either holds, else 0                                              (utils.py:53-66)
 *   target_track_depths [N,P], target_track_imgs [N,3,P]: depths[t], imgs[t] sampled bilinearly at row.xy, the coordinates clamped
 *   to the image before any address is formed (grid_sample's align_corners=True, padding_mode="border"; d4gs_lift_tracks' rule)
 * and the element tables of d4gs_track_losses_fwd, element (n, p) at n P + p: rows = n; pix = int(y) W + int(x) of the query
 * (truncated), or -1 outside the image; vis (uint8) = target_visibles and pix >= 0; weights = target_confidences
 * sum_n' exp(-2 |ts - target_ts[n']| / num_frames), 0 where pix = -1.  target_tracks_2d, target_track_depths and target_Ks are those
 * tables' tgt_2d, tgt_depth and Ks as they are.
 * status [1] int32: the launch ORs in 1 (index outside 0 .. F-1), 2 (a target outside 0 .. F-1), 4 (a target's time id outside
 * 0 .. F-1), 8 (offsets of the query frame negative, decreasing, beyond n_rows or no multiple of F).  With any of them NOTHING is
 * addressed through the offending value: the whole batch is written as padding (P_q = 0; planes, matrices and time ids 0).
 * F H W 3 and N P 3 <= 2^31 - 1. */
#define D4GS_FEED_API __attribute__((visibility("default")))
D4GS_FEED_API int d4gs_feed_draw(int64_t *counter, uint64_t seed, int32_t start, int32_t end, int32_t n, int32_t *targets, void *stream);
D4GS_FEED_API int d4gs_feed_draw_cpu(int64_t *counter /* [host] */, uint64_t seed, int32_t start, int32_t end, int32_t n,
                                     int32_t *targets /* [host] */);
D4GS_FEED_API int d4gs_feed_batch(const float *imgs, const float *depths, const float *masks, const float *valid_masks, const float *Ks,
                                  const float *w2cs, const int64_t *time_ids, const float *tracks, const int64_t *offsets, int64_t n_rows,
                                  const int32_t *index, const int32_t *targets, int32_t F, int32_t H, int32_t W, int32_t N, int32_t P,
                                  int32_t num_frames, int64_t *ts, float *w2c, float *K, float *img, float *valid_mask, float *mask,
                                  float *depth, float *query_tracks_2d, int64_t *target_ts, float *target_w2cs, float *target_Ks,
                                  float *target_tracks_2d, uint8_t *target_visibles, uint8_t *target_invisibles,
                                  float *target_confidences, float *target_track_depths, float *target_track_imgs, int32_t *pix,
                                  int32_t *rows, uint8_t *vis, float *weights, int32_t *n_queries, int32_t *status, void *stream);

/* LPIPS (appended; D4GS_VERSION unchanged): everything of the validator's ninth metric that is not a convolution - the reference's
 * PNetLin(pnet_type='alex', version='0.1') (models/networks_basic.py) as flow3d/metrics.py:250-279 and run_compute_metrics.py use it.
 * The AlexNet trunk's five convolutions run in torch (deblur4dgs_amd/lpips.py); these entry points are what surrounds them.  The block
 * is declared under a macro of its own, like the five before it: D4GS_LPIPS_API is the binding's LPIPS_PROTOTYPES; exported, parsed by
 * the same strict rules and bound by the same call.  csrc/lpips.hip; DESIGN.md section 29.  Every pointer is DEVICE memory unless
 * marked, tensors are contiguous fp32 unless stated, every launch is on `stream`, nothing is read on the host, no atomics, every result
 * is bitwise reproducible, and nothing has a backward.  D4GS_EINVAL with a message that names the argument, by host arithmetic alone and
 * before any HIP call: a NULL required pointer, a misaligned pointer, a size < 1, H or W < 31 (the trunk's smallest image), C > 4096, or
 * a size beyond the grid.  masks == NULL stands for one mask of ones (M must be 1).
 *
 * d4gs_lpips_prepare: ONE launch.  pred, target [B,H,W,3] channel-last, masks [M,B,H,W] or NULL -> out [2,M,B,3,H,W] (pred first), the
 * trunk's input: x = image * mask (with masks), x = x * 2 - 1 (normalize != 0), then the scaling layer (x - shift) / scale with shift
 * (-.030, -.088, -.188) and scale (.458, .448, .450) - a division; each step rounded to fp32 in this order, as torch evaluates it.
 *
 * d4gs_lpips_layer: ONE launch per layer.  f0, f1 [n,C,h,w] (NCHW), weights [C] -> out [n,h,w]:
 *   d = sum_c weights_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2,  |f| = sqrt(sum_c f_c^2) over the pixel's column,
 * in the direct form (identical inputs give exactly 0.0; an all-zero column normalises to zero), accumulated in double and rounded once.
 * 1 <= C <= 4096.  From C = 128 on a block holds 16 pixels x 16 channel slices, below that 64 x 4: the choice depends on C alone, so a
 * pixel's value does not depend on n.  n h w <= 2^31 - 1.
 *
 * d4gs_lpips_score: two launches.  layers [5] (a HOST array of device pointers): the layer maps [M B, h_k, w_k]; sizes [10] (HOST):
 * h_0, w_0, ... h_4, w_4.  Every map is upsampled to H x W as nn.Upsample(scale_factor=(1.*H/h, 1.*W/w), mode='bilinear',
 * align_corners=False) does (source = (dst + 0.5) / scale_factor - 0.5, clamped at 0; in double), the five are added in layer order, and
 * the sum is rounded to fp32: score_map [M,B,H,W], written when not NULL.  out [M B, 2] doubles = sum score * mask, sum mask per (m, b),
 * from the fp32 scores, by block partials and one ordered total: partials is [d4gs_lpips_score_blocks(M,B,H,W), 2] doubles of scratch,
 * 8-byte aligned.  The result of an (m, b) does not depend on M.  d4gs_lpips_score_blocks is host arithmetic alone and returns 0 for
 * sizes the entry point refuses (M B <= 65535).
 *
 * d4gs_lpips_mean: ONE launch.  layers, sizes as above with maps [n, h_k, w_k] -> out [n] doubles: the mean over h_k x w_k of every
 * layer map (an ordered total in double), added in layer order - the reference's spatial=False form. */
#define D4GS_LPIPS_API __attribute__((visibility("default")))
D4GS_LPIPS_API int d4gs_lpips_prepare(const float *pred, const float *target, const float *masks, int32_t M, int32_t B, int32_t H,
                                      int32_t W, int32_t normalize, float *out, void *stream);
D4GS_LPIPS_API int d4gs_lpips_layer(const float *f0, const float *f1, const float *weights, int32_t n, int32_t C, int32_t h, int32_t w,
                                    float *out, void *stream);
D4GS_LPIPS_API int64_t d4gs_lpips_score_blocks(int32_t M, int32_t B, int32_t H, int32_t W);
D4GS_LPIPS_API int d4gs_lpips_score(const float *const *layers, const int32_t *sizes /* [host] */, const float *masks, int32_t M,
                                    int32_t B, int32_t H, int32_t W, float *score_map, double *partials, double *out, void *stream);
D4GS_LPIPS_API int d4gs_lpips_mean(const float *const *layers, const int32_t *sizes /* [host] */, int32_t n, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D4GS_H */
