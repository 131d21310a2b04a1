/*
 * skelsplat_hip.h -- C ABI of libskelsplat_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the hot path of laurabragagnolo/SkelSplat: everything the reference binds through
 * pybind11 in submodules/diff-gaussian-rasterization-{h36m,panoptic,op}/ext.cpp:14-18
 * (rasterize_gaussians, rasterize_gaussians_backward, mark_visible; signatures rasterize_points.h:18-71),
 * submodules/fused-ssim/ext.cpp (fusedssim, fusedssim_backward) and submodules/simple-knn/ext.cpp (distCUDA2).
 * "DGR/" = submodules/diff-gaussian-rasterization-h36m/.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer into caller-owned, contiguous fp32 / int32 storage unless marked HOST;
 *    NULL means "not provided" (the reference uses data<float>() of an empty CPU tensor for that,
 *    DGR/diff_gaussian_rasterization_h36m/__init__.py:184-194);
 *  - the library never allocates, frees or synchronises; all work is enqueued on `stream`
 *    (a hipStream_t passed as void*), so calls are capturable into hipGraphs;
 *  - V views that share the Gaussian parameters and the image size are processed by ONE launch sequence
 *    (the reference renders one view per call; its loop, train.py:130-222, keeps the parameters fixed for
 *    `accumulation_steps` consecutive views, which is what makes the batch legal);
 *  - matrices are the reference's transposed 4x4 (row-major memory == column-major matrix), 16 floats per view;
 *  - return value: 0 ok, <0 invalid argument, >0 hipError_t; text via sks_last_error() (thread-local).
 */
#ifndef SKELSPLAT_HIP_H
#define SKELSPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKS_MAX_VIEWS 64      /* views per call */
#define SKS_MAX_CHANNELS 32   /* feature channels (reference: NUM_CHANNELS 15 / 17 / 19, config.h:15) */
#define SKS_SMALL_P 256       /* P <= SKS_SMALL_P: fused per-band path, no global binning */

/* flags */
#define SKS_ANTIALIASING 1u   /* raster_settings.antialiasing */
#define SKS_CLAMP01      2u   /* fold gaussian_renderer's rendered_image.clamp(0,1) (gaussian_renderer/__init__.py:129)
                                 into the forward store and its pass-through mask into the backward */
#define SKS_FORCE_BINNED 4u   /* use the binned (large-P) path even when P <= SKS_SMALL_P (tests) */
#define SKS_DEBUG_SYNC   8u   /* raster_settings.debug: hipStreamSynchronize + error check after each stage
                                 (CHECK_CUDA, DGR/cuda_rasterizer/auxiliary.h:178-185) */

#define SKS_NO_NT_STORES 16u  /* tuning: plain instead of non-temporal stores for the dense forward planes.  Non-temporal (the
                                 default) streams past the 256 MB Infinity Cache at the rate HBM takes writes; plain stores may
                                 stay in it: faster where a call rewrites the same ~cache-sized output step after step and
                                 nothing runs beside it (H36M: 46.5 -> 38-41 us), 40 % slower on outputs many times the cache.
                                 No result bit depends on it (rasterizer.tune_forward / Workspace.tune time the fill configurations) */

/* tuning: bits 8..15 of `flags` = 4 KB passes per fill block of the fused forward (0 = automatic) */
#define SKS_RAW_PARAMS   32u   /* opacities / scales / rotations are the LEAF parameters (_opacity logits, _scaling
                                 log-scales, raw _rotation); sigmoid / exp / normalize (scene/gaussian_model.py:39-47)
                                 run inside the kernels (sks_geometry, sks_forward, sks_backward*) */
#define SKS_RAW_GRADS    128u   /* sks_backward with SKS_RAW_PARAMS: dL_dopacity / dL_dscales / dL_drotations are the gradients of the
                                  LEAF parameters (the activation Jacobians applied here) instead of those of the activated ones */
#define SKS_BIN_CLEAN    64u    /* accepted and ignored since sks_version 9: it used to promise that `binning` was as the previous
                                  sks_forward left it (per-tile counters zero again) so that a clearing launch could be skipped.
                                  The binned path no longer accumulates into the buffer -- every counter is written before it is
                                  read -- so a buffer needs no clearing and may hold anything on entry */
/* bits 16..18: binned path (P > SKS_SMALL_P), the views of a call are processed as (value + 1) VIEW GROUPS (at most 7, at most V):
   the binning kernels run once for all views, the forward's fill + composite launch and the backward's tile launch once per group.
   No result bit depends on it.  sks_forward_backward uses it to run group g's backward on the second stream while group g + 1's
   forward streams on the first; sks_backward must be given the value its sks_forward had (like every other flag).  A field of
   zero asks for the default: one group, unless the build sets SKS_BIN_FB_GROUPS or the process's SKS_BIN_GROUPS environment
   variable (a tuning sweep; read once) names another count -- the same for every entry point.
   The SMALL path has no view groups and reads the same three bits as the early fill's E (SKS_EARLY_FILL below): a caller that
   passes SKS_BIN_GROUPS(n) whatever P is forces E = (n - 1) sixteenths of the planes on its small-path calls instead of the
   measured default -- the same bits in the results, possibly a few microseconds slower. */
#define SKS_BIN_GROUPS_SHIFT 16
#define SKS_BIN_GROUPS(n) ((unsigned)(((n) - 1) & 7) << SKS_BIN_GROUPS_SHIFT)
#define SKS_FILL_LINEAR (1u << 21)  /* tuning/tests: forward fill blocks always in linear (pass-major) mode */
#define SKS_FILL_ROWS (1u << 22)    /* tuning/tests: row-aligned fill blocks whenever W % 4 == 0 */
/* bits 26..29: tuning, composite blocks per (view, Gaussian) of the small-path forward (0 = default 4) */
#define SKS_BWD_LDS_LIST (1u << 20) /* tests: use the LDS-list backward even when P <= 64 (default: wave-resident) */
/* bits 23..25: tuning/tests, workgroups per (view, Gaussian) of the wave-resident backward = 16 >> (value - 1)
   (0 = automatic: 16 for a few views, fewer and longer ones when V x P is large; the results do not depend on it) */
#define SKS_BWD_WG_SHIFT 23
/* Small path, plain sks_forward with cover rows and no debug planes: the geometry launch also zeroes the call's LAST E (view, plane)
   planes, whole, with nothing in front of its stores (k_geom_fwd_fill), and the fill + composite launch behind it streams the rest and
   stores every covered tile, the early planes' included ("Early fill").  No result bit depends on either of the two: */
#define SKS_NO_EARLY_FILL (1u << 30)   /* tuning/tests: the geometry launch fills nothing, the fill + composite launch streams every plane */
/* tuning/tests, E: on the small path, which has no view groups, the three bits 16..18 (SKS_BIN_GROUPS_SHIFT) are E's field:
   0 = automatic (the rule in sks_raster.hip, early_fill_planes); n = 1..6: n sixteenths of the (C + 1) * V planes, rounded up;
   7: every plane.  Ignored where the early fill is not used (the cases above, sks_forward_backward, SKS_DEBUG_SYNC, row-aligned
   fill blocks).  Bits 19 and 31 stay free. */
#define SKS_EARLY_FILL(n) (((unsigned)(n) & 7u) << SKS_BIN_GROUPS_SHIFT)

const char* sks_last_error(void);
int sks_version(void);

/* Scratch sizes in bytes for one call (replaces the resizeFunctional callbacks, DGR/rasterize_points.cu:27-33).
 * geom: per-view per-Gaussian records kept for backward ("geomBuffer");
 * binning: the binned path's state ("binningBuffer" + "imgBuffer" of the reference), only used when P > SKS_SMALL_P or with
 *          SKS_FORCE_BINNED; bin_capacity = max (Gaussian, tile) pairs per view it must hold.  Since sks_version 8 it holds, per
 *          view: 48 B of entry records + 64 B of backward rows per pair of capacity (128 B in version 6), per 16x16 tile 2 KB of
 *          {final T, last contributor} for the backward + counters, range, descriptors, channel mask (~160 B) and a few KB of
 *          per-plane cover rows, per Gaussian 8 B -- e.g.
 *          0.65 GB for 8 views at 2048x2048 with a capacity of 400 000 pairs.  Sizes and layout are private to a library version:
 *          always ask the library that will be called;
 * accum:  backward partial-sum slots (plain scratch: no initialisation needed, contents undefined afterwards). */
int sks_scratch_bytes(int V, int P, int C, int W, int H, size_t bin_capacity,
                      size_t* geom_bytes, size_t* binning_bytes, size_t* accum_bytes);

/* Which launch forms a call of this shape takes (added to sks_version 14).  Host only, no GPU call: the answer comes from the
 * functions the launchers themselves call, so a test can assert that a shape reaches the branch it was chosen for and fails loudly
 * when a threshold is retuned.  out: SKS_REGIME_INTS ints, indexed by the names below.  flags as for sks_forward; out_aligned128:
 * non-zero = out_color and out_invdepth are 128-byte aligned (every torch allocation is), 0 = only 16-byte aligned.
 * Images beyond the limits of every entry point (W <= 65536, H <= 1048560, V <= SKS_MAX_VIEWS, C <= SKS_MAX_CHANNELS) are
 * refused here with the same error. */
#define SKS_REGIME_PATH        0   /* 0 = small path, 1 = binned path */
#define SKS_REGIME_COVER       1   /* cover rows of the forward's fill role: 0 = none (the rects are tested directly), 1 = a row per
                                      (view, band), 2 = a row per (view, plane, band) */
#define SKS_REGIME_CW          2   /* words per cover row */
#define SKS_REGIME_PPT         3   /* pixels per lane of a fill pass: 4 (16-byte stores) or 1 */
#define SKS_REGIME_HALF        4   /* 1 = a 16-byte store is two independently masked pairs (W % 4 == 2, even H) */
#define SKS_REGIME_ROWMODE     5   /* 1 = row-aligned fill blocks, 0 = linear passes */
#define SKS_REGIME_PB          6   /* passes per fill block (linear) or rows per fill block (row-aligned) */
#define SKS_REGIME_FSPLIT      7   /* fill blocks per (plane, band) */
#define SKS_REGIME_W_MAGIC     8   /* 1 = pixel index % W as a multiply-high in the fill blocks, 0 = plain % */
#define SKS_REGIME_BWD         9   /* compositing backward: 0 = wave-resident, 1 = LDS-list gather, 2 = per tile (binned path) */
#define SKS_REGIME_GX         10   /* tile columns */
#define SKS_REGIME_GY         11   /* tile rows (bands) */
#define SKS_REGIME_BPC        12   /* binned path: tile bands per block of the scan launch (0 on the small path) */
#define SKS_REGIME_WAVE_GROUPS 13  /* wave-resident backward: workgroups per (view, Gaussian) (0 elsewhere) */
#define SKS_REGIME_LEAD       14   /* 31 = a band's first fill pass is a short one that ends on a 128-byte line (outputs, plane or band
                                      stride not whole lines), 0 = every pass is whole lines */
#define SKS_REGIME_INTS       16
int sks_launch_regime(int V, int P, int C, int W, int H, unsigned flags, int out_aligned128, int* out);

/* The list lengths at which the binned path changes how it orders or walks a tile's list.  Host only, no GPU call, like
 * sks_launch_regime: the values are the kernels' own constants, so a test can place a list on either side of each and fails loudly
 * when one is retuned.  out: SKS_LIST_REGIME_INTS ints, indexed by the names below. */
#define SKS_LIST_WAVE_SORT     0   /* lists up to this many entries are ranked by the forward's wavefront as it loads them */
#define SKS_LIST_WAVE_K        1   /* ... up to this many: sorted in one wavefront's registers ahead of its compositing */
#define SKS_LIST_SORT_LDS      2   /* ... up to this many: sorted by the scatter workgroup in LDS; longer ones in global memory */
#define SKS_LIST_LONG_LIST     3   /* a band with up to this many lists beyond SKS_LIST_WAVE_K remembers their columns; with more
                                      it finds them again by a walk over all columns */
#define SKS_LIST_CLASSES       4   /* tile classes by list length: class c holds [2^c, 2^(c+1)), the last one the rest */
#define SKS_LIST_BAND_THREADS  5   /* threads of the workgroup that scatters a band and sorts its long lists */
#define SKS_LIST_REGIME_INTS   8
int sks_list_regime(int* out);

/* Replaces _C.rasterize_gaussians (DGR/rasterize_points.cu:35-124 -> rasterizer_impl.cu:198-341).
 * features: (P,C) -- the reference reads them from `sh` with M == 1.
 * Outputs: out_color (V,C,H,W), out_invdepth (V,1,H,W), radii (V,P); every element is written
 * (no pre-zeroing needed) -- on the small path by two launches back to back, the geometry launch, which also zeroes the call's last
 * few planes (SKS_NO_EARLY_FILL: it fills nothing), and the fill + composite launch; the outputs are complete in `stream` order
 * behind the second.  out_color / out_invdepth must be 16-byte aligned (refused otherwise); 128-byte aligned
 * buffers -- every torch allocation is -- take the fastest fill (whole cache lines per pass).  Optional debug outputs final_T (V,H,W) / n_contrib (V,H,W) reproduce the
 * reference's ImageState (rasterizer_impl.h:52-60) for parity tests; pass NULL on the fast path.
 * num_rendered_dev (V ints, may be NULL): number of (Gaussian,tile) pairs, written on the binned path. */
int sks_forward(int V, int P, int C, int W, int H,
                const float* viewmatrix, const float* projmatrix,
                const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/,
                const float* means3D, const float* features, const float* opacities,
                const float* scales, const float* rotations, const float* cov3D_precomp,
                float scale_modifier, unsigned flags,
                float* out_color, float* out_invdepth, int* radii,
                void* geom, void* binning, size_t bin_capacity, int* num_rendered_dev,
                float* final_T, uint32_t* n_contrib, void* stream);

/* Replaces _C.rasterize_gaussians_backward (DGR/rasterize_points.cu:126-223 -> rasterizer_impl.cu:345-450).
 * geom / binning are the buffers sks_forward filled for the same inputs.  bg: C floats or NULL (zeros).
 * dL_dout_invdepth may be NULL (treated as zeros; the reference always receives a materialised zero grad, Q4).
 * Per-view gradients (V,P,...): dL_dmeans3D 3, dL_dmeans2D 3 (z = 0), dL_dopacity 1, dL_dscales 3, dL_drotations 4,
 * dL_dcov3D 6; dL_dfeatures (V,P,C) only when non-NULL (true dL/dfeature, SURVEY quirk Q5 is NOT reproduced).
 * dL_dscales / dL_drotations may be NULL when cov3D_precomp is given. */
int sks_backward(int V, int P, int C, int W, int H,
                 const float* viewmatrix, const float* projmatrix,
                 const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/,
                 const float* bg,
                 const float* means3D, const float* features, const float* opacities,
                 const float* scales, const float* rotations, const float* cov3D_precomp,
                 float scale_modifier, unsigned flags,
                 const int* radii, const void* geom, const void* binning, size_t bin_capacity,
                 const float* dL_dout_color, const float* dL_dout_invdepth,
                 void* accum,
                 float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dopacity,
                 float* dL_dscales, float* dL_drotations, float* dL_dcov3D, float* dL_dfeatures,
                 float* dL_dmeans3D_mean /* optional (P,3): the mean of dL_dmeans3D over the V views, summed in view order --
                 what the reference's loop forms right after the backward (xyz.grad = accumulated_grads.mean(dim=0),
                 train.py:215-217); for V * P <= 256 it comes out of the same launch as the geometry backward */,
                 void* stream);

/* Prefill (added to sks_version 14): the small-path backward zeroes planes for the NEXT forward.  A two-call step -- sks_forward,
 * a loss that reads the image, sks_backward -- leaves HBM idle for the backward's two latency-bound launches (the compositing
 * backward k_render_bwd_wave and the geometry backward k_geom_bwd_all), and a step's only mandatory bytes that do not depend on its
 * own inputs are the zeros of the forward's output.  A caller that keeps TWO output sets and alternates between them lets the
 * backward of step N write zeros over the last planes of the set step N + 1 renders into (the image of step N, in the other set,
 * stays the caller's):
 *
 *  sks_prefill_planes: host only.  The rule: how many whole planes the compositing backward's launch (planes_wave) and the geometry
 *  backward's launch (planes_geom) should carry for this call -- a function of the call (V, P, the image size, flags), 0 / 0 where
 *  there is no prefill: off the wave-resident small path (P > 64, SKS_FORCE_BINNED), without 16-byte stores (they need W % 4 == 0, or
 *  W % 4 == 2 with an even H), with SKS_NO_NT_STORES or SKS_DEBUG_SYNC -- and outside what its constants were measured on (the H36M
 *  step): V * P outside 51 .. 85, C > 20, W % 4 != 0.  A caller that also asks for dL_dfeatures should not prefill either.  Together with the forward's own early region
 *  (SKS_EARLY_FILL) never more than half of the (C + 1) * V planes.
 *
 *  sks_backward_prefill: sks_backward, bit for bit, whose launches also store 0.0f over the LAST planes_wave + planes_geom planes
 *  of the set (next_color (V,C,H,W), next_invdepth (V,1,H,W)), in the plane order view-major, a view's C colour planes then its
 *  inverse depth -- whole planes, non-temporal 16-byte stores, in blocks that run behind the launches' own (extra blockIdx.z layers
 *  of k_render_bwd_wave, blocks 1.. of k_geom_bwd_all) and leave before any load or barrier.  Nothing else of the set is touched.  The
 *  geometry backward's share rides in its launch when that is k_geom_bwd_all (dL_dmeans3D_mean given and V * P <= 256) and in the
 *  compositing launch otherwise.  Both counts 0: exactly sks_backward (the set may be NULL).  Counts the call cannot carry are
 *  refused, not ignored: off the wave-resident small path, without 16-byte stores, with SKS_DEBUG_SYNC (SKS_NO_NT_STORES in ITS flags
 *  is ignored: that is the forward's store kind).  Any count on any other shape is carried, also where the rule answers 0 / 0.  The zeros are complete in `stream` order behind the call.
 *
 *  sks_forward_prefilled: sks_forward told that the LAST prefilled_planes planes of (out_color, out_invdepth) are zero already
 *  -- written by nothing since an sks_backward_prefill of at least that many planes ordered before this call on `stream` (or by
 *  anything else that left them 0.0f).  The fill + composite launch then streams the planes in front of them only (the geometry
 *  launch's early region sits right in front of the prefilled one) and the composite blocks store their tiles on every plane, as
 *  ever: the outputs are bit for bit those of sks_forward.  0: exactly sks_forward.  The promise is IGNORED -- every plane is
 *  filled -- with final_T / n_contrib, with SKS_DEBUG_SYNC, off the small path, and for a launch that the measurement hook samples
 *  without having bracketed the backward in front of it (below).  sks_forward_backward neither prefills nor takes a promise. */
int sks_prefill_planes(int V, int P, int C, int W, int H, unsigned flags, int* planes_wave, int* planes_geom);
int sks_forward_prefilled(int V, int P, int C, int W, int H,
                          const float* viewmatrix, const float* projmatrix,
                          const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/,
                          const float* means3D, const float* features, const float* opacities,
                          const float* scales, const float* rotations, const float* cov3D_precomp,
                          float scale_modifier, unsigned flags,
                          float* out_color, float* out_invdepth, int* radii,
                          void* geom, void* binning, size_t bin_capacity, int* num_rendered_dev,
                          float* final_T, uint32_t* n_contrib, int prefilled_planes, void* stream);
int sks_backward_prefill(int V, int P, int C, int W, int H,
                         const float* viewmatrix, const float* projmatrix,
                         const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/,
                         const float* bg,
                         const float* means3D, const float* features, const float* opacities,
                         const float* scales, const float* rotations, const float* cov3D_precomp,
                         float scale_modifier, unsigned flags,
                         const int* radii, const void* geom, const void* binning, size_t bin_capacity,
                         const float* dL_dout_color, const float* dL_dout_invdepth,
                         void* accum,
                         float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dopacity,
                         float* dL_dscales, float* dL_drotations, float* dL_dcov3D, float* dL_dfeatures,
                         float* dL_dmeans3D_mean,
                         float* next_color, float* next_invdepth, int planes_wave, int planes_geom, void* stream);

/* sks_forward + sks_backward of the same inputs as ONE call, for a caller whose upstream gradient does not depend on the image
 * this call renders (dL_dout_color / dL_dout_invdepth complete in `stream` order when the call is made: a known gradient, or the
 * previous evaluation's).  On the small path (P <= SKS_SMALL_P) the backward needs the forward's geometry records, not its image,
 * so with a second stream it runs BESIDE the dense forward instead of behind it: k_geom_fwd on `stream`; the backward's launches on
 * `aux_stream`, ordered behind the geometry kernel by an event; the fill + composite launch on `stream`; `stream` then waits for
 * the backward -- outputs and gradients are the caller's in `stream` order, exactly as after the two separate calls, and bit for
 * bit the same numbers.  The latency-bound backward (a few thousand short workgroups) hides under the HBM-bound forward: the H36M
 * step 67 -> ~57 us.  aux_stream NULL (or == stream, or the binned path, whose backward starts from what the forward's
 * compositor left per pixel, or more than 400 (view, Gaussian) pairs without SKS_FB_NO_JOIN -- there the backward's wavefronts
 * would cost the forward more than they hide: all 31 Panoptic views): the two calls one after the other.  Arguments as for sks_forward (without the two debug outputs)
 * followed by sks_backward's.  On the binned path with a second stream and SKS_BIN_GROUPS(n > 1) in `flags`, view group g's
 * backward runs on aux_stream beside group g + 1's forward (bit-identical; measured SLOWER than the plain sequence on the stress
 * scene, so it is not the default).  The library keeps a handful of hipEvents per host thread for the hand-overs (created by the
 * first combined call of a thread, re-created when the thread moves to another device, never destroyed: process-lifetime objects).
 * After an error behind the hand-over `stream` is made to wait for what aux_stream already holds, whatever fb_flags says.
 * fb_flags: SKS_FB_NO_JOIN = `stream` does NOT wait for the backward at the end: the caller has more to enqueue behind the
 * gradients on aux_stream -- a view-sharded step's collective on the joint gradients, which then also hides under the forward --
 * and makes `stream` wait for aux_stream itself (an event recorded on aux_stream, hipStreamWaitEvent on stream).  With a distinct
 * aux_stream the gradients are ordered on aux_stream on EVERY branch: where the call ran its two halves one after the other on
 * `stream` (P == 0, SKS_DEBUG_SYNC, the binned path in one view group) aux_stream is made to wait for all of it.
 * The view-group count of a binned call is resolved by sks_forward, sks_backward and this call alike: SKS_BIN_GROUPS(n) in `flags`,
 * or, when the field is zero, the build's default (one group) / the SKS_BIN_GROUPS environment variable of a tuning sweep.  One
 * rule in one place rather than a count injected here: a state this call made is then walked by a later sks_backward with the
 * caller's flags group for group as its forward laid it out, and no result bit depends on the count. */
#define SKS_FB_NO_JOIN 1u
int sks_forward_backward(int V, int P, int C, int W, int H,
                         const float* viewmatrix, const float* projmatrix,
                         const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/,
                         const float* means3D, const float* features, const float* opacities,
                         const float* scales, const float* rotations, const float* cov3D_precomp,
                         float scale_modifier, unsigned flags,
                         float* out_color, float* out_invdepth, int* radii,
                         void* geom, void* binning, size_t bin_capacity, int* num_rendered_dev,
                         const float* bg, const float* dL_dout_color, const float* dL_dout_invdepth, void* accum,
                         float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dopacity,
                         float* dL_dscales, float* dL_drotations, float* dL_dcov3D, float* dL_dfeatures,
                         float* dL_dmeans3D_mean, void* stream, void* aux_stream, unsigned fb_flags);

/* xyz.grad = accumulated_grads.mean(dim=0) (train.py:215-217) on its own: mean over the V views of (V,P,3) joint gradients,
 * summed in view order.  shard_world = N > 1: the rows are where all_gather_into_tensor leaves them when view v is local view
 * v / N of rank v % N and every rank contributes ceil(V / N) rows (see sks_loop_adam_step) -- the exchange step of a
 * view-sharded caller is then all_gather + this one launch, with no re-ordering pass in between. */
int sks_mean_views(int V, int P, const float* dL_dmeans3D, int shard_world, float* mean_out /* (P,3) */, void* stream);

/* Replaces _C.mark_visible (DGR/rasterize_points.cu:225-244; checkFrustum rasterizer_impl.cu:54-66).
 * present: P bytes (bool). */
int sks_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

/* Debug / parity: copies the binned path's per-view lists out of `binning` in the reference's layout:
 * point_list (V,bin_capacity) uint32, ranges (V,Tx*Ty,2) uint32 (BinningState / ImageState::ranges). */
int sks_export_lists(int V, int W, int H, const void* binning, size_t bin_capacity,
                     uint32_t* point_list, uint32_t* ranges, void* stream);

/* Fused masked-L2 heat-map loss of the loop (utils/loss_utils.py:86-100 `l2_loss_gaussian`, called at train.py:150
 * on the clamped render; its autograd backward at train.py:161).  Per view v over n_per_view = C*H*W elements:
 *   N_v = #{gt > 0 or render > 0},  S_v = sum over that mask of (render - gt)^2  (loss_v = S_v / N_v),
 *   dL_unscaled = 2 (render - gt) on the mask, 0 elsewhere  (may be NULL: loss only).
 * The true gradient is dL_unscaled / N_v; everything downstream is linear in it, so callers scale the resulting
 * parameter gradients by 1 / N_v instead of re-reading the image.  sums: V x {S_v, N_v} doubles (zeroed by the call). */
int sks_masked_l2(int V, size_t n_per_view, const float* render, const float* gt, float* dL_unscaled, double* sums,
                  void* stream);
/* What sks_masked_l2 launches for views of n_per_view elements: out[0] = workgroups per view, out[1] = threads per workgroup
 * (both 0 for n_per_view == 0, where nothing is launched).  Host only, no GPU call, like sks_launch_regime: from these and n the
 * tests work out which of the kernel's loops a shape reaches (tests/masked_l2_cases.py). */
int sks_masked_l2_launch(size_t n_per_view, int* out /* blocks, threads */);
/* The same as a criterion: additionally loss[v] = S_v / N_v and scale[v] = 1 / N_v (mean != 0; an empty mask gives NaN like the
 * reference's `error[mask].mean()`), or S_v and 1 (mean == 0): what `l2_loss_gaussian(..., reduction="mean" / "sum")` returns
 * and what its backward scales dL_unscaled by -- formed on the device by one more tiny launch instead of five tensor ops. */
int sks_masked_l2_loss(int V, size_t n_per_view, const float* render, const float* gt, float* dL_unscaled, double* sums,
                       float* loss /* V */, float* scale /* V */, int mean, void* stream);

/* The 2D keypoint read out of heat-map planes (utils/loss_utils.py:41-64 `softargmax2d`, which the reference's keypoint criteria
 * l2 / l2_sqrt / huber / cauchy call with beta = 100 on the render).  img: `planes` contiguous (H, W) planes (V * C of them), 4-byte
 * aligned.  Per plane, p = softmax(beta * img) over its H * W pixels:
 *   xy[plane] = {sum p * col, sum p * row} in pixels (the reference's [result_c, result_r]);
 *   stats[plane] = SKS_SOFTARGMAX_STATS floats {m = max img, 1 / sum exp(beta (img - m)), E[col], E[row], and what the floats of
 *   E[col], E[row] miss of the fp64 expectations}: what the backward needs instead of a saved softmax (col - E[col] cancels
 *   where p is largest, so the backward takes the expectations as float pairs).
 * sks_softargmax_fwd: one read of img in two launches (per-chunk partial quadruples into `scratch`, then one wave per plane merges
 *   them in a fixed order): no atomics, bit-identical from run to run.  scratch: sks_softargmax_scratch_bytes(planes, W, H) bytes,
 *   8-byte aligned, contents irrelevant on entry (0 is returned, with the error text set, for sizes the calls below reject).
 * sks_softargmax_bwd: dL_dimg = beta p (dL_dxy[plane][0] (col - E[col]) + dL_dxy[plane][1] (row - E[row])), one read of img and
 *   one write of dL_dimg (planes x H x W, every element written). */
#define SKS_SOFTARGMAX_STATS 6
size_t sks_softargmax_scratch_bytes(int planes, int W, int H);
int sks_softargmax_fwd(int planes, int W, int H, float beta, const float* img, float* xy /* planes x 2 */,
                       float* stats /* planes x SKS_SOFTARGMAX_STATS */, void* scratch, size_t scratch_bytes, void* stream);
int sks_softargmax_bwd(int planes, int W, int H, float beta, const float* img, const float* stats /* planes x SKS_SOFTARGMAX_STATS */,
                       const float* dL_dxy /* planes x 2 */, float* dL_dimg, void* stream);

/* Pseudo-GT heat-maps of a scene (utils/general_utils.py:175-304 generate_heatmaps + normalize_heatmaps).  The
 * reference filters one 255 impulse per joint plane with cupyx gaussian_filter (V*J full-resolution calls) and
 * min-max normalises each plane; the filtered impulse is separable, so a plane is
 *   out[y][x] = (row[y] * col[x] - cmin) / den
 * with row = 255 * (1-D impulse response along y), col = the one along x, cmin = min(row) * min(col) and
 * den = max(row) * max(col) - cmin + 1e-8 (all fp32, in this order).  One pass, one write of (V,J,H,W).
 * row (V,J,H), col (V,J,W), cmin (V,J), den (V,J), out (V,J,H,W).  gt_totals (optional, V x 2 fp64): per view the sum of
 * out^2 and the count of out > 0 over all J planes -- what sks_gt_tile_stats would compute by reading the planes back. */
int sks_heatmaps(int V, int J, int W, int H, const float* row, const float* col, const float* cmin, const float* den,
                 float* out, double* gt_totals, void* stream);
/* The factors themselves, one launch (general_utils.py:189-289): lambda1/lambda2 of each joint's Gaussian in each view
 * by the reference's own transcription of the EWA projection, the scipy-'reflect' truncated (4 sigma) 1-D responses of
 * the 255 impulse at the truncated 2D detection, and the min-max constants.  Reflection rule: on an axis of n samples the
 * impulse at p has the images p + 2nk and -1 - p + 2nk for every integer k, and every image within the truncation radius
 * floor(4 sigma + 0.5) of a sample counts -- the impulse and one mirror per side while radius <= n, further bounces on a
 * coarse image or under a wide Gaussian (any radius is exact; the cost grows with radius / n).  means3D (J,3), scales (J,3) activated,
 * rotations (J,4) raw quaternions, poses_2d (V,J,2) pixel (x, y), viewmatrix (V,16) as for sks_forward,
 * tanfovx/tanfovy HOST arrays of V.
 * A plane (view, joint) DRAWS NO IMPULSE -- row = col = +0 over the view's own H and W, cmin = 0, den = 1e-8f, nothing written
 * beyond the view's size -- when (a) a lambda or a coordinate of the detection is not finite (a NaN or infinite mean gives NaN
 * lambdas), (b) !(lambda1 > 0) || !(lambda2 > 0) (lambda2 = mid - sqrt(max(mid^2 - det, 0.1)) reaches about -0.016 for a
 * footprint whose trace is below 0.032 px^2, and exactly +0), or (c) on either axis floor(4.0 * (double)sqrtf(lambda) + 0.5) >
 * SKS_HEATMAP_MAX_RADIUS.  One degenerate axis makes the whole plane the no-impulse plane; every other plane is untouched.  (c)
 * bounds the launch: per thread at most SKS_HEATMAP_MAX_RADIUS / 256 + 4 * ceil(n / 256) * (SKS_HEATMAP_MAX_RADIUS / 2n + 1) + 3 *
 * ceil(n / 256) double-precision exp on an axis of n samples.  sks_view_footprints reports the raw lambdas the rule is applied to. */
#define SKS_HEATMAP_MAX_RADIUS 262144   /* 2^18: 64 x the widest image in use; an axis of <= 4100 samples under such a kernel is flat
                                           to an fp32 ulp */
int sks_heatmap_factors(int V, int J, int W, int H, const float* means3D, const float* scales, const float* rotations,
                        float scale_modifier, const float* poses_2d, const float* viewmatrix, const float* tanfovx,
                        const float* tanfovy, float* row, float* col, float* cmin, float* den,
                        int frames /* 1; > 1: V = frames x Vf views, parameters stacked (frames,J,..), see sks_loop_fused_step */,
                        const int* view_wh /* HOST V x {W,H} or NULL: per-view sizes; row / col keep the strides H / W */,
                        void* stream);
/* {sum gt^2, count gt > 0} per view (gt_totals, V x 2 fp64) of heat-maps that are NEVER WRITTEN: computed from the
 * separable factors alone (strides H / W, per-view sizes view_wh or NULL).  Together with hm_factors of
 * sks_backward_fused_loss / sks_loop_fused_step this replaces sks_heatmaps + the (V,J,H,W) planes on the sparse path. */
int sks_heatmap_totals(int V, int J, int W, int H, const float* row, const float* col, const float* cmin, const float* den,
                       const int* view_wh, double* gt_totals, void* stream);

/* Initial joints of N frames by linear (DLT) triangulation, one launch (reference: triangulation.py:122-150).  Per (frame,
 * joint) the 2V x 4 homogeneous system with the rows x * P[2] - P[0] and y * P[2] - P[1] of every view, view-major; the result
 * is the right singular vector of the smallest singular value divided by its fourth component, in float64, by one-sided Jacobi
 * on the columns of the system itself (no normal equations).  Since sks_version 13.
 * proj: DOUBLE (V,3,4), K [R|t] per view, with rig_stride = 0 -- or one rig per frame, (N,V,3,4), with rig_stride = V * 12;
 * the detections (N,V,J,2), pixel x, y: as float (poses_2d) or as double (poses_2d_f64), exactly one of the two;
 * valid: optional (N,V,J) bytes, 0 = leave this detection out (NULL: all enter);
 * outputs, at least one of the first two: xyz (N,J,3) float -- what the loop consumes, xyzw rounded to nearest --, xyzw (N,J,4)
 * double, homogeneous with w == 1 as the reference returns, n_used (N,J) = detections that entered the system.  A joint with
 * n_used < 2 has no solution: its xyz / xyzw are NaN.  1 <= V <= SKS_MAX_VIEWS.  A frame's result does not depend on N, on its
 * place in the batch or on the stream. */
int sks_triangulate(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_2d,
                    const double* poses_2d_f64, const unsigned char* valid, float* xyz, double* xyzw, int* n_used,
                    void* stream);

/* sks_triangulate with outlier rejection: exhaustive two-view consensus (the deterministic form of RANSAC) in front of the
 * same DLT, two launches on `stream`, nothing synchronises, no atomics, no scratch.  Added to sks_version 14: the number did
 * not move (a caller that must know looks the symbol up).  Per (frame, joint), in float64, with K = the views kept by `valid`
 * (all when NULL):  |K| < 2: no solution, NaN, inliers = K, n_consensus = |K|.  |K| == 2: nothing can be tested, the DLT of the
 * two, inliers = K, n_consensus = 2.  |K| >= 3: every pair a < b of K, in lexicographic order, is a hypothesis X_ab = the DLT
 * of the four rows of views a and b, normalised to w = 1; view v of K is its inlier iff, with u = P_v X_ab, u[2] > 0 and
 * e_v = hypot(u[0] / u[2] - x_v, u[1] / u[2] - y_v) <= reject_px (comparisons with NaN are false: a NaN or inf detection is
 * never an inlier and a hypothesis built on one has none).  The winner has the most inliers; ties go to the smallest sum of the
 * inliers' e_v (added in ascending view order), then to the first pair.  inliers = the winner's set if it has at least
 * min_inliers views, else K (no consensus: the result of sks_triangulate); n_consensus = the winner's count in both cases, so
 * n_consensus < min_inliers marks the fallback.  The joint is then the DLT over `inliers` by k_triangulate itself, bit for bit
 * sks_triangulate(valid = inliers): one refit, no second inlier pass, no re-weighting; n_used = the views in `inliers`.
 * Arguments and refusals of sks_triangulate, and: reject_px finite and > 0 (pixels), 2 <= min_inliers <= SKS_MAX_VIEWS,
 * inliers (N,V,J) bytes REQUIRED (the refit reads it; it may not alias `valid`), n_consensus (N,J) optional.  A joint's outputs
 * depend on V and its own inputs only, never on N, on its place in the batch or on the stream. */
int sks_triangulate_robust(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_2d,
                           const double* poses_2d_f64, const unsigned char* valid, double reject_px, int min_inliers,
                           unsigned char* inliers, int* n_consensus, float* xyz, double* xyzw, int* n_used, void* stream);

/* Initial joints of N frames as the reprojection-error-weighted mean of the V views' monocular 3D predictions, one launch
 * (reference: compute_weighted_average_pose, dataset_tools/h36m/compute_initial_guess.py:23-116 and dataset_tools/panoptic/
 * compute_initial_guess_panoptic.py:23-117 -- the configs' initial_guess "metrabs" / "metrabs_occ_3").  Per (frame, joint), with
 * candidate X_i = view i's prediction: u_ic = the pixel of P_c [X_i; 1] (no test for points behind a camera), e_ic = |u_ic - x_c|,
 * ebar_i = mean over c, w_i = (1 / ebar_i) / sum_k (1 / ebar_k), result = sum_i w_i X_i / sum_i w_i.  Added to sks_version 14: the
 * number did not move (a caller that must know looks the symbol up).
 * proj, rig_stride, valid: as sks_triangulate takes them; the predictions (N,V,J,3), world coordinates, as float (poses_3d) or as
 * double (poses_3d_f64), exactly one of the two; the detections (N,V,J,2) likewise; float inputs are widened exactly.
 * valid[n,v,j] == 0 takes view v out of joint j of frame n in both roles: its candidate gets no weight and its detection enters
 * no ebar_i, whose mean then divides by the number of kept views.
 * norm_f32 == 0: everything is float64 (the H36M script).  != 0: u - x is rounded to float32, the norm, the mean over cameras,
 * the reciprocal and the normalisation are float32, the average multiplies the float64 candidates by the float32 weights and
 * accumulates in float64 (the Panoptic script).
 * outputs, at least one of the first two: xyz (N,J,3) float -- what the loop consumes, xyz_f64 rounded to nearest --, xyz_f64
 * (N,J,3) double; optional reproj_err (N,V,J) double = ebar_i (NaN for a view left out), n_used (N,J) = kept views.  A joint with
 * n_used == 0 comes back NaN, with n_used == 1 it is that candidate; ebar_i == 0 follows IEEE as the reference does (inf weight,
 * NaN result).  1 <= V <= SKS_MAX_VIEWS.  The sums over cameras and over candidates run in index order (numpy's order for ebar):
 * a joint's result depends on V and its own inputs only, never on N, on its place in the batch or on the stream. */
int sks_fuse_predictions(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_3d,
                         const double* poses_3d_f64, const float* poses_2d, const double* poses_2d_f64,
                         const unsigned char* valid, int norm_f32, float* xyz, double* xyz_f64, double* reproj_err,
                         int* n_used, void* stream);

/* The reprojection error of joints against the views' detections, measured and minimised (csrc/sks_reproject.hip; reference:
 * compute_reprojection_error, dataset_tools/h36m/compute_initial_guess.py:23-79).  Added to sks_version 14: the number did not
 * move (a caller that must know looks the symbol up).  One launch each on `stream`, nothing synchronises, no atomics, no scratch.
 *
 * sks_reproject: N frames of J joints into V views.  proj, rig_stride, valid: as sks_triangulate takes them; the joints (N,J,3) as
 * float (xyz) or as double (xyz_f64), exactly one of the two; the detections (N,V,J,2) as float (poses_2d) or as double
 * (poses_2d_f64), at most one of the two -- neither: project only, every pair is left out.  Float inputs are widened exactly, the
 * arithmetic is float64: u = P_v [X; 1] added in column order 0..3, uv = (u0 / u2, u1 / u2) with no test for points behind the
 * camera (as the reference), in_front = u2 > 0, err = sqrt(dx * dx + dy * dy) with (dx, dy) = uv - detection.  A pair (v, j) is
 * LEFT OUT when valid == 0, when its detection is not finite or when the joint has a NaN coordinate: its err is NaN (uv and
 * in_front are written all the same).  The means skip every NaN err and are NaN over nothing, each added in a fixed order:
 * per_joint[n,j] over the views in ascending order (all kept: the reference's mean_l2), n_used[n,j] the number of views that
 * entered it; per_view[n,v] over the joints in ascending order; per_frame[n] = (S_0 + S_1 + ..) / (C_0 + C_1 + ..) with S_v, C_v
 * the sum and count of view v as in per_view -- all kept pairs, view-major, grouped by view.
 * outputs, each optional but at least one: uv (N,V,J,2), err (N,V,J), per_joint (N,J), per_view (N,V), per_frame (N) doubles,
 * in_front (N,V,J) bytes, n_used (N,J) ints.  1 <= V <= SKS_MAX_VIEWS.  A frame's outputs depend on its own inputs, V and J only:
 * never on N, on its place in the batch or on the stream.
 *
 * sks_eval_reprojection: the means of err (N,V,J; NaN = left out) over a sequence, shaped after sks_eval_sequence.  out
 * (1 + n_groups, 1 + V + J) doubles: row 0 over all frames, row 1 + g over the frames with group_ids[i] == g (an id outside
 * 0 .. n_groups - 1 enters row 0 only); a row holds the overall mean, then the V per-view and the J per-joint means over the
 * non-NaN entries, NaN where there are none.  Thread t of a row's workgroup takes frames t, t + 256, ... in index order and the
 * 256 partial sums meet in a fixed tree.  0 <= n_groups <= SKS_EVAL_MAX_GROUPS; group_ids (N) ints, NULL with n_groups == 0.
 *
 * sks_triangulate_refine: per (frame, joint) minimises cost(X) = sum over the kept views of rho(e_v), e_v = sks_reproject's err,
 * rho(e) = e * e -- or, with huber_px = d > 0, e * e for e <= d and 2 d e - d * d beyond -- from the start xyz0 by damped
 * Gauss-Newton in float64.  A view is kept when valid != 0 and its detection is finite.  One trip: with J_v the 2 x 3 Jacobian
 * rows (P_v[k,:3] - uv_k * P_v[2,:3]) / u2, r_v = uv - detection and w_v = min(1, d / e_v) (1 without Huber), A = sum w_v J_v^T
 * J_v and g = sum w_v J_v^T r_v (butterfly sums over the next power of two >= V lanes), (A + lambda diag A) delta = -g by
 * Cholesky, trial = X + delta; the trial is ACCEPTED only if its cost is strictly smaller and every kept view has u2 > 0 there
 * (and the Cholesky pivots were > 0).  lambda starts at 1e-3, x 0.1 on acceptance, x 10 on rejection.  A joint stops after an
 * accepted trip that lowered the cost by less than 1e-6 x the cost (scale-free), or after max_iters trips (1 ..
 * SKS_REFINE_MAX_ITERS); iters = its trips, accepted or not.  A joint with fewer than two kept views, with a start that is not
 * finite, or with a kept view that has u2 <= 0 at the start comes back unchanged with iters = 0.
 * proj, rig_stride, valid, the detections: as sks_triangulate takes them; the start (N,J,3) as float (xyz0) or as double
 * (xyz0_f64), exactly one of the two; huber_px finite and >= 0 (0: plain squares).  outputs, at least one of the first two: xyz
 * (N,J,3) float (rounded to nearest; it may be xyz0 itself: in place), xyz_f64 (N,J,3) double; optional cost (N,J,2) doubles =
 * {at the start, at the result} and iters (N,J) ints.  A joint's result depends on V and its own inputs only, never on N, on its
 * place in the batch, on its neighbours in the wavefront or on the stream. */
#define SKS_REFINE_MAX_ITERS 16
int sks_reproject(int N, int V, int J, const double* proj, size_t rig_stride, const float* xyz, const double* xyz_f64,
                  const float* poses_2d, const double* poses_2d_f64, const unsigned char* valid, double* uv, double* err,
                  unsigned char* in_front, double* per_joint, double* per_view, double* per_frame, int* n_used, void* stream);
int sks_eval_reprojection(int N, int V, int J, const double* err, const int* group_ids, int n_groups, double* out, void* stream);
int sks_triangulate_refine(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_2d,
                           const double* poses_2d_f64, const unsigned char* valid, const float* xyz0, const double* xyz0_f64,
                           double huber_px, int max_iters, float* xyz, double* xyz_f64, double* cost, int* iters, void* stream);

/* Covariance-weighted temporal smoothing of a sequence, and the smoothness figures that go with it (csrc/sks_smooth.hip; added to
 * sks_version 14: the number did not move).  The reference optimises every frame on its own; this is the local polynomial fit a
 * consumer of its poses runs afterwards, with every joint's optimised 3x3 covariance (sks_joint_uncertainty's cov6) as the weight
 * of its frame.  What it gains on real sequences depends on how well those covariances are calibrated (sks_calibration) and has
 * NOT been measured.  One launch each on `stream`, nothing synchronises, no atomics, no scratch.  Device memory unless marked HOST.
 *
 * THE FIT (one definition: the kernel, smoothing.smooth_host and tests/smooth_ref.py follow it).  Inputs: xyz (N,J,3) floats;
 * optional cov6 (N,J,6) floats xx, xy, xz, yy, yz, zz; optional weights (N,J) floats; optional valid (N,J) bytes; optional
 * group_ids (N) ints; half_window h, degree d, taper, cov_floor >= 0 (mm^2).  For every target (f, j) the taps are the frames
 * k = max(0, f - h) .. min(N - 1, f + h) in ASCENDING order, t = k - f.  A tap is USABLE when group_ids[k] == group_ids[f],
 * valid[k,j] != 0, xyz[k,j] is finite, weights[k,j] is finite and > 0 (each where given) and, with cov6, the covariance
 * C = cov6[k,j] widened to float64 with cov_floor added to xx, yy, zz has three finite pivots > 0 in this LDL^T (all float64, one
 * rounding per operation, no fused multiply-add anywhere below):
 *     d0 = xx;  l10 = xy / d0;  l20 = xz / d0;  d1 = yy - l10 * xy;  e = yz - l20 * xy;  z1 = zz - l20 * xz;  l21 = e / d1;
 *     d2 = z1 - l21 * e.
 * Its information matrix Lambda = C^-1 (the identity without cov6) is, with i0 = 1 / d0, i1 = 1 / d1, i2 = 1 / d2 and
 * m = l21 * l10 - l20:
 *     xx = (i0 + (l10 * l10) * i1) + (m * m) * i2;  xy = -(l10 * i1) - (m * l21) * i2;  xz = m * i2;
 *     yy = i1 + (l21 * l21) * i2;  yz = -(l21 * i2);  zz = i2.
 * Its weight is omega = w * taper with w = weights[k,j] widened (1 without weights) and taper = 1 (SKS_SMOOTH_BOX) or, with
 * u = |t| / (h + 1) and q = 1 - (u * u) * u, (q * q) * q (SKS_SMOOTH_TRICUBE).  With n usable taps the effective degree is
 * d_eff = min(d, n - 1) and the fit minimises  sum_k omega_k (x_k - sum_i c_i t^i)^T Lambda_k (x_k - sum_i c_i t^i)  over the
 * 3-vectors c_0 .. c_d_eff through its normal equations, formed about x_0 = the FIRST usable tap's position (a difference of two
 * floats is exact in float64).  Per usable tap, in ascending k, starting from zeros:
 *     W = omega * Lambda (six products);  dx = x_k - x_0;  v_r = (W_r0 * dx_0 + W_r1 * dx_1) + W_r2 * dx_2;
 *     t^0 .. t^4 = 1, t, t * t, (t * t) * t, (t * t) * (t * t)  (exact);
 *     M_p = M_p + t^p * W  for p = 0 .. 2d;   r_a = r_a + t^a * v  for a = 0 .. d.
 * The unknowns are ordered c_d_eff, .., c_1, c_0 (the position LAST): B = [M_(2 d_eff - a - b)] in 3x3 blocks a, b = 0 .. d_eff,
 * y = [r_(d_eff - a)], m = 3 (d_eff + 1) rows.  LDL^T in place on the lower triangle, right-looking, the right-hand side with it:
 *     for j = 0 .. m-1:  for i = j+1 .. m-1: l_i = B[i][j] / B[j][j];
 *                        for i = j+1 .. m-1, for c = j+1 .. i: B[i][c] = B[i][c] - l_i * B[c][j]   (B[c][j] still undivided);
 *                        for i = j+1 .. m-1: B[i][j] = l_i, y[i] = y[i] - l_i * y[j];
 *     for j = 0 .. m-1:  y[j] = y[j] / B[j][j];
 *     for j = m-1 .. 1:  for i = 0 .. j-1: y[i] = y[i] - B[j][i] * y[j].
 * c_0 = y[m-3 .. m-1], c_1 = y[m-6 .. m-4].  The trailing 3x3 of the factor is the LDL^T of the position's Schur complement, so the
 * fit's own covariance of the position -- the top-left block of the inverse normal matrix in the order c_0, c_1, .. -- is Lambda's
 * formula above on d0, d1, d2 = B[m-3][m-3], B[m-2][m-2], B[m-1][m-1] and l10, l20, l21 = B[m-2][m-3], B[m-1][m-3], B[m-1][m-2].
 * Outputs, each rounded to float once: joints = c_0 + x_0 (added in float64), velocity = c_1 in mm per frame (0 when d_eff = 0),
 * cov6 as above, n_used = n.  With n = 0 the three float outputs are NaN and n_used is 0.  A joint whose own row is NaN or
 * masked out but has usable taps in its window receives a value: the gap is filled.
 *
 * sks_smooth_sequence: the fit of all N x J targets.  1 <= N <= 2^30, 1 <= J <= SKS_SMOOTH_MAX_JOINTS, 1 <= half_window <=
 *   SKS_SMOOTH_MAX_HALF_WINDOW, 0 <= degree <= 2, cov_floor finite and >= 0; xyz and out_xyz (N,J,3) are required and must not
 *   overlap (a workgroup reads the frames of its neighbours); out_vel (N,J,3), out_cov6 (N,J,6), n_used (N,J) ints are optional.
 *   One (frame, joint) per lane; a workgroup of 256 threads owns a tile of T consecutive frames x all J joints, stages the tile and
 *   half_window halo frames on each side once -- usable?, weight, position and Lambda per staged (frame, joint), 64 bytes, in LDS --
 *   and each lane then walks its own taps in ascending order.  Where T + 2 half_window frames of all joints would not fit 64 KiB
 *   (large J x half_window), the joints are split into equal runs and a workgroup owns T frames of one run.  A target's outputs
 *   depend on its own window only: never on N, on its place in a tile, on the launch shape or on the stream.
 * sks_smooth_launch: HOST only, no GPU call: out[SKS_SMOOTH_TILE] = T, out[SKS_SMOOTH_GROUPS] = the workgroups,
 *   out[SKS_SMOOTH_THREADS] = the threads per workgroup, out[SKS_SMOOTH_LDS_BYTES] = the LDS bytes of a workgroup, for a call of
 *   this N, J and half_window.
 * sks_eval_accel: the sequence's "Accel" and "Accel error" of the video-pose literature.  xyz, gt (N,J,3) floats (gt or NULL),
 *   group_ids (N) ints or NULL, 0 <= n_groups <= SKS_EVAL_MAX_GROUPS (n_groups > 0 needs group_ids; group_ids with n_groups = 0
 *   still fence the frames).  Per joint a_f = (x_(f-1) - 2 * x_f) + x_(f+1) per coordinate in float64, |a| = sqrt((a_0 * a_0 +
 *   a_1 * a_1) + a_2 * a_2); the error is the same norm of a - a_gt.  Frame f (1 .. N-2) of joint j ENTERS the first figure when
 *   its three positions are finite and frames f-1, f, f+1 carry the same group id, the second when the ground truth's three are
 *   finite too.  out (1 + n_groups, 2, 1 + J) doubles: row 0 over all frames, row 1 + g over the frames with group_ids[f] == g;
 *   [.,0,.] the mean |a|, [.,1,.] the mean error (NaN without gt); column 0 over all joints (a frame's joints in index order),
 *   column 1 + j over joint j; NaN where nothing entered.  One workgroup per row: thread t takes frames 1 + t, 1 + t + 256, ... in
 *   index order and the 256 partial sums and counts meet in a fixed tree, so every figure is bitwise the same from run to run. */
#define SKS_SMOOTH_MAX_JOINTS       256
#define SKS_SMOOTH_MAX_HALF_WINDOW  32
#define SKS_SMOOTH_BOX              0
#define SKS_SMOOTH_TRICUBE          1
#define SKS_SMOOTH_TILE       0
#define SKS_SMOOTH_GROUPS     1
#define SKS_SMOOTH_THREADS    2
#define SKS_SMOOTH_LDS_BYTES  3
#define SKS_SMOOTH_LAUNCH_INTS 4
int sks_smooth_sequence(int N, int J, const float* xyz, const float* cov6, const float* weights, const unsigned char* valid,
                        const int* group_ids, int half_window, int degree, int taper, double cov_floor, float* out_xyz,
                        float* out_vel, float* out_cov6, int* n_used, void* stream);
int sks_smooth_launch(int N, int J, int half_window, int* out /*HOST SKS_SMOOTH_LAUNCH_INTS*/);
int sks_eval_accel(int N, int J, const float* xyz, const float* gt, const int* group_ids, int n_groups, double* out, void* stream);

/* Constant limb lengths over a sequence (csrc/sks_bones.hip; added to sks_version 14: the number did not move).  The reference
 * optimises every frame on its own and knows the skeleton only through the left/right symmetry prior of its loss; this is what a
 * consumer of its poses runs afterwards: measure every bone in every frame, take a recording's median lengths, and move every
 * frame onto them with each joint's optimised 3x3 covariance (sks_joint_uncertainty's cov6, or the smoothing's) saying which end
 * of a wrong bone moves, and where to.  WHAT THE FIT IS: a pose that meets the lengths, reached by successive Sigma-closest
 * projections onto the linearised constraints.  It is NOT the Sigma-closest feasible pose (that needs the constraints' curvature
 * and a (3J+B)-sized KKT solve; MEASUREMENTS.md "Constant limb lengths" says how far above it the cost ends), and no covariance
 * of the projected pose is given.  What it gains on real sequences has NOT been measured.  One launch each on `stream`, nothing
 * synchronises, no floating-point atomics, no scratch.  Device memory unless marked HOST.
 *
 * COMMON.  bones: HOST (B,2) ints, (parent, child) joint of bone b; 2 <= J <= SKS_BONES_MAX_JOINTS, 1 <= B <=
 * SKS_BONES_MAX_JOINTS - 1, every index in 0 .. J-1, and the bones must form a FOREST (no cycle, which also rules out a bone from
 * a joint to itself and a repeated pair): checked on the host with a union-find over the bones in index order and refused
 * otherwise -- with it A has full row rank and S below is positive definite.  1 <= N <= 2^26.  groups: (N) ints, the recording of
 * every frame, with 1 <= n_groups <= SKS_BONES_MAX_GROUPS, or NULL with n_groups = 1 (one group, id 0); a frame whose id lies
 * outside 0 .. n_groups-1 enters no group's statistic and is copied by the projection.  An END (a joint of a frame) is USABLE when
 * its three floats are finite and valid[f,j] != 0 (valid (N,J) bytes, optional).  All arithmetic below is IEEE float64, one rounding
 * per operation, no fused multiply-add.  For a symmetric 3x3 M = {xx, xy, xz, yy, yz, zz} and 3-vectors a, b:
 *     M b = w with w_r = (M_r0 * b_0 + M_r1 * b_1) + M_r2 * b_2;      a^T M b = (a_0 * w_0 + a_1 * w_1) + a_2 * w_2.
 *
 * sks_bone_measure: measured (N,B) floats.  Per (frame f, bone b = (p, c)), coordinates widened to float64:
 *     d_k = x_c,k - x_p,k (k = x, y, z);  n = sqrt((d_0 * d_0 + d_1 * d_1) + d_2 * d_2);  measured[f,b] = (float)n.
 *   NaN when an end is not usable.  With cov6 ((N,J,6) floats; then max_sigma_mm must be finite and >= 0): u_k = d_k / n,
 *   Sigma = cov6[f,p] + cov6[f,c] entry by entry (widened), var = u^T Sigma u as above, and the measure is NaN unless
 *   var <= max_sigma_mm * max_sigma_mm (a NaN variance -- a non-finite covariance, n = 0 -- leaves the frame out).  cov6 NULL: no
 *   gate, max_sigma_mm is not read.  One lane per (frame, bone).
 * sks_bone_lengths: per (group g, bone b) the lower median and the MAD of the group's measures.  A measure is USABLE when it is
 *   finite and its sign bit is clear (sks_bone_measure writes nothing else except NaN and, on float overflow, +inf).  With n
 *   usable measures in the group and k = (n - 1) / 2 (integer division): length[g,b] = the k-th smallest (0-based) of them;
 *   mad[g,b] = the k-th smallest of |l - length[g,b]| over the same measures, the subtraction and the absolute value in FLOAT32;
 *   n_used[g,b] = n.  n = 0: NaN, NaN, 0.  Both are SELECTED by integer counts (an MSB-first radix select over the bit patterns,
 *   eight bits a pass, a 256-bin histogram in LDS filled by integer atomics; one workgroup of 256 threads per (group, bone), a
 *   group longer than 256 frames takes several trips per pass), so each is one of the inputs resp. one of the float32 deviations,
 *   exactly, whatever the order the frames are counted in.  length, mad (n_groups,B) floats, n_used (n_groups,B) ints.
 * sks_bone_project: per frame, from its joints y (widened) and the lengths L_b = (double)lengths[g,b] of its group g, the iterate
 *   x starts at y.  Sigma_j = the identity without cov6, else cov6[f,j] widened with cov_floor (finite, >= 0, mm^2) added to xx,
 *   yy, zz.  A joint is FIT when it is usable and, with cov6, its six entries of Sigma_j are finite and the three pivots of
 *   Sigma_j's LDL^T (sks_smooth_sequence's sequence above: d0, l10, l20, d1, e, z1, l21, d2) are finite and > 0.  Bone b is
 *   ACTIVE when both ends are fit, L_b is finite and > 0 and its frame's group id is in range; it turns inactive for the rest of
 *   the frame at the first trip that finds n_b == 0.  One TRIP, at most max_iters (1 .. SKS_BONES_MAX_ITERS) of them:
 *     1. per active bone b = (p, c):  d = x_c - x_p;  n_b = sqrt((d_0 * d_0 + d_1 * d_1) + d_2 * d_2);  n_b == 0: inactive, else
 *        u_b = d / n_b (three divisions) and r_b = n_b - L_b.  rho = the largest of |r_b| over the active bones (+inf for an
 *        r_b that is not finite), n_active = their number.  n_active == 0: the frame ENDS and keeps the rho of the trip before (NaN at the first).
 *        rho <= tol_mm (finite, >= 0) or max_iters trips done: the frame ENDS.  This test is the same in every lane of the
 *        wavefront.
 *     2. S (B x B, lower triangle): for a >= b, both active, starting from s = 0 and in this order:  if p_a == p_b:
 *        s = s + u_a^T Sigma_(p_a) u_b;  if p_a == c_b: s = s - u_a^T Sigma_(p_a) u_b;  if c_a == p_b: s = s - u_a^T Sigma_(c_a) u_b;
 *        if c_a == c_b: s = s + u_a^T Sigma_(c_a) u_b  (row a of A holds +u_a at c_a and -u_a at p_a; the diagonal is the same
 *        rule with a == b).  An inactive bone's row and column are the identity's (1 on the diagonal, 0 elsewhere) and its
 *        right-hand side is 0; y_b = r_b for an active one.
 *     3. LDL^T of S in place on the lower triangle with the right-hand side, then the two substitutions: sks_smooth_sequence's
 *        three loops above with m = B.  A pivot S[j][j] that is not finite and > 0 when step j reads it ENDS the frame at the
 *        current x (it cannot happen in exact arithmetic).  lambda = y.
 *     4. per joint j, g = (0, 0, 0), then over the ACTIVE bones b = 0 .. B-1 in index order:  if c_b == j: g_k = g_k + lambda_b *
 *        u_b,k;  if p_b == j: g_k = g_k - lambda_b * u_b,k.  A joint no active bone touches is left alone; any other:
 *        x_j,k = x_j,k - ((Sigma_j,k0 * g_0 + Sigma_j,k1 * g_1) + Sigma_j,k2 * g_2).
 *   This is x <- x - Sigma A^T (A Sigma A^T)^-1 (n(x) - L): the Sigma-metric closest point to x on the constraints linearised at
 *   x.  (The trip that re-solves from y each time is the textbook SQP step without curvature; it does not converge once the
 *   covariances are needles: DESIGN.md "Constant limb lengths".)  Outputs: out_xyz (N,J,3) floats, must not overlap xyz: a joint
 *   that step 4 moved at least once is (float)x_j, every other joint is its input BIT FOR BIT (NaN payloads included; DESIGN.md
 *   "Unobserved joints"), so a frame with no active bone is a copy; residual (N) floats = (float) of the last rho computed, NaN when no
 *   bone was ever active; n_trips (N) ints = the trips that moved the frame (0 .. max_iters); n_active (N) ints at the
 *   end.  A frame CONVERGED when residual <= tol_mm.  A bone that turns inactive at a trip after the first has already moved its
 *   ends: the bit-for-bit promise holds for joints whose bones were inactive from the start, the only case input data can reach
 *   by construction (coincident joints, NaN, masks, bad covariances, bad lengths).  One wavefront (a workgroup of 64 threads)
 *   per frame; x, Sigma, u, S and y live in LDS; lane b owns bone b and row b, lane j joint j.
 * sks_bones_launch: HOST only, no GPU call: the workgroups, threads per workgroup and LDS bytes per workgroup of the three launches
 *   for a call of this N, J, B and n_groups, at the SKS_BONES_* indices below (the measure uses no LDS). */
#define SKS_BONES_MAX_JOINTS   32
#define SKS_BONES_MAX_GROUPS   256
#define SKS_BONES_MAX_ITERS    16
#define SKS_BONES_MEASURE_GROUPS     0
#define SKS_BONES_MEASURE_THREADS    1
#define SKS_BONES_LENGTHS_GROUPS     2
#define SKS_BONES_LENGTHS_THREADS    3
#define SKS_BONES_LENGTHS_LDS_BYTES  4
#define SKS_BONES_PROJECT_GROUPS     5
#define SKS_BONES_PROJECT_THREADS    6
#define SKS_BONES_PROJECT_LDS_BYTES  7
#define SKS_BONES_LAUNCH_INTS        8
int sks_bone_measure(int N, int J, int B, const int* bones /*HOST (B,2)*/, const float* xyz, const float* cov6,
                     const unsigned char* valid, double max_sigma_mm, float* measured, void* stream);
int sks_bone_lengths(int N, int B, const float* measured, const int* groups, int n_groups, float* length, float* mad, int* n_used,
                     void* stream);
int sks_bone_project(int N, int J, int B, const int* bones /*HOST (B,2)*/, const float* xyz, const float* cov6,
                     const unsigned char* valid, const int* groups, int n_groups, const float* lengths, double cov_floor,
                     int max_iters, double tol_mm, float* out_xyz, float* residual, int* n_trips, int* n_active, void* stream);
int sks_bones_launch(int N, int J, int B, int n_groups, int* out /*HOST SKS_BONES_LAUNCH_INTS*/);

/* People (csrc/sks_people.hip; added to sks_version 14: the number did not move).  A 2D detector returns an unordered list of
 * skeletons per image; every other pose entry point takes (N,V,J,2), one person whose detections are already matched across the
 * views.  These two put several people in front of them: ASSOCIATION decides per frame which detections of different views show
 * the same person, TRACKING decides over the frames which person of frame t is which person of frame t-1.  One launch each on
 * `stream` (tracking: a memset in front of it), nothing synchronises, no global atomics, no floating-point atomics, no scratch.
 * Device memory unless marked HOST.  All arithmetic below is IEEE float64 (inputs widened), one rounding per operation, no fused
 * multiply-add, IEEE division and square root.
 *
 * sks_associate_people.  detections (N,V,M,J,2), pixel x, y of up to M candidate skeletons per view in arbitrary slot order, as
 *   float (detections) or double (detections_f64), exactly one; valid optional (N,V,M,J) bytes, 0 = this joint of this candidate is
 *   not KEPT (NULL: all kept); proj, rig_stride: as sks_triangulate takes them.  1 <= V <= SKS_MAX_VIEWS, 1 <= M <=
 *   SKS_PEOPLE_MAX_SLOTS, D = V * M <= SKS_PEOPLE_MAX_DETS, 1 <= J <= SKS_MAX_CHANNELS, 1 <= K <= SKS_PEOPLE_MAX, max_px finite and
 *   >= 0, 1 <= min_joints <= J, 2 <= min_views <= SKS_MAX_VIEWS; anything else is refused on the host.  Detection a = v * M + m.
 *   FUNDAMENTAL MATRIX of views va < vb, from the two 3x4 matrices alone (Hartley & Zisserman 17.3; no pseudo-inverse, no SVD, no
 *   square root).  For a view's matrix P and i = 0, 1, 2 let r0 < r1 be the two rows other than i and
 *       m(P,i) = (m01, m02, m03, m12, m13, m23),  m_pq = r0[p] * r1[q] - r0[q] * r1[p].
 *   With A = m(P_va, i) and B = m(P_vb, j), the 4x4 determinant of [P_va without row i; P_vb without row j] is expanded along its
 *   first two rows in this order:
 *       det = ((((A01 * B23 - A02 * B13) + A03 * B12) + A12 * B03) - A13 * B02) + A23 * B01,
 *   and F[j][i] = det when i + j is even, -det when it is odd; x_b^T F x_a = 0 for the images of one point.
 *   PAIR COST of a < b in different views (va < vb), over the joints j = 0 .. J-1 in ascending order.  Joint j is skipped unless
 *   both detections are kept and their four coordinates (xa, ya), (xb, yb) are finite.  Then
 *       l_k = (F[k][0] * xa + F[k][1] * ya) + F[k][2]  (k = 0, 1, 2),  db = |(l_0 * xb + l_1 * yb) + l_2| / sqrt(l_0 * l_0 + l_1 * l_1),
 *       t_k = (F[0][k] * xb + F[1][k] * yb) + F[2][k],                 da = |(t_0 * xa + t_1 * ya) + t_2| / sqrt(t_0 * t_0 + t_1 * t_1),
 *       d = 0.5 * (db + da);
 *   a d that is not finite is skipped too; every other joint is COMMON: sum = sum + d, n = n + 1.  With n >= min_joints the pair is
 *   MEASURED and c_ab = sum / n; otherwise it is unmeasured.  A measured pair with c_ab <= max_px is an EDGE, any other measured
 *   pair a VETO.
 *   CLUSTERING (constrained complete-link agglomeration).  Every detection starts as its own cluster.  The edges are taken in
 *   ascending (c_ab, a, b); the clusters of a and b are merged unless they are the same cluster, or they share a view, or some
 *   pair (one member of each) is a veto.  Unmeasured pairs never veto.  A cluster is labelled by its lowest member.
 *   PEOPLE: the clusters with at least min_views members, by member count descending, then by label ascending.  The first K are
 *   written, the rest are counted.  Outputs: assign (N,K,V) ints, the slot m of person k in view v or -1; n_people (N) = people
 *   written, n_overflow (N) = people not written; n_unassigned (N) = detections with at least one joint that is kept and has
 *   two finite coordinates, and that are in no written person; cost (N,K) doubles = the mean of the edges' c_ab over the pairs a < b
 *   of the person's members, added in ascending (a, b) and divided by their number, NaN for an empty slot; and the gathered
 *   detections (N,K,V,J,2) in the input's type (gathered resp. gathered_f64): the input's own bits where person k has a detection
 *   in view v and the joint is kept, NaN elsewhere -- as (N*K,V,J,2) what sks_triangulate takes.  CONTRACT: a NaN or inf coordinate
 *   drops its joint from every pair (it is copied by the gather); a frame without detections has no people and every slot empty;
 *   a person seen in one view is no person and is counted in n_unassigned; of two near-identical detections in one view at most
 *   one joins the person (the view rule), the other is unassigned.  A frame's outputs depend on its own inputs, V, M, J, K and the
 *   three parameters only, never on N, on its place in the batch or on the stream.
 *   One workgroup of 256 threads per frame; the pair costs are spread over the threads; the edge list is compacted and sorted
 *   (bitonic, one sorter for every length, on (bits of c_ab, a, b)) in LDS; the merge walk is sequential over the edges, its three
 *   tests run across the lanes of one wavefront over 128-bit member masks, 64-bit view masks and the D x D veto bit matrix.
 * sks_track_people.  joints (N,K,J,3) floats, the triangulated people, an absent person all NaN; groups (N) ints, the recording of
 *   every frame, with 1 <= n_groups <= SKS_PEOPLE_MAX_GROUPS, or NULL with n_groups = 1; 1 <= K <= SKS_PEOPLE_MAX, 1 <= J <=
 *   SKS_MAX_CHANNELS, max_mm finite and >= 0, max_gap >= 0 frames, 1 <= min_joints <= J.  Each recording is tracked on its own, its
 *   frames in ascending index order, with SKS_PEOPLE_MAX track slots, all free at first, and ids counted from 0.  A joint is FINITE
 *   when its three floats are.  Per frame:  person k is PRESENT with at least min_joints finite joints.  The cost of (alive slot s,
 *   present person k), with q the slot's last matched pose (the whole pose of the person it matched last), over the joints finite
 *   in both, ascending:  d = x - q per coordinate (widened), sum = sum + sqrt((d_0 * d_0 + d_1 * d_1) + d_2 * d_2), n = n + 1;  with
 *   n >= min_joints the cost is sum / n and the pair is a candidate when cost <= max_mm.  The candidates are matched greedily in
 *   ascending (cost, s, k), one to one.  A matched slot takes the person's pose and age 0, the person the slot's id.  An unmatched
 *   alive slot ages by one frame and is freed once its age exceeds max_gap -- before any track opens in the same frame.  Then the
 *   unmatched present people open tracks in ascending k: each takes the lowest free slot and the next id of its recording; with no
 *   free slot the person gets -1 and is counted.  Outputs: track_id (N,K) ints, -1 = absent or dropped (and every person of a frame
 *   whose group id names no recording); n_tracks, n_dropped (n_groups) ints.  One wavefront per recording, lane = 8 s + k.
 * sks_people_launch: HOST only, no GPU call: the threads and LDS bytes of the association's workgroup and the entries of its edge
 *   list for V views of M slots, and the tracker's threads, at the SKS_PEOPLE_* indices below. */
#define SKS_PEOPLE_MAX_DETS    128   /* detections a frame, V * M */
#define SKS_PEOPLE_MAX_SLOTS   16    /* candidates a view, M */
#define SKS_PEOPLE_MAX         8     /* people written a frame, K; track slots of a recording */
#define SKS_PEOPLE_MAX_GROUPS  65535
#define SKS_PEOPLE_ASSOC_THREADS       0
#define SKS_PEOPLE_ASSOC_LDS_BYTES     1
#define SKS_PEOPLE_ASSOC_LIST_ENTRIES  2
#define SKS_PEOPLE_TRACK_THREADS       3
#define SKS_PEOPLE_LAUNCH_INTS         4
int sks_associate_people(int N, int V, int M, int J, int K, const double* proj, size_t rig_stride, const float* detections,
                         const double* detections_f64, const unsigned char* valid, double max_px, int min_joints, int min_views,
                         int* assign, int* n_people, int* n_overflow, int* n_unassigned, double* cost, float* gathered,
                         double* gathered_f64, void* stream);
int sks_track_people(int N, int K, int J, const float* joints, const int* groups, int n_groups, double max_mm, int max_gap,
                     int min_joints, int* track_id, int* n_tracks, int* n_dropped, void* stream);
int sks_people_launch(int V, int M, int* out /*HOST SKS_PEOPLE_LAUNCH_INTS*/);

/* Replaces fusedssim (submodules/fused-ssim/ssim.cu:368-404, binding ext.cpp): img1, img2, ssim_map and the three
 * optional partial-derivative maps (train == true) are (B,CH,H,W) fp32; "same" zero padding. */
int sks_fused_ssim_fwd(int B, int CH, int H, int W, float C1, float C2, const float* img1, const float* img2,
                       float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream);

/* Replaces fusedssim_backward (ssim.cu:406-444): dL_dimg1 (B,CH,H,W); only img1 is differentiable
 * (fused_ssim/__init__.py:32). */
int sks_fused_ssim_bwd(int B, int CH, int H, int W, float C1, float C2, const float* img1, const float* img2,
                       const float* dL_dmap, const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                       float* dL_dimg1, void* stream);
/* The same backward when dL_dmap is what `.mean()` of the map hands back (fused_ssim/__init__.py:41): one value,
 * *dL_value (device memory) * dL_scale, on the image shrunk by `crop` pixels per side (5 for padding == "valid",
 * fused_ssim/__init__.py:13-14,24-26; 0 for "same") and zero outside.  No gradient image is materialised or read. */
int sks_fused_ssim_bwd_uniform(int B, int CH, int H, int W, const float* img1, const float* img2, const float* dL_value,
                               float dL_scale, int crop, const float* dm_dmu1, const float* dm_dsigma1_sq,
                               const float* dm_dsigma12, float* dL_dimg1, void* stream);
/* fused_ssim()'s `map.mean()` without the map (fused_ssim/__init__.py:34-41): *mean_out (device, fp32) = mean of the
 * SSIM map over the image shrunk by `crop` pixels per side (accumulated in fp64).  The three partial-derivative maps
 * are written when given (train == true), the map itself never.  scratch: SKS_SSIM_SCRATCH_BYTES of device memory that
 * is ZERO on entry and is left zero on exit (workgroups add to different slots, a one-wave kernel reduces and clears
 * them), so one buffer zeroed once serves every call on a stream. */
#define SKS_SSIM_SUM_SLOTS 64
#define SKS_SSIM_SCRATCH_BYTES (SKS_SSIM_SUM_SLOTS * 8)
int sks_fused_ssim_mean(int B, int CH, int H, int W, float C1, float C2, const float* img1, const float* img2, int crop,
                        float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, double* scratch, float* mean_out,
                        void* stream);

/* Replaces distCUDA2 (submodules/simple-knn/spatial.cu:15-26 -> SimpleKNN::knn simple_knn.cu:186-222):
 * points (P,3) -> mean squared distance to the 3 nearest neighbours (P). */
int sks_knn3_meandist2(int P, const float* points, float* mean_dist2, void* stream);
/* The same result (identical floats) for large clouds: exact uniform-grid search, O(P) for well-spread points
 * instead of the all-pairs sweep.  scratch: sks_knn3_scratch_bytes(P) bytes of device memory. */
size_t sks_knn3_scratch_bytes(int P);
int sks_knn3_meandist2_grid(int P, const float* points, float* mean_dist2, void* scratch, size_t scratch_bytes, void* stream);

/* Sparse fused training step (no dense image, no dense gradient).  In the loop the render is only ever compared with the
 * constant pseudo-GT heat-maps (train.py:148-152), and it is exactly zero outside the tiles some Gaussian rect covers,
 * so render + clamp + masked-L2 + backward can be evaluated on the covered tiles alone.  Where the render is zero the
 * loss only sees the heat-maps (mask gt > 0, error gt^2): a per-frame constant; where it is positive the exact term
 * replaces that constant.
 *  sks_gt_tile_stats (once per frame): per-view totals {sum of gt^2 over the pixels with gt > 0, count of gt > 0} (V x 2
 *      doubles) -- the masked-L2 sums S and N of an all-zero render, whose mask leaves out every pixel with gt <= 0: planes
 *      need not be normalised to [0, 1], a negative entry adds to neither (for planes without negative entries the first is
 *      the plain sum of squares); optionally (tile_S / tile_N non-NULL) the same per (view, tile, channel) as (V, Ty*Tx, C) floats;
 *  sks_geometry: the geometry stage of sks_forward alone (fills `geom` and `radii`);
 *  sks_backward_fused_loss: like sks_backward, but takes the heat-maps `gt` (V,C,H,W) instead of dL/d(render):
 *      re-composites each covered pixel, forms 2 (clamp(r) - gt) on the mask {gt > 0 or r > 0} on the fly, and
 *      returns per-view {S, N} (loss_v = S/N) in loss_sums = gt_totals + the corrections of the pixels with a
 *      positive render; gradients are UNSCALED (multiply by 1/N_v, e.g. with sks_loop_pack_grads).  P <= 64.
 *      tile_S / tile_N are not read (may be NULL).  A view whose mask is empty (all-zero heat-maps, nothing rendered)
 *      returns {0, 0} and gradients that are exactly zero; packed_raw_grads, which divides by N_v, is scaled by 1 for such
 *      a view (N_v < 1) and stays finite: zero.
 *  Views of different image sizes in ONE launch sequence (H36M mixes 1000- and 1002-wide sensors,
 *  scene/dataset_readers.py:68-80): nothing dense is written on this path, so sks_geometry, sks_backward_fused_loss
 *  and sks_loop_fused_step accept view_wh = V x {W_v, H_v} (W, H arguments: the largest) and, for the heat-maps,
 *  gt_offsets = V offsets in floats from `gt` to view v's (C,H_v,W_v) planes inside one flat buffer.  NULL = all W x H
 *  and gt is one (V,C,H,W) tensor.  A `geom` filled with view_wh serves the fused-loss calls, not sks_forward. */
int sks_gt_tile_stats(int V, int C, int W, int H, const float* gt, float* tile_S, float* tile_N, double* totals, void* stream);
int sks_geometry(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                 const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/, const float* means3D,
                 const float* opacities, const float* scales, const float* rotations, const float* cov3D_precomp,
                 float scale_modifier, unsigned flags, int* radii, void* geom,
                 const int* view_wh /*HOST V x {W,H} or NULL: see below*/, int frames /* 1, or see sks_loop_fused_step */,
                 void* stream);
int sks_backward_fused_loss(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                            const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/, const float* bg,
                            const float* means3D, const float* features, const float* opacities, const float* scales,
                            const float* rotations, const float* cov3D_precomp, float scale_modifier, unsigned flags,
                            const int* radii, const void* geom, const float* gt, const float* tile_S, const float* tile_N,
                            const double* gt_totals, void* accum, float* dL_dmeans3D, float* dL_dmeans2D,
                            float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                            double* loss_sums, float* packed_raw_grads /* optional (V,P,11), see sks_loop_pack_grads:
                            with SKS_RAW_PARAMS the activation Jacobians and the 1/N_v scale are applied here */,
                            const int* view_wh /*HOST V x {W,H} or NULL*/, const size_t* gt_offsets /*HOST V or NULL*/,
                            const float* const* hm_factors /*HOST 4 device pointers or NULL, see below*/, void* stream);
/* hm_factors = {row (V,C,H), col (V,C,W), cmin (V,C), den (V,C)} (sks_heatmap_factors' outputs, strides H / W = this
 * call's W, H): the pseudo-GT is evaluated where it is needed, gt(v,c,y,x) = (row[y] * col[x] - cmin) / den -- the value
 * sks_heatmaps would have stored, bit for bit -- and `gt` / `gt_offsets` are not read (may be NULL); gt_totals then comes
 * from sks_heatmap_totals.  No heat-map plane exists anywhere on that path. */

/* Device-side tail of the multi-view loop (train.py:160-222), so that one accumulation group is a fixed launch
 * sequence with no host state (capturable into a hipGraph):
 * sks_loop_pack_grads: sks_backward's per-view gradients wrt the ACTIVATED tensors (V,P,..) -> packed (V,P,11) gradients
 *   wrt the RAW leaf parameters [xyz 3 | _scaling 3 | _rotation 4 | _opacity 1] through the exp / normalize / sigmoid
 *   Jacobians (scene/gaussian_model.py:39-47), times 1/N_v when loss_sums (V x {S,N} doubles of sks_masked_l2) is given.
 * sks_loop_adam_step: one optimiser step of the reference loop: slots[v] = grads[v].xyz + limb-symmetry gradient for the
 *   views in group_mask (utils/loss_utils.py:226-250, train.py:150-152,175), xyz.grad = mean over the V slots
 *   (train.py:215-217), scaling/rotation/opacity gradients of `last_view` (quirk Q7), exponential LR schedule evaluated at
 *   the stepping iteration (utils/general_utils.py:38-71, quirk Q9), torch.optim.Adam update (eps from the caller; the
 *   reference uses 1e-15, gaussian_model.py:218).  counters (device, 2 ints): [0] iteration, advanced by acc_steps,
 *   [1] Adam step count.  exp_avg / exp_avg_sq: (P,11) each, zero-initialised by the caller.  P <= SKS_SMALL_P. */
int sks_loop_pack_grads(int V, int P, const float* dL_dmeans3D, const float* dL_dscales, const float* dL_drotations,
                        const float* dL_dopacity, const float* raw_scaling, const float* raw_rotation,
                        const float* raw_opacity, const double* loss_sums, float* packed, void* stream);
int sks_loop_adam_step(int V, int P, const float* grads, float* slots, unsigned long long group_mask, int last_view,
                       float* xyz, float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq,
                       int* counters, int acc_steps, const double* lr_sched /*HOST 5: init, final, delay_mult, delay_steps, max_steps*/,
                       const double* lrs /*HOST 3: scaling, rotation, opacity*/, const double* adam /*HOST 3: beta1, beta2, eps*/,
                       float lambda_consistency, const int* limb /*HOST 8 ints or NULL*/,
                       int shard_world /* layout of grads: 1 = (V,P,11) view-major; N > 1 = the buffer all_gather leaves when
                       view v is local view v / N of rank v % N and every rank contributes ceil(V / N) rows: (N, ceil(V/N), P, 11),
                       read in place -- the exchange step of the view-sharded loop needs no re-ordering pass */,
                       void* stream);

/* sks_loop_adam_step with the reference's early-stopping criterion ON THE DEVICE (training.early_stopping = opt_early_stopping:
 * utils/general_utils.py:467-491 fed at train.py:155, the break at train.py:182-233).  Before the step, one thread appends the
 * losses of the group's iterations -- loss_v = S_v / max(N_v, 1) + lambda x limb loss, fp32, in iteration order -- to the history
 * and tests the last `es_window` against the `es_window` before them (|difference| < es_tolerance, fp32).  When the criterion fires
 * at the k-th iteration of the group, only the first k views refresh their slots, view k's scaling / rotation / opacity gradients
 * win, the optimiser steps at once, `es_state[1]` (and *es_host_flag, pinned host memory, when given) receives that iteration --
 * and every later launch of this entry point on the same state does nothing: a caller keeps enqueueing groups without ever
 * reading a loss back and looks at the flag when it likes (no host synchronisation per group; the group is hipGraph-capturable).
 * es_state: 2 + 2 * es_window ints, zero at the start of a scene ([0] losses seen, [1] stopping iteration or 0, then the ring).
 * loss_sums: V x {S, N} doubles of the group's views (sks_masked_l2 / sks_backward_fused_loss).  shard_world = N > 1 and
 * loss_sums == NULL: every rank's block of `grads` is sks_loop_shard_floats(V, P, N) floats -- its ceil(V / N) x P x 11 gradient
 * rows (padded to an even count) followed by its views' {S, N} as doubles -- so gradients AND losses cross in the step's ONE
 * all_gather and every rank takes the identical decision. */
int sks_loop_adam_step_es(int V, int P, const float* grads, float* slots, unsigned long long group_mask, int last_view,
                          float* xyz, float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq,
                          int* counters, int acc_steps, const double* lr_sched /*HOST 5*/, const double* lrs /*HOST 3*/,
                          const double* adam /*HOST 3*/, float lambda_consistency, const int* limb /*HOST 8 or NULL*/,
                          int shard_world, const double* loss_sums, int* es_state, int es_window, float es_tolerance,
                          int* es_host_flag /*pinned HOST int or NULL*/, void* stream);
size_t sks_loop_shard_floats(int V, int P, int shard_world);

/* torch.optim.Adam's update (no amsgrad, no weight decay; scene/gaussian_model.py:218 builds it with eps = 1e-15 over six parameter
 * groups, train.py:219 steps it) for up to 8 fp32 tensors in ONE launch:
 *   exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2);
 *   param.addcdiv_(exp_avg, exp_avg_sq.sqrt() / sqrt(1 - beta2^step) + eps, value = -lr / (1 - beta1^step)).
 * params / grads / exp_avg / exp_avg_sq: HOST arrays of n_tensors device pointers; numel, lr, step: HOST arrays (step = the
 * tensor's count AFTER this step, >= 1: torch keeps one per parameter).  What skelsplat_amd.optim.Adam.step() calls. */
int sks_adam_multi(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                   const long long* numel, const double* lr, const long long* step, double beta1, double beta2, double eps, void* stream);

/* One accumulation group of the sparse loop on ONE GPU in two launches (train.py:130-222 for acc_steps views):
 * the fused-loss compositing backward (as sks_backward_fused_loss) and a single-workgroup tail that runs the geometry
 * backward of every view, the optimiser step (as sks_loop_adam_step) and the geometry forward of the UPDATED parameters.
 * Precondition: `geom` / `radii` hold the geometry of the current parameters (sks_geometry with SKS_RAW_PARAMS, or the
 * previous sks_loop_fused_step); on return they hold the geometry of the updated ones.  xyz / scaling / rotation / opacity
 * are the RAW leaf parameters (updated in place); packed: (V,P,11) scratch (the group's raw-parameter gradients on
 * return); loss_sums: out, V x {S, N}.  P <= 64.  Results are bit-identical to the separate calls.
 *
 * frames > 1 batches INDEPENDENT frames (the reference optimises one frame after the other, train.py:74-99, and a
 * 17-Gaussian skeleton leaves most of the chip idle): V = frames x Vf views, view f*Vf + j is frame f's j-th view (the
 * camera rows are repeated per frame), and every frame owns a slice of the stacked tensors -- xyz/scaling (frames,P,3),
 * rotation (frames,P,4), opacity (frames,P), exp_avg/exp_avg_sq (frames,P,11), slots (frames,Vf,P,3), counters
 * (frames,2).  group_mask (bit j = view j of EVERY frame) and last_view are per frame (0 <= last_view < Vf); features,
 * the optimiser's hyper-parameters and the limb pairs are shared.  Each frame's results are bit-identical to running
 * it alone with frames = 1.
 *
 * sks_loop_fused_step_es (since sks_version 12): the same step with the reference's opt_early_stopping criterion run PER FRAME
 * on the device, as sks_loop_adam_step_es runs it for one scene: the tail workgroup of frame f feeds the criterion its views'
 * losses (S_v / max(N_v, 1) as fp32, plus lambda x the limb loss of the pre-step xyz) in iteration order, after the geometry
 * backward and before the optimiser step.  When it fires at the k-th iteration of the group, frame f steps at once on the first
 * k views (view k's scaling / rotation / opacity gradients win, counters[f][0] advances by k, the LR schedule is taken at that
 * iteration), the geometry of the updated parameters is written as usual, and es_state[f][1] and es_host_flags[f] receive the
 * iteration.  At every later launch frame f costs nothing: its compositing-backward workgroups read the stopped word and
 * leave, and its tail workgroup leaves before writing anything (parameters, moments, slots, counters, geometry, radii, loss
 * sums).  The other frames go on; each frame stays bit-identical to sks_loop_adam_step_es running it alone.
 * es_state: frames x (2 + 2 * es_window) ints on the device, zero at the start of the frames, each frame's slice laid out as
 * sks_loop_adam_step_es's state; 1 <= es_window <= 16; es_host_flags: pinned HOST memory of `frames` ints, or NULL. */
int sks_loop_fused_step(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                        const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/, const float* features,
                        float scale_modifier, unsigned flags, int* radii, void* geom, const float* gt,
                        const double* gt_totals, void* accum, double* loss_sums, float* packed, float* slots,
                        unsigned long long group_mask, int last_view, float* xyz, float* scaling, float* rotation,
                        float* opacity, float* exp_avg, float* exp_avg_sq, int* counters, int acc_steps,
                        const double* lr_sched /*HOST 5*/, const double* lrs /*HOST 3*/, const double* adam /*HOST 3*/,
                        float lambda_consistency, const int* limb /*HOST 8 or NULL*/,
                        const int* view_wh /*HOST V x {W,H} or NULL*/, const size_t* gt_offsets /*HOST V or NULL*/,
                        int frames, const float* const* hm_factors /*HOST 4 or NULL, as for sks_backward_fused_loss*/,
                        void* stream);
int sks_loop_fused_step_es(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                           const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/, const float* features,
                           float scale_modifier, unsigned flags, int* radii, void* geom, const float* gt,
                           const double* gt_totals, void* accum, double* loss_sums, float* packed, float* slots,
                           unsigned long long group_mask, int last_view, float* xyz, float* scaling, float* rotation,
                           float* opacity, float* exp_avg, float* exp_avg_sq, int* counters, int acc_steps,
                           const double* lr_sched /*HOST 5*/, const double* lrs /*HOST 3*/, const double* adam /*HOST 3*/,
                           float lambda_consistency, const int* limb /*HOST 8 or NULL*/,
                           const int* view_wh /*HOST V x {W,H} or NULL*/, const size_t* gt_offsets /*HOST V or NULL*/,
                           int frames, const float* const* hm_factors /*HOST 4 or NULL, as for sks_backward_fused_loss*/,
                           int* es_state, int es_window, float es_tolerance, int* es_host_flags /*pinned HOST frames or NULL*/,
                           void* stream);

/* Frame batches whose frames are seen by DIFFERENT camera rigs (since sks_version 14).  The entry points above take the per-view
 * scalars (tanfovx / tanfovy / view_wh) and the LR schedule as HOST arrays and hand them to their kernels by value, so a captured
 * hipGraph holds them; the *_dv twins below read them from DEVICE memory, so that the cameras of a batch can be exchanged under a
 * captured graph by writing a few buffers.
 *  views_dev: 4 x SKS_MAX_VIEWS words on the device -- float tanfovx[SKS_MAX_VIEWS], float tanfovy[SKS_MAX_VIEWS],
 *      int W_v[SKS_MAX_VIEWS], int H_v[SKS_MAX_VIEWS] --, entries [0, V) valid, every size within [1, W] x [1, H];
 *  lr_sched_dev: frames x 5 doubles on the device, row f = frame f's schedule as {log lr_init, log lr_final, delay_mult, delay_steps,
 *      max_steps} -- sks_loop_adam_step's five numbers with the two logarithms (log 0 = -inf) already taken, on the host;
 *  sks_rig_select: fills both -- and the view / projection rows and K [R|t] -- for a batch of `frames` frames from a bank of R
 *      rigs, all device memory: rig_ids (frames) ints; bank_viewmatrix / bank_projmatrix (R,V,16); bank_tan (R,V,2) = {tanfovx,
 *      tanfovy}; slot_wh (V,2) = {W_j, H_j} of view slot j (the same in every rig); bank_proj (R,V,3,4) doubles or NULL (with
 *      proj NULL); bank_sched (R,5) doubles, rows as lr_sched_dev's.  Frame f receives rig rig_ids[f]: viewmatrix / projmatrix
 *      rows [f*V, (f+1)*V), the same entries of views_dev, proj (frames,V,3,4) -- what sks_triangulate takes with rig_stride =
 *      V * 12 -- and row f of lr_sched_dev.  One launch on `stream`, nothing synchronises.  An id outside [0, R) writes nothing
 *      for its frame and stores 1 + f into *error_word (device or pinned host memory, zeroed by the caller; one of them when
 *      several frames do);
 *  sks_geometry_dv, sks_heatmap_factors_dv, sks_heatmap_totals_dv: as the entry points they are named after, views_dev in place
 *      of tanfovx / tanfovy / view_wh (sks_heatmap_factors_dv: the same no-impulse rule, SKS_HEATMAP_MAX_RADIUS included);
 *  sks_loop_fused_step_dv, sks_loop_fused_step_es_dv: views_dev in place of tanfovx / tanfovy, lr_sched_dev in place of lr_sched
 *      (the tail workgroup of frame f reads row f).  view_wh stays a HOST argument with the same sizes as views_dev holds: the
 *      compositing backward reads nothing but the sizes, which are fixed per view slot, and keeps them in its argument segment.
 *  Results are bit-identical to the by-value entry points given the same numbers. */
int sks_rig_select(int R, int V, int frames, const int* rig_ids, const float* bank_viewmatrix, const float* bank_projmatrix,
                   const float* bank_tan, const int* slot_wh, const double* bank_proj, const double* bank_sched,
                   float* viewmatrix, float* projmatrix, void* views_dev, double* proj, double* lr_sched_dev, int* error_word,
                   void* stream);
int sks_geometry_dv(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix, const void* views_dev,
                    const float* means3D, const float* opacities, const float* scales, const float* rotations,
                    const float* cov3D_precomp, float scale_modifier, unsigned flags, int* radii, void* geom, int frames,
                    void* stream);
int sks_heatmap_factors_dv(int V, int J, int W, int H, const float* means3D, const float* scales, const float* rotations,
                           float scale_modifier, const float* poses_2d, const float* viewmatrix, const void* views_dev,
                           float* row, float* col, float* cmin, float* den, int frames, void* stream);
int sks_heatmap_totals_dv(int V, int J, int W, int H, const float* row, const float* col, const float* cmin, const float* den,
                          const void* views_dev, double* gt_totals, void* stream);
int sks_loop_fused_step_dv(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                           const void* views_dev, const float* features, float scale_modifier, unsigned flags, int* radii,
                           void* geom, const float* gt, const double* gt_totals, void* accum, double* loss_sums, float* packed,
                           float* slots, unsigned long long group_mask, int last_view, float* xyz, float* scaling,
                           float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq, int* counters, int acc_steps,
                           const double* lr_sched_dev, const double* lrs /*HOST 3*/, const double* adam /*HOST 3*/,
                           float lambda_consistency, const int* limb /*HOST 8 or NULL*/,
                           const int* view_wh /*HOST V x {W,H} or NULL*/, const size_t* gt_offsets /*HOST V or NULL*/, int frames,
                           const float* const* hm_factors /*HOST 4 or NULL*/, void* stream);
int sks_loop_fused_step_es_dv(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                              const void* views_dev, const float* features, float scale_modifier, unsigned flags, int* radii,
                              void* geom, const float* gt, const double* gt_totals, void* accum, double* loss_sums,
                              float* packed, float* slots, unsigned long long group_mask, int last_view, float* xyz,
                              float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq, int* counters,
                              int acc_steps, const double* lr_sched_dev, const double* lrs /*HOST 3*/,
                              const double* adam /*HOST 3*/, float lambda_consistency, const int* limb /*HOST 8 or NULL*/,
                              const int* view_wh /*HOST V x {W,H} or NULL*/, const size_t* gt_offsets /*HOST V or NULL*/,
                              int frames, const float* const* hm_factors /*HOST 4 or NULL*/, int* es_state, int es_window,
                              float es_tolerance, int* es_host_flags /*pinned HOST frames or NULL*/, void* stream);

/* View agreement: each view's xyz gradient weighted by how well it agrees with the others' (csrc/sks_loop_dev.h; added to
 * sks_version 14: the number did not move).  The reference keeps the views' position gradients apart until the optimiser step
 * (train.py:121,175,215-217) for the sake of utils/similarity_utils.py -- pairwise_cosine_similarity, compute_scaling_weights /
 * weight_function, identify_consistent_views -- which weight or select views PER JOINT; these three entry points run them inside
 * the step's own launch, where the plain ones take the mean of the V slots.  Scaling / rotation / opacity gradients stay
 * last_view's.
 *
 * One fixed fp32 sequence (no contraction, IEEE division and square root), applied to joint j AFTER the group's slots are
 * refreshed, so it sees the slots exactly as the plain mean does: the limb gradient every slot carries, the stale slots of views
 * outside group_mask (quirk Q8), the slots an early stop leaves.  For views a, b in [0, V):
 *   g_a = slot (a, j, :);  n_a = sqrtf((g0*g0 + g1*g1) + g2*g2) + 1e-8f;  u_a = g_a / n_a, component by component;
 *   c_ab = (u_a0*u_b0 + u_a1*u_b1) + u_a2*u_b2 for a != b, c_aa = 1                              (pairwise_cosine_similarity)
 * vw_mode 1, "scale" (compute_scaling_weights):
 *   s_a = (sum over b != a, ascending, of c_ab) / (float)(V - 1), clamped to [-1, 1]; a NaN s_a gives w_a = 0;
 *   s_a < 0: w_a = 0.8f * (s_a + 1.0f); otherwise w_a = (float)(0.54 * (log(2.0 + (double)s_a) / log(3.0)) + 0.46), in double;
 *   xyz.grad = (sum over a, ascending, of w_a * g_a) / (float)V.  V < 2: every weight is 1.
 * vw_mode 2, "select" (identify_consistent_views):
 *   k_a = the number of b != a with c_ab >= vw_threshold; view a is kept when k_a >= 2; with n >= 1 views kept
 *   xyz.grad = (sum over kept a, ascending, of g_a) / (float)n; with none kept (always so for V < 3) the plain mean, in the same
 *   bits as the plain entry points.  The weights written out are 1.0 / 0.0.
 * vw_mode 0: off, bit-identical to the entry point without _vw; anything else is an error.
 * Two deviations from the reference's text: it divides by a hard-coded 3 (right for four views), here by V - 1; and its
 * weight_function gives weight 0 where s rounds above 1 -- views in perfect agreement -- hence the clamp.
 * No atomics; every sum has the order above, so results are bitwise reproducible.  The device's double log is not correctly
 * rounded: a "scale" weight may differ from a correctly rounded evaluation by one fp32 ulp.
 *
 * Parameters: those of sks_loop_adam_step_es / sks_loop_fused_step_es / sks_loop_fused_step_es_dv with four more in front of
 * `stream`; es_state == NULL is the step without a criterion (es_window, es_tolerance, the flags and -- sks_loop_adam_step_vw --
 * loss_sums are then not read), so one entry serves both forms.
 * vw_weights (frames,V,P) and vw_similarity (frames,P,V,V) -- frames = 1 for sks_loop_adam_step_vw, V the views of one frame --:
 * optional device outputs of the step taken, written by the same launch; either may be NULL; a frame that has stopped writes
 * nothing.  Shapes with V * P * 3 <= 8192 (4 x 17, 5 x 15, 31 x 19) spread the pairwise work over the workgroup from LDS; larger
 * ones take a per-joint walk with the same results. */
int sks_loop_adam_step_vw(int V, int P, const float* grads, float* slots, unsigned long long group_mask, int last_view,
                          float* xyz, float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq,
                          int* counters, int acc_steps, const double* lr_sched /*HOST 5*/, const double* lrs /*HOST 3*/,
                          const double* adam /*HOST 3*/, float lambda_consistency, const int* limb /*HOST 8 or NULL*/,
                          int shard_world, const double* loss_sums, int* es_state /*NULL: no criterion*/, int es_window,
                          float es_tolerance, int* es_host_flag /*pinned HOST int or NULL*/, int vw_mode, float vw_threshold,
                          float* vw_weights, float* vw_similarity, void* stream);
int sks_loop_fused_step_vw(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                           const float* tanfovx /*HOST V*/, const float* tanfovy /*HOST V*/, const float* features,
                           float scale_modifier, unsigned flags, int* radii, void* geom, const float* gt,
                           const double* gt_totals, void* accum, double* loss_sums, float* packed, float* slots,
                           unsigned long long group_mask, int last_view, float* xyz, float* scaling, float* rotation,
                           float* opacity, float* exp_avg, float* exp_avg_sq, int* counters, int acc_steps,
                           const double* lr_sched /*HOST 5*/, const double* lrs /*HOST 3*/, const double* adam /*HOST 3*/,
                           float lambda_consistency, const int* limb /*HOST 8 or NULL*/,
                           const int* view_wh /*HOST V x {W,H} or NULL*/, const size_t* gt_offsets /*HOST V or NULL*/,
                           int frames, const float* const* hm_factors /*HOST 4 or NULL*/,
                           int* es_state /*NULL: no criterion*/, int es_window, float es_tolerance,
                           int* es_host_flags /*pinned HOST frames or NULL*/, int vw_mode, float vw_threshold,
                           float* vw_weights, float* vw_similarity, void* stream);
int sks_loop_fused_step_vw_dv(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                              const void* views_dev, const float* features, float scale_modifier, unsigned flags, int* radii,
                              void* geom, const float* gt, const double* gt_totals, void* accum, double* loss_sums,
                              float* packed, float* slots, unsigned long long group_mask, int last_view, float* xyz,
                              float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq, int* counters,
                              int acc_steps, const double* lr_sched_dev, const double* lrs /*HOST 3*/,
                              const double* adam /*HOST 3*/, float lambda_consistency, const int* limb /*HOST 8 or NULL*/,
                              const int* view_wh /*HOST V x {W,H} or NULL*/, const size_t* gt_offsets /*HOST V or NULL*/,
                              int frames, const float* const* hm_factors /*HOST 4 or NULL*/,
                              int* es_state /*NULL: no criterion*/, int es_window, float es_tolerance,
                              int* es_host_flags /*pinned HOST frames or NULL*/, int vw_mode, float vw_threshold,
                              float* vw_weights, float* vw_similarity, void* stream);

/* What the reference reports about a pose while and after it optimises it (train.py:184-213, 227-229, 239-242; eval.py:115-142),
 * on the device (csrc/sks_report.hip; added to sks_version 14).  One launch each on `stream`, nothing synchronises, no atomics;
 * every sum has a fixed order, so every result is bitwise the same from run to run.  Device memory unless marked HOST.
 *
 * sks_pose_errors: pred, gt (N,P,3) floats -> per_joint (N,P,2) or NULL, mean (N,2).  Column 0 is ||pred - gt|| of the joint,
 *   column 1 ||(pred - pred[0]) - (gt - gt[0])|| (root-relative, in that order of operations); the mean runs over the frame's P
 *   joints in float, a fixed order that depends on P alone.  Any N >= 1, any P >= 1.  A NaN joint poisons its own frame's means.
 *
 * sks_loop_report: the per-group launch of a frame batch (behind sks_loop_fused_step*; once behind the initialisation of the
 *   frames, where it finds n = 0).  One wavefront per frame reads counters (frames,2), es_state (as sks_loop_fused_step_es's, with
 *   its es_window; NULL: no early stopping), xyz (frames,P,3), gt (frames,P,3) or NULL, loss_sums (frames*V,2) or NULL, and with
 *   n = counters[f,1], the Adam steps frame f has made, writes
 *     trace_err (frames,capacity,2): row n = sks_pose_errors' two means of xyz[f], bit for bit (gt given);
 *     trace_loss (frames,capacity,V): row n, column v = (float)(S / max(N, 1)) of view v's loss sums, as the early-stopping
 *       criterion forms it (loss_sums given; trace_loss and loss_sums go together);
 *     final_err (frames,P,2): sks_pose_errors' per-joint errors of xyz[f] (gt given);
 *     snaps (frames,K,P,3): slot k, s = save_iterations[k] (HOST, K <= SKS_REPORT_MAX_SAVES ints >= 0, copied by value): xyz[f] if
 *       the frame is running and s / acc_steps == n, or if it stopped at exactly iteration s -- the parameters as they stood at the
 *       end of iteration s, for a frame that got there.  For a frame that stopped before s the slot is set to NaN, the value the
 *       caller initialises the slots with: the reference writes no file for an iteration a scene never ran.
 *   Rows n >= capacity are dropped, never written.  Everything written depends only on what the launch reads, so replaying it for a
 *   frame that has stopped rewrites the values that are there.  The caller fills traces and snapshots with NaN per batch.
 *
 * sks_eval_sequence: pred, gt (N,P,3) floats, group_ids (N) ints or NULL (n_groups = 0), abs_valid (N) bytes or NULL ->
 *   out (1 + n_groups, 2) doubles: row 0 = {absolute, root-relative} MPJPE over all frames (the mean of sks_pose_errors' per-joint
 *   errors over frames and joints), row 1 + g the same over the frames with group_ids == g (an id outside [0, n_groups) is in no
 *   group).  Frames with abs_valid == 0 are left out of the absolute figures only (eval.py:62-63); a row without frames is NaN.
 *   Norms in float, sums in double: one workgroup per row, thread t adds frames t, t + 256, ... in index order, then a fixed tree. */
#define SKS_REPORT_MAX_SAVES 8
#define SKS_EVAL_MAX_GROUPS 64
int sks_pose_errors(int N, int P, const float* pred, const float* gt, float* per_joint, float* mean, void* stream);
int sks_loop_report(int frames, int V, int P, const int* counters, const int* es_state, int es_window, const float* xyz,
                    const float* gt, const double* loss_sums, int acc_steps, int capacity, float* trace_err, float* trace_loss,
                    float* final_err, int K, const int* save_iterations /*HOST K or NULL*/, float* snaps, void* stream);
int sks_eval_sequence(int N, int P, const float* pred, const float* gt, const int* group_ids, int n_groups,
                      const unsigned char* abs_valid, double* out, void* stream);

/* The optimised Gaussians read back as the pose's uncertainty (csrc/sks_uncertainty.hip; added to sks_version 14: the number did
 * not move): what the reference's analysis scripts take from the covariance a scene leaves behind
 * (utils/analize_error_confidence_correlation.py, utils/analize_2D_anisotropy.py).  One launch each on `stream`, nothing
 * synchronises, no atomics, no scratch.  Everything a (frame, joint) or (view, joint) receives depends on its own inputs only --
 * never on N, on its place in the batch or on the stream --, so a NaN or inf input poisons those outputs of its own joint that
 * depend on it and nobody else's.  Bad arguments are refused before any HIP call.  Device memory unless marked HOST.
 *
 * sks_joint_uncertainty: scales (N,P,3) ACTIVATED, rotations (N,P,4) raw quaternions, as sks_heatmap_factors takes them; xyz
 *   (N,P,3) and gt (N,P,3) go together with d2, or gt and d2 are NULL (xyz is then not read).  One thread per (frame, joint).
 *     cov6 (N,P,6): xx, xy, xz, yy, yz, zz (strip_symmetric, general_utils.py:73-85) of Sigma = L L^T, L = R diag(sd),
 *       sd_k = scale_modifier * s_k, R from the NORMALISED quaternion -- the float sequence sks_heatmap_factors forms Sigma with
 *       (one __device__ function, csrc/sks_gauss.h): Sigma[a][b] = (L[a][0] L[b][0] + L[a][1] L[b][1]) + L[a][2] L[b][2].
 *     spectrum (N,P,6): l1 >= l2 >= l3, trace, det, anisotropy.  Sigma = R S^2 R^T, so its eigenvalues ARE sd_k * sd_k:
 *       the three float products, sorted (a NaN stays in its slot); no eigen-solver, which on a needle would lose the small ones.
 *       trace = (xx + yy) + zz of cov6; det = (l1 * l2) * l3; anisotropy = l1 / l3.
 *     d2 (N,P), with gt: the squared Mahalanobis distance of the ground truth, by whitening: delta = gt - xyz,
 *       w_k = ((R[0][k] delta[0] + R[1][k] delta[1]) + R[2][k] delta[2]) / sd_k, d2 = (w_0^2 + w_1^2) + w_2^2.  No 3x3 inverse is
 *       formed (the reference's np.linalg.inv(cov), analize_error_confidence_correlation.py:48-54, is the same number in exact
 *       arithmetic and worse conditioned).
 *   N x P <= 2^28 - 1.
 *
 * sks_view_footprints: lambdas (V,J,2) = l1 >= l2, the two variances in px^2 of the blob each view's pseudo-GT is drawn with: the
 *   numbers sks_heatmap_factors forms before its square roots (the reference's own transcription of the EWA projection,
 *   general_utils.py:212-262, with the 0.3 px^2 low-pass and the max(0.1, .) guard), bit for bit -- the same __device__ function.
 *   means3D / scales / rotations / scale_modifier / viewmatrix / W / H / frames as sks_heatmap_factors.  The per-view scalars come
 *   in exactly ONE of two forms: tanfovx, tanfovy HOST arrays of V with view_wh HOST V x {W,H} or NULL (sks_heatmap_factors'), or
 *   views_dev, the device table of sks_heatmap_factors_dv (then the three host pointers are NULL).  One thread per (view, joint).
 *   The ratio of analize_2D_anisotropy.py:50 is l1 / l2.
 *
 * sks_calibration: d2 (N,P) floats, valid (N) bytes or NULL, k_sigma HOST K floats (1 <= K <= SKS_CALIBRATION_MAX_K, each finite
 *   and > 0, copied by value) -> counts (1 + P, K + 1) int32.  Row 0 is over all joints, row 1 + j over joint j; column k counts
 *   the entries with d2 <= k_sigma[k] * k_sigma[k] (the product in float), column K the entries counted at all: a frame with
 *   valid != 0 (or valid NULL) and a d2 that is not NaN.  The fractions of percent_inside_sigmas / percent_inside_sigmas_per_joint
 *   (analize_error_confidence_correlation.py:38-60, 86-113) are counts[:, k] / counts[:, K].  One workgroup per row: thread t
 *   takes frames t, t + 256, ..., then a fixed tree in LDS; integers, so the counts are exact in any order.  N x P <= 2^31 - 1. */
#define SKS_CALIBRATION_MAX_K 8
int sks_joint_uncertainty(int N, int P, const float* xyz, const float* scales, const float* rotations, float scale_modifier,
                          const float* gt, float* cov6, float* spectrum, float* d2, void* stream);
int sks_view_footprints(int V, int J, int W, int H, const float* means3D, const float* scales, const float* rotations,
                        float scale_modifier, const float* viewmatrix, const float* tanfovx /*HOST V or NULL*/,
                        const float* tanfovy /*HOST V or NULL*/, const int* view_wh /*HOST V x {W,H} or NULL*/,
                        const void* views_dev /*or NULL*/, int frames, float* lambdas, void* stream);
int sks_calibration(int N, int P, const float* d2, const unsigned char* valid, int K, const float* k_sigma /*HOST K*/, int* counts,
                    void* stream);

/* Pose errors after the best per-frame alignment of the prediction onto the ground truth (csrc/sks_align.hip; added to
 * sks_version 14: the number did not move): the rigid-aligned error, PA-MPJPE ("Protocol #2") and N-MPJPE of the H36M / Panoptic
 * literature.  The reference reports MPJPE alone, so there is no reference output behind these; they are held to two textbook
 * float64 solutions (Umeyama's SVD form, Horn's quaternion form; tests/procrustes_ref.py).  Launches go on `stream`, nothing
 * synchronises, no atomics; one wavefront per frame, everything in double from the float inputs, every output rounded to its type
 * once, every sum in a fixed order (lane l adds joints l, l + 64, ..., then a butterfly): a frame's results depend on P and its own
 * numbers only, and are bitwise the same from run to run.  Bad arguments are refused before any HIP call.  Device memory.
 *
 * sks_align_poses: pred, gt (N,P,3) floats, valid (N,P) bytes or NULL (all joints) -> aligned (N,P,3) floats, transform (N,13)
 *   doubles {s, R row-major, t}, per_joint (N,P) floats, mean (N) floats; each may be NULL, not all four.  pred is fitted onto gt
 *   over the joints with valid != 0:
 *     SKS_ALIGN_RIGID, SKS_ALIGN_SIMILARITY: mu_x, mu_y the centroids, x = pred - mu_x, y = gt - mu_y, H = sum x_i y_i^T; R is the
 *       PROPER rotation that maximises trace(R H) -- V diag(1, 1, det(V U^T)) U^T of H = U S V^T, never a reflection --, found as
 *       the unit quaternion of Horn's 4x4 symmetric eigenproblem by cyclic Jacobi sweeps (csrc/sks_procrustes.h), which needs no
 *       case for a planar (rank 2), collinear (rank 1) or mirrored input; H = 0 (one joint, coincident joints) gives R = I.
 *       SIMILARITY: s = sum <R x_i, y_i> / sum |x_i|^2 (= trace(S D) / sum |x_i|^2), 1 when the denominator is 0; RIGID: s = 1.
 *       t = mu_y - s R mu_x.
 *     SKS_ALIGN_SCALE: x_i = pred_i - pred_0, y_i = gt_i - gt_0 (joint 0 is the root, as in column 1 of sks_pose_errors),
 *       s = sum <x_i, y_i> / sum <x_i, x_i>, 1 when the denominator is 0; R = I, t = gt_0 - s pred_0.  With joint 0 masked out
 *       every result of the frame is NaN.
 *   The error of joint i is ||gt_i - (s R pred_i + t)||, formed as gt_i - (s R (pred_i - o_x) + o_y) about the origins o the fit
 *   used (the centroids; joint 0), which is the same point without the cancellation of a pose far from the world's origin; mean is
 *   its mean over the valid joints.  aligned and per_joint are written for ALL joints, masked ones included, with the transform
 *   fitted on the valid ones.  A frame without a valid joint (in every mode): mean NaN, the identity transform (s = 1, R = I,
 *   t = 0), aligned = pred.  A NaN or inf in a valid joint makes every result of its own frame NaN and touches no other frame; the
 *   frame skips the fit, so it leaves the kernel no later than a clean one.
 *
 * sks_eval_sequence_aligned: the sequence's PA-MPJPE and N-MPJPE, overall and per group.  Three launches: sks_align_poses'
 *   kernel in SIMILARITY and in SCALE mode with per-joint errors into `scratch` (sks_eval_sequence_aligned_scratch_bytes(N, P)
 *   bytes at least), then one workgroup per row of out (1 + n_groups, 2) doubles = {PA-MPJPE, N-MPJPE}: row 0 the mean over all
 *   valid joints of all frames, row 1 + g over the frames with group_ids == g (an id outside [0, n_groups) is in no group); a row
 *   without valid joints is NaN.  Thread t adds frames t, t + 256, ... in index order, a frame's valid joints in index order, sums
 *   and counts in double, then a fixed tree: the fixed-order float64 means of exactly the values sks_align_poses writes to
 *   per_joint for the same inputs.  n_groups <= SKS_EVAL_MAX_GROUPS. */
#define SKS_ALIGN_RIGID       0   /* R, t;  s = 1 */
#define SKS_ALIGN_SIMILARITY  1   /* s, R, t  (PA-MPJPE) */
#define SKS_ALIGN_SCALE       2   /* s only, on root-relative poses (N-MPJPE) */
int sks_align_poses(int N, int P, const float* pred, const float* gt, const unsigned char* valid, int mode, float* aligned,
                    double* transform, float* per_joint, float* mean, void* stream);
int sks_eval_sequence_aligned(int N, int P, const float* pred, const float* gt, const unsigned char* valid, const int* group_ids,
                              int n_groups, void* scratch, size_t scratch_bytes, double* out, void* stream);
size_t sks_eval_sequence_aligned_scratch_bytes(int N, int P);

/* 8-bit grey previews of renders and heat-maps: the reference's debug pictures (train.py:279-304, save_heatmaps / save_images),
 * on the device (csrc/sks_preview.hip; added to sks_version 14: the number did not move).  Two launches per call on `stream`,
 * nothing synchronises, no atomics; min and max are exact in any order, so every byte is the same from run to run.  Bad arguments
 * are refused before any HIP call.  Device memory unless marked HOST.
 *
 * The fixed sequence of one view, all fp32, one rounding per operation:
 *   1. s = p[0]; s += p[1]; ...; s += p[C-1]: the view's channels in ascending order, per pixel;
 *   2. lo = min(s), hi = max(s) over the view's own h x w pixels; a NaN pixel makes both NaN, as torch.min does;
 *   3. t = ((s - lo) / (hi - lo)) * 255.0f;
 *   4. q = (t >= 0 && t <= 255) ? (uint8)trunc(t) : 0.
 * Step 4 is the reference's `.astype(np.uint8)` wherever the reference is defined.  A flat view (hi == lo: 0 / 0) and a view
 * that holds a NaN or an inf are undefined there (a NaN cast to uint8); HERE every pixel whose t is NaN or outside [0, 255] is 0
 * by definition, so such a view is an all-zero picture, and minmax still reports the lo, hi it was made with.
 *
 * sks_preview_planes: planes (V,C,H,W) floats -> out (V,H,W) bytes, minmax (V,2) floats {lo, hi} or NULL.  1 <= C <=
 *   SKS_MAX_CHANNELS, V <= 65535, W x H <= 2^31 - 1.  Pass A reads the planes once (16-byte loads when W % 4 == 0 and planes and
 *   out are 16-byte aligned, scalar loads otherwise), writes the sum plane into `scratch` and one {min, max} partial per workgroup;
 *   pass B reduces a view's partials, normalises and packs (one 16-byte store of 16 pixels per lane when W % 16 == 0 and the
 *   bases are aligned, bytes otherwise).  scratch: sks_preview_scratch_bytes(V, W, H) bytes at least, 16-byte aligned.
 *
 * sks_preview_factors: the same picture of the heat-maps sks_heatmap_factors describes (row (V,J,H), col (V,J,W), cmin, den
 *   (V,J); 1 <= V <= SKS_MAX_VIEWS) without a plane ever written: per pixel the very expression sks_heatmaps stores,
 *   (row[y] * col[x] - cmin) / den, for j = 0 .. J-1 in order -- bit for bit sks_preview_planes over what sks_heatmaps would have
 *   written, for finite factors.  (A joint whose row[y] and cmin are both zero contributes exactly +0 and is skipped.)  view_wh:
 *   HOST V x {W,H} or NULL, every entry within [1, W] x [1, H]; W, H are the strides of row, col and out (the largest view), as in
 *   sks_heatmap_totals; min and max run over a view's own pixels and the bytes of out outside them are written 0.
 *
 * sks_preview_scratch_bytes: host only; 0 for a shape either entry point refuses.
 * sks_preview_launch: host only, which forms a plane-path call of W x H views takes (aligned != 0: every base pointer is a multiple
 *   of 16): out[SKS_PREVIEW_LOAD_BYTES] = 16 or 4, out[SKS_PREVIEW_STORE_BYTES] = 16 or 1, out[SKS_PREVIEW_GROUPS_SUM] and
 *   out[SKS_PREVIEW_GROUPS_PACK] = the workgroups per view of pass A and pass B (256 threads each, at most 256).  The factor
 *   path's pass A takes one workgroup per band of ceil(H / 256) rows; its pass B is the plane path's. */
#define SKS_PREVIEW_LOAD_BYTES   0
#define SKS_PREVIEW_STORE_BYTES  1
#define SKS_PREVIEW_GROUPS_SUM   2
#define SKS_PREVIEW_GROUPS_PACK  3
#define SKS_PREVIEW_LAUNCH_INTS  4
int sks_preview_planes(int V, int C, int W, int H, const float* planes, void* scratch, float* minmax, unsigned char* out,
                       void* stream);
int sks_preview_factors(int V, int J, int W, int H, const float* row, const float* col, const float* cmin, const float* den,
                        const int* view_wh /*HOST V x {W,H} or NULL*/, void* scratch, float* minmax, unsigned char* out,
                        void* stream);
size_t sks_preview_scratch_bytes(int V, int W, int H);
int sks_preview_launch(int W, int H, int aligned, int* out /*HOST SKS_PREVIEW_LAUNCH_INTS*/);

/* Measurement hook used by bench.py (no reference counterpart; state per HOST THREAD, like the error text): while enabled, the dominant kernel of sks_forward
 * (kind 0: forward compositor) and of sks_backward (kind 1: backward compositor) is bracketed by hipEvents recorded
 * on the caller's stream (the small path's kernels carry the pair on their own dispatch, hipExtLaunchKernelGGL).  The low 16
 * bits of `on`: 1 = every launch, n > 1 = every n-th launch of each kind (a bracketed launch costs ~6 us of queue time, so
 * sampling keeps the measured loop undisturbed); bits 16-17: kinds to leave OUT (bit 16: kind 0, bit 17: kind 1).  sks_prof_read waits for the recorded events, returns
 * the summed kernel time in milliseconds and the number of BRACKETED launches since the last read, and resets them.
 * A kind-0 sample is the time in which every byte of the call's output was written.  For a forward that takes prefilled planes that
 * is two intervals: its own launches, plus the launches of the sks_backward_prefill in front of it -- that call sees that the next
 * forward will be sampled, brackets its two launches with marker events and parks the pair, the forward's sample takes it over, and
 * the three readers below add the two intervals and count ONE sample per forward.  (A forward whose prefilling backward ran before
 * the hook was enabled fills every plane itself, so its sample is whole too.) */
int sks_prof_enable(int on);
/* Enqueues ONE wavefront that idles for `microseconds` (wall clock) on `stream`: a stand-in for the wire time of a latency-bound
 * collective, so that one GPU can measure what a rank of many sees when the exchange takes that long (bench.py rank_step_8gpu). */
int sks_prof_spin(double microseconds, void* stream);
/* bracketed launches of one kind collected since the last read (sks_prof_enable does not reset them: a caller may change the
 * sampling stride in the middle of a collection) */
int sks_prof_count(int kind, long long* launches);
int sks_prof_read(int kind, double* total_ms, long long* launches);
/* Same, plus the 10th / 50th / 90th percentile of the bracketed launch durations (milliseconds). */
int sks_prof_read_quantiles(int kind, double* q_ms /* 3 */, double* total_ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif
