// sks_raster.hip -- skeletal-Gaussian rasterizer for MI355X (gfx950): geometry, binning, compositing, C ABI.
//
// Replaces DGR/cuda_rasterizer/{forward.cu,backward.cu,rasterizer_impl.cu} + DGR/rasterize_points.cu of the
// reference ("DGR/" = submodules/diff-gaussian-rasterization-h36m/).  Design:
//   * one launch sequence renders V views that share the Gaussian parameters (blockIdx.z = view);
//   * P <= SKS_SMALL_P ("skeleton" regime, the reference's real configs have P = 15..19): NO global binning.
//     Forward = one kernel with two roles, fill blocks streaming zeros over everything no Gaussian rect covers and
//     composite blocks for the covered tiles (lists ordered by (depth bits, index): the order the reference gets
//     from its stable radix sort of (tile | depth) keys with index-major emission);
//     backward = gather by Gaussian: a workgroup re-composites the pixels of one Gaussian's rect and keeps only that
//     Gaussian's terms (no atomics, reproducible); final_T / n_contrib are never read back from HBM;
//   * larger P: tile-centric binning (count -> scan -> scatter -> per-tile sort), the same fill + composite forward
//     over the non-empty tiles, one workgroup per non-empty tile in backward;
//   * HBM-bound: no MFMA anywhere (there is no dense contraction in this path).
//
// One translation unit, laid out as included parts (all inside the anonymous namespace below, in this order):
//   sks_common.inc     error helpers, launch-timing hook, constants, per-view records, scratch carving
//   sks_geom_fwd.inc   k_geom_fwd (preprocessCUDA), k_mark_visible
//   sks_fwd_small.inc  LDS list + compositing core, fwd_fill_role, k_render_fwd_sparse
//   sks_bwd_small.inc  backward cores, k_render_bwd_gather / k_render_bwd_wave (+ fused loss), k_gt_tile_stats
//   sks_geom_bwd.inc   k_geom_bwd, k_step_tail (geometry backward + Adam + next geometry in one workgroup)
//   sks_binned.inc     k_bin_*, k_render_fwd_binned, k_render_bwd_binned
// followed here by the host layer:
//   helpers         with_cg (the one channel-group dispatch), is_small / TileGrid, the call records (Cameras, Gaussians, ForwardIO,
//                   Upstream, Grads -> FwdCall, BwdCall; StepRender, sksloop::Optimiser, StepHeatmaps, EarlyStop -> StepCall: the
//                   blocks of skelsplat_amd/_lib.py under the same names), the argument checks that more than one entry point makes
//   launchers       fill geometry, launch_fwd_small / _binned, launch_geom_fill / launch_geom_fwd, launch_bwd_small / _loss, prefill
//   implementations forward_impl(FwdCall), backward_impl(BwdCall), loop_fused_step_impl(StepCall)
//   extern "C"      the entry points of include/skelsplat_hip.h: each fills its record by name (SKS_TAKE_*) and calls one of the three
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <type_traits>

#include "../../include/skelsplat_hip.h"
#include "sks_math.h"
#include "sks_loop_dev.h"

using namespace sks;

namespace {

#include "sks_common.inc"
#include "sks_geom_fwd.inc"
#include "sks_fwd_small.inc"
#include "sks_bwd_small.inc"
#include "sks_geom_bwd.inc"
#include "sks_binned.inc"

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
inline int pick_cg(int C) { return C <= 4 ? 4 : C <= 16 ? 16 : C <= 20 ? 20 : 32; }
// the channel group of C as a compile-time constant: f(std::integral_constant<int, CG>) -- the launchers stay templates on CG
template <class F>
inline void with_cg(int C, F&& f)
{
    switch (pick_cg(C)) {
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 20: f(std::integral_constant<int, 20>{}); break;
        default: f(std::integral_constant<int, 32>{}); break;
    }
}

// which path a call takes, and its tile grid
inline bool is_small(int P, unsigned flags) { return P <= SKS_SMALL_P && !(flags & SKS_FORCE_BINNED); }
struct TileGrid {
    int gx, gy, NT;
    TileGrid(int W, int H) : gx((W + TILE - 1) / TILE), gy((H + TILE - 1) / TILE), NT(gx * gy) {}
};

// ---- call records: the blocks of the C ABI's argument lists under the names skelsplat_amd/_lib.py gives them ----
// An entry point fills its record BY NAME from its parameters (the SKS_TAKE_* macros in front of the entry points, one per
// block) and hands it on by const reference: nothing below an entry point counts commas.
// _CAMERAS (the tangents: HOST, V each; NO_TAN from the _dv entries, whose cameras' scalars are in StepCall::views_dev)
struct Cameras { int V, P, C, W, H; const float *viewmatrix, *projmatrix, *tanfovx, *tanfovy; };
// _GAUSSIANS
struct Gaussians { const float *means3D, *features, *opacities, *scales, *rotations, *cov3D_precomp; float scale_modifier; unsigned flags; };
// _FORWARD_IO
struct ForwardIO { float *out_color, *out_invdepth; int* radii; void *geom, *binning; size_t bin_capacity; int* num_rendered_dev; };
// _UPSTREAM
struct Upstream { const float *dL_dout_color, *dL_dout_invdepth; void* accum; };
// _GRADS
struct Grads { float *dL_dmeans3D, *dL_dmeans2D, *dL_dopacity, *dL_dscales, *dL_drotations, *dL_dcov3D, *dL_dfeatures, *dL_dmeans3D_mean; };
// FORWARD_PARAMS
struct FwdCall { Cameras cam; Gaussians g; ForwardIO io; float* final_T; uint32_t* n_contrib; hipStream_t stream; };
// BACKWARD_PARAMS
struct BwdCall {
    Cameras cam; const float* bg; Gaussians g; const int* radii; const void *geom, *binning; size_t bin_capacity;
    Upstream up; Grads grads; hipStream_t stream;
};
// _STEP_RENDER
struct StepRender {
    const float* features; float scale_modifier; unsigned flags; int* radii; void* geom; const float* gt; const double* gt_totals;
    void* accum; double* loss_sums; float* packed;
};
// _STEP_HEATMAPS (view_wh: HOST, V x {W, H}, or null; gt_offsets: HOST, V, or null; hm_factors: HOST row of 4 device pointers, or null)
struct StepHeatmaps { const int* view_wh; const size_t* gt_offsets; int frames; const float* const* hm_factors; };
// _ES + the per-frame host flags; es_state == null: the step without a criterion
struct EarlyStop { int* es_state; int es_window; float es_tolerance; int* es_host_flags; };
// LOOP_FUSED_STEP{,_ES,_DV,_ES_DV}_PARAMS.  views_dev: the _dv entries' device view table, else null; opt: OPTIMISER_PARAMS (_dv:
// opt.lr_sched is NO_SCHED and every frame's schedule row is read in the kernel from lr_sched_dev)
// vw: the *_vw entries' view agreement (mode 0: off, the plain entries; weights (frames,Vf,P) / similarity (frames,P,Vf,Vf) or null)
struct StepCall {
    Cameras cam; const void* views_dev; StepRender r; sksloop::Optimiser opt; const double* lr_sched_dev; StepHeatmaps hm; EarlyStop es;
    hipStream_t stream; sksloop::ViewWeightArgs vw;
};

int check_common(int V, int P, int C, int W, int H)
{
    if (V < 1 || V > SKS_MAX_VIEWS) return fail(-1, "V=%d out of range [1,%d]", V, SKS_MAX_VIEWS);
    if (P < 0) return fail(-1, "P=%d negative", P);
    if (C < 1 || C > SKS_MAX_CHANNELS) return fail(-1, "C=%d out of range [1,%d]", C, SKS_MAX_CHANNELS);
    if (W < 1 || H < 1 || W > 4096 * TILE || H > 65535 * TILE) return fail(-1, "image %dx%d out of range", W, H);
    return 0;
}
inline int check_common(const Cameras& c) { return check_common(c.V, c.P, c.C, c.W, c.H); }
// the argument checks more than one entry point makes, one owner each
inline int require(std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs)
        if (!p) return fail(-2, "missing required pointer");
    return 0;
}
inline int need_cov(const float* scales, const float* rotations, const float* cov3D_precomp)
{
    return (!cov3D_precomp && (!scales || !rotations)) ? fail(-2, "need scales+rotations or cov3D_precomp") : 0;
}
inline int check_frames(int V, int frames) { return (frames < 1 || V % frames) ? fail(-1, "frames must divide the number of views (V = %d, frames = %d)", V, frames) : 0; }
inline int check_hm_factors(const float* const* hm) { return (hm && (!hm[0] || !hm[1] || !hm[2] || !hm[3])) ? fail(-2, "hm_factors: row, col, cmin, den must all be given") : 0; }
inline int check_wh_offsets(const float* const* hm_factors, const int* view_wh, const size_t* gt_offsets)
{
    return (!hm_factors && (view_wh != nullptr) != (gt_offsets != nullptr)) ? fail(-2, "view_wh and gt_offsets go together") : 0;
}
inline int bad_view_wh() { return fail(-1, "view_wh: every view's size must be within [1, W] x [1, H] (pass the largest as W, H)"); }   // (fill_views said no)

// Fill-block geometry shared by the two forward launchers.  Row-aligned mode when the image width keeps >= 90% of
// the lanes of a 1024-pixel chunk busy AND a row is a whole number of 128-byte lines (1920, 2048 ... wide images;
// measured +2% at 1920, +12% on the 2048-wide stress config): blocks per band = chunks * row blocks (~8 per band),
// `pb` is returned NEGATIVE = -(rows per block).  Otherwise linear mode, pb passes of 4 KB per block: every pass is
// 32 whole lines whatever the width (at W = 1000 a row is 31.25 lines and the row-aligned mode loses 7% to the
// partial lines at both ends of every row).
// 16-byte stores need every band of every plane on a 16-byte boundary: W % 4 == 0, or W % 4 == 2 with an even H (then a
// float4 is two independently masked pairs, fwd_fill_role<.., HALF>); anything else streams 4 bytes per lane
inline bool fill_half_mode(const FwdArgs& a) { return a.W % 4 == 2 && a.H % 2 == 0 && !(a.flags & SKS_NO_NT_STORES); }

// FwdArgs::w_magic: ceil(2^32 / W) where the fill blocks take pixel index % W as a multiply-high, 0 where they use plain %
inline unsigned fill_w_magic(int W) { return (W >= 2 && W < 16384) ? (unsigned)(((1ull << 32) + (unsigned)W - 1) / (unsigned)W) : 0u; }
// 31: a band's first fill pass is a short one that ends on a 128-byte line of the address (fill_geometry), 0: every pass is whole lines
// (a null set: a rule asks -- it is answered for the worst alignment a 16-byte aligned set can have, so that what it promises the call accepts)
inline int fill_lead(const float* color, const float* invdepth, int W, int H)
{
    const bool lines = color && invdepth && (((uintptr_t)color | (uintptr_t)invdepth) & 127u) == 0;
    return (lines && (long long)H * W % 32 == 0 && TILE * W % 32 == 0) ? 0 : 31;
}
inline int fill_lead(const FwdArgs& a) { return fill_lead(a.out_color, a.out_invdepth, a.W, a.H); }

inline void fill_geometry(const FwdArgs& a, bool have_cover, bool binned, int& fsplit, int& pb)
{
    const int ppt = (a.W % 4 == 0 || fill_half_mode(a)) ? 4 : 1;
    // (+31: a band that does not start on a 128-byte line begins with a short pass, fwd_fill_role's `shift`, which the
    // kernel derives from the ADDRESS: the plane and band strides must be whole lines and so must the two base pointers --
    // torch allocations are, a direct C-ABI caller's 16-byte aligned sub-buffer need not be)
    const int lead = fill_lead(a);
    const int passes = (TILE * a.W + lead + 256 * ppt - 1) / (256 * ppt);
    const int tune = (int)((a.flags >> 8) & 0xff);                    // tuning knob: passes (or rows) per fill block
    const int chunks = (a.W + 1023) / 1024;
    const bool rowmode = ((ppt == 4 && a.W % 4 == 0 && have_cover && a.W % 32 == 0 && (long long)a.W * 10 >= (long long)chunks * 1024 * 9) ||
                          (ppt == 4 && a.W % 4 == 0 && have_cover && (a.flags & SKS_FILL_ROWS))) && !(a.flags & SKS_FILL_LINEAR);
    if (rowmode) {
        int pbr = tune;
        // rows per block, interleaved A/B on one box: 1920 wide small path 2 rows 860 us / 3: 898 / 4: 907 / 6: 915;
        // 2048 wide binned path (8 composite-role blocks per row) 2 rows 0.632 ms / 3: 0.579 / 4: 0.637 / 6: 0.571
        if (pbr <= 0) pbr = binned ? 3 : 2;
        if (pbr > TILE) pbr = TILE;
        fsplit = chunks * ((TILE + pbr - 1) / pbr);
        pb = -pbr;
        return;
    }
    pb = tune;
    if (pb <= 0) pb = passes / 8 > 2 ? (passes + 4) / 8 : 2;          // ~8 fill blocks per (plane, band) row measured best
    if (pb > 32) pb = 32;                                             // (one skip bit per pass)
    fsplit = (passes + pb - 1) / pb;                                  // fill blocks per (plane, band) row
}

// zfill: the fill role runs for the planes zid < zfill only (the rest were zeroed by the launch in front, launch_geom_fill); the
// composite role runs for every (view, Gaussian) and stores its tiles on whatever plane they are
template <int CG>
void launch_fwd_small(const FwdArgs& a_in, int V, int gy, int zfill, hipStream_t st, const ProfScope& prof)
{
    FwdArgs a = a_in;
    const int ncomp = a.tslots * a.P * V;
    a.ncomp = ncomp;
    int fsplit, pb;
    fill_geometry(a, a.g.cover != nullptr, false, fsplit, pb);
    if (zfill == 0) fsplit = 0;                                       // (no plane left to fill: one z slice of composite blocks)
    const int rows_zy = (zfill > 0 ? zfill : 1) * gy;                 // the composite blocks index the rows of THIS grid
    const int xc = (ncomp + rows_zy - 1) / rows_zy;                   // composite blocks appended to every row
    const int cap = (a.P + 15) & ~15;
    const size_t lds = DynList<CG>::bytes(cap, CG);
    dim3 grid(fsplit + xc, gy, zfill > 0 ? zfill : 1);
    const bool nt = !(a.flags & SKS_NO_NT_STORES);
    if (a.W % 4 == 0) {
        if (nt) SKS_LAUNCH(prof, (k_render_fwd_sparse<CG, 4, true>), grid, dim3(256), lds, st, a, a.cp1_magic, gy, fsplit, pb, (const uint32_t*)a.g.cover);
        else SKS_LAUNCH(prof, (k_render_fwd_sparse<CG, 4, false>), grid, dim3(256), lds, st, a, a.cp1_magic, gy, fsplit, pb, (const uint32_t*)a.g.cover);
    } else if (fill_half_mode(a)) {
        SKS_LAUNCH(prof, (k_render_fwd_sparse<CG, 4, true, true>), grid, dim3(256), lds, st, a, a.cp1_magic, gy, fsplit, pb, (const uint32_t*)a.g.cover);
    } else {
        SKS_LAUNCH(prof, (k_render_fwd_sparse<CG, 1, false>), grid, dim3(256), lds, st, a, a.cp1_magic, gy, fsplit, pb, (const uint32_t*)a.g.cover);
    }
}

// ---- early fill: the last E (view, plane) planes of a plain small-path forward are zeroed by the geometry launch ----
// How many.  The early region should keep the stores going for as long as the geometry blocks need beside them and no
// longer (its blocks run at the geometry role's occupancy, and every plane moved costs the main launch nothing but
// leaves the geometry launch's tail exposed): a fixed number of BYTES, whatever the call -- the geometry role's duration
// depends on P, not on the image --, in whole planes, and never more than a quarter of the call.
// SKS_EARLY_FILL_BYTES = 36 MB: the interleaved sweep on the H36M two-call step (72 planes of 4 MB; E = 0 / 5 / 9 / 14 / 18
// planes: 65.3 / 63.2 / 62.5 / 62.6 / 63.3 us per step, profiles/early_fill_sweep.jsonl, NOTES_experiments.md "Early fill");
// 31 Panoptic views (620 planes of 8.3 MB) get 5 planes = 41 MB for the same geometry latency (measured: 882 -> 878 us).
#ifndef SKS_EARLY_FILL_BYTES
#define SKS_EARLY_FILL_BYTES (36u << 20)
#endif
inline int early_fill_planes(unsigned flags, int planes, size_t plane_bytes)
{
    const int field = (int)((flags >> SKS_BIN_GROUPS_SHIFT) & 7u);
    if (field == 7) return planes;
    if (field) return (planes * field + 15) / 16;
    const size_t want = ((size_t)SKS_EARLY_FILL_BYTES + plane_bytes / 2) / plane_bytes;
    return (int)(want < (size_t)(planes / 4) ? want : (size_t)(planes / 4));
}

inline unsigned magic32(unsigned d) { return (unsigned)(((1ull << 32) + d - 1) / d); }   // x / d == umulhi(x, magic32(d)) for x * d < 2^32 (d >= 2)

// The geometry launch with the early-fill role (k_geom_fwd_fill) for the planes zid0 <= zid < zid1 (zid1 = every plane of the call,
// or the first plane a backward already zeroed: sks_forward_prefilled).  The early blocks are always
// linear (pass-major) fill blocks, also where the main launch uses row-aligned ones: whole planes change hands, so the
// two launches need not agree on how a band is cut.
// early_fill_cut: the early region's fill blocks per (plane, band) row and passes per block; false where the kernel's block
// index arithmetic would not be exact (a forced large E on very large images: the caller then keeps the one-launch layout).
bool early_fill_cut(const FwdArgs& a_in, int V, int gy, int gplanes, int zid0, int zid1, int& fsplit, int& pb)
{
    FwdArgs a = a_in;
    a.flags |= SKS_FILL_LINEAR;
    fill_geometry(a, true, false, fsplit, pb);
    const long long rows = (long long)fsplit * gy, nfill = rows * (zid1 - zid0);
    return fsplit >= 1 && pb >= 1 && nfill * rows < (1ll << 32) && (long long)V * gplanes + nfill < (1ll << 31);
}

void launch_geom_fill(const FwdArgs& a, const FwdCall& c, int gy, int gplanes, int zid0, int zid1, int fsplit, int pb, const ViewTan& vt,
                      ProfScope& prof)
{
    const hipStream_t st = c.stream;
    const long long rows = (long long)fsplit * gy, nfill = rows * (zid1 - zid0);
    const int ngeom = c.cam.V * gplanes;
    const EarlyFill f{ a.out_color, a.out_invdepth, a.C, a.W, a.H, gy, gplanes, ngeom, zid0, fsplit, pb, a.cp1_magic,
                       rows > 1 ? magic32((unsigned)rows) : 0u, fsplit > 1 ? magic32((unsigned)fsplit) : 0u };   // (0: divisor 1)
    const dim3 grid((unsigned)(ngeom + nfill));
    const size_t lds = (size_t)gy * cover_cw(a.W) * 4;   // one plane's cover rows (<= COVER_MAX_WORDS words: cover_enabled)
    const bool nt = !(a.flags & SKS_NO_NT_STORES);   // (fill_half_mode implies it)
    const int ppt = (a.W % 4 == 0 || fill_half_mode(a)) ? 4 : 1;
#define SKS_GF_ARGS f, a.P, vt, c.cam.viewmatrix, c.cam.projmatrix, c.g.means3D, c.g.opacities, c.g.scales, c.g.rotations, c.g.cov3D_precomp, \
                    c.g.scale_modifier, a.flags, a.g, c.io.radii, a.features, a.cover_planes
    if (ppt == 4 && nt) SKS_LAUNCH_FIRST(prof, (k_geom_fwd_fill<4, true>), grid, dim3(256), lds, st, SKS_GF_ARGS);
    else if (ppt == 4) SKS_LAUNCH_FIRST(prof, (k_geom_fwd_fill<4, false>), grid, dim3(256), lds, st, SKS_GF_ARGS);
    else SKS_LAUNCH_FIRST(prof, (k_geom_fwd_fill<1, false>), grid, dim3(256), lds, st, SKS_GF_ARGS);
#undef SKS_GF_ARGS
}

#ifndef SKS_GEOM_BINNED_THREADS
#define SKS_GEOM_BINNED_THREADS 256
#endif
// The plain geometry launch of a forward.  b: the binned path's scratch (all null on the small path); done: the event that rides on
// the kernel's own dispatch (sks_forward_backward's small path: no marker packet), or null.
void launch_geom_fwd(const FwdCall& c, const ViewTan& vt, const Geom& g, const Bin& b, bool small, int gplanes, hipEvent_t done)
{
    const Cameras& cam = c.cam;
    const int gthreads = small ? 256 : SKS_GEOM_BINNED_THREADS;
    const dim3 grid((cam.P + gthreads - 1) / gthreads, cam.V, gplanes);
#define SKS_G_ARGS cam.P, cam.W, cam.H, vt, cam.viewmatrix, cam.projmatrix, c.g.means3D, c.g.opacities, c.g.scales, c.g.rotations, c.g.cov3D_precomp, \
                   c.g.scale_modifier, c.g.flags, g, c.io.radii, 0, b.count, b.touched, c.g.features, cam.C, b.fmask, b.hdr,                          \
                   (small && cover_per_plane(cam.P, cam.W, cam.H, cam.C)) ? 1 : 0
    if (done) hipExtLaunchKernelGGL(k_geom_fwd, grid, dim3(gthreads), 0, c.stream, nullptr, done, 0, SKS_G_ARGS);
    else hipLaunchKernelGGL(k_geom_fwd, grid, dim3(gthreads), 0, c.stream, SKS_G_ARGS);
#undef SKS_G_ARGS
}

template <int CG>
void launch_fwd_binned(const FwdArgs& a, const BinView& bv, int V, int gx, int gy, const uint32_t* cover, hipStream_t st)
{
    int fsplit, pb;
    fill_geometry(a, true, true, fsplit, pb);
    const int xc = ((gx + TGROUP - 1) / TGROUP + a.C) / (a.C + 1);   // composite blocks (TGROUP tile columns each) spread over the rows
    dim3 grid(fsplit + xc, gy, (a.C + 1) * V);
    const bool nt = !(a.flags & SKS_NO_NT_STORES);
    if (a.W % 4 == 0) {
        if (nt) hipLaunchKernelGGL((k_render_fwd_binned<CG, 4, true>), grid, dim3(256), 0, st, a, bv, gx, gy, fsplit, pb, cover);
        else hipLaunchKernelGGL((k_render_fwd_binned<CG, 4, false>), grid, dim3(256), 0, st, a, bv, gx, gy, fsplit, pb, cover);
    } else if (fill_half_mode(a)) {
        hipLaunchKernelGGL((k_render_fwd_binned<CG, 4, true, true>), grid, dim3(256), 0, st, a, bv, gx, gy, fsplit, pb, cover);
    } else {
        hipLaunchKernelGGL((k_render_fwd_binned<CG, 1, false>), grid, dim3(256), 0, st, a, bv, gx, gy, fsplit, pb, cover);
    }
}

// whole tile bands per block of k_bin_scan (<= SCAN_T * SCAN_IPT tiles)
inline int bin_scan_bands(int gx) { return gx >= SCAN_T * 8 ? 1 : (SCAN_T * 8) / gx; }

// workgroups of the binned backward: a fixed number per compute unit of the current device, each walking the tile list
inline int bwd_tile_blocks()
{
    static const int n = [] {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) {
            hipDeviceProp_t pr;
            if (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) cus = pr.multiProcessorCount;
        }
        const char* e = getenv("SKS_BWD_TILE_BLOCKS");   // tuning sweeps only
        return (e && atoi(e) > 0) ? atoi(e) : cus * BWD_TILE_BLOCKS_PER_CU;
    }();
    return n;
}

// workgroups per (view, Gaussian) of k_render_bwd_wave (they share the BWD_SPLITS partial-sum slots; see the kernel)
inline int bwd_wave_groups(int V, int P, unsigned flags)
{
    unsigned t = (flags >> SKS_BWD_WG_SHIFT) & 7u;
    static const int env = [] { const char* e = getenv("SKS_BWD_WG"); return e ? atoi(e) : 0; }();   // tuning sweeps only
    if (!t && env > 0) t = (unsigned)env;
    if (t) return t > 5 ? 1 : (BWD_SPLITS >> (t - 1));
    const int pairs = V * P;
    return pairs <= BWD_WG_PAIRS16 ? 16 : (pairs <= BWD_WG_PAIRS8 ? 8 : 4);
}

// the fused-loss variant of the wave-resident backward: heat-maps as planes or (a.hm_row) as separable factors;
// ES: the per-frame early-stopping instantiations (sks_loop_fused_step_es, a.es_stop set)
template <bool ES = false>
inline void launch_bwd_loss(const BwdArgs& a, const ViewTan& vt, const ViewOff& vo, int V, hipStream_t st)
{
    const dim3 grid(a.P, V, bwd_wave_groups(V, a.P, a.flags));   // see launch_bwd_small
    // (two dispatches, not one with the test inside: the instantiations keep the order the device code was always emitted in)
    if (a.hm_row) with_cg(a.C, [&](auto cg) { hipLaunchKernelGGL((k_render_bwd_wave<decltype(cg)::value, false, true, true, ES>), grid, dim3(256), 0, st, a, vt, vo); });
    else with_cg(a.C, [&](auto cg) { hipLaunchKernelGGL((k_render_bwd_wave<decltype(cg)::value, false, true, false, ES>), grid, dim3(256), 0, st, a, vt, vo); });
}

// ---- prefill: the small-path backward's two launches zero the last planes of the NEXT forward's output set ----
// What sks_backward_prefill asks of backward_impl: the other set and the plane counts of the two launches.
struct PrefillReq {
    float* color;
    float* invdepth;
    int planes_wave, planes_geom;
};
// Passes (4 KB) per prefill block.  Its own knob: these blocks run at the backward's occupancy (4 workgroups per CU, not the
// forward's 8), so fewer are resident and each carries more.  SKS_PREFILL_PB: tuning sweeps only.
#ifndef SKS_PREFILL_PASSES
#define SKS_PREFILL_PASSES 2   /* H36M step, 25 planes: 1 pass 59.2 us, 2: 55.1, 3: 55.2, 4: 56.1, 8: 56.1, 16: 56.5 (MEASUREMENTS.md "Prefill") */
#endif
inline int prefill_passes()
{
    static const int n = [] { const char* e = getenv("SKS_PREFILL_PB"); return (e && atoi(e) > 0) ? atoi(e) : SKS_PREFILL_PASSES; }();
    return n > 32 ? 32 : n;
}
// 16-byte non-temporal stores on the wave-resident small path, or nothing
inline bool prefill_possible(int P, int W, int H, unsigned flags)
{
    return P >= 1 && P <= 64 && is_small(P, flags) && !(flags & (SKS_NO_NT_STORES | SKS_DEBUG_SYNC | SKS_BWD_LDS_LIST)) &&
           (W % 4 == 0 || (W % 4 == 2 && H % 2 == 0));
}
// The role's arguments for the planes [zid0, zid0 + nz) of the set (color, invdepth); false where the kernel's index arithmetic
// would not be exact or the grid would not fit (`extra` = blocks per unit the fill blocks are counted in: a blockIdx.z layer of
// k_render_bwd_wave, or 1).
bool prefill_cut(PreFill& f, float* color, float* invdepth, int V, int C, int W, int H, int zid0, int nz, long long per_unit, long long max_units)
{
    const int gy = TileGrid(W, H).gy;
    const int passes = (TILE * W + fill_lead(color, invdepth, W, H) + 1023) / 1024;
    const int pb = prefill_passes();
    const int fsplit = (passes + pb - 1) / pb;
    const long long rows = (long long)fsplit * gy, nfill = rows * nz;
    if (zid0 < 0 || nz < 1 || zid0 + nz > (C + 1) * V || nfill * rows >= (1ll << 32) || (nfill + per_unit - 1) / per_unit > max_units) return false;
    f = PreFill{ color, invdepth, C, W, H, gy, zid0, (unsigned)nfill, fsplit, pb, 0, ((1u << 20) + (unsigned)C) / (unsigned)(C + 1),
                 rows > 1 ? magic32((unsigned)rows) : 0u, fsplit > 1 ? magic32((unsigned)fsplit) : 0u };
    return true;
}

// small-path backward: the wave-resident variant (k_render_bwd_wave), else the LDS-list one (k_render_bwd_gather; SKS_BWD_LDS_LIST forces it, tests)
inline bool bwd_small_wave(int P, unsigned flags) { return P <= 64 && !(flags & SKS_BWD_LDS_LIST); }

// pf: the prefill role's arguments (wave-resident variant only), or null
template <int CG>
void launch_bwd_small(const BwdArgs& a, const ViewTan& vt, const ViewOff& vo, int V, bool dfeat, hipStream_t st, const ProfScope& prof,
                      const PreFill* pf = nullptr)
{
    // slot index slowest: a (view, Gaussian) only has work for its first ceil(pixels / 256) slots, so the idle workgroups
    // (half of them on the skeleton scenes) come last in dispatch order instead of holding wave slots the working ones
    // wait for (the fused-loss kernel fits 3 workgroups per CU: 768 of H36M's 1 088 at once)
    if (bwd_small_wave(a.P, a.flags)) {
        dim3 grid(a.P, V, bwd_wave_groups(V, a.P, a.flags));
        if (pf) {
            PreFill f = *pf;
            f.zs = (int)grid.z;
            grid.z += (unsigned)((f.nfill + (unsigned)(a.P * V) - 1) / (unsigned)(a.P * V));   // (<= 65535: prefill_cut)
            if (dfeat) SKS_LAUNCH(prof, (k_render_bwd_wave<CG, true, false, false, false, PreFill>), grid, dim3(256), 0, st, a, vt, vo, f);
            else SKS_LAUNCH(prof, (k_render_bwd_wave<CG, false, false, false, false, PreFill>), grid, dim3(256), 0, st, a, vt, vo, f);
            return;
        }
        if (dfeat) SKS_LAUNCH(prof, (k_render_bwd_wave<CG, true, false>), grid, dim3(256), 0, st, a, vt, vo);
        else SKS_LAUNCH(prof, (k_render_bwd_wave<CG, false, false>), grid, dim3(256), 0, st, a, vt, vo);
        return;
    }
    dim3 grid(a.P, V, BWD_SPLITS);
    const size_t lds = GatherLds<CG>::bytes((a.P + 15) & ~15, CG, a.C);
    if (lds > 48 * 1024) {  // gfx950 has 160 KB of LDS per CU; raise the per-kernel dynamic limit when P is large
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_render_bwd_gather<CG, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_render_bwd_gather<CG, false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    if (dfeat) SKS_LAUNCH(prof, (k_render_bwd_gather<CG, true>), grid, dim3(256), lds, st, a);
    else SKS_LAUNCH(prof, (k_render_bwd_gather<CG, false>), grid, dim3(256), lds, st, a);
}

// sks_prof_spin: one wavefront that does nothing for a given time (the 100 MHz wall clock) -- stands in for the wire time of a
// latency-bound collective when one GPU measures what a rank of many would see (bench.py)
__global__ void k_spin_us(unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// What sks_forward_backward hands its forward (forward_impl; sks_forward passes none): the points of the forward's launch sequence
// behind which the backward's launches go to the second stream.
struct FwdHook {
    hipEvent_t geom_done;                              // small path: rides on k_geom_fwd's own dispatch (no marker packet), or null
    int (*after_geom)(void* ctx);                      // small path: right behind the geometry kernel
    int (*after_group)(void* ctx, int g, int v0, int nv);   // binned path: behind the forward launch of view group g (views v0 .. v0 + nv)
    void* ctx;
};
constexpr int FB_MAX_EVENTS = BIN_MAX_GROUPS;
constexpr int FB_OVERLAP_MAX_PAIRS = BWD_WG_PAIRS16;   // (view, Gaussian) pairs up to which sks_forward_backward runs the backward beside the forward
struct FbEvents {   // created by a thread's first combined call, reused by every later one on the same device
    hipEvent_t geom = nullptr, done = nullptr;
    hipEvent_t grp[FB_MAX_EVENTS] = {};
    int dev = -1;
};
thread_local FbEvents tl_fb_events;
// The calling thread's events for a combined call that hands over through `ngroups` group events (0 = only geom / done): created
// on first use, re-created when the thread moved to another device.
int fb_events(int ngroups, FbEvents*& out)
{
    FbEvents& ev = tl_fb_events;
    int cur_dev = 0;
    HIP_TRY(hipGetDevice(&cur_dev));
    if (ev.geom && ev.dev != cur_dev) {   // (events belong to a device: a thread that moved to another one gets new ones)
        (void)hipEventDestroy(ev.geom);
        (void)hipEventDestroy(ev.done);
        for (hipEvent_t& e : ev.grp)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
        ev.geom = ev.done = nullptr;
    }
    // hand-over between two queues of ONE device: a device-scope release is all the waiting side needs (the default,
    // a system-scope fence, is what a host reader of the event would want)
    unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
    if (const char* e = getenv("SKS_FB_EVENT_FLAGS")) evf = (unsigned)strtoul(e, nullptr, 0);   // tuning
    if (!ev.geom) {
        ev.dev = cur_dev;
        HIP_TRY(hipEventCreateWithFlags(&ev.geom, evf));
        HIP_TRY(hipEventCreateWithFlags(&ev.done, evf));
    }
    for (int gi = 0; gi < ngroups && gi < FB_MAX_EVENTS; gi++)
        if (!ev.grp[gi]) HIP_TRY(hipEventCreateWithFlags(&ev.grp[gi], evf));
    out = &ev;
    return 0;
}

}  // namespace

extern "C" {

const char* sks_last_error(void) { return g_err; }
void sks_set_error_(const char* msg)  // used by the other translation units of the library
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
}
int sks_version(void) { return 14; }

int sks_scratch_bytes(int V, int P, int C, int W, int H, size_t bin_capacity, size_t* geom, size_t* binning, size_t* accum)
{
    if (int rc = check_common(V, P, C, W, H)) return rc;
    const TileGrid t(W, H);
    if (geom) *geom = geom_bytes(V, P > 0 ? P : 1, W, H, C);
    if (binning) *binning = bin_bytes(V, P, t.NT, bin_capacity, C + 1, (size_t)t.gy * cover_cw(W));
    if (accum) *accum = (size_t)V * (P > 0 ? P : 1) * BWD_SPLITS * (NACC + C) * sizeof(float);
    return 0;
}

int sks_launch_regime(int V, int P, int C, int W, int H, unsigned flags, int out_aligned128, int* out)
{
    if (int rc = check_common(V, P, C, W, H)) return rc;
    if (!out) return fail(-2, "sks_launch_regime: out must be provided");
    const TileGrid t(W, H);
    const bool small = is_small(P, flags);
    const bool cover = small && cover_enabled(P, W, H), per_plane = cover && cover_per_plane(P, W, H, C);
    FwdArgs a{};
    a.P = P, a.C = C, a.W = W, a.H = H, a.flags = flags;
    a.out_color = a.out_invdepth = (float*)(uintptr_t)(out_aligned128 ? 128 : 16);   // (only the low address bits are looked at)
    int fsplit = 0, pb = 0;
    fill_geometry(a, small ? cover : true, !small, fsplit, pb);
    const int ppt = (W % 4 == 0 || fill_half_mode(a)) ? 4 : 1;
    memset(out, 0, SKS_REGIME_INTS * sizeof(int));
    out[SKS_REGIME_PATH] = small ? 0 : 1;
    out[SKS_REGIME_COVER] = small ? (per_plane ? 2 : cover ? 1 : 0) : 2;
    out[SKS_REGIME_CW] = cover_cw(W);
    out[SKS_REGIME_PPT] = ppt;
    out[SKS_REGIME_HALF] = fill_half_mode(a) ? 1 : 0;
    out[SKS_REGIME_ROWMODE] = pb < 0 ? 1 : 0;
    out[SKS_REGIME_PB] = pb < 0 ? -pb : pb;
    out[SKS_REGIME_FSPLIT] = fsplit;
    out[SKS_REGIME_W_MAGIC] = fill_w_magic(W) ? 1 : 0;
    out[SKS_REGIME_BWD] = !small ? 2 : bwd_small_wave(P, flags) ? 0 : 1;
    out[SKS_REGIME_GX] = t.gx;
    out[SKS_REGIME_GY] = t.gy;
    out[SKS_REGIME_BPC] = small ? 0 : bin_scan_bands(t.gx);
    out[SKS_REGIME_LEAD] = fill_lead(a);
    out[SKS_REGIME_WAVE_GROUPS] = (small && bwd_small_wave(P, flags)) ? bwd_wave_groups(V, P, flags) : 0;
    return 0;
}

int sks_list_regime(int* out)
{
    if (!out) return fail(-2, "sks_list_regime: out must be provided");
    memset(out, 0, SKS_LIST_REGIME_INTS * sizeof(int));
    out[SKS_LIST_WAVE_SORT] = BIN_WAVE_SORT;
    out[SKS_LIST_WAVE_K] = 64 * WSORT_K;
    out[SKS_LIST_SORT_LDS] = SORT_LDS;
    out[SKS_LIST_LONG_LIST] = LONG_LIST;
    out[SKS_LIST_CLASSES] = BIN_CLASSES;
    out[SKS_LIST_BAND_THREADS] = BAND_TS;
    return 0;
}

}  // extern "C"

namespace {

int forward_impl(const FwdCall& c, const FwdHook* hook, int prefilled)
{
    const Cameras& cam = c.cam;
    const int V = cam.V, P = cam.P, C = cam.C, W = cam.W, H = cam.H;
    const unsigned flags = c.g.flags;
    const size_t bin_capacity = c.io.bin_capacity;
    if (int rc = check_common(cam)) return rc;
    const hipStream_t st = c.stream;
    if (prefilled < 0 || prefilled > (C + 1) * V) return fail(-1, "prefilled_planes=%d out of range [0,%d]", prefilled, (C + 1) * V);
    if (!c.io.out_color || !c.io.out_invdepth) return fail(-2, "out_color / out_invdepth must be provided");
    if (((uintptr_t)c.io.out_color | (uintptr_t)c.io.out_invdepth) & 15u)
        return fail(-2, "out_color / out_invdepth must be 16-byte aligned (the planes are written with 16-byte stores)");
    const size_t HW = (size_t)H * W;
    if (P == 0) {  // rasterize_points.cu:88: nothing rendered, outputs stay zero
        HIP_TRY(hipMemsetAsync(c.io.out_color, 0, (size_t)V * C * HW * 4, st));
        HIP_TRY(hipMemsetAsync(c.io.out_invdepth, 0, (size_t)V * HW * 4, st));
        if (c.final_T) return fail(-2, "final_T not available for P == 0");
        return 0;
    }
    if (int rc = require({ cam.viewmatrix, cam.projmatrix, cam.tanfovx, cam.tanfovy, c.g.means3D, c.g.features, c.g.opacities, c.io.radii, c.io.geom }))
        return rc;
    if (int rc = need_cov(c.g.scales, c.g.rotations, c.g.cov3D_precomp)) return rc;
    ViewTan vt;
    ViewOff vo;
    fill_views(vt, &vo, V, C, W, H, cam.tanfovx, cam.tanfovy, nullptr, nullptr);
    Geom g = geom_from(c.io.geom, V, P, W, H);
    const TileGrid t(W, H);
    const int gx = t.gx, gy = t.gy, NT = t.NT;

    const bool small = is_small(P, flags);
    Bin b{};
    if (!small) {
        if (!c.io.binning) return fail(-2, "binned path needs a binning buffer");
        if (bin_capacity < 1) return fail(-1, "binned path needs bin_capacity >= 1");
        b = bin_from(c.io.binning, V, P, NT, bin_capacity);
        // (nothing to clear: k_geom_fwd zeroes the header, k_bin_band_count writes every tile's count)
    }
    if (!small) g.cover = nullptr;   // (the binned path's cover rows are per plane: Bin::coverp, k_bin_scan + k_bin_sort_long)
    const int gplanes = (small && g.cover && cover_per_plane(P, W, H, C)) ? C + 1 : 1;     // a block per plane's cover rows
    FwdArgs a{ P, C, W, H, flags, g, c.g.features, c.io.out_color, c.io.out_invdepth, c.final_T, c.n_contrib, composite_slots(flags, V, P),
               ((1u << 20) + (unsigned)C) / (unsigned)(C + 1), 0, (!small || (g.cover && cover_per_plane(P, W, H, C))) ? 1 : 0,
               fill_w_magic(W) };
    // Plain small-path forward with cover rows: the geometry launch zeroes the last `early` planes (launch_geom_fill), the fill +
    // composite launch streams the planes in front of them, and ONE kind-0 scope spans both -- the time in which every byte of the
    // output was written.  Not for sks_forward_backward (its geom_done event fires when the geometry records exist, not when
    // the early fill has drained), not with the debug planes, not with a synchronise between the stages.
    const int planes = (C + 1) * V;
    // sks_forward_prefilled: the planes zid >= zp are zero already (the composite blocks still store their tiles there, as they
    // do behind the early region).  Ignored -- everything is filled -- with the debug planes, SKS_DEBUG_SYNC, the one-call hook, off
    // the small path, and where this launch is a kind-0 sample whose prefilling launches were not bracketed (the hook was enabled
    // in between): a sample is the time in which EVERY byte of the output was written.
    int pre = 0;
    if (prefilled > 0 && small && !hook && !c.final_T && !c.n_contrib && !(flags & SKS_DEBUG_SYNC) &&
        !(prof_next_forward_sampled() && !prof_has_parked(st)))
        pre = prefilled;
    const int zp = planes - pre;
    int early = 0;
    if (small && !hook && g.cover && !c.final_T && !c.n_contrib && !(flags & (SKS_DEBUG_SYNC | SKS_NO_EARLY_FILL))) {
        early = early_fill_planes(flags, planes, HW * 4);
        if (early > zp) early = zp;
    }
    int efs = 0, epb = 0;
    if (early > 0 && early_fill_cut(a, V, gy, gplanes, zp - early, zp, efs, epb)) {
        ProfScope prof(0, st, true, pre > 0);
        launch_geom_fill(a, c, gy, gplanes, zp - early, zp, efs, epb, vt, prof);
        with_cg(C, [&](auto cg) { launch_fwd_small<decltype(cg)::value>(a, V, gy, zp - early, st, prof); });
        HIP_TRY(hipGetLastError());
        return 0;
    }
    launch_geom_fwd(c, vt, g, b, small, gplanes, (hook && small) ? hook->geom_done : nullptr);
    STAGE_CHECK("geometry");
    if (hook && small && hook->after_geom) {   // (sks_forward_backward: the backward behind the geometry, on its own stream)
        if (int rc = hook->after_geom(hook->ctx)) return rc;
    }

    if (small) {
        {
            ProfScope prof(0, st, true, pre > 0);
            with_cg(C, [&](auto cg) { launch_fwd_small<decltype(cg)::value>(a, V, gy, zp, st, prof); });
        }
        STAGE_CHECK("render(small)");
        return 0;
    }
    uint32_t* cover = b.coverp;   // a row per (view, plane, band)
    const int cw = cover_cw(W);
    hipLaunchKernelGGL(k_bin_band_count, dim3(gy, V), dim3(BAND_TC), (size_t)2 * gx * 4, st, P, gx, g, b);
    int vg, ng;
    bin_groups(flags, V, vg, ng);
    {
        const int bpc = bin_scan_bands(gx);
        const int nchunk_t = (gy + bpc - 1) / bpc, nchunk_g = (P + SCAN_G - 1) / SCAN_G;
        hipLaunchKernelGGL(k_bin_scan, dim3(nchunk_t + nchunk_g, V), dim3(SCAN_T), (size_t)bpc * cw * 4, st, P, gx, gy, cw, bpc,
                           nchunk_t, bin_capacity, b, cover, c.io.num_rendered_dev, V, C + 1, vg);
    }
    hipLaunchKernelGGL(k_bin_band_scatter, dim3(gy, V), dim3(BAND_TS), (size_t)2 * gx * 4, st, P, gx, bin_capacity, g, b, C, cw);
    STAGE_CHECK("binning");
    const BinView bv_all = bin_view(b, NT, bin_capacity);
    {
        // one fill + composite launch per view group (one group = every view unless SKS_BIN_GROUPS asks for more): a group's launch
        // sees ITS views as views 0 .. nv - 1 -- every per-view array is handed over from the group's first view on; only the tile
        // descriptors (BinView::tlist, addressed through Bin::tidx) keep their call-wide positions
        ProfScope prof(0, st);
        for (int gi = 0; gi < ng; gi++) {
            const int v0 = gi * vg, nv = (V - v0 < vg) ? V - v0 : vg;
            FwdArgs ag = a;
            ag.out_color = a.out_color + (size_t)v0 * C * HW;
            ag.out_invdepth = a.out_invdepth + (size_t)v0 * HW;
            if (a.final_T) ag.final_T = a.final_T + (size_t)v0 * HW;
            if (a.n_contrib) ag.n_contrib = a.n_contrib + (size_t)v0 * HW;
            BinView bv = bv_all;
            bv.ranges += (size_t)v0 * NT;
            bv.tidx += (size_t)v0 * NT;
            bv.aux += (size_t)v0 * NT * TILE * TILE;
            bv.e_co += (size_t)v0 * bin_capacity;
            bv.e_xyd += (size_t)v0 * bin_capacity;
            bv.e_ids += (size_t)v0 * bin_capacity;
            bv.part += (size_t)v0 * bin_capacity * BIN_ROWS * NACC;
            const uint32_t* cov_g = cover + (size_t)v0 * (C + 1) * gy * cw;
            with_cg(C, [&](auto cg) { launch_fwd_binned<decltype(cg)::value>(ag, bv, nv, gx, gy, cov_g, st); });
            if (hook && hook->after_group)
                if (int rc = hook->after_group(hook->ctx, gi, v0, nv)) return rc;
        }
    }
    STAGE_CHECK("render(binned)");
    return 0;
}

// sks_backward in two phases, so that sks_forward_backward can place them: BWD_RENDER = the compositing backward (binned path:
// of view group `group`, or of every group in turn when group < 0), BWD_GEOM = the geometry backward behind it (binned path: of
// view group `group`'s views, or of all views when group < 0).
constexpr unsigned BWD_RENDER = 1u, BWD_GEOM = 2u;
int backward_impl(const BwdCall& c, unsigned phases, int group, const PrefillReq* pre)
{
    const Cameras& cam = c.cam;
    const int V = cam.V, P = cam.P, C = cam.C, W = cam.W, H = cam.H;
    const unsigned flags = c.g.flags;
    const Grads& gr = c.grads;
    if (int rc = check_common(cam)) return rc;
    if (P == 0) return 0;
    const hipStream_t st = c.stream;
    if (int rc = require({ cam.viewmatrix, cam.projmatrix, cam.tanfovx, cam.tanfovy, c.g.means3D, c.g.features, c.g.opacities, c.radii, c.geom,
                           c.up.dL_dout_color, c.up.accum, gr.dL_dmeans3D, gr.dL_dmeans2D, gr.dL_dopacity }))
        return rc;
    if (int rc = need_cov(c.g.scales, c.g.rotations, c.g.cov3D_precomp)) return rc;
    ViewTan vt;
    ViewOff vo;
    fill_views(vt, &vo, V, C, W, H, cam.tanfovx, cam.tanfovy, nullptr, nullptr);
    Geom g = geom_from(const_cast<void*>(c.geom), V, P, W, H);
    const TileGrid t(W, H);
    const int gx = t.gx, NT = t.NT;
    BwdArgs a{ P, C, W, H, flags, g, c.g.features, c.bg, c.up.dL_dout_color, c.up.dL_dout_invdepth, (float*)c.up.accum, nullptr, nullptr };
    const bool dfeat = gr.dL_dfeatures != nullptr;
    const bool small = is_small(P, flags);
    int vg = V, ng = 1;
    if (!small) bin_groups(flags, V, vg, ng);
    if (group >= ng) return fail(-1, "view group %d of %d", group, ng);
    // the geometry backward of all views in one workgroup (with the mean over the views): the launch that can carry planes_geom
    const bool geom_all = gr.dL_dmeans3D_mean && V * P <= 256 && small;
    PreFill pfw{}, pfg{};
    bool have_pfw = false, have_pfg = false;
    if (pre && pre->planes_wave + pre->planes_geom > 0) {
        // the call's last planes: the compositing backward's share first, the geometry backward's behind it -- all of them in the
        // compositing launch where the geometry backward is not k_geom_bwd_all
        const int planes = (C + 1) * V, n = pre->planes_wave + pre->planes_geom;
        const int n_geom = geom_all ? pre->planes_geom : 0, nw = n - n_geom;
        if (nw > 0) {
            if (!prefill_cut(pfw, pre->color, pre->invdepth, V, C, W, H, planes - n, nw, (long long)P * V, 65535 - BWD_SPLITS))
                return fail(-1, "sks_backward_prefill: %d planes of %dx%d do not fit the compositing backward's launch", nw, W, H);
            have_pfw = true;
        }
        if (n_geom > 0) {
            if (!prefill_cut(pfg, pre->color, pre->invdepth, V, C, W, H, planes - n_geom, n_geom, 1, (1ll << 31) - 2))
                return fail(-1, "sks_backward_prefill: %d planes of %dx%d do not fit the geometry backward's launch", n_geom, W, H);
            have_pfg = true;
        }
        // the next forward's kind-0 launch will be bracketed: so are the launches that write part of its output
        if (prof_next_forward_sampled()) prof_park_begin(st);
    }
    if ((phases & BWD_RENDER) && small) {
        ProfScope prof(1, st, true);
        const PreFill* pf = have_pfw ? &pfw : nullptr;
        with_cg(C, [&](auto cg) { launch_bwd_small<decltype(cg)::value>(a, vt, vo, V, dfeat, st, prof, pf); });
        STAGE_CHECK("render-backward(small)");
    } else if (phases & BWD_RENDER) {
        if (!c.binning) return fail(-2, "binned path needs the forward's binning buffer");
        Bin b = bin_from(const_cast<void*>(c.binning), V, P, NT, c.bin_capacity);
        BinView bv = bin_view(b, NT, c.bin_capacity);
        // the per-Gaussian sums go through the slot rows of the binning scratch (plain stores, every row written); only the
        // feature gradient, when wanted, is accumulated with atomics
        if (dfeat && group <= 0) HIP_TRY(hipMemsetAsync(c.up.accum, 0, (size_t)V * P * (NACC + C) * sizeof(float), st));
        dim3 grid(bwd_tile_blocks());
        const unsigned magic_nt = magic32((unsigned)NT), magic_gx = magic32((unsigned)gx);
        const bool extra = c.bg != nullptr || c.up.dL_dout_invdepth != nullptr;
        for (int gi = group < 0 ? 0 : group; gi < (group < 0 ? ng : group + 1); gi++) {
            // a view group's tiles: its stretch of every class's descriptor region, its class counters (k_bin_scan)
            const uint4* tl = b.tlist + (size_t)gi * vg * NT;
            const uint32_t* hd = b.hdr + gi * BIN_CLASSES;
            ProfScope prof(1, st);
            if (dfeat) hipLaunchKernelGGL((k_render_bwd_tile<true, true>), grid, dim3(BWD_TILE_THREADS), 0, st, a, bv, gx, V, magic_nt, magic_gx, tl, hd);
            else if (extra) hipLaunchKernelGGL((k_render_bwd_tile<false, true>), grid, dim3(BWD_TILE_THREADS), 0, st, a, bv, gx, V, magic_nt, magic_gx, tl, hd);
            else hipLaunchKernelGGL((k_render_bwd_tile<false, false>), grid, dim3(BWD_TILE_THREADS), 0, st, a, bv, gx, V, magic_nt, magic_gx, tl, hd);
        }
        STAGE_CHECK("render-backward(binned)");
    }
    if (!(phases & BWD_GEOM)) return 0;
    GeomBwdArgs ga{ P, C, W, H, flags, cam.viewmatrix, cam.projmatrix, c.g.means3D, c.g.opacities, c.g.scales, c.g.rotations, c.g.cov3D_precomp,
                    c.g.scale_modifier, c.radii, (const float*)c.up.accum, small ? BWD_SPLITS : 0, nullptr, nullptr, nullptr, gr.dL_dmeans3D, gr.dL_dmeans2D,
                    gr.dL_dopacity, gr.dL_dscales, gr.dL_drotations, gr.dL_dcov3D, gr.dL_dfeatures };
    if (!small) {
        Bin b = bin_from(const_cast<void*>(c.binning), V, P, NT, c.bin_capacity);
        ga.rect = g.rect;
        ga.goff = b.goff;
        ga.part = b.part;
        ga.cap = c.bin_capacity;
        ga.bin_hdr = b.hdr;
    }
    if (geom_all) {   // (the binned path's k_geom_bwd also re-arms the work cursors)
        if (have_pfg) hipLaunchKernelGGL((k_geom_bwd_all<PreFill>), dim3(1u + pfg.nfill), dim3(256), 0, st, ga, vt, V, gr.dL_dmeans3D_mean, pfg);
        else hipLaunchKernelGGL((k_geom_bwd_all<>), dim3(1), dim3(256), 0, st, ga, vt, V, gr.dL_dmeans3D_mean);
    } else {
        if (small) hipLaunchKernelGGL(k_geom_bwd, dim3((P + 255) / 256, V), dim3(256), 0, st, ga, vt);
        else {
            const int v0 = group < 0 ? 0 : group * vg, nv = group < 0 ? V : ((V - v0 < vg) ? V - v0 : vg);
            ga.v0 = v0;
            hipLaunchKernelGGL(k_geom_bwd_binned, dim3((P + GEOMB_G - 1) / GEOMB_G, nv), dim3(256), 0, st, ga, vt);
        }
        // (the mean over the views wants every view's gradients: with view groups, behind the last group's geometry backward)
        if (gr.dL_dmeans3D_mean && (small || group < 0 || group == ng - 1))
            hipLaunchKernelGGL(k_mean_views, dim3((3 * P + 255) / 256), dim3(256), 0, st, V, P, gr.dL_dmeans3D, gr.dL_dmeans3D_mean);
    }
    if (have_pfw || have_pfg) prof_park_end(st);
    STAGE_CHECK("geometry-backward");
    return 0;
}

// What the _dv entries of the fused step put where the host arrays of the plain ones stand:
const float NO_TAN[SKS_MAX_VIEWS] = {};                  // the by-value record carries the sizes only
const double NO_SCHED[5] = { 1.0, 1.0, 1.0, 0.0, 1.0 };  // every frame's schedule is read in the kernel
// sks_loop_fused_step{,_es,_dv,_es_dv}: the same two launches; with a criterion (c.es.es_state) in the early-stopping instantiations
// of both kernels.  c.views_dev (the _dv entries): the tail reads the per-view scalars from that device table and frame f's LR
// schedule from row f of c.lr_sched_dev; the compositing backward reads only the views' SIZES, which stay in its argument
// segment (view_wh: fixed per view slot)
int loop_fused_step_impl(const StepCall& c)
{
    const Cameras& cam = c.cam;
    const sksloop::Optimiser& opt = c.opt;
    const int V = cam.V, P = cam.P, C = cam.C, W = cam.W, H = cam.H, frames = c.hm.frames;
    const float* const* const hm_factors = c.hm.hm_factors;
    if (int rc = check_common(cam)) return rc;
    if (P < 1 || P > 64) return fail(-1, "fused step needs 1 <= P <= 64 (got %d)", P);
    if (int rc = check_frames(V, frames)) return rc;
    if (c.vw.mode < 0 || c.vw.mode > 2) return fail(-1, "fused step: vw_mode = %d, expected 0 (off), 1 (scale) or 2 (select)", c.vw.mode);
    if (c.es.es_state && (c.es.es_window < 1 || c.es.es_window > sksloop::ES_MAX_WINDOW))
        return fail(-1, "fused step: early-stopping window %d out of range [1, %d]", c.es.es_window, sksloop::ES_MAX_WINDOW);
    const int Vf = V / frames;   // views of one frame: the optimiser's V (slots, group mask, last_view are per frame)
    if (int rc = require({ cam.viewmatrix, cam.projmatrix, cam.tanfovx, cam.tanfovy, c.r.features, c.r.radii, c.r.geom,
                           c.r.gt ? (const void*)c.r.gt : (const void*)hm_factors, c.r.gt_totals, c.r.accum, c.r.loss_sums, c.r.packed }))
        return rc;
    if (int rc = check_hm_factors(hm_factors)) return rc;
    const hipStream_t st = c.stream;
    ViewTan vt;
    ViewOff vo;
    if (!fill_views(vt, &vo, V, C, W, H, cam.tanfovx, cam.tanfovy, c.hm.view_wh, c.hm.gt_offsets)) return bad_view_wh();
    if (int rc = check_wh_offsets(hm_factors, c.hm.view_wh, c.hm.gt_offsets)) return rc;
    const unsigned flags = c.r.flags | SKS_RAW_PARAMS | SKS_CLAMP01;
    sksloop::AdamArgs aa;
    if (const char* err = sksloop::fill_adam_args(aa, Vf, P, c.r.packed, opt)) return fail(-2, "%s", err);
    const bool es = c.es.es_state != nullptr;
    if (es) { aa.es_state = c.es.es_state; aa.es_window = c.es.es_window; aa.es_tol = c.es.es_tolerance; aa.es_host_flag = c.es.es_host_flags; }
    Geom g = geom_from(c.r.geom, V, P, W, H);
    g.cover = nullptr;   // no forward render on this path
    BwdArgs a{ P, C, W, H, flags, g, c.r.features, nullptr, c.r.gt, nullptr, (float*)c.r.accum, nullptr, nullptr };
    if (hm_factors) { a.hm_row = hm_factors[0]; a.hm_col = hm_factors[1]; a.hm_cmin = hm_factors[2]; a.hm_den = hm_factors[3]; }
    if (es) { a.es_stop = c.es.es_state + 1; a.es_stride = 2 + 2 * c.es.es_window; a.es_views = Vf; }
    {
        ProfScope prof(1, st);
        if (!es) launch_bwd_loss(a, vt, vo, V, st);
        else launch_bwd_loss<true>(a, vt, vo, V, st);
    }
    STAGE_CHECK("render-backward(fused loss)");
    GeomBwdArgs ga{ P, C, W, H, flags, cam.viewmatrix, cam.projmatrix, opt.xyz, opt.opacity, opt.scaling, opt.rotation, nullptr, c.r.scale_modifier,
                    c.r.radii, (const float*)c.r.accum, BWD_SPLITS, c.r.gt_totals, c.r.loss_sums, c.r.packed, nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, nullptr };
    if (c.vw.mode) {   // the view-agreement instantiations: the same four forms with the weights' record behind the arguments
        const sksloop::ViewWeightArgs vw = c.vw;
        if (c.views_dev) {
            const ViewTanDev vd = views_dev_from(c.views_dev, c.lr_sched_dev);
            if (es) hipLaunchKernelGGL((k_step_tail_vw<true, ViewTanDev>), dim3(frames), dim3(256), 0, st, ga, vd, aa, Vf, g, c.r.radii, vw);
            else hipLaunchKernelGGL((k_step_tail_vw<false, ViewTanDev>), dim3(frames), dim3(256), 0, st, ga, vd, aa, Vf, g, c.r.radii, vw);
        } else if (es) hipLaunchKernelGGL(k_step_tail_vw<true>, dim3(frames), dim3(256), 0, st, ga, vt, aa, Vf, g, c.r.radii, vw);
        else hipLaunchKernelGGL(k_step_tail_vw<false>, dim3(frames), dim3(256), 0, st, ga, vt, aa, Vf, g, c.r.radii, vw);
    } else if (c.views_dev) {
        const ViewTanDev vd = views_dev_from(c.views_dev, c.lr_sched_dev);
        if (es) hipLaunchKernelGGL((k_step_tail<true, ViewTanDev>), dim3(frames), dim3(256), 0, st, ga, vd, aa, Vf, g, c.r.radii);
        else hipLaunchKernelGGL((k_step_tail<false, ViewTanDev>), dim3(frames), dim3(256), 0, st, ga, vd, aa, Vf, g, c.r.radii);
    } else if (es) hipLaunchKernelGGL(k_step_tail<true>, dim3(frames), dim3(256), 0, st, ga, vt, aa, Vf, g, c.r.radii);
    else hipLaunchKernelGGL(k_step_tail<false>, dim3(frames), dim3(256), 0, st, ga, vt, aa, Vf, g, c.r.radii);
    STAGE_CHECK("step tail");
    return 0;
}

}  // namespace

extern "C" {

// An entry point's parameters carry the names of include/skelsplat_hip.h, and so do the records' fields: each macro fills one
// block from the parameters of the SAME NAME (a parameter that is missing or misnamed does not compile).
#define SKS_TAKE_CAMERAS(r)                                                                                                                    \
    ((r).V = V, (r).P = P, (r).C = C, (r).W = W, (r).H = H, (r).viewmatrix = viewmatrix, (r).projmatrix = projmatrix, (r).tanfovx = tanfovx, (r).tanfovy = tanfovy)
#define SKS_TAKE_GAUSSIANS(r)                                                                                                                  \
    ((r).means3D = means3D, (r).features = features, (r).opacities = opacities, (r).scales = scales, (r).rotations = rotations,                \
     (r).cov3D_precomp = cov3D_precomp, (r).scale_modifier = scale_modifier, (r).flags = flags)
#define SKS_TAKE_FORWARD_IO(r)                                                                                                                 \
    ((r).out_color = out_color, (r).out_invdepth = out_invdepth, (r).radii = radii, (r).geom = geom, (r).binning = binning,                    \
     (r).bin_capacity = bin_capacity, (r).num_rendered_dev = num_rendered_dev)
#define SKS_TAKE_UPSTREAM(r) ((r).dL_dout_color = dL_dout_color, (r).dL_dout_invdepth = dL_dout_invdepth, (r).accum = accum)
#define SKS_TAKE_GRADS(r)                                                                                                                      \
    ((r).dL_dmeans3D = dL_dmeans3D, (r).dL_dmeans2D = dL_dmeans2D, (r).dL_dopacity = dL_dopacity, (r).dL_dscales = dL_dscales,                 \
     (r).dL_drotations = dL_drotations, (r).dL_dcov3D = dL_dcov3D, (r).dL_dfeatures = dL_dfeatures, (r).dL_dmeans3D_mean = dL_dmeans3D_mean)
// (ft, nc: final_T / n_contrib, which sks_forward_backward does not have)
#define SKS_TAKE_FWD_CALL(c, ft, nc) \
    (SKS_TAKE_CAMERAS((c).cam), SKS_TAKE_GAUSSIANS((c).g), SKS_TAKE_FORWARD_IO((c).io), (c).final_T = (ft), (c).n_contrib = (nc), (c).stream = (hipStream_t)stream)
#define SKS_TAKE_BWD_CALL(c)                                                                                                                   \
    (SKS_TAKE_CAMERAS((c).cam), (c).bg = bg, SKS_TAKE_GAUSSIANS((c).g), (c).radii = radii, (c).geom = geom, (c).binning = binning,             \
     (c).bin_capacity = bin_capacity, SKS_TAKE_UPSTREAM((c).up), SKS_TAKE_GRADS((c).grads), (c).stream = (hipStream_t)stream)
// (the fused step; the _dv entries: tanfovx = tanfovy = NO_TAN, sched = NO_SCHED, views_dev / lr_sched_dev set beside the macro)
#define SKS_TAKE_STEP_CALL(c, sched)                                                                                                           \
    (SKS_TAKE_CAMERAS((c).cam), (c).r.features = features, (c).r.scale_modifier = scale_modifier, (c).r.flags = flags, (c).r.radii = radii,    \
     (c).r.geom = geom, (c).r.gt = gt, (c).r.gt_totals = gt_totals, (c).r.accum = accum, (c).r.loss_sums = loss_sums, (c).r.packed = packed,   \
     SKS_TAKE_OPTIMISER((c).opt, sched), (c).hm.view_wh = view_wh, (c).hm.gt_offsets = gt_offsets, (c).hm.frames = frames,                     \
     (c).hm.hm_factors = hm_factors, (c).stream = (hipStream_t)stream)
#define SKS_TAKE_ES(r) ((r).es_state = es_state, (r).es_window = es_window, (r).es_tolerance = es_tolerance, (r).es_host_flags = es_host_flags)

int sks_forward(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                const float* tanfovx, const float* tanfovy, const float* means3D, const float* features,
                const float* opacities, const float* scales, const float* rotations, const float* cov3D_precomp,
                float scale_modifier, unsigned flags, float* out_color, float* out_invdepth, int* radii, void* geom,
                void* binning, size_t bin_capacity, int* num_rendered_dev, float* final_T, uint32_t* n_contrib,
                void* stream)
{
    FwdCall c;
    SKS_TAKE_FWD_CALL(c, final_T, n_contrib);
    return forward_impl(c, nullptr, 0);
}

int sks_backward(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                 const float* tanfovx, const float* tanfovy, const float* bg, const float* means3D,
                 const float* features, const float* opacities, const float* scales, const float* rotations,
                 const float* cov3D_precomp, float scale_modifier, unsigned flags, const int* radii, const void* geom,
                 const void* binning, size_t bin_capacity, const float* dL_dout_color, const float* dL_dout_invdepth,
                 void* accum, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dopacity, float* dL_dscales,
                 float* dL_drotations, float* dL_dcov3D, float* dL_dfeatures, float* dL_dmeans3D_mean, void* stream)
{
    BwdCall c;
    SKS_TAKE_BWD_CALL(c);
    return backward_impl(c, BWD_RENDER | BWD_GEOM, -1, nullptr);
}

int sks_forward_prefilled(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                          const float* tanfovx, const float* tanfovy, const float* means3D, const float* features,
                          const float* opacities, const float* scales, const float* rotations, const float* cov3D_precomp,
                          float scale_modifier, unsigned flags, float* out_color, float* out_invdepth, int* radii, void* geom,
                          void* binning, size_t bin_capacity, int* num_rendered_dev, float* final_T, uint32_t* n_contrib,
                          int prefilled_planes, void* stream)
{
    FwdCall c;
    SKS_TAKE_FWD_CALL(c, final_T, n_contrib);
    return forward_impl(c, nullptr, prefilled_planes);
}

int sks_backward_prefill(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                         const float* tanfovx, const float* tanfovy, const float* bg, const float* means3D,
                         const float* features, const float* opacities, const float* scales, const float* rotations,
                         const float* cov3D_precomp, float scale_modifier, unsigned flags, const int* radii, const void* geom,
                         const void* binning, size_t bin_capacity, const float* dL_dout_color, const float* dL_dout_invdepth,
                         void* accum, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dopacity, float* dL_dscales,
                         float* dL_drotations, float* dL_dcov3D, float* dL_dfeatures, float* dL_dmeans3D_mean,
                         float* next_color, float* next_invdepth, int planes_wave, int planes_geom, void* stream)
{
    if (int rc = check_common(V, P, C, W, H)) return rc;
    if (planes_wave < 0 || planes_geom < 0 || (long long)planes_wave + planes_geom > (long long)(C + 1) * V)
        return fail(-1, "sks_backward_prefill: planes_wave=%d planes_geom=%d out of range (the call has %d planes)", planes_wave, planes_geom, (C + 1) * V);
    const PrefillReq req{ next_color, next_invdepth, planes_wave, planes_geom };
    if (planes_wave + planes_geom > 0) {
        // (SKS_NO_NT_STORES is the store kind of the FORWARD's fill role: it has no bearing on these stores, and a backward's recorded
        // flags may carry it from a forward that has since been re-tuned)
        if (!prefill_possible(P, W, H, flags & ~SKS_NO_NT_STORES))
            return fail(-1, "sks_backward_prefill: no prefill for this call (wave-resident small path with 16-byte non-temporal stores only: "
                            "1 <= P <= 64, W %% 4 == 0 or W %% 4 == 2 with an even H, no SKS_NO_NT_STORES / SKS_DEBUG_SYNC / SKS_FORCE_BINNED)");
        if (!next_color || !next_invdepth) return fail(-2, "sks_backward_prefill: next_color / next_invdepth must be provided");
        if (((uintptr_t)next_color | (uintptr_t)next_invdepth) & 15u) return fail(-2, "next_color / next_invdepth must be 16-byte aligned");
    }
    BwdCall c;
    SKS_TAKE_BWD_CALL(c);
    return backward_impl(c, BWD_RENDER | BWD_GEOM, -1, planes_wave + planes_geom > 0 ? &req : nullptr);
}

// The rule: how many of the call's last planes the small-path backward's two launches should zero for the next forward.  A function
// of the call, like early_fill_planes: BYTES per launch in whole planes, because what the bytes hide under is the launches' latency,
// not the image.  Together with the early region at most half of the call's planes.
// It answers 0 / 0 outside what was measured: the constants were swept on the H36M step alone -- 68 (view, Gaussian) pairs, one
// round of 1088 workgroups of the compositing backward at 4 per CU (the CG <= 20 instantiations without the feature gradient),
// 16-byte stores on W % 4 == 0 -- and beside a store stream the backward can lengthen by more than the forward shortens.  So:
// V * P within a quarter of 68 either way (51 .. 85) at 16 workgroups per pair, C <= 20, W % 4 == 0 (not the pair-masked
// W % 4 == 2 images: 1002 wide); a caller that also asks for the feature gradient (the 1-wave-per-SIMD instantiations) should
// not prefill either -- the rule cannot see that, rasterizer.Workspace does.  sks_backward_prefill itself carries any count on
// any shape it can store 16 bytes on: whoever measures a case outside this widens the rule.
// Constants from the interleaved sweep on the H36M two-call step (planes of 4 MB; MEASUREMENTS.md "Prefill"; us per step):
// compositing launch alone 0 / 6 / 12 / 18 planes: 62.0 / 60.4 / 58.2 / 57.0; geometry launch alone 0 / 4 / 7: 62.0 / 61.2 / 60.4;
// both: (12, 4) 57.2, (12, 7) 56.3, (18, 7) 56.1, (20, 7) 56.8; and at 2 passes per block (12, 7) 55.0, (14, 7) 54.9, (16, 7) 55.3,
// (18, 7) 55.5, (20, 7) 55.8, (18, 5) 56.0, (18, 9) 55.1 -- 56 MB and 28 MB are the smallest sizes beyond which nothing is gained.
#ifndef SKS_PREFILL_WAVE_BYTES
#define SKS_PREFILL_WAVE_BYTES 56000000u
#endif
#ifndef SKS_PREFILL_GEOM_BYTES
#define SKS_PREFILL_GEOM_BYTES 28000000u
#endif
int sks_prefill_planes(int V, int P, int C, int W, int H, unsigned flags, int* planes_wave, int* planes_geom)
{
    if (int rc = check_common(V, P, C, W, H)) return rc;
    if (!planes_wave || !planes_geom) return fail(-2, "sks_prefill_planes: planes_wave / planes_geom must be provided");
    *planes_wave = *planes_geom = 0;
    if (!prefill_possible(P, W, H, flags) || !cover_enabled(P, W, H)) return 0;
    const int planes = (C + 1) * V;
    const size_t plane_bytes = (size_t)H * W * 4;
    const int early = (flags & SKS_NO_EARLY_FILL) ? 0 : early_fill_planes(flags, planes, plane_bytes);
    int room = planes / 2 - early;
    if (room <= 0) return 0;
    if (W % 4 != 0 || C > 20 || V * P < 51 || V * P > 85 || bwd_wave_groups(V, P, flags) != 16) return 0;   // (not measured: see above)
    long long nw = ((long long)SKS_PREFILL_WAVE_BYTES + plane_bytes / 2) / plane_bytes;
    long long ng = ((long long)SKS_PREFILL_GEOM_BYTES + plane_bytes / 2) / plane_bytes;
    if (nw > room) nw = room;
    if (ng > room - nw) ng = room - nw;
    PreFill f;   // (what the launches could not index is not promised)
    if (nw > 0 && !prefill_cut(f, nullptr, nullptr, V, C, W, H, planes - (int)(nw + ng), (int)nw, (long long)P * V, 65535 - BWD_SPLITS)) nw = 0;
    if (ng > 0 && !prefill_cut(f, nullptr, nullptr, V, C, W, H, planes - (int)ng, (int)ng, 1, (1ll << 31) - 2)) ng = 0;
    *planes_wave = (int)nw;
    *planes_geom = (int)ng;
    return 0;
}

int sks_forward_backward(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                         const float* tanfovx, const float* tanfovy, const float* means3D, const float* features,
                         const float* opacities, const float* scales, const float* rotations, const float* cov3D_precomp,
                         float scale_modifier, unsigned flags, float* out_color, float* out_invdepth, int* radii, void* geom,
                         void* binning, size_t bin_capacity, int* num_rendered_dev, const float* bg,
                         const float* dL_dout_color, const float* dL_dout_invdepth, void* accum, float* dL_dmeans3D,
                         float* dL_dmeans2D, float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                         float* dL_dfeatures, float* dL_dmeans3D_mean, void* stream, void* aux_stream, unsigned fb_flags)
{
    const bool small = is_small(P, flags);
    // the binned path overlaps by VIEW GROUPS (the backward of a group starts from what the forward's compositor left per pixel of
    // ITS views); how many: bin_groups, as for sks_forward / sks_backward (the flags stay the caller's)
    int vg = V, ng = 1;
    if (!small && V >= 1) bin_groups(flags, V, vg, ng);
    const hipStream_t st = (hipStream_t)stream, aux = (hipStream_t)aux_stream;
    FwdCall fwd;
    SKS_TAKE_FWD_CALL(fwd, nullptr, nullptr);
    BwdCall bwd;
    SKS_TAKE_BWD_CALL(bwd);
    struct Ctx {
        const BwdCall& bwd;   // the call's backward on the second stream
        hipStream_t s;
        bool ext, handed;     // handed: the second stream holds work of this call
        int rc_aux;
    } c{ bwd, st, true, false, 0 };
    {
        static const bool ext_off = [] { const char* e = getenv("SKS_FB_EXT"); return e && atoi(e) == 0; }();   // tuning
        if (ext_off) c.ext = false;
    }
    const bool no_join = (fb_flags & SKS_FB_NO_JOIN) != 0;
    // The step's form per workload: beside the forward the small path's backward pays while it is a handful of workgroups (H36M's 4
    // views: 1 088, step 66 -> 58 us; one rank's 4 Panoptic views) and costs more than it hides once its wavefronts crowd the fill
    // blocks out (all 31 Panoptic views, 589 (view, Gaussian) pairs: 0.908 ms beside, 0.893 behind -- the forward 817 -> 866 us, the
    // backward 56 -> 133).  Beyond FB_OVERLAP_MAX_PAIRS the call runs its two halves one after the other -- unless the caller
    // keeps the second stream's tail for itself (SKS_FB_NO_JOIN: a sharded step's collective wants the gradients THERE).
    const bool crowded = small && (long long)V * P > FB_OVERLAP_MAX_PAIRS && !no_join;
    if (!aux_stream || aux_stream == stream || P == 0 || (flags & SKS_DEBUG_SYNC) || (!small && ng < 2) || crowded) {
        // nothing to run side by side: one after the other on the caller's stream (the one-call form keeps its launch layout on
        // every route: no early fill)
        fwd.g.flags |= SKS_NO_EARLY_FILL;
        if (int rc = forward_impl(fwd, nullptr, 0)) return rc;
        if (int rc = backward_impl(bwd, BWD_RENDER | BWD_GEOM, -1, nullptr)) return rc;
        // SKS_FB_NO_JOIN: the caller enqueues what follows the gradients on aux_stream -- they must be ordered THERE on this branch
        // as on the overlapped ones (aux_stream waits for everything the call put on `stream`)
        if (no_join && aux_stream && aux_stream != stream) {
            FbEvents* ev = nullptr;
            if (int rc = fb_events(0, ev)) return rc;
            HIP_TRY(hipEventRecord(ev->done, st));
            HIP_TRY(hipStreamWaitEvent(aux, ev->done, 0));
        }
        return 0;
    }
    FbEvents* evp = nullptr;
    if (int rc = fb_events(small ? 0 : ng, evp)) return rc;
    FbEvents& ev = *evp;
    bwd.stream = aux;
    struct Run {
        // small path: behind the geometry kernel, i.e. behind everything the caller enqueued -- the whole backward
        static int after_geom(void* p)
        {
            Ctx& k = *(Ctx*)p;
            FbEvents& e = tl_fb_events;
            if (!k.ext) HIP_TRY(hipEventRecord(e.geom, k.s));   // (else it rode on k_geom_fwd's dispatch)
            HIP_TRY(hipStreamWaitEvent(k.bwd.stream, e.geom, 0));
            k.handed = true;
            return k.rc_aux = backward_impl(k.bwd, BWD_RENDER | BWD_GEOM, -1, nullptr);
        }
        // binned path: view group g's forward is enqueued -- its compositing and geometry backward go to the second stream, where
        // they run beside the forward of group g + 1
        static int after_group(void* p, int g, int, int)
        {
            Ctx& k = *(Ctx*)p;
            FbEvents& e = tl_fb_events;
            HIP_TRY(hipEventRecord(e.grp[g], k.s));
            HIP_TRY(hipStreamWaitEvent(k.bwd.stream, e.grp[g], 0));
            k.handed = true;
            return k.rc_aux = backward_impl(k.bwd, BWD_RENDER | BWD_GEOM, g, nullptr);
        }
    };
    const FwdHook hook{ (small && c.ext) ? ev.geom : nullptr, small ? &Run::after_geom : nullptr, small ? nullptr : &Run::after_group, &c };
    int rc = forward_impl(fwd, &hook, 0);
    if (rc == 0 && !c.handed) rc = fail(-3, "sks_forward_backward: the forward did not reach the point the backward starts from");
    // The gradients are the caller's in stream order -- unless the caller has more to enqueue behind the backward on aux_stream
    // (a view-sharded step's collective: hidden under the forward as well) and joins the two streams itself.  After an ERROR
    // behind the hand-over the join is made whatever the caller asked for: what the second stream already holds reads `geom` and
    // writes the gradient tensors, and the caller's stream must not run ahead of it.
    if (c.handed && (!no_join || rc != 0)) {
        const hipError_t e1 = hipEventRecord(ev.done, aux);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(c.s, ev.done, 0) : e1;
        if (rc == 0 && e2 != hipSuccess) rc = fail((int)e2, "sks_forward_backward: joining the two streams: %s", hipGetErrorString(e2));
    }
    return rc;
}

int sks_mean_views(int V, int P, const float* dL_dmeans3D, int shard_world, float* mean_out, void* stream)
{
    if (V < 1 || P < 1 || shard_world < 1) return fail(-1, "mean_views: bad shape");
    if (!dL_dmeans3D || !mean_out) return fail(-2, "mean_views: missing pointer");
    hipLaunchKernelGGL(k_mean_views, dim3((3 * P + 255) / 256), dim3(256), 0, (hipStream_t)stream, V, P, dL_dmeans3D, mean_out,
                       shard_world);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sks_gt_tile_stats(int V, int C, int W, int H, const float* gt, float* tile_S, float* tile_N, double* totals, void* stream)
{
    if (int rc = check_common(V, 1, C, W, H)) return rc;
    if (!gt || !totals) return fail(-2, "gt_tile_stats: missing pointer");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(totals, 0, (size_t)V * 2 * sizeof(double), st));
    dim3 grid(TileGrid(W, H).gy, C, V);
    hipLaunchKernelGGL(k_gt_tile_stats, grid, dim3(256), 0, st, C, W, H, gt, tile_S, tile_N, totals);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sks_backward_fused_loss(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                            const float* tanfovx, const float* tanfovy, const float* bg, const float* means3D,
                            const float* features, const float* opacities, const float* scales, const float* rotations,
                            const float* cov3D_precomp, float scale_modifier, unsigned flags, const int* radii,
                            const void* geom, const float* gt, const float* tile_S, const float* tile_N,
                            const double* gt_totals, void* accum, float* dL_dmeans3D, float* dL_dmeans2D,
                            float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                            double* loss_sums, float* packed_raw_grads, const int* view_wh, const size_t* gt_offsets,
                            const float* const* hm_factors, void* stream)
{
    if (int rc = check_common(V, P, C, W, H)) return rc;
    if (P < 1 || P > 64) return fail(-1, "fused-loss backward needs 1 <= P <= 64 (got %d)", P);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = require({ viewmatrix, projmatrix, tanfovx, tanfovy, means3D, features, opacities, radii, geom,
                           gt ? (const void*)gt : (const void*)hm_factors, gt_totals, accum, dL_dmeans3D, dL_dmeans2D, dL_dopacity, loss_sums }))
        return rc;
    if (int rc = check_hm_factors(hm_factors)) return rc;
    if (int rc = need_cov(scales, rotations, cov3D_precomp)) return rc;
    ViewTan vt;
    ViewOff vo;
    if (!fill_views(vt, &vo, V, C, W, H, tanfovx, tanfovy, view_wh, gt_offsets)) return bad_view_wh();
    if (int rc = check_wh_offsets(hm_factors, view_wh, gt_offsets)) return rc;
    Geom g = geom_from(const_cast<void*>(geom), V, P, W, H);
    BwdArgs a{ P, C, W, H, flags | SKS_CLAMP01, g, features, bg, gt, nullptr, (float*)accum, tile_S, tile_N };
    if (hm_factors) { a.hm_row = hm_factors[0]; a.hm_col = hm_factors[1]; a.hm_cmin = hm_factors[2]; a.hm_den = hm_factors[3]; }
    {
        ProfScope prof(1, st);
        launch_bwd_loss(a, vt, vo, V, st);
    }
    STAGE_CHECK("fused loss + render-backward");
    GeomBwdArgs ga{ P, C, W, H, flags, viewmatrix, projmatrix, means3D, opacities, scales, rotations, cov3D_precomp,
                    scale_modifier, radii, (const float*)accum, BWD_SPLITS, gt_totals, loss_sums, packed_raw_grads, dL_dmeans3D, dL_dmeans2D,
                    dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, nullptr };
    hipLaunchKernelGGL(k_geom_bwd, dim3((P + 255) / 256, V), dim3(256), 0, st, ga, vt);
    STAGE_CHECK("geometry-backward");
    return 0;
}

int sks_geometry(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix, const float* tanfovx,
                 const float* tanfovy, const float* means3D, const float* opacities, const float* scales,
                 const float* rotations, const float* cov3D_precomp, float scale_modifier, unsigned flags, int* radii,
                 void* geom, const int* view_wh, int frames, void* stream)
{
    if (int rc = check_common(V, P, C, W, H)) return rc;
    if (P < 1) return fail(-1, "P must be positive");
    if (int rc = check_frames(V, frames)) return rc;
    if (int rc = require({ viewmatrix, projmatrix, tanfovx, tanfovy, means3D, opacities, radii, geom })) return rc;
    if (int rc = need_cov(scales, rotations, cov3D_precomp)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ViewTan vt;
    if (!fill_views(vt, nullptr, V, C, W, H, tanfovx, tanfovy, view_wh, nullptr)) return bad_view_wh();
    Geom g = geom_from(geom, V, P, W, H);
    g.cover = nullptr;   // (the cover rows serve the dense forward: sks_forward makes its own)
    hipLaunchKernelGGL(k_geom_fwd, dim3((P + 255) / 256, V), dim3(256), 0, st, P, W, H, vt, viewmatrix, projmatrix,
                       means3D, opacities, scales, rotations, cov3D_precomp, scale_modifier, flags, g, radii,
                       frames > 1 ? V / frames : 0);
    STAGE_CHECK("geometry");
    return 0;
}

int sks_geometry_dv(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix, const void* views_dev,
                    const float* means3D, const float* opacities, const float* scales, const float* rotations,
                    const float* cov3D_precomp, float scale_modifier, unsigned flags, int* radii, void* geom, int frames,
                    void* stream)
{
    if (int rc = check_common(V, P, C, W, H)) return rc;
    if (P < 1) return fail(-1, "P must be positive");
    if (int rc = check_frames(V, frames)) return rc;
    if (int rc = require({ viewmatrix, projmatrix, views_dev, means3D, opacities, radii, geom })) return rc;
    if (int rc = need_cov(scales, rotations, cov3D_precomp)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Geom g = geom_from(geom, V, P, W, H);
    g.cover = nullptr;
    hipLaunchKernelGGL(k_geom_fwd_dv, dim3((P + 255) / 256, V), dim3(256), 0, st, P, views_dev_from(views_dev), viewmatrix,
                       projmatrix, means3D, opacities, scales, rotations, cov3D_precomp, scale_modifier, flags, g, radii,
                       frames > 1 ? V / frames : 0);
    STAGE_CHECK("geometry");
    return 0;
}

// The four forms of the fused step (loop_fused_step_impl): each fills the StepCall from its parameters
int sks_loop_fused_step(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                        const float* tanfovx, const float* tanfovy, const float* features, float scale_modifier,
                        unsigned flags, int* radii, void* geom, const float* gt, const double* gt_totals, void* accum,
                        double* loss_sums, float* packed, float* slots, unsigned long long group_mask, int last_view,
                        float* xyz, float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq,
                        int* counters, int acc_steps, const double* lr_sched, const double* lrs, const double* adam,
                        float lambda_consistency, const int* limb, const int* view_wh, const size_t* gt_offsets, int frames,
                        const float* const* hm_factors, void* stream)
{
    StepCall c{};
    SKS_TAKE_STEP_CALL(c, lr_sched);
    return loop_fused_step_impl(c);
}

int sks_loop_fused_step_es(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                           const float* tanfovx, const float* tanfovy, const float* features, float scale_modifier,
                           unsigned flags, int* radii, void* geom, const float* gt, const double* gt_totals, void* accum,
                           double* loss_sums, float* packed, float* slots, unsigned long long group_mask, int last_view,
                           float* xyz, float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq,
                           int* counters, int acc_steps, const double* lr_sched, const double* lrs, const double* adam,
                           float lambda_consistency, const int* limb, const int* view_wh, const size_t* gt_offsets, int frames,
                           const float* const* hm_factors, int* es_state, int es_window, float es_tolerance,
                           int* es_host_flags, void* stream)
{
    if (!es_state)
        return fail(-2, "loop_fused_step_es: es_state is required (sks_loop_fused_step is the step without a criterion)");
    if (es_window < 1 || es_window > sksloop::ES_MAX_WINDOW)
        return fail(-1, "loop_fused_step_es: window %d out of range [1, %d]", es_window, sksloop::ES_MAX_WINDOW);
    StepCall c{};
    SKS_TAKE_STEP_CALL(c, lr_sched);
    SKS_TAKE_ES(c.es);
    return loop_fused_step_impl(c);
}

int sks_loop_fused_step_dv(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                           const void* views_dev, const float* features, float scale_modifier, unsigned flags, int* radii,
                           void* geom, const float* gt, const double* gt_totals, void* accum, double* loss_sums, float* packed,
                           float* slots, unsigned long long group_mask, int last_view, float* xyz, float* scaling,
                           float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq, int* counters, int acc_steps,
                           const double* lr_sched_dev, const double* lrs, const double* adam, float lambda_consistency,
                           const int* limb, const int* view_wh, const size_t* gt_offsets, int frames,
                           const float* const* hm_factors, void* stream)
{
    if (!views_dev || !lr_sched_dev) return fail(-2, "loop_fused_step_dv: views_dev and lr_sched_dev are required");
    const float *const tanfovx = NO_TAN, *const tanfovy = NO_TAN;
    StepCall c{};
    SKS_TAKE_STEP_CALL(c, NO_SCHED);
    c.views_dev = views_dev, c.lr_sched_dev = lr_sched_dev;
    return loop_fused_step_impl(c);
}

int sks_loop_fused_step_es_dv(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                              const void* views_dev, const float* features, float scale_modifier, unsigned flags, int* radii,
                              void* geom, const float* gt, const double* gt_totals, void* accum, double* loss_sums,
                              float* packed, float* slots, unsigned long long group_mask, int last_view, float* xyz,
                              float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq, int* counters,
                              int acc_steps, const double* lr_sched_dev, const double* lrs, const double* adam,
                              float lambda_consistency, const int* limb, const int* view_wh, const size_t* gt_offsets,
                              int frames, const float* const* hm_factors, int* es_state, int es_window, float es_tolerance,
                              int* es_host_flags, void* stream)
{
    if (!views_dev || !lr_sched_dev) return fail(-2, "loop_fused_step_es_dv: views_dev and lr_sched_dev are required");
    if (!es_state)
        return fail(-2, "loop_fused_step_es_dv: es_state is required (sks_loop_fused_step_dv is the step without a criterion)");
    if (es_window < 1 || es_window > sksloop::ES_MAX_WINDOW)
        return fail(-1, "loop_fused_step_es_dv: window %d out of range [1, %d]", es_window, sksloop::ES_MAX_WINDOW);
    const float *const tanfovx = NO_TAN, *const tanfovy = NO_TAN;
    StepCall c{};
    SKS_TAKE_STEP_CALL(c, NO_SCHED);
    c.views_dev = views_dev, c.lr_sched_dev = lr_sched_dev;
    SKS_TAKE_ES(c.es);
    return loop_fused_step_impl(c);
}

// The view-agreement forms: es_state == NULL is the step without a criterion, vw_mode == 0 the plain mean (loop_fused_step_impl)
#define SKS_TAKE_VW(r) ((r).mode = vw_mode, (r).threshold = vw_threshold, (r).weights = vw_weights, (r).similarity = vw_similarity)
int sks_loop_fused_step_vw(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                           const float* tanfovx, const float* tanfovy, const float* features, float scale_modifier,
                           unsigned flags, int* radii, void* geom, const float* gt, const double* gt_totals, void* accum,
                           double* loss_sums, float* packed, float* slots, unsigned long long group_mask, int last_view,
                           float* xyz, float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq,
                           int* counters, int acc_steps, const double* lr_sched, const double* lrs, const double* adam,
                           float lambda_consistency, const int* limb, const int* view_wh, const size_t* gt_offsets, int frames,
                           const float* const* hm_factors, int* es_state, int es_window, float es_tolerance,
                           int* es_host_flags, int vw_mode, float vw_threshold, float* vw_weights, float* vw_similarity,
                           void* stream)
{
    StepCall c{};
    SKS_TAKE_STEP_CALL(c, lr_sched);
    if (es_state) SKS_TAKE_ES(c.es);
    SKS_TAKE_VW(c.vw);
    return loop_fused_step_impl(c);
}

int sks_loop_fused_step_vw_dv(int V, int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                              const void* views_dev, const float* features, float scale_modifier, unsigned flags, int* radii,
                              void* geom, const float* gt, const double* gt_totals, void* accum, double* loss_sums,
                              float* packed, float* slots, unsigned long long group_mask, int last_view, float* xyz,
                              float* scaling, float* rotation, float* opacity, float* exp_avg, float* exp_avg_sq, int* counters,
                              int acc_steps, const double* lr_sched_dev, const double* lrs, const double* adam,
                              float lambda_consistency, const int* limb, const int* view_wh, const size_t* gt_offsets,
                              int frames, const float* const* hm_factors, int* es_state, int es_window, float es_tolerance,
                              int* es_host_flags, int vw_mode, float vw_threshold, float* vw_weights, float* vw_similarity,
                              void* stream)
{
    if (!views_dev || !lr_sched_dev) return fail(-2, "loop_fused_step_vw_dv: views_dev and lr_sched_dev are required");
    const float *const tanfovx = NO_TAN, *const tanfovy = NO_TAN;
    StepCall c{};
    SKS_TAKE_STEP_CALL(c, NO_SCHED);
    c.views_dev = views_dev, c.lr_sched_dev = lr_sched_dev;
    if (es_state) SKS_TAKE_ES(c.es);
    SKS_TAKE_VW(c.vw);
    return loop_fused_step_impl(c);
}

int sks_prof_spin(double microseconds, void* stream)
{
    if (!(microseconds >= 0.0) || microseconds > 1e6) return fail(-1, "prof_spin: 0 .. 1e6 us");
    hipLaunchKernelGGL(k_spin_us, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long)(microseconds * 100.0));
    HIP_TRY(hipGetLastError());
    return 0;
}

int sks_prof_enable(int on)
{
    if (!tl_prof) {
        if (!on) return 0;
        tl_prof = new ProfState();
    }
    tl_prof->on = on != 0;
    tl_prof->every = (on & 0xffff) > 1 ? (on & 0xffff) : 1;
    tl_prof->skip = (on >> 16) & 3;
    tl_prof->recorded = (on >> 18) & 1;
    tl_prof->seen[0] = tl_prof->seen[1] = 0;
    tl_prof->parked = false;
    return 0;
}

int sks_prof_count(int kind, long long* launches)
{
    if (kind < 0 || kind > 1 || !launches) return fail(-2, "bad profile query");
    *launches = tl_prof ? tl_prof->kind[kind].n : 0;
    return 0;
}

int sks_prof_read(int kind, double* total_ms, long long* launches)
{
    if (kind < 0 || kind > 1 || !total_ms || !launches) return fail(-2, "bad profile query");
    if (!tl_prof) { *total_ms = 0.0; *launches = 0; return 0; }
    ProfKind& p = tl_prof->kind[kind];
    double tot = 0;
    for (int i = 0; i < p.n; i++) {
        float ms = 0;
        HIP_TRY(prof_elapsed(p, i, &ms));
        tot += ms;
    }
    *total_ms = tot;
    *launches = p.n;
    p.n = 0;
    return 0;
}

int sks_prof_read_quantiles(int kind, double* q_ms /* 3: p10, p50, p90 */, double* total_ms, long long* launches)
{
    if (kind < 0 || kind > 1 || !q_ms || !total_ms || !launches) return fail(-2, "bad profile query");
    if (!tl_prof) { q_ms[0] = q_ms[1] = q_ms[2] = 0.0; *total_ms = 0.0; *launches = 0; return 0; }
    ProfKind& p = tl_prof->kind[kind];
    static thread_local float t[PROF_MAX];
    double tot = 0;
    for (int i = 0; i < p.n; i++) {
        HIP_TRY(prof_elapsed(p, i, &t[i]));
        tot += t[i];
    }
    const int n = p.n;
    for (int i = 1; i < n; i++) {   // insertion sort: n is a few dozen samples
        const float v = t[i];
        int j = i - 1;
        for (; j >= 0 && t[j] > v; j--) t[j + 1] = t[j];
        t[j + 1] = v;
    }
    q_ms[0] = n ? t[(int)(0.1 * (n - 1) + 0.5)] : 0.0;
    q_ms[1] = n ? t[(n - 1) / 2] : 0.0;
    q_ms[2] = n ? t[(int)(0.9 * (n - 1) + 0.5)] : 0.0;
    *total_ms = tot;
    *launches = n;
    p.n = 0;
    return 0;
}

int sks_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     void* stream)
{
    (void)projmatrix;  // in_frustum only uses the view-space depth (auxiliary.h:166)
    if (P < 0) return fail(-1, "P negative");
    if (P == 0) return 0;
    if (int rc = require({ means3D, viewmatrix, present })) return rc;
    hipLaunchKernelGGL(k_mark_visible, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, means3D, viewmatrix, present);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sks_export_lists(int V, int W, int H, const void* binning, size_t bin_capacity, uint32_t* point_list,
                     uint32_t* ranges, void* stream)
{
    if (int rc = require({ binning, point_list, ranges })) return rc;
    const int NT = TileGrid(W, H).NT;
    Bin b = bin_from(const_cast<void*>(binning), V, 1, NT, bin_capacity);   // (nothing per Gaussian is read: its arrays come last)
    const size_t m = bin_capacity > (size_t)NT ? bin_capacity : (size_t)NT;
    hipLaunchKernelGGL(k_export_lists, dim3((unsigned)((m + 255) / 256), V), dim3(256), 0, (hipStream_t)stream, NT,
                       bin_capacity, b.ranges, b.nrend, point_list, ranges);
    hipLaunchKernelGGL(k_export_sorted, dim3((NT + 3) / 4, V), dim3(256), 0, (hipStream_t)stream, bin_view(b, NT, bin_capacity),
                       point_list);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
