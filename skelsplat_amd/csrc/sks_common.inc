// sks_common.inc -- part of the sks_raster.hip translation unit (included inside its anonymous namespace, in order):
// error helpers, launch-timing hook, constants, per-view records and scratch carving.
thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail((int)e_, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

#define STAGE_CHECK(name)                                                                      \
    do {                                                                                       \
        HIP_TRY(hipGetLastError());                                                            \
        if (flags & SKS_DEBUG_SYNC) {                                                          \
            hipError_t e_ = hipStreamSynchronize(st);                                          \
            if (e_ != hipSuccess) return fail((int)e_, "stage %s: %s", name, hipGetErrorString(e_)); \
        }                                                                                      \
    } while (0)

// ---- measurement hook (sks_prof_enable / sks_prof_read) ----
// Per host thread (the library's only other state is the thread-local error text): a thread that never enables the hook
// pays one thread-local pointer test per launch sequence, and two threads driving two GPUs do not share event lists.
constexpr int PROF_MAX = 16384;
struct ProfKind {
    hipEvent_t b[PROF_MAX], e[PROF_MAX];
    int created = 0, n = 0;
    // kind 0 only: sample i's second interval, the prefill-carrying launches of the backward in front of its forward (ProfState::park)
    hipEvent_t xb[PROF_MAX], xe[PROF_MAX];
    bool hasx[PROF_MAX];
    int xcreated = 0;
};
struct ProfState {
    bool on = false;
    int every = 1;        // bracket every n-th launch of a kind (an event pair costs ~3 us of queue time per launch)
    int skip = 0;         // bit k: launches of kind k are not bracketed
    bool recorded = false;   // bracket with hipEventRecord marker packets even where the launch could carry the pair itself
    int seen[2] = { 0, 0 };
    ProfKind kind[2];
    // A backward that zeroes planes of the NEXT forward's outputs (sks_backward_prefill) while that forward's kind-0 launch will be
    // bracketed brackets its own launches with this pair and parks it; the forward's scope takes it over (ProfScope, take_parked),
    // so that a kind-0 sample stays the time in which every byte of the call's output was written.
    hipEvent_t park_b = nullptr, park_e = nullptr;
    bool parked = false;
    hipStream_t park_st = nullptr;
};
thread_local ProfState* tl_prof = nullptr;   // allocated by the first sks_prof_enable of the thread

struct ProfScope {  // brackets ONE kernel launch -- or two back to back, SKS_LAUNCH_FIRST -- with a begin / end event pair
    // Two ways: recorded = hipEventRecord before and after (two marker packets in the queue: ~3 us of queue time per
    // bracketed launch, measured: 68 -> 73 -> 82 us per H36M step bracketing no / every 8th / every launch); ext = the
    // pair is handed to hipExtLaunchKernelGGL, which stamps it from the kernel's own dispatch packet (SKS_LAUNCH below).
    ProfKind* k = nullptr;
    hipStream_t st;
    bool ext;
    bool began = false;   // the begin event already stands in front of, or rides on, an earlier dispatch of this scope (SKS_LAUNCH_FIRST)
    // take_parked (kind 0): this forward renders into planes the backward in front of it zeroed -- its parked pair joins the sample
    ProfScope(int kind, hipStream_t s, bool ext_ = false, bool take_parked = false) : st(s), ext(ext_)
    {
        ProfState* ps = tl_prof;
        if (!ps) return;
        const bool parked = kind == 0 && ps->parked && take_parked && ps->park_st == s;
        if (kind == 0) ps->parked = false;   // (a parked pair belongs to the very next forward or to none)
        if (!ps->on || ((ps->skip >> kind) & 1)) return;
        if (ps->seen[kind]++ % ps->every != 0) return;
        ProfKind& p = ps->kind[kind];
        if (p.n >= PROF_MAX) return;
        if (p.n >= p.created) {
            if (hipEventCreate(&p.b[p.created]) != hipSuccess || hipEventCreate(&p.e[p.created]) != hipSuccess) return;
            p.created++;
        }
        p.hasx[p.n] = false;
        if (parked) {
            while (p.xcreated <= p.n) {
                if (hipEventCreate(&p.xb[p.xcreated]) != hipSuccess || hipEventCreate(&p.xe[p.xcreated]) != hipSuccess) return;
                p.xcreated++;
            }
            hipEvent_t t = p.xb[p.n]; p.xb[p.n] = ps->park_b; ps->park_b = t;
            t = p.xe[p.n]; p.xe[p.n] = ps->park_e; ps->park_e = t;
            p.hasx[p.n] = true;
        }
        k = &p;
        if (ps->recorded) ext = false;
        if (!ext) (void)hipEventRecord(p.b[p.n], st);
    }
    hipEvent_t eb() const { return k->b[k->n]; }
    hipEvent_t ee() const { return k->e[k->n]; }
    ~ProfScope()
    {
        if (!k) return;
        if (!ext) (void)hipEventRecord(k->e[k->n], st);
        k->n++;
    }
};
// Will the next kind-0 scope of this thread be a sample?  (what a prefilling backward and a prefill-consuming forward ask)
inline bool prof_next_forward_sampled()
{
    const ProfState* ps = tl_prof;
    return ps && ps->on && !(ps->skip & 1) && ps->seen[0] % ps->every == 0 && ps->kind[0].n < PROF_MAX;
}
inline bool prof_has_parked(hipStream_t st) { return tl_prof && tl_prof->parked && tl_prof->park_st == st; }
// the prefilling backward's bracket: marker packets in front of its first and behind its last launch
inline void prof_park_begin(hipStream_t st)
{
    ProfState* ps = tl_prof;
    ps->parked = false;
    if (!ps->park_b && (hipEventCreate(&ps->park_b) != hipSuccess || hipEventCreate(&ps->park_e) != hipSuccess)) { ps->park_b = ps->park_e = nullptr; return; }
    ps->park_st = st;
    ps->parked = hipEventRecord(ps->park_b, st) == hipSuccess;
}
inline void prof_park_end(hipStream_t st)
{
    ProfState* ps = tl_prof;
    if (ps && ps->parked && ps->park_st == st && hipEventRecord(ps->park_e, st) != hipSuccess) ps->parked = false;
}
// a sample's duration: its own pair plus, where a parked pair joined it, that one
inline hipError_t prof_elapsed(ProfKind& p, int i, float* ms)
{
    hipError_t e = hipEventSynchronize(p.e[i]);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, p.b[i], p.e[i]);
    if (e == hipSuccess && p.hasx[i]) {
        float x = 0;
        e = hipEventSynchronize(p.xe[i]);
        if (e == hipSuccess) e = hipEventElapsedTime(&x, p.xb[i], p.xe[i]);
        *ms += x;
    }
    return e;
}
// launch inside an `ext` ProfScope: the scope's events ride on the kernel's dispatch when it is active
#define SKS_LAUNCH(prof, kernel, grid, block, lds, stream, ...)                                                  \
    do {                                                                                                         \
        if ((prof).k)                                                                                            \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, (prof).began ? nullptr : (prof).eb(), (prof).ee(), 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                  \
    } while (0)
// the first of TWO launches one scope brackets: the begin event rides on this dispatch, the end event on the SKS_LAUNCH behind it
#define SKS_LAUNCH_FIRST(prof, kernel, grid, block, lds, stream, ...)                                            \
    do {                                                                                                         \
        if ((prof).k && (prof).ext) hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, (prof).eb(), nullptr, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);   /* (recorded: the scope's marker is in front) */ \
        (prof).began = (prof).k != nullptr;                                                                      \
    } while (0)

constexpr int NACC = 8;           // per-Gaussian accumulators before the feature block:
                                  // 0,1 dL_dmean2D.xy  2,3,4 dL_dconic.{x,y,w}  5 dL_dopacity  6 dL_dinvdepth  7 pad
constexpr int BWD_SPLITS = 16;    // small path backward: partial-sum slots per (view, Gaussian)
constexpr int BWD_WG_PAIRS16 = 400;   // wave-resident backward: up to this many (view, Gaussian) pairs one workgroup per slot,
constexpr int BWD_WG_PAIRS8 = 4096;   // up to this many two slots per workgroup, beyond four (bwd_wave_groups; measured, fused
                                      // loss: 68 / 272 / 1088 pairs = 26.3 / 37.9 / 87.9 us per group with 16, 28.8 / 38.6 / 80.7
                                      // with 8; Panoptic's 589 pairs through sks_backward: 64.7 / 60.0 / 64.2 us with 16 / 8 / 4)

struct ViewTan {   // per-view camera scalars, handed to the kernels by value (kernel-argument segment: scalar loads)
    float x[SKS_MAX_VIEWS];
    float y[SKS_MAX_VIEWS];
    int w[SKS_MAX_VIEWS];   // image size of each view: one launch sequence may carry views of different sizes on the
    int h[SKS_MAX_VIEWS];   // paths that write no dense (V,C,H,W) tensor (H36M mixes 1000- and 1002-wide sensors, Q11)
};
// where view v's planes start inside dL_dout_color / the heat-maps (floats from the base pointer); uniform sizes:
// v * C * H * W (one (V,C,H,W) tensor), mixed sizes: the caller's per-view offsets into one flat buffer
struct ViewOff {
    unsigned long long off[SKS_MAX_VIEWS];
};
// host: fills both; view_wh (V x {W,H}) / plane_off (V) may be NULL = uniform W x H.  Returns false on a bad size.
// The same record where it lives in DEVICE memory (the *_dv entry points: the table sks_rig_select fills, laid out as a ViewTan):
// `vt.x[v]` reads alike from either, so the geometry code is written once and the kernels' _dv twins differ in this argument only.
// A captured hipGraph then holds a pointer, not the cameras' scalars.  sched: the tail's per-frame LR schedule rows
// (sks_loop_fused_step_dv's lr_sched_dev), nullptr elsewhere.
struct ViewTanDev {
    const float* x;
    const float* y;
    const int* w;
    const int* h;
    const double* sched;
};
inline ViewTanDev views_dev_from(const void* views_dev, const double* sched = nullptr)
{
    const ViewTan* t = (const ViewTan*)views_dev;
    return ViewTanDev{ t->x, t->y, t->w, t->h, sched };   // (addresses only: nothing is read on the host)
}
inline bool fill_views(ViewTan& vt, ViewOff* vo, int V, int C, int W, int H, const float* tanfovx, const float* tanfovy,
                       const int* view_wh, const size_t* plane_off)
{
    for (int v = 0; v < V; v++) {
        vt.x[v] = tanfovx[v];
        vt.y[v] = tanfovy[v];
        vt.w[v] = view_wh ? view_wh[2 * v] : W;
        vt.h[v] = view_wh ? view_wh[2 * v + 1] : H;
        if (vt.w[v] < 1 || vt.h[v] < 1 || vt.w[v] > W || vt.h[v] > H) return false;
        if (vo) vo->off[v] = plane_off ? (unsigned long long)plane_off[v] : (unsigned long long)v * C * H * W;
    }
    return true;
}

struct Geom {  // per-(view, Gaussian) records kept for backward ("geomBuffer")
    float4* co;    // conic.x, conic.y, conic.z, opacity * h_convolution_scaling   (forward.cu:269)
    float4* xyd;   // pixel centre x, y, view depth, 1/depth
    uint4* rect;   // tile rect xmin, ymin, xmax, ymax (all 0 when culled)
    uint32_t* cover;  // per (view, tile band): word 0 = "some rect crosses this band", then one bit per tile column;
                      // nullptr when not produced (P > SKS_SMALL_P or the image has too many tiles)
};

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// SKS_RAW_PARAMS: the caller passes the LEAF parameters (_opacity logits, _scaling log-scales, _rotation raw
// quaternions) and the activations of scene/gaussian_model.py:39-47 (sigmoid / exp / F.normalize) run in-kernel.
struct Activated {
    float opacity, s[3], q[4], qnorm;
};
__device__ __forceinline__ Activated activate(bool raw, float op, const float s[3], const float q[4])
{
    Activated a;
    if (raw) {
        a.opacity = 1.0f / (1.0f + expf_fixed(-op));
#pragma unroll
        for (int k = 0; k < 3; k++) a.s[k] = expf_fixed(s[k]);
        const float nn = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        a.qnorm = fmaxf(sqrtf(nn), 1e-12f);
#pragma unroll
        for (int k = 0; k < 4; k++) a.q[k] = q[k] / a.qnorm;
    } else {
        a.opacity = op;
        a.qnorm = 1.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) a.s[k] = s[k];
#pragma unroll
        for (int k = 0; k < 4; k++) a.q[k] = q[k];
    }
    return a;
}

#ifndef SKS_COVER_MAX_WORDS
#define SKS_COVER_MAX_WORDS 6144
#endif
constexpr int COVER_MAX_WORDS = SKS_COVER_MAX_WORDS;  // LDS bitmap of k_geom_fwd (24 KB): bands x words of one view, x (C + 1) planes when that fits
// words per (view, band) cover row: [any, bit words...], padded to a multiple of 4 so that a row is 16-byte aligned and a
// fill block fetches it with ONE scalar load (two for rows of 5..8 words)
__host__ __device__ inline int cover_cw(int W) { return (1 + (((W + TILE - 1) / TILE) + 31) / 32 + 3) & ~3; }
inline bool cover_enabled(int P, int W, int H)
{
    return P <= SKS_SMALL_P && ((H + TILE - 1) / TILE) * cover_cw(W) <= COVER_MAX_WORDS;
}
// A row set per output PLANE (the compositor then stores only the planes its tile's list touches, the fill role zeroes the others
// in whole rows) when a view's (C + 1) row sets fit k_geom_fwd's LDS bitmap: H36M 18 x 63 x 4 words, occlusion-person 16 x 45 x 4;
// not Panoptic's 20 x 68 x 8 -- there the 20 x larger row set through the scalar cache cost the forward more than the planes saved
// (809 -> 815 us) and the geometry kernel 5.6 -> 9.0 us.
inline bool cover_per_plane(int P, int W, int H, int C)
{
    return cover_enabled(P, W, H) && (C + 1) * ((H + TILE - 1) / TILE) * cover_cw(W) <= COVER_MAX_WORDS;
}
inline Geom geom_from(void* base, int V, int P, int W, int H)
{
    char* p = (char*)base;
    Geom g;
    size_t n = (size_t)V * P;
    g.co = (float4*)p; p += align256(n * sizeof(float4));
    g.xyd = (float4*)p; p += align256(n * sizeof(float4));
    g.rect = (uint4*)p; p += align256(n * sizeof(uint4));
    g.cover = cover_enabled(P, W, H) ? (uint32_t*)p : nullptr;   // (a row per (view, band), or per (view, plane, band): cover_per_plane)
    return g;
}
inline size_t geom_bytes(int V, int P, int W, int H, int C)
{
    const int planes = cover_per_plane(P, W, H, C) ? C + 1 : 1;
    return 3 * align256((size_t)V * P * 16) + align256((size_t)V * planes * ((H + TILE - 1) / TILE) * cover_cw(W) * 4);
}

// Binned path scratch ("binningBuffer" + ImageState::ranges, rasterizer_impl.h:29-73), carved from the caller's buffer.
// Entries (the reference's (key, Gaussian index) pairs, rasterizer_impl.cu:70-108) are RECORDS here: the scatter kernel copies
// what the compositors need of a Gaussian next to its index, so a tile's wavefront fetches its list in one round trip.  Lists of
// up to BIN_WAVE_SORT entries are scattered in arrival order; the forward's compositor orders them by (depth bits, index) in
// registers and writes them back in that order (with each entry's strip mask), so the backward and the export read sorted
// lists; longer ones are sorted in place by k_bin_band_scatter before the forward.
constexpr int BIN_WAVE_SORT = 64;
// The other list-length switches of the binned path (sks_binned.inc), kept here so that sks_list_regime reports what the kernels use:
constexpr int WSORT_K = 4;             // lists of BIN_WAVE_SORT + 1 .. 64 * WSORT_K entries: sort_list_wave, in the forward's wavefront
constexpr int SORT_LDS = 2048;         // longer ones: sort_long_tile, in LDS up to SORT_LDS keys, beyond in the partial-sum rows
constexpr int LONG_LIST = 256;         // long tiles of a band remembered by column in k_bin_band_scatter (more: found again by a walk)
constexpr int BIN_ROWS = 2;            // partial-sum rows per slot: one per 8-row half of the tile (a wavefront of the backward)
constexpr int BIN_CLASSES = 8;         // tile classes by list length: class c holds lengths [2^c, 2^(c+1)), the last one the rest
constexpr int BIN_HDR_CLASS = 8;        // Bin::hdr[BIN_HDR_CLASS + g * BIN_CLASSES + c]: number of non-empty tiles of class c in view group g
constexpr int BIN_MAX_GROUPS = 7;       // view groups of one call (the 64-word header holds 7 x BIN_CLASSES counters behind its 8 fixed words)
// sks_forward_backward's default on the binned path (with a second stream): ONE group = the forward, then the backward.  Measured on
// the stress scene (8 views at 2048 x 2048, interleaved with the two calls on one box, ms per step): 1 group 0.559 (two calls
// 0.558), 2 groups 0.652, 4 groups 0.767, 7 groups 0.773, the second stream at high priority the same -- the tile backward's
// 128-register wavefronts take the wave slots the forward's fill blocks live on, and the forward loses more than the backward's
// whole duration (NOTES_experiments.md, round 6).  The mechanism stays (SKS_BIN_GROUPS, tests hold it bit-identical).
#ifndef SKS_BIN_FB_GROUPS
#define SKS_BIN_FB_GROUPS 1
#endif
constexpr int BIN_FB_GROUPS = SKS_BIN_FB_GROUPS;
// views per group / number of groups for a call's SKS_BIN_GROUPS request (both sides of a forward / backward pair derive them
// from the same flags and V).  Every binned entry point -- sks_forward, sks_backward, sks_forward_backward -- resolves the count
// HERE and nowhere else: a field of zero (the caller chose no count) is the build's default BIN_FB_GROUPS, or the SKS_BIN_GROUPS
// environment variable of a tuning sweep (read once per process), so a state's later backward walks the groups its forward laid out
// whichever entry point made either half.
inline int bin_groups_default()
{
    static const int n = [] {
        const char* e = getenv("SKS_BIN_GROUPS");
        const int want = (e && atoi(e) > 0) ? atoi(e) : BIN_FB_GROUPS;
        return want < 1 ? 1 : (want > BIN_MAX_GROUPS ? BIN_MAX_GROUPS : want);
    }();
    return n;
}
inline void bin_groups(unsigned flags, int V, int& vg, int& ng)
{
    const unsigned field = (flags >> SKS_BIN_GROUPS_SHIFT) & 7u;
    int want = field ? 1 + (int)field : bin_groups_default();
    if (want > BIN_MAX_GROUPS) want = BIN_MAX_GROUPS;
    if (want > V) want = V;
    vg = (V + want - 1) / want;
    ng = (V + vg - 1) / vg;
}
struct Bin {
    uint32_t* hdr;      // 64 words: [0] arena overflow flag, [1] number of lists longer than a wavefront, [BIN_HDR_CLASS + g *
                        // BIN_CLASSES + c] number of non-empty tiles of length class c in view group g (bin_groups; one group = all
                        // views unless the caller asks for more); cleared by k_geom_fwd
    uint32_t* count;    // V*NT   entries per tile (k_bin_band_count writes every one, k_bin_scan reads)
    uint32_t* cursor;   // V*NT   exclusive scan of count in tile order (k_bin_band_scatter keeps its cursors in LDS)
    uint2* ranges;      // V*NT   the reference's ImageState::ranges: [begin, end) into the view's entry arrays, (0,0) when empty
    int* nrend;         // V      entries per view (the reference's num_rendered)
    uint32_t* longt;    // V*(cap/BIN_WAVE_SORT + 1): view * NT + tile of the tiles with more than BIN_WAVE_SORT entries
    uint4* tlist;       // BIN_CLASSES * V*NT: {view * NT + tile, range begin, range end, channels} of the non-empty tiles, one
                        //        region of V*NT per length class (view group g's tiles from g * vg * NT on), any order inside a
                        //        (class, group): what the backward's workgroups walk,
                        //        longest lists first (a fixed round-robin over a list ordered by cost stays balanced; in tile
                        //        order the slowest workgroup of the stress scene carried 2.7 x the mean).  k_bin_scan writes the
                        //        first three words; `channels` = the channels the tile's list can touch (OR of the entries'
                        //        masks), set by the forward's compositor
    uint32_t* tidx;     // V*NT   per tile: its index into tlist (valid for non-empty tiles)
    float4* e_co;       // V*cap  conic.xyz, opacity        } copies of Geom::co / Geom::xyd of the entry's Gaussian
    float4* e_xyd;      // V*cap  pixel x, y, depth, 1/depth }
    uint4* e_ids;       // V*cap  {Gaussian index (bits 28..31: the strips of the tile the entry can be accepted in, set by the
                        //         forward), partial-sum slot = goff[Gaussian] + index of the tile inside its rect,
                        //         mask of the channels its feature row is not zero on, the feature on the lowest of them}
    float* part;        // V*cap*BIN_ROWS*NACC: the backward's per-(entry, half tile) sums, two 32-byte rows per slot (a Gaussian's rows are
                        // consecutive: k_geom_bwd adds them in order -- no atomics, reproducible); key scratch of the long-list sort before
    uint2* aux;         // V*NT*256 : per pixel of a COVERED tile {final T bits, last contributor} as the forward left them
                        // (the reference's ImageState accum_alpha / n_contrib, rasterizer_impl.h:52-60, kept for covered
                        // tiles only): the backward starts from them instead of re-compositing front to back
    uint32_t* touched;  // V*P    tiles in the Gaussian's rect (the reference's tiles_touched), 0 when culled
    uint32_t* goff;     // V*P    exclusive scan of touched within the view (the reference's point_offsets, shifted)
    uint2* fmask;       // P      {bit ch = "feature ch of the Gaussian is not zero" (one bit set on the skeleton scenes),
                        //         the feature on the lowest set channel}
    uint32_t* tchm;     // V*NT   per tile: OR of its entries' channel masks (k_bin_band_count)
    uint32_t* coverp;   // V*(C+1)*gy*cw: cover rows PER PLANE for the forward's fill role (row layout of Geom::cover): plane C
                        //        (inverse depth) = the non-empty tiles (k_bin_scan), plane ch < C = the tiles whose list touches
                        //        channel ch (k_bin_band_scatter, from tchm) -- the compositor stores only those planes of a tile, the
                        //        fill role streams zeros over all the others in whole rows
};
__host__ __device__ inline size_t bin_long_cap(size_t cap) { return cap / BIN_WAVE_SORT + 1; }
inline Bin bin_from(void* base, int V, int P, int NT, size_t cap)   // (tchm / coverp come last: callers that pass a dummy P never read them)
{
    char* p = (char*)base;
    Bin b;
    b.hdr = (uint32_t*)p; p += 256;
    b.count = (uint32_t*)p; p += align256((size_t)V * NT * 4);
    b.cursor = (uint32_t*)p; p += align256((size_t)V * NT * 4);
    b.ranges = (uint2*)p; p += align256((size_t)V * NT * 8);
    b.nrend = (int*)p; p += align256((size_t)V * 4);
    b.longt = (uint32_t*)p; p += align256((size_t)V * bin_long_cap(cap) * 4);
    b.tlist = (uint4*)p; p += align256((size_t)BIN_CLASSES * V * NT * 16);
    b.tidx = (uint32_t*)p; p += align256((size_t)V * NT * 4);
    b.e_co = (float4*)p; p += align256((size_t)V * cap * 16);
    b.e_xyd = (float4*)p; p += align256((size_t)V * cap * 16);
    b.e_ids = (uint4*)p; p += align256((size_t)V * cap * 16);
    b.part = (float*)p; p += align256((size_t)V * cap * BIN_ROWS * NACC * 4);
    b.aux = (uint2*)p; p += align256((size_t)V * NT * TILE * TILE * 8);
    b.touched = (uint32_t*)p; p += align256((size_t)V * (P > 0 ? P : 1) * 4);
    b.goff = (uint32_t*)p; p += align256((size_t)V * (P > 0 ? P : 1) * 4);
    b.fmask = (uint2*)p; p += align256((size_t)(P > 0 ? P : 1) * 8);
    b.tchm = (uint32_t*)p; p += align256((size_t)V * NT * 4);
    b.coverp = (uint32_t*)p;
    return b;
}
inline size_t bin_bytes(int V, int P, int NT, size_t cap, int planes, size_t cover_words /* per (view, plane): gy * cover_cw(W) */)
{
    return 256 + 3 * align256((size_t)V * NT * 4) + align256((size_t)BIN_CLASSES * V * NT * 16) + align256((size_t)V * NT * 8) + align256((size_t)V * 4) +
           align256((size_t)V * bin_long_cap(cap) * 4) + 3 * align256((size_t)V * cap * 16) +
           align256((size_t)V * cap * BIN_ROWS * NACC * 4) + align256((size_t)V * NT * TILE * TILE * 8) +
           2 * align256((size_t)V * (P > 0 ? P : 1) * 4) + align256((size_t)(P > 0 ? P : 1) * 8) + align256((size_t)V * NT * 4) +
           align256((size_t)V * planes * cover_words * 4);
}
