// sks_binned.inc -- part of the sks_raster.hip translation unit (included inside its anonymous namespace, in order):
// binned path (P > SKS_SMALL_P): binning kernels, tile-per-wavefront forward / backward.
// ------------------------------------------------------------------------------------------------------------
// Tile-centric replacement of InclusiveSum + duplicateWithKeys + DeviceRadixSort::SortPairs + identifyTileRanges
// (rasterizer_impl.cu:70-138, 280-320).  Per tile the reference's sorted order is (depth bits, Gaussian index)
// ascending (stable LSD sort, index-major emission); it is reproduced exactly (sks_export_lists).  Launches of one
// forward: k_geom_fwd (geometry) -> k_bin_band_count (per-tile counts and channel masks, a workgroup per tile band, LDS atomics only)
// -> k_bin_scan (tile ranges, the inverse-depth plane's cover rows, Gaussian slot offsets) -> k_bin_band_scatter (entry RECORDS, the
// colour planes' cover rows, lists longer than a wavefront sorted) -> k_render_fwd_binned.
// ------------------------------------------------------------------------------------------------------------
constexpr uint32_t ID_MASK = 0x0fffffffu;   // e_ids.x: Gaussian index; the four bits above it: strip mask
struct BinView {   // what the compositors read of the Bin scratch
    const uint2* ranges;
    float4* e_co;
    float4* e_xyd;
    uint4* e_ids;
    float* part;
    uint2* aux;
    uint4* tlist;
    const uint32_t* tidx;
    size_t cap;
    int NT;
};
inline BinView bin_view(const Bin& b, int NT, size_t cap) { return BinView{ b.ranges, b.e_co, b.e_xyd, b.e_ids, b.part, b.aux, b.tlist, b.tidx, cap, NT }; }

// ---- k_bin_scan: exclusive scans in chunks; a block derives its chunk's base from everything in front of it ----
// (a handful of L2-resident loads per thread at the sizes of this path: 16 384 tiles or 4 352 Gaussians per view; no
// hand-over between workgroups, no second launch.)
constexpr int SCAN_T = 256;      // threads per block
constexpr int SCAN_IPT = 16;     // items per thread, at most
constexpr int SCAN_G = SCAN_T * 8;   // Gaussians per chunk

// this thread's share of in[0] + ... + in[t0 - 1]
__device__ __forceinline__ uint32_t scan_sum_before(const uint32_t* __restrict__ in, int t0, int tid)
{
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(in) & 15u) == 0) {
        const uint4* in4 = reinterpret_cast<const uint4*>(in);
        const int n4 = t0 >> 2;
        int i = tid;
        for (; i + 3 * SCAN_T < n4; i += 4 * SCAN_T) {   // four independent 16-byte loads in flight
            const uint4 a = in4[i], b = in4[i + SCAN_T], c = in4[i + 2 * SCAN_T], d = in4[i + 3 * SCAN_T];
            s0 += (a.x + a.y) + (a.z + a.w);
            s1 += (b.x + b.y) + (b.z + b.w);
            s2 += (c.x + c.y) + (c.z + c.w);
            s3 += (d.x + d.y) + (d.z + d.w);
        }
        for (; i < n4; i += SCAN_T) {
            const uint4 a = in4[i];
            s0 += (a.x + a.y) + (a.z + a.w);
        }
        done = n4 << 2;
    }
    int j = done + tid;
    for (; j + 3 * SCAN_T < t0; j += 4 * SCAN_T) {
        s0 += in[j];
        s1 += in[j + SCAN_T];
        s2 += in[j + 2 * SCAN_T];
        s3 += in[j + 3 * SCAN_T];
    }
    for (; j < t0; j += SCAN_T) s0 += in[j];
    return (s0 + s1) + (s2 + s3);
}

// exclusive prefix of x over the block's threads; total = the block's sum.  s_w: 4 words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* s_w, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_T / 64; w++) {
        const uint32_t t = s_w[w];
        base += w < wv ? t : 0u;
        total += t;
    }
    __syncthreads();
    return base + inc - x;
}

__device__ __forceinline__ int tile_class(uint32_t cnt) { return min(BIN_CLASSES - 1, 31 - __builtin_clz(cnt)); }   // cnt > 0

// grid (nchunk_t + nchunk_g, V).  Blocks [0, nchunk_t): `bpc` whole tile bands each -> cursor, ranges, the bands' cover rows
// (word 0 = any, then one bit per tile column: the layout k_geom_fwd writes for the small path), the long-tile list, the
// view's entry count.  Blocks behind them: SCAN_G Gaussians each -> goff (first partial-sum slot of every Gaussian).
// vg: views per VIEW GROUP (V = one group).  The tile lists the backward walks are kept per (length class, view group): class
// c's region of V * NT descriptors holds group g's tiles from g * vg * NT on, counted in hdr[BIN_HDR_CLASS + g * BIN_CLASSES + c]
// -- so that a backward launch can take ONE group's tiles while the forward of the next group is still running
// (sks_forward_backward on the binned path).
__global__ __launch_bounds__(SCAN_T) void k_bin_scan(int P, int gx, int gy, int cw, int bpc, int nchunk_t, size_t cap, Bin b,
                                                      uint32_t* __restrict__ cover, int* __restrict__ nrend_user, int V, int planes,
                                                      int vg)
{
    extern __shared__ uint32_t s_cov[];
    __shared__ uint32_t s_w[SCAN_T / 64];
    const int v = blockIdx.y, tid = threadIdx.x;
    const int NT = gx * gy;
    const bool tiles = (int)blockIdx.x < nchunk_t;
    const int chunk = tiles ? (int)blockIdx.x : (int)blockIdx.x - nchunk_t;
    const int clen = tiles ? bpc * gx : SCAN_G;
    const int n = tiles ? NT : P;
    const uint32_t* in = tiles ? b.count + (size_t)v * NT : b.touched + (size_t)v * P;
    const int t0 = chunk * clen, m = min(clen, n - t0);
    const int ipt = (clen + SCAN_T - 1) / SCAN_T;
    const int i0 = tid * ipt;
    uint32_t c[SCAN_IPT], mine = 0;
#pragma unroll
    for (int i = 0; i < SCAN_IPT; i++) {
        c[i] = (i < ipt && i0 + i < m) ? in[t0 + i0 + i] : 0u;
        mine += c[i];
    }
    const uint32_t pre = scan_sum_before(in, t0, tid);
    uint32_t tot_mine, tot_pre;
    const uint32_t ex = block_excl_scan(mine, s_w, tot_mine);
    (void)block_excl_scan(pre, s_w, tot_pre);
    uint32_t run = tot_pre + ex;
    if (!tiles) {
        uint32_t* go = b.goff + (size_t)v * P + t0;
#pragma unroll
        for (int i = 0; i < SCAN_IPT; i++) {
            if (i < ipt && i0 + i < m) go[i0 + i] = run;
            run += c[i];
        }
        return;
    }
    const int nb = min(bpc, gy - chunk * bpc);
    for (int i = tid; i < nb * cw; i += SCAN_T) s_cov[i] = 0u;
    __syncthreads();
    uint32_t* cur = b.cursor + (size_t)v * NT + t0;
    uint2* rng = b.ranges + (size_t)v * NT + t0;
    int band = i0 / gx, tx = i0 - band * gx;
    const unsigned long_cap = (unsigned)((size_t)V * bin_long_cap(cap));
    // the non-empty tiles of this chunk go on the lists the backward walks, one per length class: the block counts its tiles
    // per class in LDS, reserves room in every class's region with one atomic each, then places them (any order inside a class)
    __shared__ uint32_t s_cls[BIN_CLASSES], s_cbase[BIN_CLASSES];
    if (tid < BIN_CLASSES) s_cls[tid] = 0u;
    __syncthreads();
    {
        uint32_t run_ne = run;
#pragma unroll
        for (int i = 0; i < SCAN_IPT; i++) {
            if (c[i] && run_ne < cap) atomicAdd(&s_cls[tile_class(c[i])], 1u);
            run_ne += c[i];
        }
    }
    __syncthreads();
    if (tid < BIN_CLASSES) {
        const uint32_t nn = s_cls[tid];
        s_cbase[tid] = nn ? atomicAdd(&b.hdr[BIN_HDR_CLASS + (v / vg) * BIN_CLASSES + tid], nn) : 0u;
        s_cls[tid] = 0u;
    }
    __syncthreads();
    const size_t VNT = (size_t)V * NT, goff_t = (size_t)(v / vg) * vg * NT;
#pragma unroll
    for (int i = 0; i < SCAN_IPT; i++) {
        if (i < ipt && i0 + i < m) {
            const uint32_t cnt = c[i];
            cur[i0 + i] = run;
            rng[i0 + i] = cnt ? make_uint2(run, run + cnt) : make_uint2(0u, 0u);   // (0,0): the reference's zero-initialised ranges
            if (cnt && run < cap) {   // entries the arena holds
                atomicOr(&s_cov[band * cw], 1u);
                atomicOr(&s_cov[band * cw + 1 + (tx >> 5)], 1u << (tx & 31));
                const int cls = tile_class(cnt);
                const uint32_t tpos = (uint32_t)(cls * VNT + goff_t + s_cbase[cls] + atomicAdd(&s_cls[cls], 1u));
                b.tidx[(size_t)v * NT + t0 + i0 + i] = tpos;
                b.tlist[tpos] = make_uint4((uint32_t)((size_t)v * NT + t0 + i0 + i), run, run + cnt, 0u);
            }
            if (cnt > (uint32_t)BIN_WAVE_SORT) {
                const unsigned li = atomicAdd(&b.hdr[1], 1u);
                if (li < long_cap) b.longt[li] = (uint32_t)((size_t)v * NT + t0 + i0 + i);
            }
            run += cnt;
            if (++tx == gx) { tx = 0; band++; }
        }
    }
    __syncthreads();
    // (the rows of the inverse-depth plane, the last of the view's `planes`: every non-empty tile; the colour planes' rows need
    // the lists' channels: k_bin_band_scatter)
    uint32_t* crow = cover + (((size_t)v * planes + (planes - 1)) * gy + (size_t)chunk * bpc) * cw;
    for (int i = tid; i < nb * cw; i += SCAN_T) crow[i] = s_cov[i];
    if (chunk == nchunk_t - 1 && tid == 0) {
        const int total = (int)(tot_pre + tot_mine);
        b.nrend[v] = total;
        if (nrend_user) nrend_user[v] = total;
    }
}

// ---- band-centric binning: no global atomics ----
// The reference derives a tile's entries from a device-wide sort of (tile | depth) keys (rasterizer_impl.cu:70-138).  Until round 5
// this path counted entries per tile with one global atomic per (Gaussian, tile) pair inside k_geom_fwd and placed them with a second
// one in a scatter kernel: value-returning atomics run at the memory side, one by one per address -- 14 + 19 us on the stress scene,
// plus a sort kernel behind them (61 us from the geometry kernel to the compositor).  Now a workgroup owns a (view, tile band): it
// walks the view's P rects (16 bytes each, L2-resident), keeps the Gaussians that cross its band, and does everything per tile in
// LDS -- counts and channel masks in k_bin_band_count, positions, records, the colour planes' cover rows and the sort of lists
// longer than a wavefront in k_bin_band_scatter.  Entries land in arrival order (the compositor orders lists of up to
// BIN_WAVE_SORT entries in registers and writes them back sorted, as before); results do not depend on it.
#ifndef SKS_BAND_TC
#define SKS_BAND_TC 512
#endif
#ifndef SKS_BAND_TS
#define SKS_BAND_TS 512
#endif
constexpr int BAND_TC = SKS_BAND_TC, BAND_TS = SKS_BAND_TS;   // threads of k_bin_band_count / k_bin_band_scatter
constexpr int BAND_MAX_GX = 4096;    // tile columns (check_common: W <= 4096 * TILE)
constexpr int BAND_SOLO = 8;         // a rect crossing more tile columns of the band than this is walked by its whole wavefront

__device__ __forceinline__ float rlf(float x, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane)); }
// What a (Gaussian, tile) pair's record is made of, fetched ONCE per Gaussian and band (k_bin_band_scatter)
struct BandRec {
    float4 co, xyd;
    uint32_t s0;      // first partial-sum slot of the Gaussian (Bin::goff)
    uint2 fm;
};
// One Gaussian's pairs with the band: its tile columns one by one, or (a rect crossing more than BAND_SOLO columns) handed to the
// whole wavefront.  Wave-uniform call sites only (the ballot).
template <bool REC, typename F>
__device__ __forceinline__ void band_emit(int idx, const uint4& r, int wt, const BandRec& rec, F&& f)
{
    const int lane = threadIdx.x & 63;
    if (wt > 0 && wt <= BAND_SOLO)
        for (unsigned tx = r.x; tx < r.z; tx++) f(idx, r, (int)tx, rec);
    for (unsigned long long big = __ballot(wt > BAND_SOLO); big; big &= big - 1) {
        const int src = __builtin_ctzll(big);
        const uint4 rr = make_uint4(rlu(r.x, src), rlu(r.y, src), rlu(r.z, src), rlu(r.w, src));
        const int ii = __builtin_amdgcn_readlane(idx, src);
        BandRec rb;
        rb.fm = make_uint2(rlu(rec.fm.x, src), rlu(rec.fm.y, src));
        if (REC) {
            rb.co = make_float4(rlf(rec.co.x, src), rlf(rec.co.y, src), rlf(rec.co.z, src), rlf(rec.co.w, src));
            rb.xyd = make_float4(rlf(rec.xyd.x, src), rlf(rec.xyd.y, src), rlf(rec.xyd.z, src), rlf(rec.xyd.w, src));
            rb.s0 = rlu(rec.s0, src);
        }
        for (int tx = (int)rr.x + lane; tx < (int)rr.z; tx += 64) f(ii, rr, tx, rb);
    }
}
// Calls f(gaussian index, rect, tile column, record) for every (Gaussian, tile) pair of band `band` of view v.  The walk over the
// view's rects is a chain of round trips: U rect loads are in flight per trip, then (REC) the records of the crossing Gaussians
// are all requested before the first pair is handed out.  (Handing the band's Gaussians from the count kernel to the scatter
// kernel as a list, so that the second walk is one trip, measured the same: the walk is not what the scatter kernel waits for.)
template <bool REC, int BAND_T, typename F, int U = 4>
__device__ __forceinline__ void for_band_pairs(int P, int v, int band, const Geom& g, const Bin& b, F&& f)
{
    for (int base = 0; base < P; base += U * BAND_T) {    // (uniform trip count: the ballots are wave-wide)
        uint4 rr4[U];
        BandRec rec[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int idx = base + u * BAND_T + (int)threadIdx.x;
            rr4[u] = idx < P ? g.rect[(size_t)v * P + idx] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int idx = base + u * BAND_T + (int)threadIdx.x;
            const uint4 r = rr4[u];
            const bool on = (int)r.y <= band && band < (int)r.w && r.z > r.x;
            rec[u].fm = make_uint2(0u, 0u);
            if (on) {
                const size_t o = (size_t)v * P + idx;
                rec[u].fm = b.fmask[idx];
                if (REC) { rec[u].co = g.co[o]; rec[u].xyd = g.xyd[o]; rec[u].s0 = b.goff[o]; }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int idx = base + u * BAND_T + (int)threadIdx.x;
            const uint4 r = rr4[u];
            const bool on = (int)r.y <= band && band < (int)r.w && r.z > r.x;
            band_emit<REC>(idx, r, on ? (int)(r.z - r.x) : 0, rec[u], f);
        }
    }
}
// grid (gy, V): entries and channel mask of every tile of the band -> Bin::count, Bin::tchm (plain stores: every tile is written)
__global__ __launch_bounds__(BAND_TC) void k_bin_band_count(int P, int gx, Geom g, Bin b)
{
    extern __shared__ uint32_t s_band[];          // [gx] counts, [gx] channel masks
    uint32_t* s_cnt = s_band;
    uint32_t* s_chm = s_band + gx;
    const int band = blockIdx.x, v = blockIdx.y, NT = gx * (int)gridDim.x;
    for (int i = threadIdx.x; i < 2 * gx; i += BAND_TC) s_band[i] = 0u;
    __syncthreads();
    auto count_pair = [&](int, const uint4&, int tx, const BandRec& rec) {
        atomicAdd(&s_cnt[tx], 1u);
        if (rec.fm.x) atomicOr(&s_chm[tx], rec.fm.x);
    };
#ifndef SKS_COUNT_U
#define SKS_COUNT_U 9      // rect loads in flight per thread and trip: 4 352 rects = ONE trip of 512 threads (9.35 -> 8.8 us against 4)
#endif
    for_band_pairs<false, BAND_TC, decltype(count_pair)&, SKS_COUNT_U>(P, v, band, g, b, count_pair);
    __syncthreads();
    const size_t row = (size_t)v * NT + (size_t)band * gx;
    for (int i = threadIdx.x; i < gx; i += BAND_TC) {
        b.count[row + i] = s_cnt[i];
        b.tchm[row + i] = s_chm[i];
    }
}

// Lists longer than a wavefront (never on the skeleton scenes): ascending sort of the (depth bits << 32 | index) keys through the
// whole workgroup's all-ascending bitonic network with virtual +inf padding (in LDS up to SORT_LDS keys, else in the still unused
// partial-sum rows), then the records are written again in that order.  Called by every thread of the workgroup that placed the
// tile's records (their stores are drained and fenced by the caller).  (SORT_LDS: sks_common.inc)
__device__ inline void sort_long_tile(int v, int P, int gx, int tile, size_t cap, const Geom& g, const Bin& b, unsigned long long* s)
{
    const int tid = threadIdx.x;
    const size_t vt = (size_t)v * (gx * (int)gridDim.x) + tile;
    const uint2 r = b.ranges[vt];
    const int n = (int)(min((size_t)r.y, cap) - min((size_t)r.x, cap));
    if (n <= BIN_WAVE_SORT) return;   // clipped by the arena: the readers order what is left themselves
    const size_t eb = (size_t)v * cap + r.x;
    unsigned long long* a = n <= SORT_LDS ? s : reinterpret_cast<unsigned long long*>(b.part + (size_t)v * cap * BIN_ROWS * NACC) + r.x;
    __syncthreads();
    for (int i = tid; i < n; i += BAND_TS)
        a[i] = ((unsigned long long)__float_as_uint(b.e_xyd[eb + i].z) << 32) | (b.e_ids[eb + i].x & ID_MASK);
    __syncthreads();
    int N = 1;
    while (N < n) N <<= 1;
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += BAND_TS) {
                const int p = (j == (k >> 1)) ? (i ^ (k - 1)) : (i ^ j);  // flip on the first sub-step, then disperse
                if (p > i && p < n) {
                    const unsigned long long x = a[i], y = a[p];
                    if (x > y) { a[i] = y; a[p] = x; }
                }
            }
            __syncthreads();
        }
    }
    const int ty = tile / gx, tx = tile - ty * gx;
    for (int i = tid; i < n; i += BAND_TS) {
        const uint32_t id = (uint32_t)a[i];
        const size_t o = (size_t)v * P + id;
        const uint4 rc = g.rect[o];
        b.e_co[eb + i] = g.co[o];
        b.e_xyd[eb + i] = g.xyd[o];
        b.e_ids[eb + i] = make_uint4(id, b.goff[o] + (uint32_t)((ty - (int)rc.y) * (int)(rc.z - rc.x) + (tx - (int)rc.x)), b.fmask[id].x, b.fmask[id].y);
    }
    __syncthreads();
}

// A list of 65 .. 64 * WSORT_K entries, ordered by ONE wavefront: lane l holds entries l, l + 64, ...; every key is broadcast once
// (v_readlane) and each lane counts the keys below its own -- keys are distinct, so the counts are the positions --, then every
// lane holds its whole records in registers before the first one is written back to its position.  Called by the FORWARD's
// wavefront that owns the tile, right before it composites it: the lists of this size are spread over the whole launch there
// (inside k_bin_band_scatter they were 6 us on the critical path of the few bands that hold them all); only lists beyond
// 64 * WSORT_K entries are sorted ahead of the forward, by k_bin_band_scatter's workgroup-wide network.  (WSORT_K: sks_common.inc)
__device__ __forceinline__ void sort_list_wave(float4* __restrict__ e_co, float4* __restrict__ e_xyd, uint4* __restrict__ e_ids, size_t eb, int n)
{
    const int lane = threadIdx.x & 63;
    float4 co[WSORT_K], xyd[WSORT_K];
    uint4 ids[WSORT_K];
    unsigned kd[WSORT_K], ki[WSORT_K];
#pragma unroll
    for (int k = 0; k < WSORT_K; k++) {
        const int e = lane + 64 * k;
        const bool on = e < n;
        const size_t eo = eb + (on ? e : 0);
        co[k] = e_co[eo]; xyd[k] = e_xyd[eo]; ids[k] = e_ids[eo];
        kd[k] = on ? __float_as_uint(xyd[k].z) : 0xffffffffu;
        ki[k] = on ? (ids[k].x & ID_MASK) : 0xffffffffu;
    }
    int rank[WSORT_K];
#pragma unroll
    for (int k = 0; k < WSORT_K; k++) rank[k] = 0;
    const int kn = (n + 63) >> 6;               // registers per lane in use (wave-uniform): 2 for the usual 65 .. 128 entries
#pragma unroll
    for (int s = 0; s < WSORT_K; s++) {
        const int m = min(64, n - 64 * s);      // (wave-uniform)
        for (int j = 0; j < m; j++) {
            const unsigned dj = rlu(kd[s], j), ij = rlu(ki[s], j);
#pragma unroll
            for (int k = 0; k < WSORT_K; k++)
                if (k < kn) rank[k] += (dj < kd[k] || (dj == kd[k] && ij < ki[k])) ? 1 : 0;
        }
    }
    // every record of the list is in registers before the first one goes back (the ranks needed the keys, i.e. the xyd and ids
    // loads; `co` is waited for explicitly); the wavefront's later loads of the list see these stores (one wavefront, one L1)
    __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
    for (int k = 0; k < WSORT_K; k++) {
        if (lane + 64 * k < n) {
            const size_t eo = eb + rank[k];
            e_co[eo] = co[k]; e_xyd[eo] = xyd[k]; e_ids[eo] = ids[k];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0);
}

// grid (gy, V), behind k_bin_scan (ranges, goff, the inverse-depth plane's cover rows).  An entry is written as a record: the two
// 16-byte geometry records of its Gaussian, its index, its partial-sum slot, its feature mask; its position comes from the tile's
// cursor in LDS.  Then the band's cover rows of the colour planes (Bin::coverp: plane ch = the tiles whose list touches channel
// ch; lane = tile column, one ballot per plane) and the sort of the band's long lists.
__global__ __launch_bounds__(BAND_TS) void k_bin_band_scatter(int P, int gx, size_t cap, Geom g, Bin b, int C, int cw)
{
    extern __shared__ uint32_t s_band[];          // [gx] cursors, [gx] channel masks
    __shared__ unsigned long long s_sort[SORT_LDS];
    __shared__ int s_nlong;                       // long tiles of the band, up to LONG_LIST of them remembered by column
    __shared__ unsigned short s_long[LONG_LIST];
    __shared__ unsigned s_any[SKS_MAX_CHANNELS];
    uint32_t* s_cur = s_band;
    uint32_t* s_chm = s_band + gx;
    const int band = blockIdx.x, v = blockIdx.y, gy = (int)gridDim.x, NT = gx * gy;
    const size_t row = (size_t)v * NT + (size_t)band * gx;
    if (threadIdx.x == 0) s_nlong = 0;
    if (threadIdx.x < SKS_MAX_CHANNELS) s_any[threadIdx.x] = 0u;
    for (int i = threadIdx.x; i < gx; i += BAND_TS) {
        const uint2 r = b.ranges[row + i];
        s_cur[i] = r.x;
        s_chm[i] = b.tchm[row + i];
        if (r.y - r.x > (uint32_t)(64 * WSORT_K)) {
            const int k = atomicAdd(&s_nlong, 1);
            if (k < LONG_LIST) s_long[k] = (unsigned short)i;
        }
    }
    __syncthreads();
    for_band_pairs<true, BAND_TS>(P, v, band, g, b, [&](int idx, const uint4& r, int tx, const BandRec& rec) {
        const uint32_t e = atomicAdd(&s_cur[tx], 1u);
        if (e < cap) {
            const size_t eo = (size_t)v * cap + e;
            b.e_co[eo] = rec.co;
            b.e_xyd[eo] = rec.xyd;
            b.e_ids[eo] = make_uint4((uint32_t)idx, rec.s0 + (uint32_t)((band - (int)r.y) * (int)(r.z - r.x) + (tx - (int)r.x)), rec.fm.x, rec.fm.y);
        } else {
            b.hdr[0] = 1u;
        }
    });
    // colour-plane cover rows of this band (only tiles the arena holds entries of -- the inverse-depth plane's bits, from
    // k_bin_scan: a tile whose list was clipped away entirely is the fill role's on every plane)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, planes = C + 1, groups = (gx + 63) / 64;
    const uint32_t* irow = b.coverp + (((size_t)v * planes + C) * gy + band) * cw;
    for (int gq = wave; gq < groups; gq += BAND_TS / 64) {
        const int x = gq * 64 + lane;
        const uint32_t iw = irow[1 + (x >> 5) < cw ? 1 + (x >> 5) : 0];
        const bool held = x < gx && ((iw >> (x & 31)) & 1u);
        const uint32_t m = held ? s_chm[x] : 0u;
        for (int pch = 0; pch < C; pch++) {
            const unsigned long long bits = __ballot((m >> pch) & 1u);
            if (lane == 0) {
                uint32_t* prow = b.coverp + (((size_t)v * planes + pch) * gy + band) * cw;
                prow[1 + 2 * gq] = (uint32_t)bits;
                if (2 + 2 * gq < cw) prow[2 + 2 * gq] = (uint32_t)(bits >> 32);
                if (bits) atomicOr(&s_any[pch], 1u);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {   // word 0 = "some tile of the band touches this plane"; the row's padding words
        uint32_t* prow = b.coverp + (((size_t)v * planes + threadIdx.x) * gy + band) * cw;
        prow[0] = s_any[threadIdx.x];
        for (int w = 1 + 2 * groups; w < cw; w++) prow[w] = 0u;
    }
    if (s_nlong == 0) return;           // (workgroup-uniform)
    __threadfence_block();              // this workgroup's record stores, before its own reads of them
    __syncthreads();
    const int nlong = s_nlong;      // (tiles beyond 64 entries; those up to 64 * WSORT_K are the forward's)
    if (nlong <= LONG_LIST) {
        for (int k = 0; k < nlong; k++) {
            const int tx = (int)s_long[k];
            const uint2 r = b.ranges[row + tx];
            const int n = (int)(min((size_t)r.y, cap) - min((size_t)r.x, cap));
            if (n > 64 * WSORT_K) sort_long_tile(v, P, gx, band * gx + tx, cap, g, b, s_sort);
        }
    } else {
        for (int tx = 0; tx < gx; tx++) {
            const uint2 r = b.ranges[row + tx];
            const int n = (int)(min((size_t)r.y, cap) - min((size_t)r.x, cap));
            if (n > 64 * WSORT_K) sort_long_tile(v, P, gx, band * gx + tx, cap, g, b, s_sort);
        }
    }
}

// ---- a chunk (<= 64 entries) of a tile's list in registers: lane k = the chunk's k-th entry in compositing order ----
struct Chunk {
    float4 co, xyd;
    uint32_t id, slot, fmask;
    float f0;   // the feature on the lowest channel of fmask (all there is to a one-hot row)
};
__device__ __forceinline__ float permf(int addr, float x) { return __int_as_float(__builtin_amdgcn_ds_permute(addr, __float_as_int(x))); }
__device__ __forceinline__ uint32_t permu(int addr, uint32_t x) { return (uint32_t)__builtin_amdgcn_ds_permute(addr, (int)x); }

// cn entries starting at eb.  `sort`: they are in arrival order (a list of up to BIN_WAVE_SORT entries): every lane ranks its
// (depth bits, index) key against the others' (v_readlane broadcasts; keys are distinct) and the records move to the lane
// of their rank (ds_permute: the LDS crossbar, no LDS memory) -- the same order in every kernel that reads the list.
__device__ __forceinline__ void load_chunk(const BinView& b, size_t eb, int cn, bool sort, Chunk& c)
{
    const int lane = threadIdx.x & 63;
    const size_t e = eb + (lane < cn ? lane : 0);
    c.co = b.e_co[e];
    c.xyd = b.e_xyd[e];
    const uint4 ids = b.e_ids[e];
    c.id = ids.x & ID_MASK;   // (bits 28..31: strip mask, once the forward has been over the list)
    c.slot = ids.y;
    c.fmask = lane < cn ? ids.z : 0u;
    c.f0 = __uint_as_float(ids.w);
    if (!sort || cn < 2) return;
    const unsigned d = __float_as_uint(c.xyd.z);
    int rank = 0;
    for (int j = 0; j < cn; j++) {
        const unsigned dj = rlu(d, j), ij = rlu(c.id, j);
        rank += (dj < d || (dj == d && ij < c.id)) ? 1 : 0;
    }
    const int addr = (lane < cn ? rank : lane) << 2;
    c.co.x = permf(addr, c.co.x); c.co.y = permf(addr, c.co.y); c.co.z = permf(addr, c.co.z); c.co.w = permf(addr, c.co.w);
    c.xyd.x = permf(addr, c.xyd.x); c.xyd.y = permf(addr, c.xyd.y); c.xyd.z = permf(addr, c.xyd.z); c.xyd.w = permf(addr, c.xyd.w);
    c.id = permu(addr, c.id);
    c.slot = permu(addr, c.slot);
    c.fmask = permu(addr, c.fmask);
    c.f0 = permf(addr, c.f0);
}

// parity / debug export of the reference's point_list and ranges.  grid (ceil(max(NT, cap) / 256), V): ranges, zeros behind
// the view's entries; then k_export_sorted (one wavefront per tile) writes every list in compositing order.
__global__ void k_export_lists(int NT, size_t cap, const uint2* __restrict__ ranges, const int* __restrict__ nrend,
                               uint32_t* __restrict__ point_list, uint32_t* __restrict__ out_ranges)
{
    const int v = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)NT) {
        const uint2 r = ranges[(size_t)v * NT + i];
        out_ranges[((size_t)v * NT + i) * 2] = r.x;
        out_ranges[((size_t)v * NT + i) * 2 + 1] = r.y;
    }
    if (i < cap && i >= (size_t)max(nrend[v], 0)) point_list[(size_t)v * cap + i] = 0u;
}
__global__ __launch_bounds__(256) void k_export_sorted(BinView b, uint32_t* __restrict__ point_list)
{
    const int v = blockIdx.y, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= b.NT) return;
    const uint2 r = b.ranges[(size_t)v * b.NT + t];
    const unsigned r_lo = __builtin_amdgcn_readfirstlane(r.x), r_hi = __builtin_amdgcn_readfirstlane(r.y);
    const int total = (int)(min((size_t)r_hi, b.cap) - min((size_t)r_lo, b.cap));
    const size_t eb = (size_t)v * b.cap + r_lo;
    // (the forward's compositor wrote every list back in compositing order)
    for (int i = lane; i < total; i += 64) point_list[eb + i] = b.e_ids[eb + i].x & ID_MASK;
}

// Which of a tile's four 4-row strips can an entry be ACCEPTED in (forward.cu:358-366: power <= 0 and alpha >= 1/255)?
// alpha >= 1/255 needs opacity * exp(power) >= 1/255, i.e. the pixel inside the ellipse  conic(d, d) <= 2 ln(255 opacity),
// whose bounding box is +- sqrt(2 tau conic.{z, x} / det).  The box is taken with generous margins (1 % and 0.1 on tau, 1 % and
// one pixel on the extents: far beyond fp32 rounding of `power` and of expf), so a strip outside it holds no pixel the
// compositor would accept: skipping the entry there changes no output bit.  Anything not a proper ellipse is never skipped.
__device__ __forceinline__ unsigned strip_mask(const float4& co, const float4& xyd, int tx, int ty)
{
    const float lim = 255.0f * co.w;
    const float det = co.x * co.z - co.y * co.y;
    if (!(lim == lim) || !(det > 0.0f) || !(co.x > 0.0f) || !(co.z > 0.0f) || !(det < 3.0e38f) || !(lim < 3.0e38f)) return 0xfu;
    if (lim * 1.0625f < 1.0f) return 0u;   // opacity below 1/255: alpha < 1/255 everywhere
    const float tau = __logf(fmaxf(lim, 1.0f)) * 1.01f + 0.1f;
    const float s = 2.0f * tau / det;
    const float rx = sqrtf(s * co.z) * 1.01f + 1.0f, ry = sqrtf(s * co.x) * 1.01f + 1.0f;
    if (!(rx < 3.0e38f) || !(ry < 3.0e38f)) return 0xfu;
    const float tx0 = (float)(tx * TILE), ty0 = (float)(ty * TILE);
    if (xyd.x + rx < tx0 || xyd.x - rx > tx0 + (float)(TILE - 1)) return 0u;
    unsigned m = 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float r0 = ty0 + (float)(4 * q);
        m |= (xyd.y + ry < r0 || xyd.y - ry > r0 + 3.0f) ? 0u : (1u << q);
    }
    return m;
}

// The channels a tile's list can touch (features != 0 somewhere in it), NB at a time: position j of group grp <-> channel.
constexpr int BIN_NB = 8;          // the backward's group (its feature-gradient reduction is wave_sum8)
#ifndef SKS_FWD_NB
#define SKS_FWD_NB 8
#endif
constexpr int FWD_NB = SKS_FWD_NB;   // the forward's
template <int NB = BIN_NB>
struct ChanGroupT {
    int chan[NB];   // wave-uniform
    int n;              // channels in this group
};
typedef ChanGroupT<BIN_NB> ChanGroup;
template <int NB = BIN_NB>
__device__ __forceinline__ ChanGroupT<NB> chan_group(unsigned chm, int nc, int grp)
{
    ChanGroupT<NB> cgp;
    unsigned r = chm;
    for (int j = 0; j < grp * NB; j++) r &= r - 1;
#pragma unroll
    for (int j = 0; j < NB; j++) {
        cgp.chan[j] = r ? __builtin_ctz(r) : 0;
        r &= r - 1;
    }
    cgp.n = max(0, min(NB, nc - grp * NB));
    return cgp;
}
// OR of x over the first cn lanes (lists are short: one v_readlane per entry beats a butterfly)
__device__ __forceinline__ unsigned wave_or_first(unsigned x, int cn)
{
    unsigned r = 0u;
    for (int j = 0; j < cn; j++) r |= rlu(x, j);
    return r;
}
// lane = entry: its feature values on the group's channels and which of them are not zero.  A row with a single non-zero
// feature (every row of a skeleton scene) came with the record; only denser rows go back to the feature tensor.
template <int NB>
__device__ __forceinline__ unsigned load_group_features(const float* __restrict__ features, int C, const Chunk& ck, bool on,
                                                        const ChanGroupT<NB>& cgp, float (&cf)[NB])
{
    const unsigned fm = on ? ck.fmask : 0u;
    const bool dense = (fm & (fm - 1u)) != 0u;   // more than one bit
    const int ch0 = fm ? __builtin_ctz(fm) : -1;
    unsigned ecm = 0u;
#pragma unroll
    for (int j = 0; j < NB; j++) {
        const bool has = j < cgp.n && ((fm >> cgp.chan[j]) & 1u);
        float f = (has && cgp.chan[j] == ch0) ? ck.f0 : 0.0f;
        if (has && dense) f = features[(size_t)ck.id * C + cgp.chan[j]];
        cf[j] = f;
        ecm |= f != 0.0f ? (1u << j) : 0u;
    }
    return ecm;
}

constexpr int TGROUP = 4;         // consecutive tile columns per composite block: one per wavefront (a second tile per wave would
                                  // load its list behind the first one's 72 stores: vmcnt retires in order; measured +40 %)

// binned forward, "fill + sparse composite" like k_render_fwd_sparse: grid (fsplit + xc, gy, (C+1) * V).
//   * fill role (x < fsplit): fwd_fill_role over the cover rows k_bin_scan wrote -- empty tiles (the vast majority
//     of a skeleton scene) are zero-filled in long contiguous rows instead of 64-byte tile rows;
//   * composite role (the xc extra blocks of every row): block -> (view, band, four tile columns), ONE WAVEFRONT PER TILE.
//     The wave holds the tile's list in registers (lane k = k-th entry, load_chunk) and composites eight pixel rows at a
//     time, two per lane, exactly like forward.cu:346-386; the entry being composited is broadcast with v_readlane (wave-uniform values
//     in scalar registers: no LDS, no barrier), an entry is only visited in the strips its footprint can reach
//     (strip_mask), and only the channels the list can touch are accumulated (BIN_NB at a time, compacted; an entry adds
//     to a channel only where its own feature is not zero: a wave-uniform branch -- one-hot features make the other C - 1
//     multiply-adds exact zeros); every other plane of the tile is stored as zeros.  The launch is bound by the life
//     time of its blocks (the fill blocks need every wave slot they can get to keep the store stream going), and a tile's
//     load -> composite -> store chain is latency, not work: lists average ~5 entries.
// (5 workgroups per CU = 96 registers: the composite role with two pixel rows per lane spills 15 registers at 80 and 24 at 72 --
// scratch traffic under the store flood --, and the fill role, which is most of the launch, lives on wave slots; interleaved A/B
// on the stress scene, us: one row per lane 5 per CU 430, 6: 425, 7: 419, 8: 435; two rows per lane 4: 436, 5: 413-422, 6: 424-433,
// 7: 436 against 424-430 for one row at 7 on the same boxes.  A ninth channel per group -- 7 % of this scene's tiles, with 27 % of
// its entries, touch nine channels and take two passes -- measured the same at 5 and worse at 6.)
typedef int v2i __attribute__((ext_vector_type(2)));
// expf_fixed on two values at once: the same operation sequence per component (packed multiplies and fused multiply-adds),
// the two range branches as selects -- bit-identical to expf_fixed for every input, NaN included
__device__ __forceinline__ v2f expf_fixed2(v2f x)
{
    const v2i lo = x < -80.0f, hi = x > 88.0f;
    const v2f xc = lo ? (v2f){ -80.0f, -80.0f } : x;
    const v2f t = xc * 1.44269504088896341f;
    const v2f k = __builtin_elementwise_rint(t);
    v2f r = __builtin_elementwise_fma(k, (v2f){ -0.693145751953125f, -0.693145751953125f }, xc);
    r = __builtin_elementwise_fma(k, (v2f){ -1.42860682030941723e-6f, -1.42860682030941723e-6f }, r);
    v2f p = { 1.98412698412698413e-4f, 1.98412698412698413e-4f };
    p = __builtin_elementwise_fma(p, r, (v2f){ 1.38888888888888894e-3f, 1.38888888888888894e-3f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 8.33333333333333322e-3f, 8.33333333333333322e-3f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 4.16666666666666644e-2f, 4.16666666666666644e-2f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 1.66666666666666657e-1f, 1.66666666666666657e-1f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 0.5f, 0.5f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 1.0f, 1.0f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 1.0f, 1.0f });
    const v2i ki = __builtin_convertvector(k, v2i);
    const v2i bits = __builtin_bit_cast(v2i, p) + ki * (1 << 23);
    const v2f e = __builtin_bit_cast(v2f, bits);
    const v2f z = { 0.0f, 0.0f }, inf = { __builtin_huge_valf(), __builtin_huge_valf() };
    return lo ? z : (hi ? inf : e);
}
#ifndef SKS_FWD_BIN_OCC
#define SKS_FWD_BIN_OCC 5
#endif
#ifndef SKS_BWD_EXACT
#define SKS_BWD_EXACT 0
#endif
// expf_fixed_neg on two values (the backward walk is held to a tolerance: packed multiplies and fused multiply-adds)
__device__ __forceinline__ v2f expf_neg2(v2f x)
{
    x = (v2f){ fmaxf(x.x, -80.0f), fmaxf(x.y, -80.0f) };
    const v2f k = __builtin_elementwise_rint(x * 1.44269504088896341f);
    v2f r = __builtin_elementwise_fma(k, (v2f){ -0.693145751953125f, -0.693145751953125f }, x);
    r = __builtin_elementwise_fma(k, (v2f){ -1.42860682030941723e-6f, -1.42860682030941723e-6f }, r);
    v2f p = { 1.98412698412698413e-4f, 1.98412698412698413e-4f };
    p = __builtin_elementwise_fma(p, r, (v2f){ 1.38888888888888894e-3f, 1.38888888888888894e-3f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 8.33333333333333322e-3f, 8.33333333333333322e-3f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 4.16666666666666644e-2f, 4.16666666666666644e-2f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 1.66666666666666657e-1f, 1.66666666666666657e-1f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 0.5f, 0.5f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 1.0f, 1.0f });
    p = __builtin_elementwise_fma(p, r, (v2f){ 1.0f, 1.0f });
    const v2i ki = __builtin_convertvector(k, v2i);
    return __builtin_bit_cast(v2f, __builtin_bit_cast(v2i, p) + ki * (1 << 23));
}
__device__ __forceinline__ v2f sel2(bool ca, bool cb, v2f t, v2f f) { return (v2f){ ca ? t.x : f.x, cb ? t.y : f.y }; }
// The exponent of forward.cu:358 in the forward compositor's operation order, NOT contracted (this function sits outside the
// backward walk's `fp contract(fast)` block on purpose): whether an entry counts at a pixel -- power <= 0, alpha >= 1/255 -- must
// come out as the forward decided it.  With the multiply-adds fused differently a pixel on the 1/255 contour of a footprint
// dropped out of the backward (one pixel of a 3 x 3-tile Gaussian: 0.3 % of its gradient, tests/test_fullsize_gpu.py 1002 mix).
__device__ __forceinline__ v2f power_of2(const float4& co, float dx, v2f dy)
{
    const float a1 = co.x * dx * dx, b1 = co.y * dx;
    return -0.5f * (a1 + co.z * dy * dy) - b1 * dy;
}

// One entry of the back-to-front walk (backward.cu:556-635) at a lane's two pixels: the terms of the entry's seven sums over THIS
// lane's pixels in vals[0..6] (vals[7] = 0) and the walk state moved on where the entry is active.  Returns false (nothing
// touched) when the entry is active at no pixel of the wavefront.  Shared by k_render_bwd_tile and the forward's fused backward
// (k_render_fwd_binned<.., BWD>): the same instruction sequence, the same bits.  gk: the entry's position in the tile's list; glA /
// glB: the pixels' last contributors; cdot: the entry's colour . dL at the two pixels.
struct WalkState {
    v2f T, rec, lst, la, ainv, linv;   // (ainv / linv: the inverse-depth recursion, EXTRA only)
};
template <bool EXTRA>
__device__ __forceinline__ bool walk_entry(const float4& co, const float4& xyd, float pxf, v2f py2, v2f cdot, int glA, int glB, int gk, v2f dLi,
                                           v2f Tf, v2f bgd, float ddelx_dx, float ddely_dy, WalkState& s, float (&vals)[8],
                                           v2f& dchannel_dcolor, bool& actA, bool& actB)
{
#if !SKS_BWD_EXACT
#pragma clang fp contract(fast)
#endif
    const float dx = xyd.x - pxf;
    const v2f dy = xyd.y - py2;
    const v2f power = power_of2(co, dx, dy);
    const v2f Gv = expf_neg2(power);
    const v2f cg = co.w * Gv;
    const v2f alpha = { fminf(0.99f, cg.x), fminf(0.99f, cg.y) };
    actA = glA >= gk && !(power.x > 0.0f) && !(alpha.x < 1.0f / 255.0f);
    actB = glB >= gk && !(power.y > 0.0f) && !(alpha.y < 1.0f / 255.0f);
    if (!__any(actA || actB)) return false;
    // (every lane computes; the state moves where the entry is active)
    const v2f one_a = 1.0f - alpha;
#if SKS_BWD_EXACT
    const v2f rcp1a = { 1.0f / one_a.x, 1.0f / one_a.y };
#else
    const v2f rcp1a = { __builtin_amdgcn_rcpf(one_a.x), __builtin_amdgcn_rcpf(one_a.y) };
#endif
    const v2f Tn = s.T * rcp1a;
    dchannel_dcolor = alpha * Tn;
    const v2f recn = s.la * s.lst + (1.0f - s.la) * s.rec;
    v2f dL_dalpha = cdot - recn;
    const v2f zero2 = { 0.0f, 0.0f };
#pragma unroll
    for (int j = 0; j < 8; j++) vals[j] = 0.0f;
    v2f ainvn = zero2;
    if (EXTRA) {
        ainvn = s.la * s.linv + (1.0f - s.la) * s.ainv;
        dL_dalpha += (xyd.w - ainvn) * dLi;
        const v2f v6 = sel2(actA, actB, dchannel_dcolor * dLi, zero2);
        vals[6] = v6.x + v6.y;
    }
    dL_dalpha *= Tn;
    if (EXTRA) dL_dalpha += (-Tf * rcp1a) * bgd;
    const v2f dL_dG = sel2(actA, actB, co.w * dL_dalpha, zero2);
    const v2f gdx = Gv * dx, gdy = Gv * dy;
    const v2f dG_ddelx = -gdx * co.x - gdy * co.y;
    const v2f dG_ddely = -gdy * co.z - gdx * co.y;
    const v2f v0 = dL_dG * dG_ddelx, v1 = dL_dG * dG_ddely;
    const v2f v2 = gdx * dx * dL_dG, v3 = gdx * dy * dL_dG, v4 = gdy * dy * dL_dG;
    const v2f v5 = sel2(actA, actB, Gv * dL_dalpha, zero2);
    vals[0] = (v0.x + v0.y) * ddelx_dx;
    vals[1] = (v1.x + v1.y) * ddely_dy;
    vals[2] = -0.5f * (v2.x + v2.y);
    vals[3] = -0.5f * (v3.x + v3.y);
    vals[4] = -0.5f * (v4.x + v4.y);
    vals[5] = v5.x + v5.y;
    s.T = sel2(actA, actB, Tn, s.T);
    s.rec = sel2(actA, actB, recn, s.rec);
    s.lst = sel2(actA, actB, cdot, s.lst);
    s.la = sel2(actA, actB, alpha, s.la);
    if (EXTRA) {
        s.ainv = sel2(actA, actB, ainvn, s.ainv);
        s.linv = sel2(actA, actB, (v2f){ xyd.w, xyd.w }, s.linv);
    }
    return true;
}

// (Round 6 tried a variant whose composite wavefronts also run the tile backward of their tile -- from the final T, the last
// contributors and the list they still hold in registers, through walk_entry: bit for bit k_render_bwd_tile's rows.  The stress
// step went 0.566 -> 0.649 ms: the variant needs 128 registers, which costs EVERY block of the launch, the fill role included, a
// fifth of its wave slots, and the longer composite wavefronts hold slots the fill blocks live on.  Like the backward on a second
// stream (SKS_BIN_GROUPS) it trades wave-slot time for wave-slot time; commit 2b49fbf has the code, NOTES_experiments.md the A/B.)
template <int CG, int PPT, bool NT, bool HALF = false>
__global__ __launch_bounds__(256, SKS_FWD_BIN_OCC) void k_render_fwd_binned(FwdArgs a, BinView b, int gx, int gy, int fsplit, int pb,
                                                           const uint32_t* __restrict__ cover)
{
    const int tid = threadIdx.x;
    const int xq = blockIdx.x, band_id = blockIdx.y, zid = blockIdx.z;
    if (xq < fsplit) {
        fwd_fill_role<PPT, NT, HALF>(a, a.cp1_magic, xq, band_id, zid, gy, pb, cover);
        return;
    }
    const int xc = gridDim.x - fsplit;
    const int cb = (zid * gy + band_id) * xc + (xq - fsplit);
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform per wavefront: say so)
    const int gpb = (gx + TGROUP - 1) / TGROUP, NG = gpb * gy;
    const int v = cb / NG;
    if (v >= (int)(gridDim.z / (a.C + 1))) return;
    const int g = cb - v * NG;
    const int ty = g / gpb, tx = (g - ty * gpb) * TGROUP + wv;
    if (tx >= gx) return;
    const int C = a.C, W = a.W, H = a.H;
    const size_t HW = (size_t)H * W;
    const size_t tile = (size_t)v * b.NT + (size_t)ty * gx + tx;
    const uint2 range = b.ranges[tile];
    const uint32_t tpos = b.tidx[tile];   // (requested with the range: only meaningful for a non-empty tile)
    const unsigned r_lo = __builtin_amdgcn_readfirstlane(range.x), r_hi = __builtin_amdgcn_readfirstlane(range.y);
    const int total = (int)(min((size_t)r_hi, b.cap) - min((size_t)r_lo, b.cap));
    if (total == 0) return;  // a fill block zeroes this tile
    const size_t eb = (size_t)v * b.cap + r_lo;
    const bool sort = total <= BIN_WAVE_SORT;
    const bool do_clamp = a.flags & SKS_CLAMP01;
    Chunk ck;
    unsigned chm = 0u, smask = 0u;
    if (sort) {
        load_chunk(b, eb, total, true, ck);
        chm = wave_or_first(ck.fmask, total);
        smask = lane < total ? strip_mask(ck.co, ck.xyd, tx, ty) : 0u;
        if (lane < total) {   // the list, in compositing order and with the strips each entry can reach: what the backward reads
            b.e_co[eb + lane] = ck.co;
            b.e_xyd[eb + lane] = ck.xyd;
            b.e_ids[eb + lane] = make_uint4(ck.id | (smask << 28), ck.slot, ck.fmask, __float_as_uint(ck.f0));
        }
    } else {
        // a list longer than a wavefront (sorted by k_bin_band_scatter): its channels, and every entry's strip mask for the backward
        // -- here, over the whole list: the compositing loop below leaves a list as soon as all its pixels are saturated, and
        // an entry behind that point in one half of the tile can still count in the other.  Lists of up to 64 * WSORT_K entries
        // arrive unsorted and are ordered here first, by this wavefront (longer ones were sorted by k_bin_band_scatter).
        if (total <= 64 * WSORT_K) sort_list_wave(b.e_co, b.e_xyd, b.e_ids, eb, total);
        for (int c0 = 0; c0 < total; c0 += 64) {
            const int cn = min(64, total - c0);
            load_chunk(b, eb + c0, cn, false, ck);
            chm |= wave_or_first(ck.fmask, cn);
            if (lane < cn) b.e_ids[eb + c0 + lane].x = ck.id | (strip_mask(ck.co, ck.xyd, tx, ty) << 28);
        }
    }
    if (lane == 0) b.tlist[tpos].w = chm;   // (the backward walks the same channels: part of the tile's descriptor)
    const int nc = __popc(chm);
    const int ngroups = nc > 0 ? (nc + FWD_NB - 1) / FWD_NB : 1;
    const int x = tx * TILE + (lane & 15);
    const float pxf = (float)x;
    float* outc = a.out_color + (size_t)v * C * HW;
    for (int grp = 0; grp < ngroups; grp++) {
        const ChanGroupT<FWD_NB> cgp = chan_group<FWD_NB>(chm, nc, grp);
        float cf[FWD_NB];
        unsigned ecm = 0u;
        if (sort) ecm = load_group_features(a.features, C, ck, lane < total, cgp, cf);
        // Two pixel rows per lane (rows r and r + 4 of an 8-row half of the tile): an entry is fetched from the list's lanes
        // once for both (ten v_readlane and the wave-uniform bookkeeping per visit), the pixel column and everything that only
        // depends on it is shared, the rest is packed two-wide (v_pk_mul / v_pk_add / v_pk_fma_f32: the same IEEE operations
        // in the same order as the one-pixel form, bit for bit).
        for (int h = 0; h < 2; h++) {
            const int yA = ty * TILE + h * 8 + (lane >> 4), yB = yA + 4;
            const v2f py2 = { (float)yA, (float)yB };
            const bool insideA = x < W && yA < H, insideB = x < W && yB < H;
            v2f T2 = { 1.0f, 1.0f }, inv2 = { 0.0f, 0.0f }, acc2[FWD_NB];
#pragma unroll
            for (int j = 0; j < FWD_NB; j++) acc2[j] = (v2f){ 0.0f, 0.0f };
            uint32_t lastA = 0, lastB = 0;
            bool doneA = !insideA, doneB = !insideB;
            for (int c0 = 0; c0 < total; c0 += 64) {
                if (__all(doneA && doneB)) break;
                if (!sort) {
                    const int cn = min(64, total - c0);
                    load_chunk(b, eb + c0, cn, false, ck);
                    ecm = load_group_features(a.features, C, ck, lane < cn, cgp, cf);
                    smask = lane < cn ? strip_mask(ck.co, ck.xyd, tx, ty) : 0u;
                }
                for (unsigned long long m = __ballot(((smask >> (2 * h)) & 3u) != 0u); m; m &= m - 1) {   // forward.cu:346-386
                    if (__all(doneA && doneB)) break;
                    const int k = __builtin_ctzll(m);
                    const float ex = rl(ck.xyd.x, k), ey = rl(ck.xyd.y, k), einvd = rl(ck.xyd.w, k);
                    const float cx = rl(ck.co.x, k), cy = rl(ck.co.y, k), cz = rl(ck.co.z, k), cw = rl(ck.co.w, k);
                    const unsigned em = rlu(ecm, k);
                    const float dx = ex - pxf;
                    const v2f dy = ey - py2;
                    const float a1 = cx * dx * dx, b1 = cy * dx;
                    const v2f power = -0.5f * (a1 + cz * dy * dy) - b1 * dy;
                    const v2f ca = cw * expf_fixed2(power);
                    const v2f alpha = { fminf(0.99f, ca.x), fminf(0.99f, ca.y) };
                    const v2f test_T = T2 * (1.0f - alpha);
                    const bool passA = !doneA && !(power.x > 0.0f) && !(alpha.x < 1.0f / 255.0f);
                    const bool passB = !doneB && !(power.y > 0.0f) && !(alpha.y < 1.0f / 255.0f);
                    const bool stopA = passA && test_T.x < 0.0001f, stopB = passB && test_T.y < 0.0001f;
                    const bool acceptA = passA && !stopA, acceptB = passB && !stopB;
#pragma unroll
                    for (int j = 0; j < FWD_NB; j++) {
                        // wave-uniform branch (a zero feature adds an exact zero).  (For one-hot rows a three-level decision tree
                        // to the entry's channel instead of these eight tests measured 6 % SLOWER: 410 -> 435 us.)
                        if ((em >> j) & 1u) {
                            const v2f add = rl(cf[j], k) * alpha * T2;
                            acc2[j] += (v2f){ acceptA ? add.x : 0.0f, acceptB ? add.y : 0.0f };
                        }
                    }
                    const v2f inv_n = inv2 + einvd * alpha * T2;
                    if (acceptA) { inv2.x = inv_n.x; T2.x = test_T.x; lastA = (uint32_t)(c0 + k + 1); }
                    if (acceptB) { inv2.y = inv_n.y; T2.y = test_T.y; lastB = (uint32_t)(c0 + k + 1); }
                    doneA = doneA || stopA;
                    doneB = doneB || stopB;
                }
            }
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const bool inside = r ? insideB : insideA;
                const int y = r ? yB : yA;
                const float T = r ? T2.y : T2.x, inv = r ? inv2.y : inv2.x;
                const uint32_t last = r ? lastB : lastA;
                if (inside) {
                    const size_t pix = (size_t)y * W + x;
#pragma unroll
                    for (int j = 0; j < FWD_NB; j++) {
                        const float av = r ? acc2[j].y : acc2[j].x;
                        if (j < cgp.n) outc[(size_t)cgp.chan[j] * HW + pix] = do_clamp ? clamp01(av) : av;
                    }
                    if (grp == 0) {
                        // (the planes no entry of the list has a feature for are the fill role's: Bin::coverp -- unless the arena
                        // clipped this list: then the cover rows, made from the unclipped lists, may name planes these entries
                        // do not touch)
                        if ((size_t)r_hi > b.cap)
                            for (int ch = 0; ch < C; ch++)
                                if (!((chm >> ch) & 1u)) outc[(size_t)ch * HW + pix] = 0.0f;
                        a.out_invdepth[(size_t)v * HW + pix] = inv;
                        if (a.final_T) a.final_T[(size_t)v * HW + pix] = T;
                        if (a.n_contrib) a.n_contrib[(size_t)v * HW + pix] = last;
                    }
                }
                // what the backward starts from (pixel q * 64 + lane = row-major index inside the tile): one 8-byte store.
                // (with the clamp folded in the backward re-composites -- the pre-clamp colours decide where the gradient passes)
                if (grp == 0 && !do_clamp) b.aux[(tile << 8) + (2 * h + r) * 64 + lane] = make_uint2(__float_as_uint(T), inside ? last : 0u);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// binned backward (backward.cu:452-638).  A fixed number of workgroups walk the lists of non-empty tiles k_bin_scan left (no
// dispatch of the ~80 % empty tiles), longest lists first, round-robin; a workgroup is two wavefronts and takes one tile at a
// time, each wavefront one 8-row half of it, two pixels per lane (rows r and r + 4) -- and that is all the wavefronts share: no
// barrier, no common LDS.  A wavefront
//   * has requested, one tile ago, everything its task needs from memory (BwdBundle): the tile's list as the forward's
//     compositor left it (compositing order, lane k = entry k, strip masks in the index word), its pixels' {final T, last
//     contributor} and dL/d(render) on the channels the list can touch (the tile's descriptor names them: BIN_NB at a time,
//     compacted) -- no memory round trip is waited for in front of a walk; the descriptor after next is on its way too;
//   * keeps the records and its pixels' dL in its own 6 KB of LDS: the entry being walked is a broadcast read, the pixel's
//     dL on that entry's channel a read at a wave-uniform row (one-hot features: one channel per entry);
//   * walks back to front over the entries that can reach ITS half (a wave-uniform bit test on the two strip bits), carries the
//     colour recursion of backward.cu:581-594 as two dot products with the pixel's dL (it is linear and only
//     sum_ch (c - accum_rec) dL is used) for both of a lane's pixels in packed two-wide arithmetic, adds the two pixels' terms and
//     reduces an entry's seven sums over the wavefront with ONE transpose reduction (wave_sum8) per (entry, half) -- with a pixel
//     per lane and a wavefront per 4-row strip it was one per (entry, strip): 144-147 -> 133-138 us on the stress scene;
//   * stores them as the (entry, half) row of `part`: BIN_ROWS = two 32-byte rows per slot, the rows of a Gaussian consecutive
//     (slot = goff + tile index inside its rect); rows of halves an entry cannot reach are stored as zeros.  k_geom_bwd_binned adds
//     a Gaussian's rows in a fixed order.
// No atomics anywhere, no zeroed scratch, bitwise reproducible gradients.  (dL/dfeatures, when asked for, is the one
// exception: it is accumulated with float atomics.)  Every per-Gaussian sum is linear in dL/dalpha, a sum over channels,
// so channel groups simply accumulate.  The walk itself is held to a tolerance, not bit for bit (the reference's own
// atomicAdd order is arbitrary): it contracts multiply-adds and takes 1 / (1 - alpha) from v_rcp_f32.
// EXTRA: the inverse-depth gradient and the background term (per-pixel state only this variant pays registers for).
// ------------------------------------------------------------------------------------------------------------
constexpr int BWD_TILE_BLOCKS_PER_CU = 128;  // a few tiles per workgroup: the hardware's dispatch then evens out what the cost-ordered
                                            // list leaves (sweep on the stress scene with 4-wave workgroups, us: 6 per CU 186, 12: 157,
                                            // 24: 142, 36 / 48 / 96: 141; with two-wavefront workgroups 32: 126, 48: 123, 64: 120,
                                            // 96: 120, 128: 117, 192 / 256: 117)
constexpr int BWD_TILE_THREADS = 128;        // two wavefronts: the upper and the lower 8 rows of the tile
struct BwdWaveLds {
    float4 co[64];
    float4 xyd[64];
    float d[BIN_NB][128];   // dL/d(render) of this half's pixels on the group's channels: [..][lane] rows r, [..][64 + lane] rows r + 4
};
struct BwdBundle {   // a (tile, half) task's first pass (channel group 0, the list's last chunk) as it comes from memory
    uint4 ids;
    float4 co, xyd;
    uint2 axA, axB;
    float gvA[BIN_NB], gvB[BIN_NB];
    float dLiA, dLiB;
};
// n / d for n < 2^31 with m = ceil(2^32 / d) (host): the tile coordinates of a descriptor, without the division sequence
__device__ __forceinline__ unsigned div_magic(unsigned n, unsigned d, unsigned m)
{
    unsigned q = d == 1u ? n : __umulhi(n, m);
    if (q * d > n) q--;
    else if ((q + 1u) * d <= n) q++;
    return q;
}
// (launch bound: 4 wavefronts per SIMD = 128 registers -- the two-pixel state and the next task's prefetched bundle want 131;
// at 3 per SIMD 139-141 us, at 4: 133-138, at 6 (80 registers, 50 of them spilled): 345)
#ifndef SKS_BWD_TILE_OCC
#define SKS_BWD_TILE_OCC 2
#endif
#ifndef SKS_BWD_REQ_UNMASKED
#define SKS_BWD_REQ_UNMASKED 1   // (round 6, interleaved A/B on the stress scene: 450 -> 392 scalar and 696 -> 747 vector instructions per
#endif                            // wavefront, backward 123-125 -> 121-122 us: the scalar half is not what binds this kernel)
template <bool DFEAT, bool EXTRA>
__global__ __launch_bounds__(BWD_TILE_THREADS, 2 * SKS_BWD_TILE_OCC) void k_render_bwd_tile(BwdArgs a, BinView b, int gx, int nviews, unsigned magic_nt,
                                                                           unsigned magic_gx, const uint4* __restrict__ tlist,
                                                                           const uint32_t* __restrict__ hdr)
{
    // (tlist / hdr: the caller's view group -- tlist + g * vg * NT, hdr + g * BIN_CLASSES; see k_bin_scan)
    constexpr int NB = BIN_NB;
    __shared__ BwdWaveLds s_l[BWD_TILE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform per wavefront: say so)
    BwdWaveLds& L = s_l[wv];
    const int P = a.P, C = a.C, W = a.W, H = a.H;
    const size_t HW = (size_t)H * W;
    const bool do_clamp = a.flags & SKS_CLAMP01;
    const bool all_ch = DFEAT || a.bg != nullptr;
    const float ddelx_dx = (float)(0.5 * W), ddely_dy = (float)(0.5 * H);   // backward.cu:527-528
    const unsigned chm_all = C >= 32 ? 0xffffffffu : (1u << C) - 1u;
    const size_t VNT = (size_t)b.NT * nviews;
    const unsigned smask_bits = 3u << (28 + 2 * wv);   // the two strips of this wavefront's half in an entry's index word
    // list position p counts through the classes from the longest lists down
    unsigned cum[BIN_CLASSES + 1];
    cum[0] = 0u;
#pragma unroll
    for (int c = 0; c < BIN_CLASSES; c++) cum[c + 1] = cum[c] + hdr[BIN_HDR_CLASS + (BIN_CLASSES - 1 - c)];
    const unsigned ntiles = cum[BIN_CLASSES];
    auto entry = [&](unsigned p) -> const uint4* {
        int c = 0;
#pragma unroll
        for (int k = 1; k < BIN_CLASSES; k++) c = p >= cum[k] ? k : c;
        return tlist + (size_t)(BIN_CLASSES - 1 - c) * VNT + (p - cum[c]);
    };
    struct Task {   // wave-uniform
        int v, tx, ty, total, cn_last, c0_last;
        size_t tile, eb;
        unsigned chm;
    };
    auto make_task = [&](const uint4& dv) -> Task {
        Task t;
        const unsigned vt = __builtin_amdgcn_readfirstlane(dv.x);
        const unsigned r_lo = __builtin_amdgcn_readfirstlane(dv.y), r_hi = __builtin_amdgcn_readfirstlane(dv.z);
        t.chm = all_ch ? chm_all : __builtin_amdgcn_readfirstlane(dv.w);
        t.v = (int)div_magic(vt, (unsigned)b.NT, magic_nt);
        const unsigned tl = vt - (unsigned)t.v * (unsigned)b.NT;
        t.ty = (int)div_magic(tl, (unsigned)gx, magic_gx);
        t.tx = (int)(tl - (unsigned)t.ty * (unsigned)gx);
        t.tile = vt;
        t.total = (int)(min((size_t)r_hi, b.cap) - min((size_t)r_lo, b.cap));
        t.eb = (size_t)t.v * b.cap + r_lo;
        t.c0_last = t.total > 0 ? ((t.total - 1) >> 6) << 6 : 0;
        t.cn_last = t.total - t.c0_last;
        return t;
    };
    auto request = [&](const Task& t, BwdBundle& B) {   // every load of the task's first pass; nothing is waited for here
        const int x = t.tx * TILE + (lane & 15), yA = t.ty * TILE + 8 * wv + (lane >> 4), yB = yA + 4;
        const bool inA = x < W && yA < H, inB = x < W && yB < H;
        const size_t pixA = inA ? (size_t)yA * W + x : 0, pixB = inB ? (size_t)yB * W + x : 0;
        const size_t e = t.eb + t.c0_last + (lane < t.cn_last ? lane : 0);
        B.ids = b.e_ids[e];
        B.co = b.e_co[e];
        B.xyd = b.e_xyd[e];
        B.axA = B.axB = make_uint2(0u, 0u);
        if (!do_clamp) {   // (forward: final T, last contributor; backward.cu:505-506)
            B.axA = b.aux[(t.tile << 8) + 128 * wv + lane];
            B.axB = b.aux[(t.tile << 8) + 128 * wv + 64 + lane];
        }
        const ChanGroup cgp = chan_group(t.chm, __popc(t.chm), 0);
        const float* dLc = a.dL_color + (size_t)t.v * C * HW;
        // (for every pixel of the half, not only where something contributes: the addresses depend on no other load)
#if SKS_BWD_REQ_UNMASKED
        // every lane loads -- a lane outside the image from pixel 0 of the plane, a valid address -- and the value is selected
        // behind the load: one wave-uniform branch per channel instead of that plus an exec-masked region per pixel (the per-task
        // prologue is where this kernel's scalar instructions are: ~20 per channel before, round 6)
#pragma unroll
        for (int j = 0; j < NB; j++) {
            float va = 0.0f, vb = 0.0f;
            if (j < cgp.n) {
                const float* pl = dLc + (size_t)cgp.chan[j] * HW;
                va = pl[pixA];
                vb = pl[pixB];
            }
            B.gvA[j] = inA ? va : 0.0f;
            B.gvB[j] = inB ? vb : 0.0f;
        }
#else
#pragma unroll
        for (int j = 0; j < NB; j++) {
            B.gvA[j] = (j < cgp.n && inA) ? dLc[(size_t)cgp.chan[j] * HW + pixA] : 0.0f;
            B.gvB[j] = (j < cgp.n && inB) ? dLc[(size_t)cgp.chan[j] * HW + pixB] : 0.0f;
        }
#endif
        B.dLiA = (EXTRA && a.dL_invdepth && inA) ? a.dL_invdepth[(size_t)t.v * HW + pixA] : 0.0f;
        B.dLiB = (EXTRA && a.dL_invdepth && inB) ? a.dL_invdepth[(size_t)t.v * HW + pixB] : 0.0f;
    };

    unsigned p = blockIdx.x;
    if (p >= ntiles) return;
    const unsigned G = gridDim.x;
    Task cur = make_task(*entry(p));
    uint4 dv_next = p + G < ntiles ? *entry(p + G) : make_uint4(0u, 0u, 0u, 0u);
    BwdBundle B;
    request(cur, B);
    for (;;) {
        const Task t = cur;
        const int x = t.tx * TILE + (lane & 15), yA = t.ty * TILE + 8 * wv + (lane >> 4), yB = yA + 4;
        const float pxf = (float)x;
        const v2f py2 = { (float)yA, (float)yB };
        const bool inA = x < W && yA < H, inB = x < W && yB < H;
        const size_t pixA = inA ? (size_t)yA * W + x : 0, pixB = inB ? (size_t)yB * W + x : 0;
        float* part = b.part + (size_t)t.v * b.cap * BIN_ROWS * NACC;
        // this task's first pass arrives: records and dL into LDS, the rest stays in registers
        uint4 ids = B.ids;
        __builtin_amdgcn_wave_barrier();   // every lane is through with the previous task's LDS
        L.co[lane] = B.co;
        L.xyd[lane] = B.xyd;
        const uint2 axA0 = B.axA, axB0 = B.axB;
        float gvA[NB], gvB[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) { gvA[j] = B.gvA[j]; gvB[j] = B.gvB[j]; }
        const v2f dLi0 = { B.dLiA, B.dLiB };
        // the next task: its descriptor has arrived, its first pass is requested now, the descriptor after it too
        const bool more = p + G < ntiles;
        if (more) {
            cur = make_task(dv_next);
            if (p + 2 * G < ntiles) dv_next = *entry(p + 2 * G);
            request(cur, B);
        }
        const int nc = __popc(t.chm);
        const int ngroups = nc > 0 ? (nc + NB - 1) / NB : 1;   // all-zero features: the inverse-depth terms still flow
        v2f T0 = { 1.0f, 1.0f };   // group 0's final T and last contributor serve the later groups too
        int glA0 = -1, glB0 = -1;
        for (int grp = 0; grp < ngroups && t.total > 0; grp++) {
            const ChanGroup cgp = chan_group(t.chm, nc, grp);
            unsigned gmask = 0u;   // the group's channels
#pragma unroll
            for (int j = 0; j < NB; j++) gmask |= j < cgp.n ? (1u << cgp.chan[j]) : 0u;
            if (grp > 0) {
                const float* dLc = a.dL_color + (size_t)t.v * C * HW;
#pragma unroll
                for (int j = 0; j < NB; j++) {
                    gvA[j] = (j < cgp.n && inA) ? dLc[(size_t)cgp.chan[j] * HW + pixA] : 0.0f;
                    gvB[j] = (j < cgp.n && inB) ? dLc[(size_t)cgp.chan[j] * HW + pixB] : 0.0f;
                }
            }
            // per-pixel state
            v2f T = T0;
            int glA = glA0, glB = glB0;
            if (grp == 0 && !do_clamp) {
                T = (v2f){ __uint_as_float(axA0.x), __uint_as_float(axB0.x) };
                glA = inA ? (int)axA0.y - 1 : -1;
                glB = inB ? (int)axB0.y - 1 : -1;
            }
            if (do_clamp) {
                // re-composite front to back (forward.cu:346-386): final T, last contributor and this group's pre-clamp
                // colours, which decide where the clamp lets the gradient through
                v2f col[NB];
#pragma unroll
                for (int j = 0; j < NB; j++) col[j] = (v2f){ 0.0f, 0.0f };
                T = (v2f){ 1.0f, 1.0f };
                glA = glB = -1;
                bool doneA = !inA, doneB = !inB;
                for (int c0 = 0; c0 < t.total; c0 += 64) {
                    if (__all(doneA && doneB)) break;
                    const int cn = min(64, t.total - c0);
                    const size_t e = t.eb + c0 + (lane < cn ? lane : 0);
                    const uint4 idc = b.e_ids[e];
                    __builtin_amdgcn_wave_barrier();
                    L.co[lane] = b.e_co[e];
                    L.xyd[lane] = b.e_xyd[e];
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    for (unsigned long long m = __ballot(lane < cn && (idc.x & smask_bits)); m; m &= m - 1) {
                        if (__all(doneA && doneB)) break;
                        const int k = __builtin_ctzll(m);
                        const float4 co = L.co[k], xyd = L.xyd[k];
                        const uint32_t eid = rlu(idc.x, k) & ID_MASK;
                        const unsigned efm = rlu(idc.z, k) & gmask;
                        const float ef0 = __uint_as_float(rlu(idc.w, k));
                        const float dx = xyd.x - pxf;
                        const v2f dy = xyd.y - py2;
                        const v2f power = power_of2(co, dx, dy);
                        const v2f ca = co.w * expf_fixed2(power);
                        const v2f alpha = { fminf(0.99f, ca.x), fminf(0.99f, ca.y) };
                        const v2f test_T = T * (1.0f - alpha);
                        const bool passA = !doneA && !(power.x > 0.0f) && !(alpha.x < 1.0f / 255.0f);
                        const bool passB = !doneB && !(power.y > 0.0f) && !(alpha.y < 1.0f / 255.0f);
                        const bool stopA = passA && test_T.x < 0.0001f, stopB = passB && test_T.y < 0.0001f;
                        const bool accA = passA && !stopA, accB = passB && !stopB;
                        const int ch0 = __builtin_ctz(rlu(idc.z, k) | 0x80000000u);
                        for (unsigned f = efm; f; f &= f - 1) {   // (wave-uniform: the entry's channels inside this group)
                            const int ch = __builtin_ctz(f);
                            const float fv = ch == ch0 ? ef0 : a.features[(size_t)eid * C + ch];
                            const v2f add = fv * alpha * T;
                            const int j = __popc(gmask & ((1u << ch) - 1u));
#pragma unroll
                            for (int jj = 0; jj < NB; jj++)
                                col[jj] += (v2f){ (jj == j && accA) ? add.x : 0.0f, (jj == j && accB) ? add.y : 0.0f };
                        }
                        if (accA) { T.x = test_T.x; glA = c0 + k; }
                        if (accB) { T.y = test_T.y; glB = c0 + k; }
                        doneA = doneA || stopA;
                        doneB = doneB || stopB;
                    }
                }
                // torch.clamp backward passes the gradient where min <= x <= max
#pragma unroll
                for (int j = 0; j < NB; j++) {
                    if (!(col[j].x >= 0.0f && col[j].x <= 1.0f)) gvA[j] = 0.0f;
                    if (!(col[j].y >= 0.0f && col[j].y <= 1.0f)) gvB[j] = 0.0f;
                }
            }
            if (grp == 0) { T0 = T; glA0 = glA; glB0 = glB; }
            const bool needA = glA >= 0, needB = glB >= 0;
            const v2f Tf = T;
            v2f bgd = { 0.0f, 0.0f };
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const v2f g = { needA ? gvA[j] : 0.0f, needB ? gvB[j] : 0.0f };
                if (EXTRA && a.bg && j < cgp.n) bgd += a.bg[cgp.chan[j]] * g;
                L.d[j][lane] = g.x;
                L.d[j][64 + lane] = g.y;
            }
            const v2f dLi = (grp == 0) ? (v2f){ needA ? dLi0.x : 0.0f, needB ? dLi0.y : 0.0f } : (v2f){ 0.0f, 0.0f };   // group 0's
            WalkState ws;
            ws.T = T;
            ws.la = ws.rec = ws.lst = ws.ainv = ws.linv = (v2f){ 0.0f, 0.0f };
            const bool any_need = __any(needA || needB);
            const int glmax = max(glA, glB);
            // back to front over the chunks (backward.cu:552-636)
            for (int c0 = t.c0_last; c0 >= 0; c0 -= 64) {
                const int cn = min(64, t.total - c0);
                if (grp > 0 || do_clamp || c0 != t.c0_last) {   // (anything but the first pass: fetched here)
                    const size_t e = t.eb + c0 + (lane < cn ? lane : 0);
                    ids = b.e_ids[e];
                    __builtin_amdgcn_wave_barrier();   // every lane is through with the previous chunk's records
                    L.co[lane] = b.e_co[e];
                    L.xyd[lane] = b.e_xyd[e];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                unsigned long long m = any_need ? __ballot(lane < cn && (ids.x & smask_bits)) : 0ull;
                unsigned long long written = 0ull;
                {
#if !SKS_BWD_EXACT
#pragma clang fp contract(fast)
#endif
                    while (m) {
                        const int k = 63 - __builtin_clzll(m);   // back to front
                        m &= ~(1ull << k);
                        const int gk = c0 + k;
                        if (!__any(glmax >= gk)) continue;   // behind every pixel's last contributor
                        const float4 co = L.co[k], xyd = L.xyd[k];
                        const unsigned efm = rlu(ids.z, k) & gmask;
                        const int ch0 = __builtin_ctz(rlu(ids.z, k) | 0x80000000u);
                        // this entry's colour . dL: its channels inside the group (wave-uniform; one on the skeleton scenes)
                        v2f cdot = { 0.0f, 0.0f };
                        for (unsigned f = efm; f; f &= f - 1) {
                            const int ch = __builtin_ctz(f);
                            const float fv = ch == ch0 ? __uint_as_float(rlu(ids.w, k)) : a.features[(size_t)(rlu(ids.x, k) & ID_MASK) * C + ch];
                            const int j = __popc(gmask & ((1u << ch) - 1u));
                            cdot += fv * (v2f){ L.d[j][lane], L.d[j][64 + lane] };
                        }
                        float vals[8];
                        v2f dchannel_dcolor;
                        bool actA, actB;
                        if (!walk_entry<EXTRA>(co, xyd, pxf, py2, cdot, glA, glB, gk, dLi, Tf, bgd, ddelx_dx, ddely_dy, ws, vals, dchannel_dcolor, actA, actB))
                            continue;
                        const float r = wave_sum8(vals);   // lane j < 8: the total of value j
                        const uint32_t slot = rlu(ids.y, k);
                        if (lane < 8 && slot < b.cap) {
                            float* ps = part + ((size_t)slot * BIN_ROWS + wv) * NACC + lane;
                            // later groups add to what this wavefront stored for the group before: read past this CU's L1 (an
                            // L1 line fetched for the previous group's read does not see the store that followed it)
                            if (grp == 0) *ps = r;
                            else *ps = __hip_atomic_load(ps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + r;
                        }
                        written |= 1ull << k;
                        if (DFEAT) {
                            float vf[NB];
#pragma unroll
                            for (int j = 0; j < NB; j++)
                                vf[j] = (actA ? dchannel_dcolor.x * L.d[j][lane] : 0.0f) + (actB ? dchannel_dcolor.y * L.d[j][64 + lane] : 0.0f);
                            const float rf = wave_sum8(vf);
                            int mych = cgp.chan[0];
#pragma unroll
                            for (int j = 1; j < NB; j++) mych = lane == j ? cgp.chan[j] : mych;
                            const uint32_t id = rlu(ids.x, k) & ID_MASK;
                            if (lane < cgp.n && rf != 0.0f) atomicAdd(&a.accum[((size_t)t.v * P + id) * (NACC + C) + NACC + mych], rf);
                        }
                    }
                }
                if (grp == 0 && lane < cn && !((written >> lane) & 1ull) && ids.y < b.cap) {   // rows nothing was added to
                    float4* ps = reinterpret_cast<float4*>(part + ((size_t)ids.y * BIN_ROWS + wv) * NACC);
                    ps[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    ps[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            }
            if (!any_need) break;   // nothing was accepted anywhere in the half (all its rows are zero now)
        }
        if (!more) break;
        p += G;
    }
}
