// sks_fwd_small.inc -- part of the sks_raster.hip translation unit (included inside its anonymous namespace, in order):
// LDS list + forward compositing core, the shared fill role, and the small-path forward kernel (fill + sparse composite).
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

struct FwdArgs {
    int P, C, W, H;
    unsigned flags;
    Geom g;
    const float* features;
    float* out_color;
    float* out_invdepth;
    float* final_T;
    uint32_t* n_contrib;
    int tslots;   // composite blocks per (view, Gaussian) on the small path (composite_slots)
    unsigned cp1_magic;   // ceil(2^20 / (C+1)): blockIdx.z / (C+1) as a multiply + shift in the fill blocks (handed to the
                          // kernels as a separate scalar argument next to fsplit: one kernarg load, no late fetch)
    int ncomp;            // composite blocks of the small-path forward = tslots * P * V
    int cover_planes;     // 1: `cover` holds a row per (view, PLANE, band) (binned path: Bin::coverp; small path when cover_per_plane)
                          // and the compositor stores only the planes a tile's list touches; 0: a row per (view, band) or no cover
                          // rows at all, the compositor writes every plane of a covered tile
    unsigned w_magic;     // ceil(2^32 / W) for 2 <= W < 16384 (else 0): pixel index % W in the fill blocks as a multiply-high --
                          // exact for index < 16 W; the division sequence was ~40 instructions per pass in blocks whose whole
                          // life is ~2 us
};

// ------------------------------------------------------------------------------------------------------------
// small path forward, "fill + sparse composite" in ONE launch.  With a skeleton (P = 15..19) a view covers ~100 of
// ~4000 tiles, so the kernel is a dense zero fill of (C+1) planes with a sprinkle of compositing.  Two roles by
// block index (the composite blocks sit in the first rows of the dispatch so their latency hides under the fill):
//   * composite role, block (slot, g, v): walks the tiles of Gaussian g's rect (slot, slot + slots, ...).  The
//     tile is rendered by the LOWEST-index Gaussian whose rect covers it (so every covered tile has exactly one
//     owner); the owner gathers the covering Gaussians, orders them by (depth bits, index) -- the order the
//     reference gets from its stable radix sort of (tile | depth) keys with index-major emission -- and composites
//     thread-per-pixel exactly like forward.cu:278-401, writing all C+1 planes of the tile;
//   * fill role, block (plane, band, v): streams zeros over its plane's 16-row band (rows*W contiguous floats,
//     16 B per lane), skipping the tile columns some Gaussian rect covers in that band.
// A pure fill of this shape runs at the rate of tensor.zero_() (46 us for the 288 MB of 4 H36M views on MI355X).
// PPT = 4 needs W % 4 == 0, or (HALF) W % 4 == 2 with an even H; PPT = 1 handles any W with 4-byte stores.
// ------------------------------------------------------------------------------------------------------------
// composite blocks per (view, Gaussian): 4 for a handful of views, 8 for many (interleaved A/B of 2..16: all within 1%);
// flag bits 26..29 override (tuning)
inline int composite_slots(unsigned flags, int V, int P)
{
    const int t = (int)((flags >> 26) & 15u);
    return t ? t : ((long long)V * P <= 128 ? 4 : 8);
}

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

typedef float v2f __attribute__((ext_vector_type(2)));

template <bool NT>
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d)
{
    v4f v = { a, b, c, d };
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(p));
    else *reinterpret_cast<v4f*>(p) = v;
}
template <bool NT>
__device__ __forceinline__ void store2(float* p, float a, float b)
{
    v2f v = { a, b };
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<v2f*>(p));
    else *reinterpret_cast<v2f*>(p) = v;
}

// dynamic-LDS list with capacity `cap` entries (cap = P rounded up to 16)
template <int CG>
struct DynList {
    float2* xy;
    float4* co;
    float* invd;
    float* feat;               // cap * CG
    unsigned long long* key;   // cap
    uint4* rect;               // cap
    __device__ DynList(char* base, int cap)
    {
        co = (float4*)base; base += (size_t)cap * 16;
        rect = (uint4*)base; base += (size_t)cap * 16;
        key = (unsigned long long*)base; base += (size_t)cap * 8;
        xy = (float2*)base; base += (size_t)cap * 8;
        invd = (float*)base; base += (size_t)cap * 4;
        feat = (float*)base;
    }
    static size_t bytes(int cap, int cg) { return (size_t)cap * (16 + 16 + 8 + 8 + 4 + 4 * (size_t)cg); }
};

// ------------------------------------------------------------------------------------------------------------
// fill role shared by the two forward kernels (fill + sparse composite): block (q, band, zid = view * (C+1) + plane)
// streams zeros over pb passes of its plane's 16-row band, skipping the tile columns whose bit is set in the
// band's `cover` row (those tiles are written by a composite block).
// A pass = 256 threads x 16 B = 4 KB of one plane; a block does pb passes (2 by default: ~8 KB per block measured best,
// tools/ab_fill.py; a standalone fill of many small blocks reaches 44-47 us for 288 MB, tools/fill_bench.hip), but only
// if nothing VECTOR-memory sits in front of the store: a dependent global_load queues behind the chip-wide flood of
// stores (measured: 2.4 TB/s).  The band's cover words written by k_geom_fwd are therefore read through the SCALAR
// cache (s_load: `cover` is a const __restrict__ kernel argument and the address is made wave-uniform).
// block order = memory order (pass, band, plane, view): concurrently running blocks write one contiguous window
// HALF (PPT == 4, W % 4 == 2 and H even -- H36M's 1002-wide sensors, dataset_readers.py:68-80): every band of every plane
// still starts on a 16-byte boundary (16 * W * 4 and H * W * 4 are multiples of 16), so the band is streamed with the same
// 16-byte stores; but rows start at 8-byte offsets, so a float4 may straddle a row end or a tile-column boundary in its
// middle (never inside a pair: W is even).  Each pass therefore carries two skip bits, one per pair, and a float4 with one
// covered pair is written as the other pair's 8 bytes.
// ------------------------------------------------------------------------------------------------------------
// the bare stream of stores of a band no rect crosses (fwd_fill_role) and of the planes k_geom_fwd_fill zeroes: npass passes of
// 256 * PPT floats from base0 on, clipped to the band's [0, Nb)
template <int PPT, bool NT>
__device__ __forceinline__ void fill_bare(float* out, float* outT, uint32_t* outN, int base0, int Nb, int npass)
{
    constexpr int PASS = 256 * PPT;
    for (int k = 0; k < npass; k++) {
        const int base = base0 + k * PASS;
        if (base >= Nb) break;
        if (base < 0) continue;          // (in front of the band: the short first pass, see `shift`)
        if (PPT == 4) store4<NT>(out + base, 0.0f, 0.0f, 0.0f, 0.0f);   // (HALF: Nb is a multiple of 4, rows are even)
        else out[base] = 0.0f;
        if (outT || outN) {
#pragma unroll
            for (int p = 0; p < PPT; p++) {
                if (outT) outT[base + p] = 1.0f;
                if (outN) outN[base + p] = 0u;
            }
        }
    }
}

template <int PPT, bool NT, bool HALF = false>
__device__ __forceinline__ void fwd_fill_role(const FwdArgs& a, unsigned cp1_magic, int q, int band, int zid, int gy, int pb,
                                              const uint32_t* __restrict__ cover)
{
    const int tid = threadIdx.x;
    const int P = a.P, C = a.C, W = a.W, H = a.H;
    const size_t HW = (size_t)H * W;
    // zid / (C+1) without the emulated integer division (exact for zid < 64 * 33 with a 20-bit reciprocal, host:
    // sks_forward).  That division sat between the kernarg fetch and the cover-row load of EVERY fill block, whose whole
    // life is ~2 us: replacing it was worth 2.3 us of 54 (interleaved A/B); the per-lane `% W` below is not on that path.
    const int v = (int)(((unsigned)zid * cp1_magic) >> 20);
    const int plane = zid - v * (C + 1);
    const bool is_inv = plane == C;
    const int cw = cover_cw(W);
    constexpr int PASS = 256 * PPT;
    const int rows = min(TILE, H - band * TILE);
    const int Nb = rows * W;  // this band of this plane: Nb contiguous floats
    const size_t band0 = (size_t)band * TILE * W;
    float* out = (is_inv ? a.out_invdepth + (size_t)v * HW : a.out_color + ((size_t)v * C + plane) * HW) + band0;
    // passes are cut on 128-byte lines of the ADDRESS, not of the band: when H * W is not a multiple of 32 floats (1002 x
    // 1000: every other plane starts 64 bytes into a line) the band's first pass is short by `shift` floats and every
    // later one is 32 whole lines again -- otherwise each 4 KB pass would end and start in a partially written line
    const int shift = (int)((reinterpret_cast<uintptr_t>(out) >> 2) & 31u);   // wave-uniform; 0 for 1000 x 1000, 1920 x 1080
    const int base0 = q * PASS * pb + tid * PPT - shift;     // this block covers passes q*pb .. q*pb + pb - 1 of the band
    float* outT = (is_inv && a.final_T) ? a.final_T + (size_t)v * HW + band0 : nullptr;
    uint32_t* outN = (is_inv && a.n_contrib) ? a.n_contrib + (size_t)v * HW + band0 : nullptr;
    // the band's cover row through the SCALAR cache (`cover` is a const __restrict__ kernel argument, the address is
    // made wave-uniform): one 16-byte load = [any, bits 0..95] (images up to 1536 px wide), a second one for up to
    // 3584 px; wider images read the bit word they need per lane (before any store, see below)
    const uint32_t* __restrict__ cwp = cover;
    v4u c0 = { 0u, 0u, 0u, 0u }, c1 = { 0u, 0u, 0u, 0u };
    if (cover) {
        const int wo = __builtin_amdgcn_readfirstlane(((a.cover_planes ? zid : v) * gy + band) * cw);
        cwp = cover + wo;
        c0 = *reinterpret_cast<const v4u*>(cwp);
        if (cw > 4) c1 = *reinterpret_cast<const v4u*>(cwp + 4);
    }
    const bool any = c0.x != 0u;   // only bands some rect crosses look at the tile bits
    const unsigned w_magic = a.w_magic;
    auto mod_w = [&](int base) -> int {   // base % W for 0 <= base < 16 W
        if (w_magic) return base - (int)__umulhi((unsigned)base, w_magic) * W;
        return base % W;
    };
    auto cover_word = [&](int wi) -> uint32_t {
        if (cw <= 4) return wi == 0 ? c0.y : wi == 1 ? c0.z : c0.w;
        if (cw <= 8) return wi == 0 ? c0.y : wi == 1 ? c0.z : wi == 2 ? c0.w : wi == 3 ? c1.x : wi == 4 ? c1.y : wi == 5 ? c1.z : c1.w;
        return cwp[1 + wi];
    };
    if (pb < 0) {
        // Row-aligned mode (PPT == 4, cover present, launcher: fill_row_mode): block q = (row block, x chunk of 1024
        // pixels); a lane keeps the same 4 pixels' column in every row, so its tile column -- and the skip bit -- is
        // computed ONCE, without the per-pass modulo of the linear mode below.
        const int pbr = -pb;
        const int chunks = (W + PASS - 1) / PASS;
        const int rb = q / chunks, chunk = q - rb * chunks;
        const int x = chunk * PASS + tid * PPT;
        if (x >= W) return;
        if (any) {
            const int tx = x >> 4;
            if ((cover_word(tx >> 5) >> (tx & 31)) & 1u) return;
        }
        const int r1 = min(rows, (rb + 1) * pbr);
        for (int r = rb * pbr; r < r1; r++) {
            const int base = r * W + x;
            store4<NT>(out + base, 0.0f, 0.0f, 0.0f, 0.0f);
            if (outT || outN) {
#pragma unroll
                for (int p = 0; p < PPT; p++) {
                    if (outT) outT[base + p] = 1.0f;
                    if (outN) outN[base + p] = 0u;
                }
            }
        }
        return;
    }
    // phase 1: which of this block's passes does this lane skip (tiles a composite block writes)?  Every look-up
    // happens BEFORE the first store: on gfx9 loads and stores share the vmcnt counter, so a load in the store loop --
    // or just the compiler's conservative wait where a path with a load joins -- makes pass k+1 wait for the store of
    // pass k to complete (measured: 3.2 us of 57 on the H36M forward).
    const int npass = min(pb, 32);
    if (cover && !any) {
        // No rect crosses this band (more than half of the bands of a skeleton scene, every band of an empty view): the
        // block is a bare stream of stores.  Kept apart from the general path below on purpose: a fill block lives ~2 us, at
        // 8 waves per SIMD the launch is bound by that life time, and every instruction in front of or between its stores
        // shows in the kernel time -- the pair logic of the HALF mode alone, never taken here, cost 4.9 us of 46 on the pure
        // fill of a 1002-wide launch while it sat in this loop (interleaved A/B, tools/width_sweep2.py).
        fill_bare<PPT, NT>(out, outT, outN, base0, Nb, npass);
        return;
    }
    unsigned skipmask = 0u, skipmask2 = 0u;   // skipmask2 (HALF): the float4's second pair
    // HALF: tile column of the second pair (two pixels on: the same row, or the start of the next one)
    auto second_tx = [&](int x0) -> int { const int x1 = x0 + 2; return (x1 >= W ? x1 - W : x1) >> 4; };
    if (any && cw <= 8) {
        // Covered band, cover row in scalar registers (images up to 3584 px wide): look-up of pass k, then store of pass k.
        // The two-phase form below exists because a LOAD between the stores couples them through vmcnt; here the look-up
        // is scalar selects and vector ALU only, and interleaving it measured 0.5 us (W = 1000) to 1.8 us (W = 1002,
        // pair masks) better than finishing all look-ups first (interleaved A/B, tools/ab_sweep.sh).
        for (int k = 0; k < npass; k++) {
            const int base = base0 + k * PASS;
            if (base >= Nb) break;
            if (base < 0) continue;
            const int x0 = mod_w(base);
            const int tx = x0 >> 4;
            const bool s0 = (cover_word(tx >> 5) >> (tx & 31)) & 1u;
            bool s1 = s0;
            if (HALF) {
                const int tx1 = second_tx(x0);
                s1 = ((cover_word(tx1 >> 5) >> (tx1 & 31)) & 1u) || base + 2 >= Nb;
            }
            if (s0 && s1) continue;
            if (PPT == 4) {
                if (!HALF || (!s0 && !s1)) store4<NT>(out + base, 0.0f, 0.0f, 0.0f, 0.0f);
                else store2<NT>(out + base + (s0 ? 2 : 0), 0.0f, 0.0f);
            } else {
                out[base] = 0.0f;
            }
            if (outT || outN) {
#pragma unroll
                for (int p = 0; p < PPT; p++) {
                    if (HALF && (p < 2 ? s0 : s1)) continue;
                    if (outT) outT[base + p] = 1.0f;
                    if (outN) outN[base + p] = 0u;
                }
            }
        }
        return;
    } else if (any) {
        for (int k = 0; k < npass; k++) {
            const int base = base0 + k * PASS;
            if (base >= Nb) break;
            if (base < 0) continue;          // (in front of the band: the short first pass, see `shift`)
            const int x0 = mod_w(base);
            const int tx = x0 >> 4;  // PPT == 4 and W % 4 == 0: the 4 pixels share one tile column
            skipmask |= ((cover_word(tx >> 5) >> (tx & 31)) & 1u) << k;
            if (HALF) {
                const int tx1 = second_tx(x0);
                skipmask2 |= ((cover_word(tx1 >> 5) >> (tx1 & 31)) & 1u) << k;
            }
        }
    } else if (!cover) {  // cover not precomputed (very large images): test the rects directly
        const uint4* grect = a.g.rect + (size_t)v * P;
        for (int i = 0; i < P; i++) {
            const uint4 r = grect[i];
            if (!((int)r.y <= band && band < (int)r.w)) continue;
            for (int k = 0; k < npass; k++) {
                const int base = base0 + k * PASS;
                if (base >= Nb) break;
                if (base < 0) continue;
                const int x0 = mod_w(base);
                const int tx = x0 >> 4;
                skipmask |= (((int)r.x <= tx && tx < (int)r.z) ? 1u : 0u) << k;
                if (HALF) {
                    const int tx1 = second_tx(x0);
                    skipmask2 |= (((int)r.x <= tx1 && tx1 < (int)r.z) ? 1u : 0u) << k;
                }
            }
        }
    }
    // phase 2: stores only
    for (int k = 0; k < npass; k++) {
        const int base = base0 + k * PASS;
        if (base >= Nb) break;
        if (base < 0) continue;
        const bool s0 = (skipmask >> k) & 1u;
        const bool s1 = HALF ? (((skipmask2 >> k) & 1u) || base + 2 >= Nb) : s0;   // (a band of an odd row count ends on a pair)
        if (s0 && s1) continue;
        if (PPT == 4) {
            if (!HALF || (!s0 && !s1)) store4<NT>(out + base, 0.0f, 0.0f, 0.0f, 0.0f);
            else store2<NT>(out + base + (s0 ? 2 : 0), 0.0f, 0.0f);
        } else {
            out[base] = 0.0f;
        }
        if (outT || outN) {  // debug planes of the reference's ImageState: T = 1, no contributor outside covered tiles
#pragma unroll
            for (int p = 0; p < PPT; p++) {
                if (HALF && (p < 2 ? s0 : s1)) continue;
                if (outT) outT[base + p] = 1.0f;
                if (outN) outN[base + p] = 0u;
            }
        }
    }
}

#ifndef SKS_FWD_WAVES_ATTR
#define SKS_FWD_WAVES_ATTR
#endif
template <int CG, int PPT, bool NT, bool HALF = false>
__global__ __launch_bounds__(256) SKS_FWD_WAVES_ATTR void k_render_fwd_sparse(FwdArgs a, unsigned cp1_magic, int gy, int fsplit, int pb,
                                                           const uint32_t* __restrict__ cover)
{
    extern __shared__ __attribute__((aligned(16))) char s_dyn[];
    __shared__ int s_n, s_min;
    __shared__ unsigned s_chm;   // the planes the tile in hand is written on: OR of its list's non-zero features
    const int tid = threadIdx.x;
    const int P = a.P, C = a.C, W = a.W, H = a.H;
    const size_t HW = (size_t)H * W;

    // grid (fsplit + xc, bands, (C+1) * V): x < fsplit are the fill passes of one (band, plane, view) row, the xc extra
    // blocks per row carry the composite role (spread through the dispatch order so that their latency -- list
    // building, barriers -- overlaps the streaming stores).  No integer division on the fill path except z / (C+1).
    const int xq = blockIdx.x, band_id = blockIdx.y, zid = blockIdx.z;
    const int xc = gridDim.x - fsplit;
    const bool comp_role = xq >= fsplit;
    if (comp_role) {
        // ---------------- composite role ----------------
        const int cb = (zid * gy + band_id) * xc + (xq - fsplit);
        if (cb >= a.ncomp) return;
        const int T_SLOTS = a.tslots;
        const int slot = cb % T_SLOTS;
        const int g = (cb / T_SLOTS) % P;
        const int v = cb / (T_SLOTS * P);
        const size_t go = (size_t)v * P;
        const float4* gco = a.g.co + go;
        const float4* gxyd = a.g.xyd + go;
        const uint4* grect = a.g.rect + go;
        const uint4 rg = grect[g];
        const int wt = (int)(rg.z - rg.x), ht = (int)(rg.w - rg.y);
        const int ntiles = wt * ht;
        if (slot >= ntiles) return;
        const int cap = (P + 15) & ~15;
        DynList<CG> L(s_dyn, cap);
        if (tid < P) L.rect[tid] = grect[tid];
        __syncthreads();
        float* outc = a.out_color + (size_t)v * C * HW;
        float* outi = a.out_invdepth + (size_t)v * HW;
        const bool do_clamp = a.flags & SKS_CLAMP01;
        for (int t = slot; t < ntiles; t += T_SLOTS) {
            const int ty = (int)rg.y + t / wt, tx = (int)rg.x + t % wt;
            if (tid == 0) { s_n = 0; s_min = 0x7fffffff; }
            __syncthreads();
            if (tid < P) {
                const uint4 r = L.rect[tid];
                if ((int)r.x <= tx && tx < (int)r.z && (int)r.y <= ty && ty < (int)r.w) {
                    atomicMin(&s_min, tid);
                    const int sl = atomicAdd(&s_n, 1);
                    L.key[sl] = ((unsigned long long)__float_as_uint(gxyd[tid].z) << 32) | (unsigned)tid;
                }
            }
            __syncthreads();
            const int n = s_n;
            if (s_min == g) {  // uniform: this block owns the tile
                if (tid < n) {
                    const unsigned long long key = L.key[tid];
                    int rank = 0;
                    for (int j = 0; j < n; j++) rank += (L.key[j] < key) ? 1 : 0;
                    const int id = (int)(unsigned)key;
                    const float4 xyd = gxyd[id];
                    L.xy[rank] = make_float2(xyd.x, xyd.y);
                    L.co[rank] = gco[id];
                    L.invd[rank] = xyd.w;
#pragma unroll
                    for (int ch = 0; ch < CG; ch++) L.feat[rank * CG + ch] = ch < C ? a.features[id * C + ch] : 0.0f;
                }
                __syncthreads();
                // with per-plane cover rows (k_geom_fwd, cover_per_plane) the planes no entry of the list has a feature on are the
                // fill role's: one lane per channel looks down the staged list, the wavefronts' findings are ORed in LDS
                unsigned chm = 0xffffffffu;
                if (a.cover_planes) {
                    bool nz = false;
                    if (tid < CG)
                        for (int k = 0; k < n; k++) nz = nz || L.feat[k * CG + tid] != 0.0f;
                    if (tid < 64) {
                        const unsigned long long bl = __ballot(nz);
                        if (tid == 0) s_chm = (unsigned)bl;
                    }
                    __syncthreads();
                    chm = s_chm;
                }
                const int x = tx * TILE + (tid & 15), y = ty * TILE + (tid >> 4);
                if (x < W && y < H) {
                    const float pxf = (float)x, pyf = (float)y;
                    float T = 1.0f, inv = 0.0f, acc[CG];
#pragma unroll
                    for (int ch = 0; ch < CG; ch++) acc[ch] = 0.0f;
                    uint32_t contributor = 0, last = 0;
                    for (int k = 0; k < n; k++) {  // forward.cu:346-386
                        contributor++;
                        const float2 xy = L.xy[k];
                        const float4 co = L.co[k];
                        const float dx = xy.x - pxf, dy = xy.y - pyf;
                        const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
                        if (power > 0.0f) continue;
                        const float alpha = fminf(0.99f, co.w * expf_fixed(power));
                        if (alpha < 1.0f / 255.0f) continue;
                        const float test_T = T * (1 - alpha);
                        if (test_T < 0.0001f) break;
#pragma unroll
                        for (int ch = 0; ch < CG; ch++) acc[ch] += L.feat[k * CG + ch] * alpha * T;
                        inv += L.invd[k] * alpha * T;
                        T = test_T;
                        last = contributor;
                    }
                    const size_t pix = (size_t)y * W + x;
#pragma unroll
                    for (int ch = 0; ch < CG; ch++)
                        if (ch < C && ((chm >> ch) & 1u)) outc[(size_t)ch * HW + pix] = do_clamp ? clamp01(acc[ch]) : acc[ch];
                    outi[pix] = inv;
                    if (a.final_T) a.final_T[(size_t)v * HW + pix] = T;
                    if (a.n_contrib) a.n_contrib[(size_t)v * HW + pix] = last;
                }
            }
            __syncthreads();
        }
        return;
    }
    // ---------------- fill role ----------------
    fwd_fill_role<PPT, NT, HALF>(a, cp1_magic, xq, band_id, zid, gy, pb, cover);
}

// ------------------------------------------------------------------------------------------------------------
// The geometry launch of a plain small-path sks_forward, carrying the zero fill of the call's LAST planes: for the ~5 us
// of k_geom_fwd (72 workgroups, two dependent round trips) the memory system carries nothing, and a fill block that
// zeroes its passes unconditionally needs nothing from the geometry -- the tiles it should have skipped are written
// again by the composite blocks of k_render_fwd_sparse, the NEXT launch in the stream, which then streams only the
// planes zid < zid0 (launch_fwd_small).  1-D grid: blocks 0 .. ngeom - 1 are k_geom_fwd's blocks (view, plane) -- first
// in dispatch order, same arithmetic, same stores --, block ngeom + e is fill block (q, band, zid) of the early
// region in memory order, e = ((zid - zid0) * gy + band) * fsplit + q.  A fill block loads nothing: every argument
// comes by value, the divisions are multiply-highs by reciprocals the host made (exact: e * rows < 2^32,
// early_fill_plan), and it runs fill_bare, the store loop of a band no rect crosses.
// ------------------------------------------------------------------------------------------------------------
struct EarlyFill {
    float* out_color;
    float* out_invdepth;
    int C, W, H, gy;
    int gplanes;          // k_geom_fwd's grid.z: C + 1 (a cover row set per plane) or 1
    int ngeom;            // V * gplanes geometry blocks in front
    int zid0;             // first early plane, zid = view * (C + 1) + plane
    int fsplit, pb;       // fill blocks per (plane, band) row / passes per block: those of the main launch (fill_geometry)
    unsigned cp1_magic;   // FwdArgs::cp1_magic
    unsigned row_magic;   // ceil(2^32 / (fsplit * gy)), 0 when that divisor is 1
    unsigned fs_magic;    // ceil(2^32 / fsplit), likewise
};

template <int PPT, bool NT>
__global__ __launch_bounds__(256) void k_geom_fwd_fill(EarlyFill f, int P, ViewTan vt, const float* __restrict__ vms,
                                                       const float* __restrict__ pms, const float* __restrict__ means,
                                                       const float* __restrict__ opac, const float* __restrict__ scales,
                                                       const float* __restrict__ rots, const float* __restrict__ cov3Dp, float smod,
                                                       unsigned flags, Geom g, int* __restrict__ radii,
                                                       const float* __restrict__ features, int cover_planes)
{
    const int b = blockIdx.x;
    if (b < f.ngeom) {
        const int v = f.gplanes == 1 ? b : (int)(((unsigned)b * f.cp1_magic) >> 20);
        extern __shared__ __attribute__((aligned(16))) char s_dyn[];   // gy * cover_cw(W) words: what the call's cover rows need, so that
                                                                       // the fill blocks behind keep 8 workgroups per CU (k_geom_fwd's fixed 24 KB: 6)
        geom_fwd_block((uint32_t*)s_dyn, 0, v, b - v * f.gplanes, P, f.W, f.H, vt, vms, pms, means, opac, scales, rots, cov3Dp, smod, flags, g, radii, 0,
                       nullptr, nullptr, features, f.C, nullptr, nullptr, cover_planes);
        return;
    }
    const unsigned e = (unsigned)(b - f.ngeom);
    const unsigned rows = (unsigned)(f.fsplit * f.gy);
    const unsigned zr = f.row_magic ? __umulhi(e, f.row_magic) : e;        // (a magic of 0 stands for the divisor 1)
    const unsigned rem = e - zr * rows;
    const int band = (int)(f.fs_magic ? __umulhi(rem, f.fs_magic) : rem);
    const int q = (int)rem - band * f.fsplit;
    const int zid = f.zid0 + (int)zr;
    const int v = (int)(((unsigned)zid * f.cp1_magic) >> 20);
    const int plane = zid - v * (f.C + 1);
    const size_t HW = (size_t)f.H * f.W;
    const int Nb = min(TILE, f.H - band * TILE) * f.W;
    float* out = (plane == f.C ? f.out_invdepth + (size_t)v * HW : f.out_color + ((size_t)v * f.C + plane) * HW) + (size_t)band * TILE * f.W;
    const int shift = (int)((reinterpret_cast<uintptr_t>(out) >> 2) & 31u);   // passes cut on 128-byte lines of the address (fwd_fill_role)
    fill_bare<PPT, NT>(out, nullptr, nullptr, q * (256 * PPT) * f.pb + (int)threadIdx.x * PPT - shift, Nb, min(f.pb, 32));
}

// ------------------------------------------------------------------------------------------------------------
// The prefill role of the small-path backward's two launches (k_render_bwd_wave, k_geom_bwd_all): while they run HBM
// carries almost nothing, so the blocks behind a launch's own grid zero the LAST planes of ANOTHER output set, the one
// the next forward renders into (sks_backward_prefill / sks_forward_prefilled).  Fill block e of the role is block
// (q, band, zid) of the region [zid0, zid0 + nz) in memory order, e = ((zid - zid0) * gy + band) * fsplit + q, as in
// k_geom_fwd_fill: every argument by value, multiply-high index splits the host checked (prefill_cut), nothing loaded,
// 16-byte non-temporal stores only (launchers: W % 4 == 0, or W % 4 == 2 with an even H).
// ------------------------------------------------------------------------------------------------------------
struct PreFill {
    float* out_color;     // the OTHER output set
    float* out_invdepth;
    int C, W, H, gy;
    int zid0;             // first plane of this launch's share, zid = view * (C + 1) + plane
    unsigned nfill;       // fill blocks of this launch: fsplit * gy * planes
    int fsplit, pb;       // fill blocks per (plane, band) row / passes per block
    int zs;               // k_render_bwd_wave: the role's own gridDim.z (the layers behind it are fill blocks)
    unsigned cp1_magic;   // FwdArgs::cp1_magic
    unsigned row_magic;   // ceil(2^32 / (fsplit * gy)), 0 when that divisor is 1
    unsigned fs_magic;    // ceil(2^32 / fsplit), likewise
};

__device__ __forceinline__ void prefill_block(const PreFill& f, unsigned e)
{
    if (e >= f.nfill) return;
    const unsigned rows = (unsigned)(f.fsplit * f.gy);
    const unsigned zr = f.row_magic ? __umulhi(e, f.row_magic) : e;        // (a magic of 0 stands for the divisor 1)
    const unsigned rem = e - zr * rows;
    const int band = (int)(f.fs_magic ? __umulhi(rem, f.fs_magic) : rem);
    const int q = (int)rem - band * f.fsplit;
    const int zid = f.zid0 + (int)zr;
    const int v = (int)(((unsigned)zid * f.cp1_magic) >> 20);
    const int plane = zid - v * (f.C + 1);
    const size_t HW = (size_t)f.H * f.W;
    const int Nb = min(TILE, f.H - band * TILE) * f.W;
    float* out = (plane == f.C ? f.out_invdepth + (size_t)v * HW : f.out_color + ((size_t)v * f.C + plane) * HW) + (size_t)band * TILE * f.W;
    const int shift = (int)((reinterpret_cast<uintptr_t>(out) >> 2) & 31u);   // passes cut on 128-byte lines of the address (fwd_fill_role)
    fill_bare<4, true>(out, nullptr, nullptr, q * 1024 * f.pb + (int)threadIdx.x * 4 - shift, Nb, min(f.pb, 32));
}
