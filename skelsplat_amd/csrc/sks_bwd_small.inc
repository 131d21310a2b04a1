// sks_bwd_small.inc -- part of the sks_raster.hip translation unit (included inside its anonymous namespace, in order):
// backward compositing cores, the gather / wave-resident small-path backward kernels, heat-map statistics.
// per-pixel state of the back-to-front walk (backward.cu:531-637), k_render_bwd_gather
template <int CG>
struct BwdPix {
    float T, T_final, last_alpha, accum_inv, last_inv, dLi, bgdot;
    float dL[CG], accum_rec[CG], last_color[CG];
};

struct BwdArgs {
    int P, C, W, H;
    unsigned flags;
    Geom g;
    const float* features;
    const float* bg;
    const float* dL_color;     // fused-loss mode: the pseudo-GT heat-maps (V,C,H,W) instead of dL/d(render)
    const float* dL_invdepth;
    float* accum;  // (V,P,NACC+C)
    const float* tile_S;       // (unused since the loss corrections are taken where the render is positive; kept
    const float* tile_N;       //  for the ABI's argument list)
    // fused-loss mode, heat-maps given by their separable factors instead of planes (never written anywhere):
    // gt(v, ch, y, x) = (hm_row[(v C + ch) H + y] * hm_col[(v C + ch) W + x] - hm_cmin[v C + ch]) / hm_den[v C + ch],
    // H / W = the strides = this struct's H / W (the largest view); nullptr = read dL_color's planes
    const float* hm_row = nullptr;
    const float* hm_col = nullptr;
    const float* hm_cmin = nullptr;
    const float* hm_den = nullptr;
    // early-stopping variant of the fused-loss kernel (ES, sks_loop_fused_step_es): es_stop[f * es_stride] != 0 when frame
    // f = view / es_views has stopped -- written only by the previous launch's step tail, on the same stream
    const int* es_stop = nullptr;
    int es_stride = 0;
    int es_views = 1;
};

// ------------------------------------------------------------------------------------------------------------
// small path backward, gathered per Gaussian: grid (BWD_SPLITS, P, V).  Workgroup (s, g, v) walks the pixels of
// Gaussian g's tile rect (256-pixel chunks s, s+BWD_SPLITS, ...), re-composites each pixel over the LDS list of
// every Gaussian whose rect meets g's rect, walks back to front like backward.cu:531-637 and keeps ONLY g's terms.
// Sums stay in registers, are reduced once per workgroup and stored to the (v, g, s) partial slot: no atomics,
// no zero-initialised scratch, bitwise reproducible gradients.
// ------------------------------------------------------------------------------------------------------------
// dynamic-LDS working set of the gather kernel, capacity `cap` = P rounded up to 16
template <int CG>
struct GatherLds {
    // raw records of ALL Gaussians of the view, indexed by Gaussian id (one global round trip fills them)
    float4* r_co;
    float4* r_xyd;
    uint4* r_rect;
    float* r_feat;  // cap * C
    unsigned long long* key;  // cap
    // the local list, ordered by (depth bits, index)
    float2* xy;
    float4* co;
    float* invd;
    int* xr;
    int* yr;
    int* id;
    float* feat;  // cap * CG, compacted channels
    __device__ GatherLds(char* p, int cap, int C)
    {
        r_co = (float4*)p; p += (size_t)cap * 16;
        r_xyd = (float4*)p; p += (size_t)cap * 16;
        r_rect = (uint4*)p; p += (size_t)cap * 16;
        co = (float4*)p; p += (size_t)cap * 16;
        key = (unsigned long long*)p; p += (size_t)cap * 8;
        xy = (float2*)p; p += (size_t)cap * 8;
        invd = (float*)p; p += (size_t)cap * 4;
        xr = (int*)p; p += (size_t)cap * 4;
        yr = (int*)p; p += (size_t)cap * 4;
        id = (int*)p; p += (size_t)cap * 4;
        feat = (float*)p; p += (size_t)cap * CG * 4;
        r_feat = (float*)p;
    }
    static size_t bytes(int cap, int cg, int C) { return (size_t)cap * (16 * 4 + 8 * 2 + 4 * 4 + 4 * (size_t)cg + 4 * (size_t)C); }
};

template <int CG, bool DFEAT>
__global__ __launch_bounds__(256) void k_render_bwd_gather(BwdArgs a)
{
    constexpr int NV = NACC + (DFEAT ? CG : 0);
    extern __shared__ __attribute__((aligned(16))) char s_dyn[];
    __shared__ float s_red[4][NV];
    __shared__ int s_chan[CG], s_act[CG];
    const int g = blockIdx.x, v = blockIdx.y, sp = blockIdx.z, tid = threadIdx.x;   // splits slowest: see launch_bwd_small
    const int P = a.P, C = a.C, W = a.W, H = a.H;
    const int NVS = NACC + C;
    const size_t HW = (size_t)H * W;
    const size_t go = (size_t)v * P;
    const float4* gco = a.g.co + go;
    const float4* gxyd = a.g.xyd + go;
    const uint4* grect = a.g.rect + go;
    // partial-sum slots, layout (v, g, value, split): the BWD_SPLITS partials of one value are one 64-byte line
    float* out = a.accum + ((size_t)v * P + g) * NVS * BWD_SPLITS + sp;
    const uint4 rg = grect[g];
    const int x0 = (int)rg.x * TILE, y0 = (int)rg.y * TILE;
    const int wpx = min(W, (int)rg.z * TILE) - x0, hpx = min(H, (int)rg.w * TILE) - y0;
    const int npx = wpx * hpx;  // 0 when culled (rect all zero)
    const int nchunks = (npx + 255) / 256;
    if (sp >= nchunks) {  // nothing for this slot (also every slot of an invisible Gaussian)
        if (tid < NVS) out[tid * BWD_SPLITS] = 0.0f;
        return;
    }
    // one global round trip: every Gaussian's record + features into LDS
    const int cap = (P + 15) & ~15;
    GatherLds<CG> L(s_dyn, cap, C);
    if (tid < P) {
        L.r_co[tid] = gco[tid];
        L.r_xyd[tid] = gxyd[tid];
        L.r_rect[tid] = grect[tid];
    }
    for (int i = tid; i < P * C; i += 256) L.r_feat[i] = a.features[i];
    __syncthreads();
    // local list: Gaussians whose tile rect intersects g's, ordered by (depth bits, index)
    unsigned long long mykey = ~0ull;
    if (tid < P) {
        const uint4 r = L.r_rect[tid];
        if (r.x < rg.z && r.z > rg.x && r.y < rg.w && r.w > rg.y)
            mykey = ((unsigned long long)__float_as_uint(L.r_xyd[tid].z) << 32) | (unsigned)tid;
        L.key[tid] = mykey;
    }
    __syncthreads();
    int n = 0, rank = 0;
    for (int j = 0; j < P; j++) {
        const unsigned long long kj = L.key[j];
        n += kj != ~0ull ? 1 : 0;
        rank += kj < mykey ? 1 : 0;
    }
    if (mykey != ~0ull) {
        const float4 xyd = L.r_xyd[tid];
        const uint4 r = L.r_rect[tid];
        L.xy[rank] = make_float2(xyd.x, xyd.y);
        L.co[rank] = L.r_co[tid];
        L.invd[rank] = xyd.w;
        L.xr[rank] = (int)(r.x | (r.z << 16));
        L.yr[rank] = (int)(r.y | (r.w << 16));
        L.id[rank] = tid;
    }
    __syncthreads();
    // channel compaction: a channel whose feature is zero for every listed Gaussian multiplies dL/dpixel by exact
    // zeros everywhere in backward.cu:581-594, so its (dense, far-apart) gradient plane is never read.
    // All channels stay active when the feature gradient or the background term needs every dL/dpixel.
    if (tid < CG) {
        bool act = false;
        if (tid < C) {
            act = DFEAT || a.bg != nullptr;
            for (int k = 0; k < n && !act; k++) act = L.r_feat[L.id[k] * C + tid] != 0.0f;
        }
        s_act[tid] = act ? 1 : 0;
    }
    __syncthreads();
    if (tid < CG && s_act[tid]) {
        int pos = 0;
        for (int c = 0; c < tid; c++) pos += s_act[c];
        s_chan[pos] = tid;  // ascending channel order: summation order over channels is fixed
    }
    int nc = 0;
    for (int c = 0; c < CG; c++) nc += s_act[c];
    __syncthreads();
    if (tid < n) {
        const int id = L.id[tid];
#pragma unroll
        for (int j = 0; j < CG; j++) L.feat[tid * CG + j] = j < nc ? L.r_feat[id * C + s_chan[j]] : 0.0f;
    }
    __syncthreads();
    int kg = 0;
    for (int k = 0; k < n; k++) kg = L.id[k] == g ? k : kg;
    const bool do_clamp = a.flags & SKS_CLAMP01;
    const float ddelx_dx = (float)(0.5 * W), ddely_dy = (float)(0.5 * H);  // backward.cu:527-528
    float sum[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) sum[j] = 0.0f;

    for (int c = sp; c < nchunks; c += BWD_SPLITS) {
        const int i = c * 256 + tid;
        if (i >= npx) continue;
        const int yy = i / wpx;
        const int x = x0 + (i - yy * wpx), y = y0 + yy;
        const int tx = x >> 4, ty = y >> 4;
        const float pxf = (float)x, pyf = (float)y;
        // re-composite front to back (forward.cu:346-386): T_final, last accepted entry, colours if clamping
        float T = 1.0f, col[CG];
#pragma unroll
        for (int ch = 0; ch < CG; ch++) col[ch] = 0.0f;
        int klast = -1;
        for (int k = 0; k < n; k++) {
            // (unsigned halves: a rect's upper tile row reaches 65535, bit 31 of the packed word)
            const unsigned xr = (unsigned)L.xr[k], yr = (unsigned)L.yr[k];
            if ((unsigned)tx < (xr & 0xffffu) || (unsigned)tx >= (xr >> 16) || (unsigned)ty < (yr & 0xffffu) || (unsigned)ty >= (yr >> 16)) continue;
            const float2 xy = L.xy[k];
            const float4 co = L.co[k];
            const float dx = xy.x - pxf, dy = xy.y - pyf;
            const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
            if (power > 0.0f) continue;
            const float alpha = fminf(0.99f, co.w * expf_fixed(power));
            if (alpha < 1.0f / 255.0f) continue;
            const float test_T = T * (1 - alpha);
            if (test_T < 0.0001f) break;
            if (do_clamp) {
#pragma unroll
                for (int ch = 0; ch < CG; ch++) col[ch] += L.feat[k * CG + ch] * alpha * T;
            }
            T = test_T;
            klast = k;
        }
        if (klast < kg) continue;  // g is behind the last contributor (or nothing contributes) at this pixel
        // upstream gradient of this pixel: only now, only the active channels (most rect pixels never get here)
        const size_t pix = (size_t)y * W + x;
        float dLraw[CG];
        {
            const float* dLc = a.dL_color + (size_t)v * C * HW + pix;
#pragma unroll
            for (int j = 0; j < CG; j++) dLraw[j] = j < nc ? dLc[(size_t)s_chan[j] * HW] : 0.0f;
        }
        const float dLi_raw = a.dL_invdepth ? a.dL_invdepth[(size_t)v * HW + pix] : 0.0f;
        BwdPix<CG> s;
        s.T = T;
        s.T_final = T;
        s.last_alpha = 0;
        s.accum_inv = 0;
        s.last_inv = 0;
        s.bgdot = 0;
        s.dLi = dLi_raw;
#pragma unroll
        for (int j = 0; j < CG; j++) {
            float d = dLraw[j];
            // torch.clamp backward passes the gradient where min <= x <= max
            if (do_clamp && !(col[j] >= 0.0f && col[j] <= 1.0f)) d = 0.0f;
            if (a.bg && j < nc) s.bgdot += a.bg[s_chan[j]] * d;
            s.dL[j] = d;
            s.accum_rec[j] = 0;
            s.last_color[j] = 0;
        }
        // back to front down to g (backward.cu:552-636); only g's own terms are kept
        for (int k = klast; k >= kg; k--) {
            // (unsigned halves: a rect's upper tile row reaches 65535, bit 31 of the packed word)
            const unsigned xr = (unsigned)L.xr[k], yr = (unsigned)L.yr[k];
            if ((unsigned)tx < (xr & 0xffffu) || (unsigned)tx >= (xr >> 16) || (unsigned)ty < (yr & 0xffffu) || (unsigned)ty >= (yr >> 16)) continue;
            const float2 xy = L.xy[k];
            const float4 co = L.co[k];
            const float dx = xy.x - pxf, dy = xy.y - pyf;
            const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
            if (power > 0.0f) continue;
            const float G = expf_fixed(power);
            const float alpha = fminf(0.99f, co.w * G);
            if (alpha < 1.0f / 255.0f) continue;
            s.T = s.T / (1.f - alpha);
            const float dchannel_dcolor = alpha * s.T;
            float dL_dalpha = 0.0f;
            const bool mine = k == kg;
#pragma unroll
            for (int ch = 0; ch < CG; ch++) {
                const float cc = L.feat[k * CG + ch];
                s.accum_rec[ch] = s.last_alpha * s.last_color[ch] + (1.f - s.last_alpha) * s.accum_rec[ch];
                s.last_color[ch] = cc;
                const float dL_dchannel = s.dL[ch];
                dL_dalpha += (cc - s.accum_rec[ch]) * dL_dchannel;
                if (DFEAT && mine) sum[NACC + ch] += dchannel_dcolor * dL_dchannel;
            }
            const float invd = L.invd[k];
            s.accum_inv = s.last_alpha * s.last_inv + (1.f - s.last_alpha) * s.accum_inv;
            s.last_inv = invd;
            dL_dalpha += (invd - s.accum_inv) * s.dLi;
            dL_dalpha *= s.T;
            s.last_alpha = alpha;
            dL_dalpha += (-s.T_final / (1.f - alpha)) * s.bgdot;
            if (mine) {
                const float dL_dG = co.w * dL_dalpha;
                const float gdx = G * dx, gdy = G * dy;
                const float dG_ddelx = -gdx * co.x - gdy * co.y;
                const float dG_ddely = -gdy * co.z - gdx * co.y;
                sum[0] += dL_dG * dG_ddelx * ddelx_dx;
                sum[1] += dL_dG * dG_ddely * ddely_dy;
                sum[2] += -0.5f * gdx * dx * dL_dG;
                sum[3] += -0.5f * gdx * dy * dL_dG;
                sum[4] += -0.5f * gdy * dy * dL_dG;
                sum[5] += G * dL_dalpha;
                sum[6] += dchannel_dcolor * s.dLi;
            }
        }
    }
    // workgroup reduction in a fixed order
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const float r = wave_sum(sum[j]);
        if (lane == 0) s_red[wv][j] = r;
    }
    __syncthreads();
    if (tid < NVS)
        out[tid * BWD_SPLITS] = tid < NV ? ((s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid])) : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------
// small path backward for P <= 64, wave-resident: same gather-by-Gaussian scheme as k_render_bwd_gather, but the
// whole working set lives in registers.  Lane i of every wavefront holds Gaussian i's record; the local list
// (Gaussians whose rect meets g's, ordered by (depth bits, index)) is a ballot mask + a per-lane rank, and the entry
// being composited is broadcast with v_readlane (wave-uniform values in SGPRs): no LDS and no barrier until the final
// cross-wave reduction, which removes the latency chain that dominates a 17-Gaussian backward.
// Unlike the LDS variant (256 consecutive pixels of the rect's rows per workgroup) a workgroup here takes one 16x16 tile
// of the rect, which makes "does this entry cover my pixels" a workgroup-uniform question.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rl(float x, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane)); }
__device__ __forceinline__ unsigned rlu(unsigned x, int lane) { return (unsigned)__builtin_amdgcn_readlane((int)x, lane); }

// LOSS = true fuses the loop's masked-L2 loss (utils/loss_utils.py:86-100 on the clamped render, train.py:150) into
// this kernel: a.dL_color holds the pseudo-GT heat-maps; dL/d(render) = 2 (r - gt) on the mask {gt > 0 or r > 0} is
// formed per pixel from the re-composited colours, so neither the rendered image nor a dense gradient ever exists.
// The loss sums over the WHOLE image are (per-view totals of the constant heat-maps: sum gt^2 and count over gt > 0,
// i.e. the loss of an all-zero render) + (corrections where the render is positive), the latter accumulated here by
// each tile's owner (lowest-index covering Gaussian) into slots 7 (S) and 8 (N).
// Image sizes and plane offsets are per view (ViewTan::w/h, ViewOff): with the fused loss nothing dense is written, so one
// launch carries a group of views with different sensors.
// HMF (with LOSS): the heat-maps are given by their separable factors (BwdArgs::hm_*) instead of planes.
// ES (with LOSS): per-frame early stopping -- a workgroup whose frame has stopped leaves before anything else (the step tail
// reads none of what it would write), so a stopped frame costs the launch nothing but that one load.
// PF (empty, or one PreFill by value -- plain variants only): the prefill role of sks_backward_prefill.  The grid then has extra
// blockIdx.z layers behind the role's own pf.zs, last in dispatch order; their blocks leave here, before any load or barrier.
// With the pack empty the kernel's signature and body are what they were without the role.
template <int CG, bool DFEAT, bool LOSS, bool HMF = false, bool ES = false, class... PF>
__global__ __launch_bounds__(256, (DFEAT || CG > 20) ? 1 : 4) void k_render_bwd_wave(BwdArgs a, ViewTan vt, ViewOff vo, PF... pf)
{
    static_assert(sizeof...(PF) <= 1 && (!LOSS || sizeof...(PF) == 0), "the prefill role belongs to the plain variants");
    if constexpr (sizeof...(PF) == 1) {
        const PreFill& f = (pf, ...);
        if ((int)blockIdx.z >= f.zs) {   // (workgroup-uniform)
            prefill_block(f, ((unsigned)((int)blockIdx.z - f.zs) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
            return;
        }
    }
    static_assert(!(DFEAT && LOSS), "the fused-loss variant has no feature gradient");
    static_assert(LOSS || !HMF, "heat-map factors belong to the fused-loss variant");
    static_assert(LOSS || !ES, "early stopping belongs to the fused-loss variant");
    if constexpr (ES) {
        if (a.es_stop[(size_t)((int)blockIdx.y / a.es_views) * a.es_stride] != 0) return;   // (workgroup-uniform)
    }
    constexpr int NV = LOSS ? NACC + 1 : NACC + (DFEAT ? CG : 0);
    __shared__ float s_red[2][4][NV];
    // gridDim.z workgroups share the BWD_SPLITS partial-sum slots of a (view, Gaussian): workgroup sp owns slots sp,
    // sp + gridDim.z, ...; slot s sums the tiles s, s + BWD_SPLITS, ... of the rect.  16 workgroups (one slot each) is the
    // shortest chain for a handful of views; with hundreds of (view, Gaussian) pairs in flight fewer, longer workgroups
    // share the header below and leave fewer empty ones.  The sums do not depend on the choice.
    int zs_ = gridDim.z;
    if constexpr (sizeof...(PF) == 1) zs_ = (pf, ...).zs;
    const int g = blockIdx.x, v = blockIdx.y, sp = blockIdx.z, zs = zs_, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int P = a.P, C = a.C, W = vt.w[v], H = vt.h[v];
    const int NVS = NACC + C;
    const size_t HW = (size_t)H * W;
    const size_t go = (size_t)v * P;
    const float* dL_view = a.dL_color + vo.off[v];   // this view's C planes (dL/d(render), or the heat-maps with LOSS)
    float* out_g = a.accum + ((size_t)v * P + g) * NVS * BWD_SPLITS;
    // lane i <- Gaussian i (one global round trip, every load independent)
    const bool has = lane < P;
    const int li = has ? lane : 0;
    const float4 m_co = a.g.co[go + li];
    const float4 m_xyd = a.g.xyd[go + li];
    uint4 m_rect = a.g.rect[go + li];
    if (!has) m_rect = make_uint4(0, 0, 0, 0);
    float m_feat[CG];
    unsigned m_fmask = 0;   // this lane's Gaussian: channels with a non-zero feature (one bit on the skeleton scenes)
#pragma unroll
    for (int ch = 0; ch < CG; ch++) {
        m_feat[ch] = (ch < C && has) ? a.features[li * C + ch] : 0.0f;
        m_fmask |= m_feat[ch] != 0.0f ? (1u << ch) : 0u;
    }

    const unsigned gx0 = rlu(m_rect.x, g), gy0 = rlu(m_rect.y, g), gx1 = rlu(m_rect.z, g), gy1 = rlu(m_rect.w, g);
    // a piece of work = one 16x16 tile of g's rect (256 pixels = this workgroup): the tile is the same for every lane, so
    // whether a list entry can matter is decided once per entry for the whole workgroup -- of the ~9 Gaussians whose
    // rects meet g's rect only the 2-4 covering this tile are walked
    const int wt = (int)gx1 - (int)gx0, ht = (int)gy1 - (int)gy0;
    const int nchunks = wt * ht;  // 0 when culled (rect all zero)
    if (sp >= nchunks) {  // nothing for this workgroup's slots (also every slot of an invisible Gaussian)
        for (int slot = sp; slot < BWD_SPLITS; slot += zs)
            if (tid < NVS) out_g[tid * BWD_SPLITS + slot] = 0.0f;
        return;
    }
    // local list = lanes whose rect intersects g's; order = rank of (depth bits, index) among them
    const bool hit = m_rect.x < gx1 && m_rect.z > gx0 && m_rect.y < gy1 && m_rect.w > gy0;
    const unsigned long long hm = __ballot(hit);
    const int n = __popcll(hm);
    const unsigned mydepth = __float_as_uint(m_xyd.z);
    int rank = 0;
    for (unsigned long long m = hm; m; m &= m - 1) {
        const int j = __builtin_ctzll(m);
        const unsigned dj = rlu(mydepth, j);
        rank += (dj < mydepth || (dj == mydepth && j < lane)) ? 1 : 0;
    }
    const int kg = __builtin_amdgcn_readlane(rank, g);
    // channels that can matter (see k_render_bwd_gather): a bit mask, uniform across the wavefront
    unsigned chmask = 0;
    if (DFEAT || a.bg != nullptr) {
        chmask = C >= 32 ? 0xffffffffu : ((1u << C) - 1u);
    } else {
        for (unsigned long long m = hm; m; m &= m - 1) chmask |= rlu(m_fmask, __builtin_ctzll(m));
    }
    const bool do_clamp = a.flags & SKS_CLAMP01;
    const float ddelx_dx = (float)(0.5 * W), ddely_dy = (float)(0.5 * H);  // backward.cu:527-528
    const unsigned chmask_all = chmask;
    const size_t HW_all = HW;
    int buf = 0;
    for (int slot = sp; slot < BWD_SPLITS; slot += zs, buf ^= 1) {
    float* out = out_g + slot;
    if (slot >= nchunks) {   // (workgroup-uniform)
        if (tid < NVS) out[tid * BWD_SPLITS] = 0.0f;
        continue;
    }
    float sum[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) sum[j] = 0.0f;
    for (int c = slot; c < nchunks; c += BWD_SPLITS) {
        // This loop runs once for all but very large rects, but the compiler hoists every per-channel invariant (20 exec
        // masks, 20 plane offsets) in front of it and spills scalar registers into vector lanes to keep them: opaque
        // copies of the two values they derive from keep those computations where they are used.
        unsigned chmask = chmask_all;
        size_t HW = HW_all;
        asm volatile("" : "+s"(chmask), "+s"(HW));
        const int tyl = c / wt;
        const int tx = (int)gx0 + (c - tyl * wt), ty = (int)gy0 + tyl;   // wave-uniform
        const int x = tx * TILE + (tid & 15), y = ty * TILE + (tid >> 4);
        const bool in = x < W && y < H;
        const float pxf = (float)x, pyf = (float)y;
        // re-composite front to back (forward.cu:346-386): T_final, last accepted entry, colours if clamping.
        // The k loop is wave-uniform (entries are broadcast); per-lane state is predicated.
        float T = 1.0f, col[CG];
#pragma unroll
        for (int ch = 0; ch < CG; ch++) col[ch] = 0.0f;
        int klast = -1;
        // the list holds every Gaussian whose rect meets g's RECT; most miss this tile: each lane tests its own rect once,
        // and an entry that does not cover the tile costs one compare per walk instead of a dozen broadcasts
        const bool hitc = hit && !((unsigned)tx < m_rect.x || (unsigned)tx >= m_rect.z || (unsigned)ty < m_rect.y || (unsigned)ty >= m_rect.w);
        const unsigned long long covm = __ballot(hitc);
        // lowest Gaussian index whose rect covers this pixel's tile (the tile's owner); lane i is Gaussian i
        const int minid = covm ? __builtin_ctzll(covm) : 0x7fffffff;
        bool alive = in;
        // channels that can matter on THIS tile: those of the entries covering it (with a background or the feature
        // gradient every channel does).  Nothing else is read below: two to four heat-map planes instead of the ~9 of
        // the whole rect's list.
        unsigned chm_t = (DFEAT || a.bg != nullptr) ? chmask : 0u;
        for (int k = 0; k < n; k++) {
            const unsigned long long sel = __ballot(hitc && rank == k);
            if (!sel) continue;      // uniform: entry k does not cover this tile
            if (!LOSS && !__any(alive)) break;
            const int lk = __builtin_ctzll(sel);
            chm_t |= chmask & rlu(m_fmask, lk);
            const float ex = rl(m_xyd.x, lk), ey = rl(m_xyd.y, lk);
            const float cx = rl(m_co.x, lk), cy = rl(m_co.y, lk), cz = rl(m_co.z, lk), cw = rl(m_co.w, lk);
            const bool cov = alive;
            const float dx = ex - pxf, dy = ey - pyf;
            const float power = -0.5f * (cx * dx * dx + cz * dy * dy) - cy * dx * dy;
            const float alpha = fminf(0.99f, cw * expf_fixed(power));
            const float test_T = T * (1 - alpha);
            const bool pass = cov && !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
            const bool stop = pass && test_T < 0.0001f;
            const bool acc = pass && !stop;
            if (do_clamp || LOSS) {
                // a zero feature adds nothing to its channel: walk the entry's own channels (one on the skeleton scenes;
                // a wave-uniform register index instead of a branch per channel, 19 of 20 of them taken)
                // (the sum is formed for every lane and selected as a VALUE: a predicated write into a register picked by a
                // wave-uniform index is compiled as a copy of the whole array; + 0.0f leaves a non-negative sum as it is)
                for (unsigned fm = chmask & rlu(m_fmask, lk); fm; fm &= fm - 1) {
                    const int ch = __builtin_ctz(fm);
                    const float f = rl(m_feat[ch], lk);
                    const float add = f * alpha * T;
                    col[ch] += acc ? add : 0.0f;
                }
            }
            if (acc) { T = test_T; klast = k; }
            if (stop) alive = false;
        }
        const bool need = in && klast >= kg;  // g is at or in front of the last contributor at this pixel
        // LOSS: the pixel's loss terms are accounted by the tile's owner, and only where the render is positive:
        // everywhere else the masked-L2 sees render = 0, which the per-view heat-map totals already contain
        // (channel loops walk the set bits of chmask -- a handful of the C channels -- with a wave-uniform register index)
        bool own = false;
        if (LOSS && in && minid == g) {
            for (unsigned fm = chm_t; fm; fm &= fm - 1) own = own || col[__builtin_ctz(fm)] > 0.0f;
        }
        if (!__any(need || own)) continue;
        // upstream gradient of this pixel: only the active channels, only the lanes that need it
        const size_t pix = (size_t)y * W + x;
        struct { float T, T_final, last_alpha, accum_inv, last_inv, bgdot, dLi; } s;   // scalars only: the per-channel
                                                                                       // values must stay in registers
        s.T = T; s.T_final = T; s.last_alpha = 0; s.accum_inv = 0; s.last_inv = 0; s.bgdot = 0;
        s.dLi = (!LOSS && need && a.dL_invdepth) ? a.dL_invdepth[(size_t)v * HW + pix] : 0.0f;
        // each channel's colour is replaced by its dL in place: the colour is dead once dL is formed, and the channels
        // outside chm_t were never accumulated (zero) and are never read again.  Four channels at a time, their loads
        // issued together: one memory round trip per tile instead of one per channel.
        {
            const float* dLc = dL_view + pix;
            for (unsigned fm = chm_t; fm;) {
                int cc[4];
                float cv[4], gv[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    cc[i] = fm ? __builtin_ctz(fm) : -1;   // (wave-uniform)
                    fm &= fm - 1;
                }
#pragma unroll
                for (int i = 0; i < 4; i++) cv[i] = col[max(cc[i], 0)];
                if (HMF) {
                    // the pseudo-GT from its factors: the expression k_heatmaps would have stored, bit for bit
                    float fr[4], fc[4], lo[4], dn[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int vc = v * C + max(cc[i], 0);   // (wave-uniform: lo, dn through the scalar cache)
                        const bool want = cc[i] >= 0 && (need || (own && cv[i] > 0.0f));
                        fr[i] = want ? a.hm_row[(size_t)vc * a.H + y] : 0.0f;
                        fc[i] = want ? a.hm_col[(size_t)vc * a.W + x] : 0.0f;
                        lo[i] = a.hm_cmin[vc];
                        dn[i] = a.hm_den[vc];
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const bool want = cc[i] >= 0 && (need || (own && cv[i] > 0.0f));
                        gv[i] = want ? (fr[i] * fc[i] - lo[i]) / dn[i] : 0.0f;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const bool want = LOSS ? (need || (own && cv[i] > 0.0f)) : need;
                        gv[i] = (cc[i] >= 0 && want) ? dLc[(size_t)max(cc[i], 0) * HW] : 0.0f;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (cc[i] < 0) break;
                    const int ch = cc[i];
                    const float gtv = gv[i];
                    float d = 0.0f;
                    if (LOSS) {
                        const bool rpos = cv[i] > 0.0f;            // clamp01(col) > 0
                        const float r = clamp01(cv[i]);            // gaussian_renderer/__init__.py:129
                        const bool msk = gtv > 0.0f || r > 0.0f;   // loss_utils.py:88-91
                        const float e = r - gtv;
                        // correction to the heat-map-only totals: (r - gt)^2 replaces gt^2 [gt > 0], 1 replaces [gt > 0]
                        if (own && rpos) { sum[7] += e * e - (gtv > 0.0f ? gtv * gtv : 0.0f); sum[8] += gtv > 0.0f ? 0.0f : 1.0f; }
                        d = msk ? 2.0f * e : 0.0f;
                        if (!(cv[i] >= 0.0f && cv[i] <= 1.0f)) d = 0.0f;   // clamp backward
                        if (!need) d = 0.0f;
                    } else {
                        d = gtv;   // (zero unless `need`)
                        // torch.clamp backward passes the gradient where min <= x <= max
                        if (do_clamp && !(cv[i] >= 0.0f && cv[i] <= 1.0f)) d = 0.0f;
                    }
                    if (a.bg) s.bgdot += a.bg[ch] * d;
                    col[ch] = d;
                }
            }
        }
        // sum over channels of accum_rec[ch] dL[ch] and of last_color[ch] dL[ch] (backward.cu:590-600): the channel
        // recursion is linear, so the two dot products with this pixel's dL are carried instead of the 2 C colours,
        // and an entry only touches the channels where its own feature is not zero
        float rec_dot = 0.0f, last_dot = 0.0f;
        if (!__any(need)) continue;
        // back to front down to g (backward.cu:552-636); only g's own terms are kept
        for (int k = n - 1; k >= kg; k--) {
            const unsigned long long sel = __ballot(hitc && rank == k);
            if (!sel) continue;   // uniform (as in the walk above)
            const int lk = __builtin_ctzll(sel);
            const bool cand = need && k <= klast;
            if (!__any(cand)) continue;
            const float ex = rl(m_xyd.x, lk), ey = rl(m_xyd.y, lk), einvd = rl(m_xyd.w, lk);
            const float cx = rl(m_co.x, lk), cy = rl(m_co.y, lk), cz = rl(m_co.z, lk), cw = rl(m_co.w, lk);
            const float dx = ex - pxf, dy = ey - pyf;
            const float power = -0.5f * (cx * dx * dx + cz * dy * dy) - cy * dx * dy;
            const float G = expf_fixed(power);
            const float alpha = fminf(0.99f, cw * G);
            const bool act = cand && !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
            if (!__any(act)) continue;
            const bool mine = k == kg;
            float Tn = s.T, dchannel_dcolor = 0.0f, dL_dalpha = 0.0f;
            if (act) {
                Tn = s.T / (1.f - alpha);
                dchannel_dcolor = alpha * Tn;
            }
            float cdot = 0.0f;   // this entry's colour . dL
            for (unsigned fm = chmask & rlu(m_fmask, lk); fm; fm &= fm - 1) {
                const int ch = __builtin_ctz(fm);
                cdot += rl(m_feat[ch], lk) * col[ch];
            }
            if (DFEAT && mine) {
#pragma unroll
                for (int ch = 0; ch < CG; ch++) {
                    if ((chmask & (1u << ch)) && act) sum[NACC + ch] += dchannel_dcolor * col[ch];
                }
            }
            if (act) {
                rec_dot = s.last_alpha * last_dot + (1.f - s.last_alpha) * rec_dot;
                last_dot = cdot;
                dL_dalpha += cdot - rec_dot;
                s.T = Tn;
                s.accum_inv = s.last_alpha * s.last_inv + (1.f - s.last_alpha) * s.accum_inv;
                s.last_inv = einvd;
                dL_dalpha += (einvd - s.accum_inv) * s.dLi;
                dL_dalpha *= s.T;
                s.last_alpha = alpha;
                dL_dalpha += (-s.T_final / (1.f - alpha)) * s.bgdot;
                if (mine) {
                    const float dL_dG = cw * dL_dalpha;
                    const float gdx = G * dx, gdy = G * dy;
                    const float dG_ddelx = -gdx * cx - gdy * cy;
                    const float dG_ddely = -gdy * cz - gdx * cy;
                    sum[0] += dL_dG * dG_ddelx * ddelx_dx;
                    sum[1] += dL_dG * dG_ddely * ddely_dy;
                    sum[2] += -0.5f * gdx * dx * dL_dG;
                    sum[3] += -0.5f * gdx * dy * dL_dG;
                    sum[4] += -0.5f * gdy * dy * dL_dG;
                    sum[5] += G * dL_dalpha;
                    sum[6] += dchannel_dcolor * s.dLi;
                }
            }
        }
    }
    // workgroup reduction in a fixed order (two LDS buffers: one barrier per slot is enough); eight values per butterfly
    // (wave_sum8: ~25 VALU ops for eight totals instead of ~12 each), what is left over one by one
    static_assert(NV >= 8, "the first eight values go through wave_sum8");
#pragma unroll
    for (int j0 = 0; j0 + 8 <= NV; j0 += 8) {
        float grp[8];
#pragma unroll
        for (int j = 0; j < 8; j++) grp[j] = sum[j0 + j];
        const float r = wave_sum8(grp);
        if (lane < 8) s_red[buf][wv][j0 + lane] = r;
    }
#pragma unroll
    for (int j = NV & ~7; j < NV; j++) {
        const float r = wave_sum(sum[j]);
        if (lane == 0) s_red[buf][wv][j] = r;
    }
    __syncthreads();
    if (tid < NVS)
        out[tid * BWD_SPLITS] = tid < NV ? ((s_red[buf][0][tid] + s_red[buf][1][tid]) + (s_red[buf][2][tid] + s_red[buf][3][tid])) : 0.0f;
    }
}

// per (view, tile, channel) statistics of the constant pseudo-GT heat-maps, once per scene: sum of gt^2 over gt > 0 and count
// of gt > 0 (what the masked-L2 loss sees wherever the render is zero: its mask leaves a pixel with gt <= 0 out, so a negative
// entry of planes that are not normalised to [0, 1] adds nothing, as in k_masked_l2 and in k_render_bwd_wave's correction),
// and their per-view totals.  For planes without negative entries the sums are the plain sums of squares, bit for bit.
// Streaming layout: block (band, channel, view); a thread owns one 4-pixel column of a tile and walks the tile's 16
// rows (16 independent 16-byte loads; a wavefront reads 1 KB contiguous per row), the four threads of a tile are
// combined with DPP quad permutes in a fixed order -- one pass over the heat-maps at streaming rate, reproducible sums.
__device__ __forceinline__ float pos_sq(float g) { return g > 0.0f ? g * g : 0.0f; }

__global__ __launch_bounds__(256) void k_gt_tile_stats(int C, int W, int H, const float* __restrict__ gt, float* __restrict__ tile_S,
                                                        float* __restrict__ tile_N, double* __restrict__ totals)
{
    __shared__ double s_t[2][4];
    const int band = blockIdx.x, ch = blockIdx.y, v = blockIdx.z, tid = threadIdx.x;
    const int gx = (W + TILE - 1) / TILE, gy = gridDim.x;
    const size_t HW = (size_t)H * W;
    const float* plane = gt + ((size_t)v * C + ch) * HW;
    const int y0 = band * TILE, rows = min(TILE, H - y0);
    const bool vec = (W & 3) == 0;
    double tS = 0.0, tN = 0.0;
    for (int t0 = 0; t0 < gx; t0 += 64) {
        const int tx = t0 + (tid >> 2), x = tx * TILE + (tid & 3) * 4;
        float S = 0.0f, N = 0.0f;
        if (tx < gx && x < W) {
            if (vec) {
                float4 g[TILE];
#pragma unroll
                for (int r = 0; r < TILE; r++)   // all loads first: 16 independent requests in flight per lane
                    g[r] = r < rows ? *reinterpret_cast<const float4*>(plane + (size_t)(y0 + r) * W + x) : make_float4(0, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < TILE; r++) {
                    S += (pos_sq(g[r].x) + pos_sq(g[r].y)) + (pos_sq(g[r].z) + pos_sq(g[r].w));
                    N += ((g[r].x > 0.0f ? 1.0f : 0.0f) + (g[r].y > 0.0f ? 1.0f : 0.0f)) +
                         ((g[r].z > 0.0f ? 1.0f : 0.0f) + (g[r].w > 0.0f ? 1.0f : 0.0f));
                }
            } else {
                for (int r = 0; r < rows; r++)
                    for (int k = 0; k < 4; k++)
                        if (x + k < W) {
                            const float g = plane[(size_t)(y0 + r) * W + x + k];
                            S += pos_sq(g);
                            N += g > 0.0f ? 1.0f : 0.0f;
                        }
            }
        }
        // the four 4-pixel columns of the tile
        S += dpp_move<0xB1>(S); N += dpp_move<0xB1>(N);
        S += dpp_move<0x4E>(S); N += dpp_move<0x4E>(N);
        if ((tid & 3) == 0 && tx < gx) {
            const size_t tb = (((size_t)v * gy + band) * gx + tx) * C + ch;
            if (tile_S) tile_S[tb] = S;
            if (tile_N) tile_N[tb] = N;
            tS += (double)S;
            tN += (double)N;
        }
    }
    tS = wave_sum_d(tS);
    tN = wave_sum_d(tN);
    if ((tid & 63) == 0) { s_t[0][tid >> 6] = tS; s_t[1][tid >> 6] = tN; }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&totals[2 * v], (s_t[0][0] + s_t[0][1]) + (s_t[0][2] + s_t[0][3]));
        atomicAdd(&totals[2 * v + 1], (s_t[1][0] + s_t[1][1]) + (s_t[1][2] + s_t[1][3]));
    }
}
