// sks_geom_fwd.inc -- part of the sks_raster.hip translation unit (included inside its anonymous namespace, in order):
// geometry forward (preprocessCUDA) and mark_visible.
// ------------------------------------------------------------------------------------------------------------
// geometry forward: preprocessCUDA, DGR/cuda_rasterizer/forward.cu:153-273 (+ in_frustum auxiliary.h:151-176)
// ------------------------------------------------------------------------------------------------------------
// one (view, Gaussian) pair; returns the tile rect (all zero when culled or !live)
template <class VT>
__device__ __forceinline__ uint4 geom_fwd_one(int P, const VT& vt, const float* __restrict__ vms,
                                              const float* __restrict__ pms, const float* __restrict__ means,
                                              const float* __restrict__ opac, const float* __restrict__ scales,
                                              const float* __restrict__ rots, const float* __restrict__ cov3Dp,
                                              float smod, unsigned flags, const Geom& g, int* __restrict__ radii,
                                              int v, int idx, bool live, bool store = true)
{
    const size_t o = (size_t)v * P + (live ? idx : 0);
    const float* V = vms + 16 * v;
    const float* PM = pms + 16 * v;
    const float tan_fovx = vt.x[v], tan_fovy = vt.y[v];
    const int W = vt.w[v], H = vt.h[v];
    const float focal_y = H / (2.0f * tan_fovy);  // rasterizer_impl.cu:224-225
    const float focal_x = W / (2.0f * tan_fovx);
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;

    int radius_out = 0;
    uint4 rect = make_uint4(0, 0, 0, 0);
    float4 co = make_float4(0, 0, 0, 0), xyd = make_float4(0, 0, 1.0f, 1.0f);

    const int li = live ? idx : 0;
    const float p_orig[3] = { means[3 * li], means[3 * li + 1], means[3 * li + 2] };
    float p_view[3];
    transformPoint4x3(p_orig, V, p_view);
    // The near-plane cull, written so that NOT being in front of the plane is what rejects: a mean with a NaN coordinate has a
    // NaN view depth, for which `z > 0.2f` is false, so an unobserved joint (DESIGN.md "Unobserved joints") is culled like a
    // Gaussian behind the camera and leaves the same record -- radius 0, rect 0.  (The reference rejects `z <= 0.2f`, which lets
    // a NaN through; for every other depth the two are the same test.)
    const bool culled = !(p_view[2] > 0.2f);
    if (live && !culled) {
        float p_hom[4];
        transformPoint4x4(p_orig, PM, p_hom);
        const float p_w = 1.0f / (p_hom[3] + 0.0000001f);
        const float p_proj[3] = { p_hom[0] * p_w, p_hom[1] * p_w, p_hom[2] * p_w };
        float cov3D[6];
        if (cov3Dp) {
#pragma unroll
            for (int i = 0; i < 6; i++) cov3D[i] = cov3Dp[6 * li + i];
        } else {
            const float s[3] = { scales[3 * li], scales[3 * li + 1], scales[3 * li + 2] };
            const float q[4] = { rots[4 * li], rots[4 * li + 1], rots[4 * li + 2], rots[4 * li + 3] };
            const Activated ac = activate(flags & SKS_RAW_PARAMS, 0.0f, s, q);
            computeCov3D(ac.s, smod, ac.q, cov3D);
        }
        Cov2D c;
        cov2d(p_orig, focal_x, focal_y, tan_fovx, tan_fovy, cov3D, V, c);
        float cov_x = c.cov.m[0][0], cov_y = c.cov.m[0][1], cov_z = c.cov.m[1][1];
        constexpr float h_var = 0.3f;
        const float det_cov = cov_x * cov_z - cov_y * cov_y;
        cov_x += h_var;
        cov_z += h_var;
        const float det_cov_plus_h_cov = cov_x * cov_z - cov_y * cov_y;
        float h_convolution_scaling = 1.0f;
        if (flags & SKS_ANTIALIASING) h_convolution_scaling = sqrtf(fmaxf(0.000025f, det_cov / det_cov_plus_h_cov));
        const float det = det_cov_plus_h_cov;
        if (det != 0.0f) {
            const float det_inv = 1.f / det;
            const float conic[3] = { cov_z * det_inv, -cov_y * det_inv, cov_x * det_inv };
            const float mid = 0.5f * (cov_x + cov_z);
            const float lambda1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
            const float lambda2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
            const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
            const float px = ndc2Pix(p_proj[0], W), py = ndc2Pix(p_proj[1], H);
            int xmin, ymin, xmax, ymax;
            getRect(px, py, (int)my_radius, gx, gy, xmin, ymin, xmax, ymax);
            if ((xmax - xmin) * (ymax - ymin) != 0) {
                radius_out = (int)my_radius;
                rect = make_uint4(xmin, ymin, xmax, ymax);
                const float op_raw = opac[li];
                const float op = (flags & SKS_RAW_PARAMS) ? 1.0f / (1.0f + expf_fixed(-op_raw)) : op_raw;
                co = make_float4(conic[0], conic[1], conic[2], op * h_convolution_scaling);
                xyd = make_float4(px, py, p_view[2], 1 / p_view[2]);
            }
        }
    }
    if (live && store) {
        radii[o] = radius_out;
        g.co[o] = co;
        g.xyd[o] = xyd;
        g.rect[o] = rect;
    }
    return rect;
}

#ifndef SKS_GEOM_COVER_THREADS
#define SKS_GEOM_COVER_THREADS 256    // (the small path: one block per (view, plane) with a cover row set per plane, else per view)
#endif
// the body of k_geom_fwd for block (bx, v, pz) -- shared with k_geom_fwd_fill (sks_fwd_small.inc), whose first blocks are
// these blocks of a small-path call; s_cov: LDS for one plane's (or view's) cover rows, gy * cover_cw(W) words (unused without g.cover)
__device__ __forceinline__ void geom_fwd_block(uint32_t* s_cov, int bx, int v, int pz, int P, int W, int H, const ViewTan& vt, const float* __restrict__ vms,
                                               const float* __restrict__ pms, const float* __restrict__ means,
                                               const float* __restrict__ opac, const float* __restrict__ scales,
                                               const float* __restrict__ rots, const float* __restrict__ cov3Dp,
                                               float smod, unsigned flags, const Geom& g, int* __restrict__ radii, int vf,
                                               uint32_t* __restrict__ count, uint32_t* __restrict__ touched,
                                               const float* __restrict__ features, int C,
                                               uint2* __restrict__ fmask, uint32_t* __restrict__ bin_hdr, int cover_planes)
{
    const int idx = bx * blockDim.x + threadIdx.x;   // (256 threads; SKS_GEOM_BINNED_THREADS on the binned path, which has no cover rows to build)
    const bool live = idx < P;
    // vf > 0: the views are vf per FRAME and every frame has its own P Gaussians (parameters stacked (F,P,..)): view v renders
    // frame v / vf.  Everything downstream is per (view, Gaussian) record and never sees the difference.
    if (vf > 0) {
        const int fr = v / vf;
        means += (size_t)fr * P * 3;
        opac += (size_t)fr * P;
        if (scales) scales += (size_t)fr * P * 3;
        if (rots) rots += (size_t)fr * P * 4;
        if (cov3Dp) cov3Dp += (size_t)fr * P * 6;
    }
    // gridDim.z > 1 (the small path with a cover row set per plane): block z builds plane z's rows only -- every block computes the
    // view's (<= 256) Gaussians, block 0 stores them.  One block per view doing all C + 1 planes one after the other (4 536 words to
    // clear, fill and write for H36M) took 5.9-6.4 us on the critical path of every step; side by side: the single plane's time.
    const uint4 rect = geom_fwd_one(P, vt, vms, pms, means, opac, scales, rots, cov3Dp, smod, flags, g, radii, v, idx, live, pz == 0);
    if (bin_hdr && bx == 0 && v == 0 && pz == 0 && threadIdx.x < 64) bin_hdr[threadIdx.x] = 0u;   // (Bin::hdr: the kernels behind add to it)
    if (count) {
        // binned path: the reference's tiles_touched (forward.cu:271); the per-tile entry counts are k_bin_band_count's (a workgroup
        // per tile band, LDS atomics: until round 5 they were one global atomic per tile of the rect here, 14 us on the stress scene)
        const int wt = (int)(rect.z - rect.x), n = wt * (int)(rect.w - rect.y);   // 0 when culled or !live
        if (live) touched[(size_t)v * P + idx] = (uint32_t)n;
        if (live && v == 0) {   // which channels of the Gaussian's feature row are not zero (the compositors walk only those)
            unsigned fm = 0u;
            float f0 = 0.0f;
            for (int ch = C - 1; ch >= 0; ch--) {
                const float f = features[(size_t)idx * C + ch];
                if (f != 0.0f) { fm |= 1u << ch; f0 = f; }
            }
            fmask[idx] = make_uint2(fm, __float_as_uint(f0));
        }
    }
    if (g.cover) {  // single block per (view [, plane]) (P <= 256): bitmap of covered tiles for the forward's fill blocks (uniform W x H) -- one, or
        // (cover_planes, when a view's C + 1 bitmaps fit: cover_per_plane) one per output PLANE: a Gaussian covers its rect on the
        // planes of its non-zero features and on the inverse-depth plane (C); the compositor stores exactly those planes of a
        // tile (the union over the Gaussians covering it), the fill role zeroes every other plane in whole rows -- with one-hot
        // skeleton features a plane's bands are almost all free of cover.
        const int gy = (H + TILE - 1) / TILE;
        const int cw = cover_cw(W), pw = gy * cw;
        for (int i = threadIdx.x; i < pw; i += blockDim.x) s_cov[i] = 0u;
        __syncthreads();
        bool mine = live && rect.z > rect.x && rect.w > rect.y;
        if (mine && cover_planes && pz < C) mine = features[(size_t)idx * C + pz] != 0.0f;     // (plane C, inverse depth: every Gaussian)
        if (mine) {
#pragma nounroll
            for (unsigned y = rect.y; y < rect.w; y++) {
                atomicOr(&s_cov[y * cw], 1u);
#pragma nounroll
                for (unsigned w0 = rect.x >> 5; w0 <= (rect.z - 1u) >> 5; w0++) {
                    const unsigned lo = max(rect.x, w0 << 5) & 31u, hi = min(rect.z - 1u, (w0 << 5) + 31u) & 31u;   // bits lo..hi
                    atomicOr(&s_cov[y * cw + 1 + w0], (0xffffffffu >> (31u - hi)) & (0xffffffffu << lo));
                }
            }
        }
        __syncthreads();
        uint32_t* out = g.cover + ((size_t)v * (cover_planes ? C + 1 : 1) + (cover_planes ? pz : 0)) * pw;
        for (int i = threadIdx.x; i < pw; i += blockDim.x) out[i] = s_cov[i];
    }
}

__global__ __launch_bounds__(SKS_GEOM_COVER_THREADS > 256 ? SKS_GEOM_COVER_THREADS : 256) void k_geom_fwd(int P, int W, int H, ViewTan vt, const float* __restrict__ vms,
                                                   const float* __restrict__ pms, const float* __restrict__ means,
                                                   const float* __restrict__ opac, const float* __restrict__ scales,
                                                   const float* __restrict__ rots, const float* __restrict__ cov3Dp,
                                                   float smod, unsigned flags, Geom g, int* __restrict__ radii, int vf,
                                                   uint32_t* __restrict__ count = nullptr, uint32_t* __restrict__ touched = nullptr,
                                                   const float* __restrict__ features = nullptr, int C = 0,
                                                   uint2* __restrict__ fmask = nullptr, uint32_t* __restrict__ bin_hdr = nullptr,
                                                   int cover_planes = 0)
{
    __shared__ uint32_t s_cov[COVER_MAX_WORDS];
    geom_fwd_block(s_cov, blockIdx.x, blockIdx.y, blockIdx.z, P, W, H, vt, vms, pms, means, opac, scales, rots, cov3Dp, smod, flags, g, radii, vf,
                   count, touched, features, C, fmask, bin_hdr, cover_planes);
}

// sks_geometry_dv: the geometry pass of the fused-loss path (no cover rows, no binning) with the per-view scalars read from the
// device table
__global__ __launch_bounds__(256) void k_geom_fwd_dv(int P, ViewTanDev vt, const float* __restrict__ vms, const float* __restrict__ pms,
                                                      const float* __restrict__ means, const float* __restrict__ opac,
                                                      const float* __restrict__ scales, const float* __restrict__ rots,
                                                      const float* __restrict__ cov3Dp, float smod, unsigned flags, Geom g,
                                                      int* __restrict__ radii, int vf)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int v = blockIdx.y;
    if (vf > 0) {   // (frames batched: as k_geom_fwd)
        const int fr = v / vf;
        means += (size_t)fr * P * 3;
        opac += (size_t)fr * P;
        if (scales) scales += (size_t)fr * P * 3;
        if (rots) rots += (size_t)fr * P * 4;
        if (cov3Dp) cov3Dp += (size_t)fr * P * 6;
    }
    geom_fwd_one(P, vt, vms, pms, means, opac, scales, rots, cov3Dp, smod, flags, g, radii, v, idx, idx < P);
}

__global__ void k_mark_visible(int P, const float* __restrict__ means, const float* __restrict__ V,
                               uint8_t* __restrict__ present)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    const float p[3] = { means[3 * idx], means[3 * idx + 1], means[3 * idx + 2] };
    float pv[3];
    transformPoint4x3(p, V, pv);
    const bool culled = !(pv[2] > 0.2f);   // (geom_fwd_one's cull: a NaN depth is not visible)
    present[idx] = !culled;
}
