// sks_geom_bwd.inc -- part of the sks_raster.hip translation unit (included inside its anonymous namespace, in order):
// geometry backward and the fused step tail of the sparse loop.
// ------------------------------------------------------------------------------------------------------------
// geometry backward: computeCov2DCUDA (backward.cu:147-326) + preprocessCUDA (:398-449) + computeCov3D
// (:330-393) fused; consumes and clears the accumulators.  SH backward (:443-444) intentionally not reproduced
// (SURVEY quirk Q5): dL_dfeatures is the true dL_dcolors of backward.cu:593.
// ------------------------------------------------------------------------------------------------------------
struct GeomBwdArgs {
    int P, C, W, H;
    unsigned flags;
    const float* vms;
    const float* pms;
    const float* means;
    const float* opac;
    const float* scales;
    const float* rots;
    const float* cov3Dp;
    float smod;
    const int* radii;
    const float* accum;
    int nsplit;
    const double* gt_totals;   // fused-loss mode: per-view {sum gt^2, count gt > 0} over the whole image, else nullptr
    double* loss_sums;         // fused-loss mode: out, per-view {S, N} of the masked-L2 loss
    float* packed;             // optional (V,P,11) raw-parameter gradients (scaled by 1/N_v when loss_sums is set)
    float* dmeans3D;
    float* dmeans2D;
    float* dopacity;
    float* dscales;
    float* drots;
    float* dcov3D;
    float* dfeat;
    // binned path (nsplit == 0, k_geom_bwd_binned): the compositing backward left BIN_ROWS rows of NACC sums per (Gaussian, tile of its rect) in `part`,
    // the rows of a Gaussian at consecutive slots from goff[view, Gaussian] (Bin); `accum` then only holds dL/dfeatures
    const uint4* rect = nullptr;
    const uint32_t* goff = nullptr;
    const float* part = nullptr;
    size_t cap = 0;
    const uint32_t* bin_hdr = nullptr;   // Bin::hdr of the forward: [0] != 0 = its arena overflowed (entries were dropped)
    int v0 = 0;                          // k_geom_bwd_binned: first view of the launch (one launch per view group: blockIdx.y + v0)
};

__device__ __forceinline__ float sq(float x) { return x * x; }

// part 1 of one (view, Gaussian) pair: the per-split partial sums -> g[0..7], dL/dfeatures, and this Gaussian's share of
// the fused loss sums (slots 7 / 8)
// dL/dfeatures of `n` consecutive (view, Gaussian) records from record o0 (small path: nsplit partial sums per value), spread
// over the workgroup: one (record, channel) per thread and trip, the 16 slots as four 16-byte loads in flight and added in slot
// order.  (Inside geom_bwd_load a Gaussian's thread walked its C x 16 slots alone, load after load: 27 us of a kernel that
// takes 5 without it -- every literal drop-in iteration pays it, because nn.Parameter(t.requires_grad_(False)) DOES require
// grad, scene/gaussian_model.py:186.)
__device__ __forceinline__ void geom_bwd_dfeat(const GeomBwdArgs& a, size_t o0, int n, int tid, int nthreads)
{
    const int ns = a.nsplit ? a.nsplit : 1, NVS = NACC + a.C;
    for (int e = tid; e < n * a.C; e += nthreads) {
        const int gi = e / a.C, ch = e - gi * a.C;
        const float* acc = a.accum + (o0 + gi) * ns * NVS + (size_t)(NACC + ch) * ns;
        float t = 0.0f;
        if (ns == BWD_SPLITS) {
            float4 q[4];
#pragma unroll
            for (int i = 0; i < 4; i++) q[i] = reinterpret_cast<const float4*>(acc)[i];
#pragma unroll
            for (int i = 0; i < 4; i++) { t += q[i].x; t += q[i].y; t += q[i].z; t += q[i].w; }
        } else {
            for (int sp = 0; sp < ns; sp++) t += acc[sp];
        }
        a.dfeat[(o0 + gi) * a.C + ch] = t;
    }
}

template <bool DFEAT_HERE = true>
__device__ __forceinline__ void geom_bwd_load(const GeomBwdArgs& a, int v, int idx, float (&g)[NACC], double& pS, double& pN)
{
    const size_t o = (size_t)v * a.P + (idx < a.P ? idx : 0);
    const int NVS = NACC + a.C;
    const float* acc = a.accum + o * (a.nsplit ? a.nsplit : 1) * NVS;  // layout (value, split)
    if (a.nsplit == BWD_SPLITS) {
        static_assert(BWD_SPLITS == 16, "4 x float4 per value");
        float4 q[NACC][4];
#pragma unroll
        for (int j = 0; j < NACC - 1; j++)   // all loads in flight before the first add
#pragma unroll
            for (int i = 0; i < 4; i++) q[j][i] = reinterpret_cast<const float4*>(acc + j * BWD_SPLITS)[i];
#pragma unroll
        for (int j = 0; j < NACC - 1; j++) {  // fixed order: reproducible
            float t = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) t += (q[j][i].x + q[j][i].y) + (q[j][i].z + q[j][i].w);
            g[j] = t;
        }
        g[NACC - 1] = 0.0f;
    } else {
#pragma unroll
        for (int j = 0; j < NACC; j++) {
            float t = 0.0f;
            for (int sp = 0; sp < a.nsplit; sp++) t += acc[j * a.nsplit + sp];
            g[j] = t;
        }
    }
    if (DFEAT_HERE && a.dfeat) {
        const int ns = a.nsplit ? a.nsplit : 1;
        for (int ch = 0; ch < a.C; ch++) {
            float t = 0.0f;
            for (int sp = 0; sp < ns; sp++) t += acc[(NACC + ch) * ns + sp];
            a.dfeat[o * a.C + ch] = t;
        }
    }
    pS = 0.0;
    pN = 0.0;
    if (a.loss_sums && idx < a.P) {
        for (int sp = 0; sp < a.nsplit; sp++) {
            pS += (double)acc[7 * a.nsplit + sp];
            pN += (double)acc[8 * a.nsplit + sp];
        }
    }
}

// geom_bwd_load in two halves (16 slots, no feature gradient): the loads alone, then the sums in geom_bwd_load's order
// (bit-identical), so that a caller can put independent work between the two while the 36 lines are on their way.
struct GeomBwdRaw {
    float4 q[NACC + 1][4];   // values 0..6: gradient sums; 7, 8: the loss corrections S, N
};
__device__ __forceinline__ void geom_bwd_issue16(const GeomBwdArgs& a, int v, int idx, GeomBwdRaw& r)
{
    const size_t o = (size_t)v * a.P + (idx < a.P ? idx : 0);
    const float* acc = a.accum + o * BWD_SPLITS * (NACC + a.C);
#pragma unroll
    for (int j = 0; j < NACC + 1; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) r.q[j][i] = reinterpret_cast<const float4*>(acc + j * BWD_SPLITS)[i];
}
__device__ __forceinline__ void geom_bwd_sum16(const GeomBwdArgs& a, int idx, const GeomBwdRaw& r, float (&g)[NACC], double& pS,
                                               double& pN)
{
#pragma unroll
    for (int j = 0; j < NACC - 1; j++) {
        float t = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; i++) t += (r.q[j][i].x + r.q[j][i].y) + (r.q[j][i].z + r.q[j][i].w);
        g[j] = t;
    }
    g[NACC - 1] = 0.0f;
    pS = 0.0;
    pN = 0.0;
    if (a.loss_sums && idx < a.P) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            pS += (double)r.q[7][i].x; pS += (double)r.q[7][i].y; pS += (double)r.q[7][i].z; pS += (double)r.q[7][i].w;
            pN += (double)r.q[8][i].x; pN += (double)r.q[8][i].y; pN += (double)r.q[8][i].z; pN += (double)r.q[8][i].w;
        }
    }
}

// the per-Gaussian inputs of part 2, fetched ahead of it by a caller that has a memory round trip to wait for anyway
struct GeomBwdIn {
    int radius;
    float mean[3], p[7], opac;   // p: cov3D_precomp[0..5], or scales[0..2] + rotations[0..3]
};
__device__ __forceinline__ void geom_bwd_fetch(const GeomBwdArgs& a, int v, int idx, GeomBwdIn& in)
{
    const size_t o = (size_t)v * a.P + idx;
    in.radius = a.radii[o];
    in.mean[0] = a.means[3 * idx]; in.mean[1] = a.means[3 * idx + 1]; in.mean[2] = a.means[3 * idx + 2];
    if (a.cov3Dp) {
#pragma unroll
        for (int i = 0; i < 6; i++) in.p[i] = a.cov3Dp[6 * idx + i];
        in.p[6] = 0.0f;
    } else {
        in.p[0] = a.scales[3 * idx]; in.p[1] = a.scales[3 * idx + 1]; in.p[2] = a.scales[3 * idx + 2];
        in.p[3] = a.rots[4 * idx]; in.p[4] = a.rots[4 * idx + 1]; in.p[5] = a.rots[4 * idx + 2]; in.p[6] = a.rots[4 * idx + 3];
    }
    in.opac = a.opac[idx];
}

// part 2: the reference's formulas; n_view = the view's mask count N_v (fused-loss mode, else unused)
template <bool PRE = false, class VT = ViewTan>
__device__ __forceinline__ void geom_bwd_finish(const GeomBwdArgs& a, const VT& vt, int v, int idx, const float (&g)[NACC],
                                                double n_view, const GeomBwdIn* pre = nullptr)
{
    const size_t o = (size_t)v * a.P + idx;
    float dmean[3] = { 0, 0, 0 }, dcov[6] = { 0, 0, 0, 0, 0, 0 }, dscale[3] = { 0, 0, 0 }, dq[4] = { 0, 0, 0, 0 };
    float sc[3] = { 0, 0, 0 }, q[4] = { 1, 0, 0, 0 }, qnorm = 1.0f;   // activated scale / rotation (raw mode: see activate())
    float dop = g[5];
    const float dm2x = g[0], dm2y = g[1];

    if ((PRE ? pre->radius : a.radii[o]) > 0) {
        const float* V = a.vms + 16 * v;
        const float* proj = a.pms + 16 * v;
        const float tan_fovx = vt.x[v], tan_fovy = vt.y[v];
        const float h_y = vt.h[v] / (2.0f * tan_fovy);
        const float h_x = vt.w[v] / (2.0f * tan_fovx);
        const float mean[3] = { PRE ? pre->mean[0] : a.means[3 * idx], PRE ? pre->mean[1] : a.means[3 * idx + 1], PRE ? pre->mean[2] : a.means[3 * idx + 2] };
        float cov3D[6];
        if (a.cov3Dp) {
#pragma unroll
            for (int i = 0; i < 6; i++) cov3D[i] = PRE ? pre->p[i] : a.cov3Dp[6 * idx + i];
        } else {
            const float rs[3] = { PRE ? pre->p[0] : a.scales[3 * idx], PRE ? pre->p[1] : a.scales[3 * idx + 1], PRE ? pre->p[2] : a.scales[3 * idx + 2] };
            const float rq[4] = { PRE ? pre->p[3] : a.rots[4 * idx], PRE ? pre->p[4] : a.rots[4 * idx + 1], PRE ? pre->p[5] : a.rots[4 * idx + 2],
                                  PRE ? pre->p[6] : a.rots[4 * idx + 3] };
            const Activated ac = activate(a.flags & SKS_RAW_PARAMS, 0.0f, rs, rq);
            sc[0] = ac.s[0]; sc[1] = ac.s[1]; sc[2] = ac.s[2];
            q[0] = ac.q[0]; q[1] = ac.q[1]; q[2] = ac.q[2]; q[3] = ac.q[3];
            qnorm = ac.qnorm;
            computeCov3D(sc, a.smod, q, cov3D);
        }
        const float dL_dconic[3] = { g[2], g[3], g[4] };
        Cov2D c;
        cov2d(mean, h_x, h_y, tan_fovx, tan_fovy, cov3D, V, c);
        const float* t = c.t;
        const float x_grad_mul = (c.txtz < -c.limx || c.txtz > c.limx) ? 0 : 1;
        const float y_grad_mul = (c.tytz < -c.limy || c.tytz > c.limy) ? 0 : 1;
        const M3& T = c.T;
        const M3& Wm = c.W;
        const M3& Vrk = c.Vrk;
        float c_xx = c.cov.m[0][0], c_xy = c.cov.m[0][1], c_yy = c.cov.m[1][1];
        constexpr float h_var = 0.3f;
        float d_inside_root = 0.f;
        const bool aa = a.flags & SKS_ANTIALIASING;
        if (aa) {
            const float det_cov = c_xx * c_yy - c_xy * c_xy;
            c_xx += h_var;
            c_yy += h_var;
            const float det_cov_plus_h_cov = c_xx * c_yy - c_xy * c_xy;
            const float h_convolution_scaling = sqrtf(fmaxf(0.000025f, det_cov / det_cov_plus_h_cov));
            const float dL_dopacity_v = dop;
            const float op_raw = PRE ? pre->opac : a.opac[idx];
            const float d_h_convolution_scaling = dL_dopacity_v * ((a.flags & SKS_RAW_PARAMS) ? 1.0f / (1.0f + expf_fixed(-op_raw)) : op_raw);
            dop = dL_dopacity_v * h_convolution_scaling;
            d_inside_root = (det_cov / det_cov_plus_h_cov) <= 0.000025f ? 0.f : d_h_convolution_scaling / (2 * h_convolution_scaling);
        } else {
            c_xx += h_var;
            c_yy += h_var;
        }
        float dL_dc_xx = 0, dL_dc_xy = 0, dL_dc_yy = 0;
        if (aa) {
            const float x = c_xx, y = c_yy, z = c_xy, w = h_var;
            const float denom_f = d_inside_root / sq(w * w + w * (x + y) + x * y - z * z);
            dL_dc_xx = w * (w * y + y * y + z * z) * denom_f;
            dL_dc_yy = w * (w * x + x * x + z * z) * denom_f;
            dL_dc_xy = -2.f * w * z * (w + x + y) * denom_f;
        }
        const float denom = c_xx * c_yy - c_xy * c_xy;
        const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
        if (denom2inv != 0) {
            dL_dc_xx += denom2inv * (-c_yy * c_yy * dL_dconic[0] + 2 * c_xy * c_yy * dL_dconic[1] + (denom - c_xx * c_yy) * dL_dconic[2]);
            dL_dc_yy += denom2inv * (-c_xx * c_xx * dL_dconic[2] + 2 * c_xx * c_xy * dL_dconic[1] + (denom - c_xx * c_yy) * dL_dconic[0]);
            dL_dc_xy += denom2inv * 2 * (c_xy * c_yy * dL_dconic[0] - (denom + 2 * c_xy * c_xy) * dL_dconic[1] + c_xx * c_xy * dL_dconic[2]);
            dcov[0] = (T.m[0][0] * T.m[0][0] * dL_dc_xx + T.m[0][0] * T.m[1][0] * dL_dc_xy + T.m[1][0] * T.m[1][0] * dL_dc_yy);
            dcov[3] = (T.m[0][1] * T.m[0][1] * dL_dc_xx + T.m[0][1] * T.m[1][1] * dL_dc_xy + T.m[1][1] * T.m[1][1] * dL_dc_yy);
            dcov[5] = (T.m[0][2] * T.m[0][2] * dL_dc_xx + T.m[0][2] * T.m[1][2] * dL_dc_xy + T.m[1][2] * T.m[1][2] * dL_dc_yy);
            dcov[1] = 2 * T.m[0][0] * T.m[0][1] * dL_dc_xx + (T.m[0][0] * T.m[1][1] + T.m[0][1] * T.m[1][0]) * dL_dc_xy + 2 * T.m[1][0] * T.m[1][1] * dL_dc_yy;
            dcov[2] = 2 * T.m[0][0] * T.m[0][2] * dL_dc_xx + (T.m[0][0] * T.m[1][2] + T.m[0][2] * T.m[1][0]) * dL_dc_xy + 2 * T.m[1][0] * T.m[1][2] * dL_dc_yy;
            dcov[4] = 2 * T.m[0][2] * T.m[0][1] * dL_dc_xx + (T.m[0][1] * T.m[1][2] + T.m[0][2] * T.m[1][1]) * dL_dc_xy + 2 * T.m[1][1] * T.m[1][2] * dL_dc_yy;
        }
        const float dL_dT00 = 2 * (T.m[0][0] * Vrk.m[0][0] + T.m[0][1] * Vrk.m[0][1] + T.m[0][2] * Vrk.m[0][2]) * dL_dc_xx +
                              (T.m[1][0] * Vrk.m[0][0] + T.m[1][1] * Vrk.m[0][1] + T.m[1][2] * Vrk.m[0][2]) * dL_dc_xy;
        const float dL_dT01 = 2 * (T.m[0][0] * Vrk.m[1][0] + T.m[0][1] * Vrk.m[1][1] + T.m[0][2] * Vrk.m[1][2]) * dL_dc_xx +
                              (T.m[1][0] * Vrk.m[1][0] + T.m[1][1] * Vrk.m[1][1] + T.m[1][2] * Vrk.m[1][2]) * dL_dc_xy;
        const float dL_dT02 = 2 * (T.m[0][0] * Vrk.m[2][0] + T.m[0][1] * Vrk.m[2][1] + T.m[0][2] * Vrk.m[2][2]) * dL_dc_xx +
                              (T.m[1][0] * Vrk.m[2][0] + T.m[1][1] * Vrk.m[2][1] + T.m[1][2] * Vrk.m[2][2]) * dL_dc_xy;
        const float dL_dT10 = 2 * (T.m[1][0] * Vrk.m[0][0] + T.m[1][1] * Vrk.m[0][1] + T.m[1][2] * Vrk.m[0][2]) * dL_dc_yy +
                              (T.m[0][0] * Vrk.m[0][0] + T.m[0][1] * Vrk.m[0][1] + T.m[0][2] * Vrk.m[0][2]) * dL_dc_xy;
        const float dL_dT11 = 2 * (T.m[1][0] * Vrk.m[1][0] + T.m[1][1] * Vrk.m[1][1] + T.m[1][2] * Vrk.m[1][2]) * dL_dc_yy +
                              (T.m[0][0] * Vrk.m[1][0] + T.m[0][1] * Vrk.m[1][1] + T.m[0][2] * Vrk.m[1][2]) * dL_dc_xy;
        const float dL_dT12 = 2 * (T.m[1][0] * Vrk.m[2][0] + T.m[1][1] * Vrk.m[2][1] + T.m[1][2] * Vrk.m[2][2]) * dL_dc_yy +
                              (T.m[0][0] * Vrk.m[2][0] + T.m[0][1] * Vrk.m[2][1] + T.m[0][2] * Vrk.m[2][2]) * dL_dc_xy;
        const float dL_dJ00 = Wm.m[0][0] * dL_dT00 + Wm.m[0][1] * dL_dT01 + Wm.m[0][2] * dL_dT02;
        const float dL_dJ02 = Wm.m[2][0] * dL_dT00 + Wm.m[2][1] * dL_dT01 + Wm.m[2][2] * dL_dT02;
        const float dL_dJ11 = Wm.m[1][0] * dL_dT10 + Wm.m[1][1] * dL_dT11 + Wm.m[1][2] * dL_dT12;
        const float dL_dJ12 = Wm.m[2][0] * dL_dT10 + Wm.m[2][1] * dL_dT11 + Wm.m[2][2] * dL_dT12;
        const float tz = 1.f / t[2];
        const float tz2 = tz * tz;
        const float tz3 = tz2 * tz;
        const float dL_dtx = x_grad_mul * -h_x * tz2 * dL_dJ02;
        const float dL_dty = y_grad_mul * -h_y * tz2 * dL_dJ12;
        float dL_dtz = -h_x * tz2 * dL_dJ00 - h_y * tz2 * dL_dJ11 + (2 * h_x * t[0]) * tz3 * dL_dJ02 + (2 * h_y * t[1]) * tz3 * dL_dJ12;
        dL_dtz -= g[6] / (t[2] * t[2]);  // inverse-depth term, backward.cu:314-315 (always taken, SURVEY Q4)
        // transformVec4x3Transpose, auxiliary.h:101-109
        dmean[0] = V[0] * dL_dtx + V[1] * dL_dty + V[2] * dL_dtz;
        dmean[1] = V[4] * dL_dtx + V[5] * dL_dty + V[6] * dL_dtz;
        dmean[2] = V[8] * dL_dtx + V[9] * dL_dty + V[10] * dL_dtz;
        // preprocessCUDA backward, backward.cu:423-440
        float m_hom[4];
        transformPoint4x4(mean, proj, m_hom);
        const float m_w = 1.0f / (m_hom[3] + 0.0000001f);
        const float mul1 = (proj[0] * mean[0] + proj[4] * mean[1] + proj[8] * mean[2] + proj[12]) * m_w * m_w;
        const float mul2 = (proj[1] * mean[0] + proj[5] * mean[1] + proj[9] * mean[2] + proj[13]) * m_w * m_w;
        dmean[0] += (proj[0] * m_w - proj[3] * mul1) * dm2x + (proj[1] * m_w - proj[3] * mul2) * dm2y;
        dmean[1] += (proj[4] * m_w - proj[7] * mul1) * dm2x + (proj[5] * m_w - proj[7] * mul2) * dm2y;
        dmean[2] += (proj[8] * m_w - proj[11] * mul1) * dm2x + (proj[9] * m_w - proj[11] * mul2) * dm2y;
        // computeCov3D backward, backward.cu:330-393
        if (!a.cov3Dp) {
            const float r = q[0], x = q[1], y = q[2], z = q[3];
            const M3 R = quatR(q);
            M3 S = {};
            const float s[3] = { a.smod * sc[0], a.smod * sc[1], a.smod * sc[2] };
            S.m[0][0] = s[0]; S.m[1][1] = s[1]; S.m[2][2] = s[2];
            const M3 M = m3mul(S, R);
            M3 dS;
            dS.m[0][0] = dcov[0]; dS.m[0][1] = 0.5f * dcov[1]; dS.m[0][2] = 0.5f * dcov[2];
            dS.m[1][0] = 0.5f * dcov[1]; dS.m[1][1] = dcov[3]; dS.m[1][2] = 0.5f * dcov[4];
            dS.m[2][0] = 0.5f * dcov[2]; dS.m[2][1] = 0.5f * dcov[4]; dS.m[2][2] = dcov[5];
            M3 M2;
#pragma unroll
            for (int cc = 0; cc < 3; cc++)
#pragma unroll
                for (int rr = 0; rr < 3; rr++) M2.m[cc][rr] = 2.0f * M.m[cc][rr];
            const M3 dL_dM = m3mul(M2, dS);
            const M3 Rt = m3T(R);
            M3 dMt = m3T(dL_dM);
#pragma unroll
            for (int k = 0; k < 3; k++)
                dscale[k] = Rt.m[k][0] * dMt.m[k][0] + Rt.m[k][1] * dMt.m[k][1] + Rt.m[k][2] * dMt.m[k][2];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int rr = 0; rr < 3; rr++) dMt.m[k][rr] *= s[k];
            dq[0] = 2 * z * (dMt.m[0][1] - dMt.m[1][0]) + 2 * y * (dMt.m[2][0] - dMt.m[0][2]) + 2 * x * (dMt.m[1][2] - dMt.m[2][1]);
            dq[1] = 2 * y * (dMt.m[1][0] + dMt.m[0][1]) + 2 * z * (dMt.m[2][0] + dMt.m[0][2]) + 2 * r * (dMt.m[1][2] - dMt.m[2][1]) - 4 * x * (dMt.m[2][2] + dMt.m[1][1]);
            dq[2] = 2 * x * (dMt.m[1][0] + dMt.m[0][1]) + 2 * r * (dMt.m[2][0] - dMt.m[0][2]) + 2 * z * (dMt.m[1][2] + dMt.m[2][1]) - 4 * y * (dMt.m[2][2] + dMt.m[0][0]);
            dq[3] = 2 * r * (dMt.m[0][1] - dMt.m[1][0]) + 2 * x * (dMt.m[2][0] + dMt.m[0][2]) + 2 * y * (dMt.m[1][2] + dMt.m[2][1]) - 4 * z * (dMt.m[1][1] + dMt.m[0][0]);
        }
    }
    if (a.dmeans3D) { a.dmeans3D[3 * o] = dmean[0]; a.dmeans3D[3 * o + 1] = dmean[1]; a.dmeans3D[3 * o + 2] = dmean[2]; }
    if (a.dmeans2D) { a.dmeans2D[3 * o] = dm2x; a.dmeans2D[3 * o + 1] = dm2y; a.dmeans2D[3 * o + 2] = 0.0f; }
    // SKS_RAW_GRADS (with SKS_RAW_PARAMS): the gradients of the LEAF parameters -- what autograd forms through torch.sigmoid /
    // torch.exp / F.normalize behind the activated ones (scene/gaussian_model.py:39-47); the same Jacobians as `packed` below
    const bool rawg = (a.flags & SKS_RAW_PARAMS) && (a.flags & SKS_RAW_GRADS);
    if (a.dopacity) {
        float oj = 1.0f;
        if (rawg) {
            const float so = 1.0f / (1.0f + expf_fixed(-(PRE ? pre->opac : a.opac[idx])));
            oj = so * (1.0f - so);
        }
        a.dopacity[o] = dop * oj;
    }
    if (a.dcov3D) {
#pragma unroll
        for (int i = 0; i < 6; i++) a.dcov3D[6 * o + i] = dcov[i];
    }
    if (a.dscales) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.dscales[3 * o + k] = dscale[k] * (rawg ? sc[k] : 1.0f);
    }
    if (a.drots) {
        float dot = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) dot += q[k] * dq[k];
#pragma unroll
        for (int k = 0; k < 4; k++) a.drots[4 * o + k] = rawg ? (dq[k] - q[k] * dot) / qnorm : dq[k];
    }
    if (a.packed) {
        // raw-parameter gradients [xyz 3 | _scaling 3 | _rotation 4 | _opacity 1] through the activation Jacobians
        // (what autograd does through exp / normalize / sigmoid), times 1/N_v of the fused masked-L2 loss
        float scl = 1.0f;
        if (a.loss_sums) scl = (float)(1.0 / (n_view < 1.0 ? 1.0 : n_view));
        float* pk = a.packed + o * 11;
        const bool raw = a.flags & SKS_RAW_PARAMS;
        pk[0] = dmean[0] * scl; pk[1] = dmean[1] * scl; pk[2] = dmean[2] * scl;
#pragma unroll
        for (int k = 0; k < 3; k++) pk[3 + k] = dscale[k] * (raw ? sc[k] : 1.0f) * scl;
        float dot = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) dot += q[k] * dq[k];
#pragma unroll
        for (int k = 0; k < 4; k++) pk[6 + k] = (raw ? (dq[k] - q[k] * dot) / qnorm : dq[k]) * scl;
        float oj = 1.0f;
        if (raw) {
            const float so = 1.0f / (1.0f + expf_fixed(-(PRE ? pre->opac : a.opac[idx])));
            oj = so * (1.0f - so);
        }
        pk[10] = dop * oj * scl;
    }
}

__global__ __launch_bounds__(256) void k_geom_bwd(GeomBwdArgs a, ViewTan vt)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int v = blockIdx.y;
    float g[NACC];
    double pS, pN;
    if (a.dfeat) geom_bwd_dfeat(a, (size_t)v * a.P + blockIdx.x * 256, min(256, a.P - (int)blockIdx.x * 256), threadIdx.x, 256);
    geom_bwd_load<false>(a, v, idx, g, pS, pN);
    double n_view = 1.0;
    if (a.loss_sums) {  // fused-loss mode (single block per view): image-wide S and N from the owners' partial sums
        __shared__ double s_l[2][4];
        pS = wave_sum_d(pS);
        pN = wave_sum_d(pN);
        if ((threadIdx.x & 63) == 0) { s_l[0][threadIdx.x >> 6] = pS; s_l[1][threadIdx.x >> 6] = pN; }
        __syncthreads();
        const double S = a.gt_totals[2 * v] + ((s_l[0][0] + s_l[0][1]) + (s_l[0][2] + s_l[0][3]));
        n_view = a.gt_totals[2 * v + 1] + ((s_l[1][0] + s_l[1][1]) + (s_l[1][2] + s_l[1][3]));
        if (threadIdx.x == 0) {
            a.loss_sums[2 * v] = S;
            a.loss_sums[2 * v + 1] = n_view;
        }
    }
    if (idx >= a.P) return;
    geom_bwd_finish(a, vt, v, idx, g, n_view);
}

// The binned path's geometry backward (nsplit == 0, no fused loss).  The compositing backward left BIN_ROWS 32-byte rows per
// (Gaussian, tile of its rect) in `part` -- one per 8-row half of the tile --, a Gaussian's rows consecutive from slot goff (Bin).
// A workgroup takes 64 Gaussians: four threads per Gaussian add its rows, thread t the rows t, t + 4, ... -- four rows in flight per
// thread, one trip for rects of up to eight tiles (a thread per Gaussian adding all its rows alone was a chain of dependent round
// trips in every wavefront: 48 us) --, the four partial sums are added in a fixed order (reproducible), then one full wavefront
// runs the reference's formulas, a Gaussian per lane; a Gaussian's own inputs were requested with the first round trip.
constexpr int GEOMB_G = 64;
__global__ __launch_bounds__(256) void k_geom_bwd_binned(GeomBwdArgs a, ViewTan vt)
{
    __shared__ float s_g[GEOMB_G][4][NACC];
    const int tid = threadIdx.x, v = blockIdx.y + a.v0;
    const int idx = blockIdx.x * GEOMB_G + tid;       // phase 2: thread tid < GEOMB_G
    GeomBwdIn in;
    const bool mine = tid < GEOMB_G && idx < a.P;
    if (mine) geom_bwd_fetch(a, v, idx, in);
    {
        const int gi = tid >> 2, st = tid & 3;          // phase 1: rows st, st + 4, ... of the block's gi-th Gaussian
        const int gidx = blockIdx.x * GEOMB_G + gi;
        float sum[NACC];
#pragma unroll
        for (int k = 0; k < NACC; k++) sum[k] = 0.0f;
        if (gidx < a.P) {
            const size_t o = (size_t)v * a.P + gidx;
            const uint4 r = a.rect[o];
            const int n = BIN_ROWS * (int)((r.z - r.x) * (r.w - r.y));
            const size_t s0 = BIN_ROWS * (size_t)a.goff[o], send = BIN_ROWS * a.cap;
            const float4* rows = reinterpret_cast<const float4*>(a.part + (size_t)v * a.cap * BIN_ROWS * NACC);
            for (int i = st; i < n; i += 16) {
                float4 q[4][2];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const bool on = i + 4 * u < n && s0 + i + 4 * u < send;
                    q[u][0] = on ? rows[(s0 + i + 4 * u) * 2] : make_float4(0, 0, 0, 0);
                    q[u][1] = on ? rows[(s0 + i + 4 * u) * 2 + 1] : make_float4(0, 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    sum[0] += q[u][0].x; sum[1] += q[u][0].y; sum[2] += q[u][0].z; sum[3] += q[u][0].w;
                    sum[4] += q[u][1].x; sum[5] += q[u][1].y; sum[6] += q[u][1].z;
                }
            }
        }
        float4* sg = reinterpret_cast<float4*>(s_g[gi][st]);
        sg[0] = make_float4(sum[0], sum[1], sum[2], sum[3]);
        sg[1] = make_float4(sum[4], sum[5], sum[6], 0.0f);
    }
    __syncthreads();
    if (!mine) return;
    float g[NACC];
#pragma unroll
    for (int k = 0; k < NACC - 1; k++) g[k] = (s_g[tid][0][k] + s_g[tid][1][k]) + (s_g[tid][2][k] + s_g[tid][3][k]);
    g[NACC - 1] = 0.0f;
    // An overflowed arena (only reachable with check_capacity "lazy" / "auto" / False: the synchronous check redoes the forward):
    // k_bin_band_scatter dropped the entries beyond the capacity, the compositing backward never wrote THEIR rows, and the rows summed
    // above are whatever an earlier step or the long-list sort's key scratch left there.  The image of that forward was already
    // missing entries; its gradients are made NaN rather than plausible numbers
    if (a.bin_hdr[0]) {
#pragma unroll
        for (int k = 0; k < NACC - 1; k++) g[k] = __int_as_float(0x7fc00000);
    }
    if (a.dfeat) {   // (accumulated with atomics by the compositing backward: accum rows of NACC + C, one per (view, Gaussian))
        const size_t o = (size_t)v * a.P + idx;
        const float* acc = a.accum + o * (NACC + a.C);
        for (int ch = 0; ch < a.C; ch++) a.dfeat[o * a.C + ch] = acc[NACC + ch];
    }
    geom_bwd_finish<true>(a, vt, v, idx, g, 1.0, &in);
}

// The same for ALL views in one workgroup (V * P <= 256: H36M's 4 x 17), plus what the reference's loop does with the
// per-view joint gradients right after the backward -- xyz.grad = accumulated_grads.mean(dim=0), train.py:215-217 -- so a
// caller that wants that mean does not pay another launch for 200 floats: thread t = (view t / P, Gaussian t % P); the views
// of a Gaussian are summed in view order, then divided by V (the summation order of sks_loop_adam_step).
// PF (empty, or one PreFill by value): the prefill role of sks_backward_prefill -- blocks 1 .. nfill zero planes of the next
// forward's output set and leave before the barrier; block 0 is the geometry backward, as without the role.
template <class... PF>
__global__ __launch_bounds__(256) void k_geom_bwd_all(GeomBwdArgs a, ViewTan vt, int V, float* __restrict__ mean_out, PF... pf)
{
    static_assert(sizeof...(PF) <= 1, "at most one PreFill");
    if constexpr (sizeof...(PF) == 1) {
        if (blockIdx.x > 0) {   // (workgroup-uniform)
            prefill_block((pf, ...), blockIdx.x - 1u);
            return;
        }
    }
    const int t = threadIdx.x;
    const int v = t / a.P, idx = t - v * a.P;
    const bool live = v < V;
    float g[NACC];
    double pS, pN;
    if (a.dfeat) geom_bwd_dfeat(a, 0, V * a.P, t, 256);
    if (live) {
        geom_bwd_load<false>(a, v, idx, g, pS, pN);
        geom_bwd_finish(a, vt, v, idx, g, 1.0);
    }
    __syncthreads();   // every view's dL_dmeans3D is written (same workgroup, same L1)
    if (t < a.P) {
        float m[3] = { 0.0f, 0.0f, 0.0f };
        for (int w0 = 0; w0 < V; w0 += 4) {   // four views' loads in flight together, added in view order
            float tv[4][3];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float* gm = a.dmeans3D + ((size_t)(w0 + j < V ? w0 + j : V - 1) * a.P + t) * 3;
                tv[j][0] = gm[0]; tv[j][1] = gm[1]; tv[j][2] = gm[2];
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (w0 + j < V) { m[0] += tv[j][0]; m[1] += tv[j][1]; m[2] += tv[j][2]; }
        }
        mean_out[3 * t] = m[0] / (float)V; mean_out[3 * t + 1] = m[1] / (float)V; mean_out[3 * t + 2] = m[2] / (float)V;
    }
}
// (V * P > 256: the mean as a tiny kernel of its own behind k_geom_bwd)
// `world` > 1: the rows are in the order all_gather_into_tensor leaves them (view w = row (w % world) * vmax + w / world,
// vmax = ceil(V / world), see sks_loop_adam_step); summed in VIEW order either way
__global__ void k_mean_views(int V, int P, const float* __restrict__ dmeans3D, float* __restrict__ mean_out, int world = 1)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * P) return;
    const int vmax = (V + world - 1) / world;
    float m = 0.0f;
    // the loads of eight views are in flight together (issued one by one behind their adds they were V dependent round
    // trips to rows another queue had just written: 9 us for 31 views); the adds keep the view order
    for (int w0 = 0; w0 < V; w0 += 8) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int w = w0 + j < V ? w0 + j : V - 1;
            const int row = world == 1 ? w : (w % world) * vmax + w / world;
            t[j] = dmeans3D[(size_t)row * P * 3 + i];
        }
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (w0 + j < V) m += t[j];
    }
    mean_out[i] = m / (float)V;
}

// ------------------------------------------------------------------------------------------------------------
// Fused tail of one accumulation group of the sparse loop on ONE GPU (sks_loop_fused_step): everything that follows the
// compositing backward and precedes the next one is tiny (V*P <= a few hundred work items) and used to be three
// launches (k_geom_bwd, k_loop_adam, k_geom_fwd of the next group) whose fixed cost and the gaps between them were a
// third of the group.  One 256-thread workgroup runs them back to back:
//   A  geometry backward of every view: wavefront w takes views w, w+4, ...; lane = Gaussian (P <= 64), so a view's
//      loss sums are one wave reduction; writes the packed raw-parameter gradients;
//   B  the optimiser step (slots, mean over views, limb gradient, LR schedule, Adam) -- sks_loop_dev.h;
//   C  geometry forward of the UPDATED parameters, i.e. the geom / radii the next group's compositor reads.
// Same arithmetic in the same order as the separate kernels (bit-identical results).
// ES (sks_loop_fused_step_es): frame f runs the early-stopping criterion on its own slice of aa.es_state between A and B,
// exactly as k_loop_adam does for one scene: a cut inside the group shortens the step (views, winning view, iterations,
// the LR schedule's iteration); a frame that stopped at an earlier launch leaves at once and writes nothing.
// ------------------------------------------------------------------------------------------------------------
// VT = ViewTan: the per-view scalars by value.  VT = ViewTanDev (sks_loop_fused_step_dv): they are read from the device table, and
// frame f's LR schedule is row f of vt.sched instead of the one schedule in `aa`.
// VW (k_step_tail_vw): phase B weights the views by their agreement (sks_loop_dev.h); frame f's rows of vw.weights (frames,V,P) and
// vw.similarity (frames,P,V,V) are written by the step it takes, never by a frame that has stopped.
template <bool ES, class VT, bool VW>
__device__ __forceinline__ void step_tail_body(GeomBwdArgs& ga, VT& vt, sksloop::AdamArgs& aa, int V, Geom& g, int* radii,
                                               sksloop::ViewWeightArgs* vw)
{
    __shared__ float s_xyz[256 * 3];
    __shared__ float s_hyp[6];
    __shared__ double s_d[4];
    __shared__ int s_it[2];
    __shared__ float s_np[64 * 11];   // the updated parameters, handed to phase C through LDS (P <= 64)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // One workgroup per FRAME (grid = frames; a single frame is the usual case): V views and P Gaussians of its own.  Global
    // view index = vb + v; the frame's parameters, moments, slots and counters sit f-th in their stacked tensors.
    const int P = ga.P;
    const int f = blockIdx.x, vb = f * V;
    if (f) {
        ga.means += (size_t)f * P * 3; ga.opac += (size_t)f * P; ga.scales += (size_t)f * P * 3; ga.rots += (size_t)f * P * 4;
        aa.grads += (size_t)vb * P * 11; aa.slots += (size_t)vb * P * 3;
        aa.xyz += (size_t)f * P * 3; aa.scaling += (size_t)f * P * 3; aa.rotation += (size_t)f * P * 4; aa.opacity += (size_t)f * P;
        aa.m += (size_t)f * P * 11; aa.vv += (size_t)f * P * 11; aa.counters += 2 * f;
    }
    if constexpr (VW) {
        if (vw->weights) vw->weights += (size_t)vb * P;
        if (vw->similarity) vw->similarity += (size_t)vb * P * V;
    }
    if constexpr (std::is_same<VT, ViewTanDev>::value) {
        // the frame's own schedule (frames of different rigs: lr = position_lr x that rig's extent), {log lr_init, log lr_final,
        // delay_mult, delay_steps, max_steps}: the logarithms were taken on the host, as fill_adam_args takes them
        const double* r = vt.sched + 5 * (size_t)f;
        aa.log_lr_init = r[0]; aa.log_lr_final = r[1]; aa.lr_delay_mult = r[2];
        aa.lr_delay_steps = (int)r[3]; aa.lr_max_steps = (int)r[4];
        aa.lr_init = r[0] == -INFINITY ? 0.0 : 1.0;      // (read only by the "schedule switched off" test: both end points zero)
        aa.lr_final = r[1] == -INFINITY ? 0.0 : 1.0;
    }
    if constexpr (ES) {
        aa.es_state += (size_t)f * (2 + 2 * aa.es_window);
        if (aa.es_host_flag) aa.es_host_flag += f;
        if (aa.es_state[1] != 0) return;   // stopped at an earlier launch (workgroup-uniform; only this workgroup writes it)
    }
    // the optimiser's scalar work (LR schedule, bias corrections: double transcendentals) needs no gradient: started
    // first, it is finished long before phase A's loads are back
    sksloop::adam_block_begin(aa, s_xyz, s_d, s_it);
    // The step sizes (a handful of double divisions and a square root by ONE thread, 1.4 us) need all four of those
    // results, i.e. a barrier: taken while each wavefront's first 36 partial-sum lines are in flight, both cost nothing.
    const bool split = ga.nsplit == BWD_SPLITS && ga.dfeat == nullptr;
    GeomBwdRaw raw;
    if (split && wv < V) geom_bwd_issue16(ga, vb + wv, lane, raw);
    __syncthreads();
    if (tid == 0) sksloop::adam_step_sizes(aa, s_d, s_hyp);
    for (int v = wv; v < V; v += 4) {
        const int vg = vb + v;
        float gs[NACC];
        double pS, pN;
        if (split) {
            if (v != wv) geom_bwd_issue16(ga, vg, lane, raw);
            geom_bwd_sum16(ga, lane, raw, gs, pS, pN);
        } else {
            geom_bwd_load(ga, vg, lane, gs, pS, pN);
        }
        pS = wave_sum_d(pS);
        pN = wave_sum_d(pN);
        const double S = ga.gt_totals[2 * vg] + pS, n_view = ga.gt_totals[2 * vg + 1] + pN;
        if (lane == 0) { ga.loss_sums[2 * vg] = S; ga.loss_sums[2 * vg + 1] = n_view; }
        if (lane < ga.P) geom_bwd_finish(ga, vt, vg, lane, gs, n_view);
    }
    __syncthreads();   // every view's packed gradients are written (same workgroup, same L1)
    if constexpr (ES) {
        // the criterion on the loss sums phase A just wrote and the pre-step xyz adam_block_begin parked in s_xyz
        __shared__ unsigned long long s_mask;
        __shared__ int s_cut[3];
        if (tid == 0)
            sksloop::early_stop_decide(aa, aa.es_state, aa.es_host_flag, s_xyz,
                                       [&](int v) { return (const double*)ga.loss_sums + 2 * (size_t)(vb + v); }, &s_mask, s_cut);
        __syncthreads();
        aa.group_mask = s_mask; aa.last_view = s_cut[0];
        if (s_cut[1] != aa.acc_steps) {   // fired inside the group (workgroup-uniform): the step happens at that iteration,
            aa.acc_steps = s_cut[1];      // so the LR schedule and the counters begin again from there
            sksloop::adam_block_begin(aa, s_xyz, s_d, s_it);
            __syncthreads();
            if (tid == 0) sksloop::adam_step_sizes(aa, s_d, s_hyp);
        }
    }
    const sksloop::AdamLdsParams mirror{ s_np, s_np + 3 * P, s_np + 6 * P, s_np + 10 * P };
    sksloop::adam_block_finish<VW>(aa, s_xyz, s_hyp, s_d, s_it, &mirror, /*step_sizes_ready=*/true, vw);
    __syncthreads();   // the parameters are updated
    for (int v = wv; v < V; v += 4)
        geom_fwd_one(P, vt, ga.vms, ga.pms, mirror.xyz, mirror.opacity, mirror.scaling, mirror.rotation, nullptr,
                     ga.smod, ga.flags, g, radii, vb + v, lane, lane < P);
}

template <bool ES = false, class VT = ViewTan>
__global__ __launch_bounds__(256) void k_step_tail(GeomBwdArgs ga, VT vt, sksloop::AdamArgs aa, int V, Geom g, int* radii)
{
    step_tail_body<ES, VT, false>(ga, vt, aa, V, g, radii, nullptr);
}
template <bool ES = false, class VT = ViewTan>
__global__ __launch_bounds__(256) void k_step_tail_vw(GeomBwdArgs ga, VT vt, sksloop::AdamArgs aa, int V, Geom g, int* radii,
                                                      sksloop::ViewWeightArgs vw)
{
    step_tail_body<ES, VT, true>(ga, vt, aa, V, g, radii, &vw);
}
