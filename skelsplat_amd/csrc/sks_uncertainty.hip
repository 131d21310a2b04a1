// sks_uncertainty.hip -- the optimised Gaussians read back as the pose's uncertainty, for MI355X: what the reference's analysis
// scripts take from the covariance a scene leaves behind.  Per joint the 3x3 covariance, its spectrum, trace, determinant and
// anisotropy, and the squared Mahalanobis distance of the ground truth (utils/analize_error_confidence_correlation.py:38-60,
// 117-143); per (view, joint) the two variances of the projected blob (utils/analize_2D_anisotropy.py:50); the share of
// ground-truth joints inside the k-sigma ellipsoids, overall and per joint (percent_inside_sigmas, .._per_joint).
//
// All three kernels are bound by launch latency (a frame is 17 joints, a sequence a few thousand frames): one thread per (frame,
// joint) or (view, joint), one workgroup per row of counts; nothing handed from one workgroup to another, no atomics, no scratch.
// What a (frame, joint) receives depends on its own inputs alone -- never on N, its place in the batch or the stream --, so a
// NaN or inf poisons the outputs of its own joint that depend on it and nobody else's.
//
// The spectrum is ANALYTIC.  Sigma = R S^2 R^T with R a rotation, so its eigenvalues are the squares of the three standard
// deviations the model stores: sorting three numbers gives them to half an ulp, where any eigen-solver run on the nine rounded
// entries of Sigma loses the small eigenvalues of a needle (scale ratio 1e6: lambda_3 / lambda_1 = 1e-12, far below float's 6e-8
// of lambda_1).  The Mahalanobis distance is formed by whitening for the same reason: w = S^-1 R^T delta, d2 = |w|^2, no 3x3
// inverse.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"
#include "sks_gauss.h"

namespace {

constexpr int UNC_THREADS = 256;

__device__ __forceinline__ void order_desc(float& a, float& b)     // (a NaN stays where it is)
{
    if (b > a) { const float t = a; a = b; b = t; }
}

// One thread per (frame, joint) i of N * P.
__global__ void __launch_bounds__(UNC_THREADS)
k_joint_uncertainty(size_t total, const float* __restrict__ xyz, const float* __restrict__ scales, const float* __restrict__ rots,
                    float scale_modifier, const float* __restrict__ gt, float* __restrict__ cov6, float* __restrict__ spectrum,
                    float* __restrict__ d2)
{
    const size_t i = (size_t)blockIdx.x * UNC_THREADS + threadIdx.x;
    if (i >= total) return;
    float R[3][3], sd[3], Sg[3][3];
    sks::gaussian_sigma(rots + 4 * i, scales + 3 * i, scale_modifier, R, sd, Sg);
    float* c = cov6 + 6 * i;        // strip_symmetric's order (general_utils.py:73-85)
    c[0] = Sg[0][0]; c[1] = Sg[0][1]; c[2] = Sg[0][2]; c[3] = Sg[1][1]; c[4] = Sg[1][2]; c[5] = Sg[2][2];
    float l1 = sd[0] * sd[0], l2 = sd[1] * sd[1], l3 = sd[2] * sd[2];
    order_desc(l1, l2); order_desc(l2, l3); order_desc(l1, l2);
    float* s = spectrum + 6 * i;
    s[0] = l1; s[1] = l2; s[2] = l3;
    s[3] = (Sg[0][0] + Sg[1][1]) + Sg[2][2];
    s[4] = (l1 * l2) * l3;
    s[5] = l1 / l3;
    if (gt) {
        const float* g = gt + 3 * i;
        const float* x = xyz + 3 * i;
        const float d[3] = { g[0] - x[0], g[1] - x[1], g[2] - x[2] };
        float w[3];
        for (int k = 0; k < 3; k++) w[k] = ((R[0][k] * d[0] + R[1][k] * d[1]) + R[2][k] * d[2]) / sd[k];
        d2[i] = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    }
}

// One thread per (view, joint) i of V * J; vf > 0: view v belongs to frame v / vf, whose J Gaussians sit frame-th in the stacked
// tensors (k_heatmap_factors' convention).
template <class TAN>
__global__ void __launch_bounds__(UNC_THREADS)
k_view_footprints(int V, int J, const float* __restrict__ means, const float* __restrict__ scales, const float* __restrict__ rots,
                  float scale_modifier, const float* __restrict__ viewmatrix, TAN tan, float* __restrict__ lambdas, int vf)
{
    const size_t i = (size_t)blockIdx.x * UNC_THREADS + threadIdx.x;
    if (i >= (size_t)V * J) return;
    const int v = (int)(i / J), j = (int)(i % J);
    const size_t g = (vf > 0 ? (size_t)(v / vf) * J : 0) + j;
    float R[3][3], sd[3], Sg[3][3], l1, l2;
    sks::gaussian_sigma(rots + 4 * g, scales + 3 * g, scale_modifier, R, sd, Sg);
    sks::ewa_lambdas(Sg, viewmatrix + 16 * v, means + 3 * g, tan.w[v], tan.h[v], tan.x[v], tan.y[v], l1, l2);
    lambdas[2 * i] = l1;
    lambdas[2 * i + 1] = l2;
}

struct KSigma { int K; float t2[SKS_CALIBRATION_MAX_K]; };

// One workgroup per row of counts (0: every joint, 1 + j: joint j).  Thread t takes frames t, t + 256, ...; the 256 partial
// counts of every column meet in a tree.  Integers: exact in any order.
__global__ void __launch_bounds__(UNC_THREADS)
k_calibration(int N, int P, const float* __restrict__ d2, const unsigned char* __restrict__ valid, KSigma ks,
              int* __restrict__ counts)
{
    __shared__ int s_cnt[SKS_CALIBRATION_MAX_K + 1][UNC_THREADS];
    const int tid = threadIdx.x, row = (int)blockIdx.x;
    const int p0 = row == 0 ? 0 : row - 1, p1 = row == 0 ? P : row;
    int c[SKS_CALIBRATION_MAX_K + 1];
#pragma unroll
    for (int k = 0; k <= SKS_CALIBRATION_MAX_K; k++) c[k] = 0;
    for (int i = tid; i < N; i += UNC_THREADS) {
        if (valid && !valid[i]) continue;
        const float* d = d2 + (size_t)i * P;
        for (int p = p0; p < p1; p++) {
            const float v = d[p];
            if (v != v) continue;
            c[SKS_CALIBRATION_MAX_K]++;
#pragma unroll
            for (int k = 0; k < SKS_CALIBRATION_MAX_K; k++) c[k] += (k < ks.K && v <= ks.t2[k]) ? 1 : 0;
        }
    }
#pragma unroll
    for (int k = 0; k <= SKS_CALIBRATION_MAX_K; k++) s_cnt[k][tid] = c[k];
    for (int o = UNC_THREADS / 2; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o)
            for (int k = 0; k <= SKS_CALIBRATION_MAX_K; k++) s_cnt[k][tid] += s_cnt[k][tid + o];
    }
    __syncthreads();
    if (tid <= ks.K) counts[(size_t)row * (ks.K + 1) + tid] = s_cnt[tid < ks.K ? tid : SKS_CALIBRATION_MAX_K][0];
}

}  // namespace

extern "C" int sks_joint_uncertainty(int N, int P, const float* xyz, const float* scales, const float* rotations,
                                     float scale_modifier, const float* gt, float* cov6, float* spectrum, float* d2, void* stream)
{
    if (N < 1 || P < 1) return fail2(-1, "joint_uncertainty: N = %d frames of P = %d joints; both must be at least 1", N, P);
    if ((long long)N * P > 0x7fffffffLL / 8) return fail2(-1, "joint_uncertainty: N x P = %d x %d joints are too many", N, P);
    if (!scales || !rotations || !cov6 || !spectrum)
        return fail2(-2, "joint_uncertainty: missing %s", !scales ? "scales" : !rotations ? "rotations" : !cov6 ? "cov6 (N,P,6)" : "spectrum (N,P,6)");
    if (gt && (!xyz || !d2)) return fail2(-2, "joint_uncertainty: gt is given, so %s is required", !xyz ? "xyz" : "d2 (N,P)");
    if (!gt && d2) return fail2(-2, "joint_uncertainty: d2 is given without gt");
    const size_t total = (size_t)N * P;
    hipLaunchKernelGGL(k_joint_uncertainty, dim3((unsigned)((total + UNC_THREADS - 1) / UNC_THREADS)), dim3(UNC_THREADS), 0,
                       (hipStream_t)stream, total, xyz, scales, rotations, scale_modifier, gt, cov6, spectrum, d2);
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" int sks_view_footprints(int V, int J, int W, int H, const float* means3D, const float* scales, const float* rotations,
                                   float scale_modifier, const float* viewmatrix, const float* tanfovx, const float* tanfovy,
                                   const int* view_wh, const void* views_dev, int frames, float* lambdas, void* stream)
{
    if (V < 1 || V > SKS_MAX_VIEWS || J < 1 || W < 1 || H < 1)
        return fail2(-1, "view_footprints: bad shape: 1 <= V <= %d (SKS_MAX_VIEWS), J, W, H >= 1", SKS_MAX_VIEWS);
    if ((long long)V * J > 0x7fffffffLL / 8) return fail2(-1, "view_footprints: V x J = %d x %d are too many", V, J);
    if (frames < 1 || V % frames) return fail2(-1, "view_footprints: frames = %d must divide the number of views %d", frames, V);
    if (!means3D || !scales || !rotations || !viewmatrix || !lambdas) return fail2(-2, "view_footprints: missing pointer");
    const bool host = tanfovx || tanfovy || view_wh;
    if (host && views_dev) return fail2(-2, "view_footprints: both view forms given: tanfovx / tanfovy / view_wh (HOST) or views_dev, not both");
    if (!views_dev && !(tanfovx && tanfovy)) return fail2(-2, "view_footprints: no view form given: tanfovx and tanfovy (HOST), or views_dev");
    const unsigned blocks = (unsigned)(((size_t)V * J + UNC_THREADS - 1) / UNC_THREADS);
    const int vf = frames > 1 ? V / frames : 0;
    if (views_dev) {
        hipLaunchKernelGGL(k_view_footprints<sks::HmTanDev>, dim3(blocks), dim3(UNC_THREADS), 0, (hipStream_t)stream, V, J, means3D,
                           scales, rotations, scale_modifier, viewmatrix, sks::hm_tan_dev(views_dev), lambdas, vf);
    } else {
        sks::HmTan tan;
        for (int v = 0; v < V; v++) {
            tan.x[v] = tanfovx[v]; tan.y[v] = tanfovy[v];
            tan.w[v] = view_wh ? view_wh[2 * v] : W; tan.h[v] = view_wh ? view_wh[2 * v + 1] : H;
            if (tan.w[v] < 1 || tan.w[v] > W || tan.h[v] < 1 || tan.h[v] > H)
                return fail2(-1, "view_footprints: every view's size must be within [1, W] x [1, H]");
        }
        hipLaunchKernelGGL(k_view_footprints<sks::HmTan>, dim3(blocks), dim3(UNC_THREADS), 0, (hipStream_t)stream, V, J, means3D,
                           scales, rotations, scale_modifier, viewmatrix, tan, lambdas, vf);
    }
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" int sks_calibration(int N, int P, const float* d2, const unsigned char* valid, int K, const float* k_sigma, int* counts,
                               void* stream)
{
    if (N < 1 || P < 1) return fail2(-1, "calibration: N = %d frames of P = %d joints; both must be at least 1", N, P);
    if ((long long)N * P > 0x7fffffffLL) return fail2(-1, "calibration: N x P = %d x %d entries are too many for int32 counts", N, P);
    if (K < 1 || K > SKS_CALIBRATION_MAX_K) return fail2(-1, "calibration: K = %d sigma levels, 1 .. %d (SKS_CALIBRATION_MAX_K)", K, SKS_CALIBRATION_MAX_K);
    if (!d2 || !k_sigma || !counts) return fail2(-2, "calibration: missing %s", !d2 ? "d2" : !k_sigma ? "k_sigma (HOST K)" : "counts (1 + P, K + 1)");
    KSigma ks;
    ks.K = K;
    for (int k = 0; k < SKS_CALIBRATION_MAX_K; k++) {
        const float s = k < K ? k_sigma[k] : 1.0f;
        if (!(s > 0.0f) || !isfinite(s)) return fail2(-1, "calibration: k_sigma[%d] = %g must be finite and > 0", k, (double)s);
        ks.t2[k] = s * s;
    }
    hipLaunchKernelGGL(k_calibration, dim3(1 + P), dim3(UNC_THREADS), 0, (hipStream_t)stream, N, P, d2, valid, ks, counts);
    HIP_TRY2(hipGetLastError());
    return 0;
}
