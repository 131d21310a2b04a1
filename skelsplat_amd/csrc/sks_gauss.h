// sks_gauss.h -- one joint's Gaussian as the reference describes it, for the kernels that need more of it than the rasterizer's
// geometry stage keeps: the 3D covariance Sigma = L L^T, L = R diag(scale_modifier * s), R from the NORMALISED quaternion
// (scene/gaussian_model.py:33-37, utils/general_utils.py:87-119), and the two variances lambda1 >= lambda2 the reference draws a
// view's pseudo-GT blob with (its own transcription of the EWA projection, utils/general_utils.py:212-262).
//
// ONE owner of both float sequences: k_heatmap_factors (sks_ops.hip) and the kernels of sks_uncertainty.hip call these two
// functions, so the footprints sks_view_footprints reports are, bit for bit, the ones the heat-maps were drawn with.  The
// library is built with -ffp-contract=off: every expression below is evaluated as written, one rounding per operation.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/skelsplat_hip.h"

namespace sks {

// The per-view scalars of the heat-map kernels, by value in the kernel's argument segment ...
struct HmTan {
    float x[SKS_MAX_VIEWS], y[SKS_MAX_VIEWS];
    int w[SKS_MAX_VIEWS], h[SKS_MAX_VIEWS];   // per-view image size (<= the W, H strides of row / col)
};

struct HmTanDev {   // ... or in device memory (the *_dv entry points: the ViewTan table sks_rig_select fills)
    const float* x;
    const float* y;
    const int* w;
    const int* h;
};
inline HmTanDev hm_tan_dev(const void* views_dev)
{
    const HmTan* t = (const HmTan*)views_dev;     // (same layout as the rasterizer's ViewTan; addresses only)
    return HmTanDev{ t->x, t->y, t->w, t->h };
}

// q: the raw quaternion (r, x, y, z); s: the ACTIVATED scales.  R: the rotation of the normalised quaternion; sd[k] =
// scale_modifier * s[k], the standard deviation along R's column k; Sg = (R diag(sd)) (R diag(sd))^T.
__device__ __forceinline__ void gaussian_sigma(const float* __restrict__ q, const float* __restrict__ s, float scale_modifier,
                                               float R[3][3], float sd[3], float Sg[3][3])
{
    const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const float qn = sqrtf(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const float r = q0 / qn, x = q1 / qn, y = q2 / qn, z = q3 / qn;
    R[0][0] = 1 - 2 * (y * y + z * z); R[0][1] = 2 * (x * y - r * z);     R[0][2] = 2 * (x * z + r * y);
    R[1][0] = 2 * (x * y + r * z);     R[1][1] = 1 - 2 * (x * x + z * z); R[1][2] = 2 * (y * z - r * x);
    R[2][0] = 2 * (x * z - r * y);     R[2][1] = 2 * (y * z + r * x);     R[2][2] = 1 - 2 * (x * x + y * y);
    float L[3][3];
    for (int k = 0; k < 3; k++) sd[k] = scale_modifier * s[k];
    for (int a = 0; a < 3; a++)
        for (int k = 0; k < 3; k++) L[a][k] = R[a][k] * sd[k];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) Sg[a][b] = (L[a][0] * L[b][0] + L[a][1] * L[b][1]) + L[a][2] * L[b][2];
}

// vm: the view's world_view_transform as stored (the matrix transposed): M[i][k] = vm[4k + i]; mean: the Gaussian's centre;
// W, H, tanx, tany: the view's own size and half-field tangents.  l1 >= l2: the eigenvalues of the reference's 2D covariance
// (R J)^T Sigma^T (R J) with the 0.3 px^2 low-pass, the discriminant guarded by max(0.1, .) -- variances in px^2, BEFORE any
// square root.
__device__ __forceinline__ void ewa_lambdas(const float Sg[3][3], const float* __restrict__ vm, const float* __restrict__ mean,
                                            int W, int H, float tanx, float tany, float& l1, float& l2)
{
    const float px = mean[0], py = mean[1], pz = mean[2];
    float t[3];
    for (int i = 0; i < 3; i++) t[i] = ((vm[i] * px + vm[4 + i] * py) + vm[8 + i] * pz) + vm[12 + i] * 1.0f;
    const float fx = (float)W / (2.0f * tanx), fy = (float)H / (2.0f * tany);
    const float tz = t[2];
    const float tx = fminf(fmaxf(t[0] / tz, -1.3f * tanx), 1.3f * tanx) * tz;
    const float ty = fminf(fmaxf(t[1] / tz, -1.3f * tany), 1.3f * tany) * tz;
    const float Jm[3][3] = { { fx / tz, 0.0f, -(fx * tx) / (tz * tz) }, { 0.0f, fy / tz, -(fy * ty) / (tz * tz) }, { 0.0f, 0.0f, 0.0f } };
    float T[3][3], A[3][3], cov[2][2];
    for (int a = 0; a < 3; a++)
        for (int c = 0; c < 3; c++) T[a][c] = (vm[a] * Jm[0][c] + vm[4 + a] * Jm[1][c]) + vm[8 + a] * Jm[2][c];
    for (int a = 0; a < 3; a++)      // A = T^T Sigma^T
        for (int b = 0; b < 3; b++) A[a][b] = (T[0][a] * Sg[b][0] + T[1][a] * Sg[b][1]) + T[2][a] * Sg[b][2];
    for (int a = 0; a < 2; a++)      // cov = A T
        for (int c = 0; c < 2; c++) cov[a][c] = (A[a][0] * T[0][c] + A[a][1] * T[1][c]) + A[a][2] * T[2][c];
    const float cx = cov[0][0] + 0.3f, cy = cov[0][1], cz = cov[1][1] + 0.3f;
    const float det = cx * cz - cy * cy;
    const float mid = 0.5f * (cx + cz);
    const float root = sqrtf(fmaxf(mid * mid - det, 0.1f));
    l1 = mid + root;
    l2 = mid - root;
}

}  // namespace sks
