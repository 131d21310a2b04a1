// sks_triangulate.hip -- batched DLT triangulation (reference: triangulation.py:122-150) for MI355X.
//
// The reference solves, per joint, the 2V x 4 homogeneous system whose rows are x * P[2] - P[0] and y * P[2] - P[1] of
// every view (view-major) by np.linalg.svd and returns the right singular vector of the smallest singular value, divided
// by its fourth component.  Here every (frame, joint) system is solved in float64 by ONE-SIDED (Hestenes) Jacobi on the
// columns of A itself: the columns differ by 3-4 orders of magnitude (focal length against focal length x distance), so
// A^T A is never formed (squaring that loses the two-view case, MEASUREMENTS.md "Batched DLT").
//
// Layout: lane = view.  A system takes W = the next power of two >= V adjacent lanes of a wavefront (64 / W systems
// per wavefront, 4 wavefronts per workgroup); a lane holds its view's two rows of A (8 doubles) and a replica of the
// 4 x 4 accumulated rotations.  The three dot products of a column pair are a butterfly over the W lanes: fp addition
// commutes, so after stage m lane i and lane i ^ m hold the same bits, every lane of a system ends with the same sum,
// and the order of additions depends on V alone -- never on N, on where the system sits in the batch or on the launch
// geometry.  (Lanes >= V and masked-out detections hold zero rows: x + 0 == x, and zero rows leave the right singular
// vectors those of the kept views' system.)  Six column pairs per sweep in a fixed order; a pair with
// |c| <= eps * sqrt(a * b) is left alone; a wavefront stops sweeping when none of its systems rotated, at most
// TRI_MAX_SWEEPS times.  A converged system's further sweeps recompute the same sums and rotate nothing, so its result
// does not depend on its neighbours in the wavefront.  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"

namespace {

constexpr int TRI_MAX_SWEEPS = 16;      // measured need: 5-7 (tests/test_triangulate_cpu.py restates the sweep)
constexpr int TRI_WAVES = 4;            // wavefronts per workgroup

__device__ __forceinline__ double group_sum(double x, int W)
{
    for (int m = 1; m < W; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// rotates columns p, q of the lane's two rows and of the accumulated right factor
__device__ __forceinline__ void rotate(double& xp, double& xq, double cs, double sn)
{
    const double p = cs * xp - sn * xq, q = sn * xp + cs * xq;
    xp = p; xq = q;
}

template <typename T2D>
__global__ void __launch_bounds__(64 * TRI_WAVES)
k_triangulate(int total /* N * J */, int V, int J, int W, const double* __restrict__ proj, size_t rig_stride,
              const T2D* __restrict__ poses_2d, const unsigned char* __restrict__ valid, float* __restrict__ xyz,
              double* __restrict__ xyzw, int* __restrict__ n_used)
{
    const int lane = threadIdx.x & 63;
    const int per_wave = 64 / W;
    const int sys = (blockIdx.x * TRI_WAVES + (threadIdx.x >> 6)) * per_wave + lane / W;
    const int v = lane & (W - 1);
    const bool live = sys < total && v < V;
    const int n = live ? sys / J : 0, j = live ? sys - n * J : 0;
    bool use = live;
    if (live && valid) use = valid[((size_t)n * V + v) * J + j] != 0;
    // this view's two rows of A
    double r0[4] = {0.0, 0.0, 0.0, 0.0}, r1[4] = {0.0, 0.0, 0.0, 0.0};
    if (use) {
        const double* Pv = proj + (size_t)n * rig_stride + (size_t)v * 12;
        const T2D* d = poses_2d + (((size_t)n * V + v) * J + j) * 2;
        const double x = (double)d[0], y = (double)d[1];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            r0[k] = x * Pv[8 + k] - Pv[k];
            r1[k] = y * Pv[8 + k] - Pv[4 + k];
        }
    }
    const int used = (int)group_sum(use ? 1.0 : 0.0, W);      // (exact: a count <= 64)
    double R[4][4];                                            // accumulated rotations, R[row][column]
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) R[a][b] = a == b ? 1.0 : 0.0;

    for (int sweep = 0; sweep < TRI_MAX_SWEEPS; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++) {
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double a = group_sum(r0[p] * r0[p] + r1[p] * r1[p], W);
                const double b = group_sum(r0[q] * r0[q] + r1[q] * r1[q], W);
                const double c = group_sum(r0[p] * r0[q] + r1[p] * r1[q], W);
                if (!(fabs(c) <= DBL_EPSILON * sqrt(a * b))) {      // (a NaN rotates: it spreads and the cap ends it)
                    rotated = true;
                    const double zeta = (b - a) / (2.0 * c);
                    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                    rotate(r0[p], r0[q], cs, sn);
                    rotate(r1[p], r1[q], cs, sn);
#pragma unroll
                    for (int k = 0; k < 4; k++) rotate(R[k][p], R[k][q], cs, sn);
                }
            }
        }
        if (!__any(rotated)) break;
    }
    // the column of the smallest singular value (ties: the lowest index), divided by its fourth component
    double best = group_sum(r0[0] * r0[0] + r1[0] * r1[0], W);
    double X[4] = {R[0][0], R[1][0], R[2][0], R[3][0]};
#pragma unroll
    for (int k = 1; k < 4; k++) {
        const double s = group_sum(r0[k] * r0[k] + r1[k] * r1[k], W);
        if (s < best) {
            best = s;
#pragma unroll
            for (int i = 0; i < 4; i++) X[i] = R[i][k];
        }
    }
    if (sys >= total || v != 0) return;
    double o[4];
    if (used < 2) {
        o[0] = o[1] = o[2] = o[3] = (double)NAN;      // no solution: one view leaves a line, none leaves everything
    } else {
        o[0] = X[0] / X[3]; o[1] = X[1] / X[3]; o[2] = X[2] / X[3]; o[3] = X[3] / X[3];
    }
    if (xyz) {
        float* d = xyz + (size_t)sys * 3;
        d[0] = (float)o[0]; d[1] = (float)o[1]; d[2] = (float)o[2];
    }
    if (xyzw) {
        double* d = xyzw + (size_t)sys * 4;
        d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; d[3] = o[3];
    }
    if (n_used) n_used[sys] = used;
}

}  // namespace

extern "C" int sks_triangulate(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_2d,
                               const double* poses_2d_f64, const unsigned char* valid, float* xyz, double* xyzw,
                               int* n_used, void* stream)
{
    if (N < 1 || J < 1) return fail2(-1, "triangulate: N and J must be at least 1");
    if (V < 1 || V > SKS_MAX_VIEWS) return fail2(-1, "triangulate: %d views, a system takes 1 .. %d (SKS_MAX_VIEWS)", V, SKS_MAX_VIEWS);
    if ((long long)N * J > 0x7fffffffLL - 64 * TRI_WAVES) return fail2(-1, "triangulate: N x J = %lld systems are too many for one call", (long long)N * J);
    if (rig_stride != 0 && rig_stride != (size_t)V * 12) return fail2(-1, "triangulate: rig_stride must be 0 (one rig) or V * 12 (one per frame)");
    if (!proj) return fail2(-2, "triangulate: missing projection matrices");
    if (!poses_2d == !poses_2d_f64) return fail2(-2, "triangulate: give the detections as float (poses_2d) or as double (poses_2d_f64), not both");
    if (!xyz && !xyzw) return fail2(-2, "triangulate: at least one of xyz / xyzw");
    int W = 1;
    while (W < V) W <<= 1;
    const int total = N * J, per_block = TRI_WAVES * (64 / W);
    const dim3 grid((total + per_block - 1) / per_block), block(64 * TRI_WAVES);
    if (poses_2d)
        hipLaunchKernelGGL(k_triangulate<float>, grid, block, 0, (hipStream_t)stream, total, V, J, W, proj, rig_stride, poses_2d,
                           valid, xyz, xyzw, n_used);
    else
        hipLaunchKernelGGL(k_triangulate<double>, grid, block, 0, (hipStream_t)stream, total, V, J, W, proj, rig_stride,
                           poses_2d_f64, valid, xyz, xyzw, n_used);
    HIP_TRY2(hipGetLastError());
    return 0;
}
