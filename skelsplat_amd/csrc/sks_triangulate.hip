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
//
// sks_triangulate_robust puts k_consensus (below, lane = two-view hypothesis) in front of the same k_triangulate: it writes
// the mask of views that agree, and the DLT then runs with that mask as `valid`.
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

// ---------------------------------------------------------------------------------------------------------------------
// Exhaustive two-view consensus in front of the DLT (sks_triangulate_robust): which of a joint's kept views agree.
//
// Layout: lane = hypothesis (a pair a < b of views, numbered in lexicographic order).  A system takes G = the next power
// of two >= min(V (V - 1) / 2, 64) adjacent lanes (64 / G systems per wavefront, 4 wavefronts per workgroup; V <= 2 has
// nothing to test and takes one lane); with more than G pairs the lanes loop over passes of G hypotheses and each keeps
// the best of its own.  A hypothesis' 4 x 4 system is solved inside its lane by the one-sided Jacobi of k_triangulate --
// same pair order, same threshold, same cap, no cross-lane sums --, so its X depends on its four rows alone; a lane whose
// pair is not among the kept views holds zero rows and never rotates.  The system's projection matrices, detections and
// kept flags are staged in LDS (V x 15 doubles), where the reprojection loop reads them as broadcasts.  The lanes of a
// system then meet in a butterfly whose comparison is the full order (count descending, sum ascending, pair index
// ascending): a total order on distinct indices, so the winner depends neither on G nor on which lane held it.
constexpr int CON_STRIDE = 15;          // doubles per staged view: P (12), x, y, kept
constexpr int CON_MAX_STAGED = 64;      // staged views per wavefront: (64 / G) x V is at most 64 for every V >= 3

__host__ __device__ inline int consensus_group(int V)
{
    const int pairs = V * (V - 1) / 2;
    int G = 1;
    while (G < pairs && G < 64) G <<= 1;
    return G;
}

struct Best {
    int c;                      // inliers; -1: no hypothesis
    int h;                      // pair index
    double s;                   // the inliers' reprojection errors, added in ascending view order
    unsigned long long set;     // the inliers
};

__device__ __forceinline__ bool better(const Best& x, const Best& y)      // x before y in (-c, s, h)
{
    if (x.c != y.c) return x.c > y.c;
    if (x.s != y.s) return x.s < y.s;
    return x.h < y.h;
}

template <typename T2D>
__global__ void __launch_bounds__(64 * TRI_WAVES)
k_consensus(int total /* N * J */, int V, int J, int G, const double* __restrict__ proj, size_t rig_stride,
            const T2D* __restrict__ poses_2d, const unsigned char* __restrict__ valid, double reject_px, int min_inliers,
            unsigned char* __restrict__ inliers, int* __restrict__ n_consensus)
{
    __shared__ double staged[TRI_WAVES][CON_MAX_STAGED * CON_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per_wave = 64 / G;
    const int slot = lane / G, g = lane & (G - 1);
    const int sys = (blockIdx.x * TRI_WAVES + wave) * per_wave + slot;
    const bool live = sys < total;
    const int n = live ? sys / J : 0, j = live ? sys - n * J : 0;
    const bool test = V >= 3;               // (uniform: V <= 2 stages nothing, its G = 1 would not fit the LDS either)
    double* mine = staged[wave] + (test ? slot * V * CON_STRIDE : 0);
    if (live && test) {
        for (int i = g; i < V * CON_STRIDE; i += G) {
            const int v = i / CON_STRIDE, k = i - v * CON_STRIDE;
            double x;
            if (k < 12) x = proj[(size_t)n * rig_stride + (size_t)v * 12 + k];
            else if (k < 14) x = (double)poses_2d[(((size_t)n * V + v) * J + j) * 2 + (k - 12)];
            else x = !valid || valid[((size_t)n * V + v) * J + j] != 0 ? 1.0 : 0.0;
            mine[i] = x;
        }
    }
    __syncthreads();
    unsigned long long kept = 0;
    if (live) {
        if (test) {
            for (int v = 0; v < V; v++)
                if (mine[v * CON_STRIDE + 14] != 0.0) kept |= 1ull << v;
        } else {
            for (int v = 0; v < V; v++)
                if (!valid || valid[((size_t)n * V + v) * J + j] != 0) kept |= 1ull << v;
        }
    }
    const int n_kept = __popcll(kept);
    const int pairs = V * (V - 1) / 2;
    Best best = {-1, 0x7fffffff, 0.0, 0ull};
    if (test) {
        // (uniform trip count: the shuffles of __any below want every lane of the wavefront in every pass)
        for (int h0 = 0; h0 < pairs; h0 += G) {
            const int h = h0 + g;
            int a = 0, b = 0;
            {
                int rem = h;
                while (a < V - 1 && rem >= V - 1 - a) { rem -= V - 1 - a; a++; }
                b = min(a + 1 + rem, V - 1);        // (h >= pairs: no hypothesis, any view will do)
            }
            const bool hyp = n_kept >= 3 && h < pairs && ((kept >> a) & 1ull) && ((kept >> b) & 1ull);
            double A[4][4], R[4][4];
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int k = 0; k < 4; k++) { A[r][k] = 0.0; R[r][k] = r == k ? 1.0 : 0.0; }
            if (hyp) {
                const double* Pa = mine + a * CON_STRIDE;
                const double* Pb = mine + b * CON_STRIDE;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    A[0][k] = Pa[12] * Pa[8 + k] - Pa[k];
                    A[1][k] = Pa[13] * Pa[8 + k] - Pa[4 + k];
                    A[2][k] = Pb[12] * Pb[8 + k] - Pb[k];
                    A[3][k] = Pb[13] * Pb[8 + k] - Pb[4 + k];
                }
            }
            for (int sweep = 0; sweep < TRI_MAX_SWEEPS; sweep++) {
                bool rotated = false;
#pragma unroll
                for (int p = 0; p < 3; p++) {
#pragma unroll
                    for (int q = p + 1; q < 4; q++) {
                        const double na = ((A[0][p] * A[0][p] + A[1][p] * A[1][p]) + A[2][p] * A[2][p]) + A[3][p] * A[3][p];
                        const double nb = ((A[0][q] * A[0][q] + A[1][q] * A[1][q]) + A[2][q] * A[2][q]) + A[3][q] * A[3][q];
                        const double c = ((A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q]) + A[3][p] * A[3][q];
                        if (!(fabs(c) <= DBL_EPSILON * sqrt(na * nb))) {      // (a NaN rotates until the cap, as in k_triangulate)
                            rotated = true;
                            const double zeta = (nb - na) / (2.0 * c);
                            const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                            const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                rotate(A[r][p], A[r][q], cs, sn);
                                rotate(R[r][p], R[r][q], cs, sn);
                            }
                        }
                    }
                }
                if (!__any(rotated)) break;
            }
            double least = ((A[0][0] * A[0][0] + A[1][0] * A[1][0]) + A[2][0] * A[2][0]) + A[3][0] * A[3][0];
            double X[4] = {R[0][0], R[1][0], R[2][0], R[3][0]};
#pragma unroll
            for (int k = 1; k < 4; k++) {
                const double s = ((A[0][k] * A[0][k] + A[1][k] * A[1][k]) + A[2][k] * A[2][k]) + A[3][k] * A[3][k];
                if (s < least) {
                    least = s;
#pragma unroll
                    for (int i = 0; i < 4; i++) X[i] = R[i][k];
                }
            }
            if (hyp) {
                const double w = X[3];
#pragma unroll
                for (int i = 0; i < 4; i++) X[i] /= w;
                Best cur = {0, h, 0.0, 0ull};
                for (int v = 0; v < V; v++) {
                    if (!((kept >> v) & 1ull)) continue;
                    const double* Pv = mine + v * CON_STRIDE;
                    double u[3];
#pragma unroll
                    for (int r = 0; r < 3; r++)
                        u[r] = ((Pv[4 * r] * X[0] + Pv[4 * r + 1] * X[1]) + Pv[4 * r + 2] * X[2]) + Pv[4 * r + 3] * X[3];
                    const double e = hypot(u[0] / u[2] - Pv[12], u[1] / u[2] - Pv[13]);
                    if (u[2] > 0.0 && e <= reject_px) {         // (false for a NaN on either side)
                        cur.c++;
                        cur.s += e;
                        cur.set |= 1ull << v;
                    }
                }
                if (better(cur, best)) best = cur;
            }
        }
        for (int m = 1; m < G; m <<= 1) {
            Best other;
            other.c = __shfl_xor(best.c, m, 64);
            other.h = __shfl_xor(best.h, m, 64);
            other.s = __shfl_xor(best.s, m, 64);
            other.set = (unsigned long long)__shfl_xor((long long)best.set, m, 64);
            if (better(other, best)) best = other;
        }
    }
    if (!live) return;
    const bool agreed = n_kept >= 3 && best.c >= min_inliers;
    const unsigned long long out = agreed ? best.set : kept;
    for (int v = g; v < V; v += G) inliers[((size_t)n * V + v) * J + j] = (unsigned char)((out >> v) & 1ull);
    if (g == 0 && n_consensus) n_consensus[sys] = n_kept >= 3 ? best.c : n_kept;
}

// k_triangulate for the checked arguments of sks_triangulate / sks_triangulate_robust
int launch_dlt(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_2d, const double* poses_2d_f64,
               const unsigned char* valid, float* xyz, double* xyzw, int* n_used, hipStream_t stream)
{
    int W = 1;
    while (W < V) W <<= 1;
    const int total = N * J, per_block = TRI_WAVES * (64 / W);
    const dim3 grid((total + per_block - 1) / per_block), block(64 * TRI_WAVES);
    if (poses_2d)
        hipLaunchKernelGGL(k_triangulate<float>, grid, block, 0, stream, total, V, J, W, proj, rig_stride, poses_2d, valid, xyz,
                           xyzw, n_used);
    else
        hipLaunchKernelGGL(k_triangulate<double>, grid, block, 0, stream, total, V, J, W, proj, rig_stride, poses_2d_f64, valid,
                           xyz, xyzw, n_used);
    HIP_TRY2(hipGetLastError());
    return 0;
}

int check_dlt(const char* who, int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_2d,
              const double* poses_2d_f64, const float* xyz, const double* xyzw)
{
    if (N < 1 || J < 1) return fail2(-1, "%s: N and J must be at least 1", who);
    if (V < 1 || V > SKS_MAX_VIEWS) return fail2(-1, "%s: %d views, a system takes 1 .. %d (SKS_MAX_VIEWS)", who, V, SKS_MAX_VIEWS);
    if ((long long)N * J > 0x7fffffffLL - 64 * TRI_WAVES) return fail2(-1, "%s: N x J = %lld systems are too many for one call", who, (long long)N * J);
    if (rig_stride != 0 && rig_stride != (size_t)V * 12) return fail2(-1, "%s: rig_stride must be 0 (one rig) or V * 12 (one per frame)", who);
    if (!proj) return fail2(-2, "%s: missing projection matrices", who);
    if (!poses_2d == !poses_2d_f64) return fail2(-2, "%s: give the detections as float (poses_2d) or as double (poses_2d_f64), not both", who);
    if (!xyz && !xyzw) return fail2(-2, "%s: at least one of xyz / xyzw", who);
    return 0;
}

}  // namespace

extern "C" int sks_triangulate(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_2d,
                               const double* poses_2d_f64, const unsigned char* valid, float* xyz, double* xyzw,
                               int* n_used, void* stream)
{
    if (int rc = check_dlt("triangulate", N, V, J, proj, rig_stride, poses_2d, poses_2d_f64, xyz, xyzw)) return rc;
    return launch_dlt(N, V, J, proj, rig_stride, poses_2d, poses_2d_f64, valid, xyz, xyzw, n_used, (hipStream_t)stream);
}

extern "C" int sks_triangulate_robust(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_2d,
                                      const double* poses_2d_f64, const unsigned char* valid, double reject_px,
                                      int min_inliers, unsigned char* inliers, int* n_consensus, float* xyz, double* xyzw,
                                      int* n_used, void* stream)
{
    if (int rc = check_dlt("triangulate_robust", N, V, J, proj, rig_stride, poses_2d, poses_2d_f64, xyz, xyzw)) return rc;
    if (!(reject_px > 0.0) || !isfinite(reject_px)) return fail2(-1, "triangulate_robust: reject_px must be finite and > 0 pixels, got %g", reject_px);
    if (min_inliers < 2 || min_inliers > SKS_MAX_VIEWS) return fail2(-1, "triangulate_robust: min_inliers = %d, a consensus takes 2 .. %d views", min_inliers, SKS_MAX_VIEWS);
    if (!inliers) return fail2(-2, "triangulate_robust: missing inliers (N,V,J), the mask the refit reads");
    const int G = consensus_group(V);
    const int total = N * J, per_block = TRI_WAVES * (64 / G);
    const dim3 grid((total + per_block - 1) / per_block), block(64 * TRI_WAVES);
    if (poses_2d)
        hipLaunchKernelGGL(k_consensus<float>, grid, block, 0, (hipStream_t)stream, total, V, J, G, proj, rig_stride, poses_2d, valid,
                           reject_px, min_inliers, inliers, n_consensus);
    else
        hipLaunchKernelGGL(k_consensus<double>, grid, block, 0, (hipStream_t)stream, total, V, J, G, proj, rig_stride, poses_2d_f64,
                           valid, reject_px, min_inliers, inliers, n_consensus);
    HIP_TRY2(hipGetLastError());
    return launch_dlt(N, V, J, proj, rig_stride, poses_2d, poses_2d_f64, inliers, xyz, xyzw, n_used, (hipStream_t)stream);
}
