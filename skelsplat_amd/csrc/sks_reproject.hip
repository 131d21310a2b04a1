// sks_reproject.hip -- the reprojection error of a multi-view estimate, measured and minimised, for MI355X: the distance in pixels
// between a joint projected into a view and that view's detection (reference: compute_reprojection_error,
// dataset_tools/h36m/compute_initial_guess.py:23-79), its means per joint, per view and per frame, its means over a sequence, and
// the triangulation that minimises it from a start (Hartley & Zisserman's "gold standard" next to sks_triangulate's DLT).
//
// One projection routine (project) serves every kernel here: u = P_v [X; 1] added in column order 0..3, x = u0 / u2, y = u1 / u2,
// float64, no test for points behind the camera.  The file is compiled without FMA contraction like the rest of the library, so
// a pair's numbers are the same bits wherever they are computed.
//
// k_reproject.  Layout: one wavefront per frame, 4 wavefronts per workgroup, nothing handed from one wavefront to another.
//   pass 1: the lanes stride over the (v, j) pairs, view-major, and write uv / err / in_front.
//   pass 2: lane l takes joints l, l + 64, ... and adds each joint's kept views in ascending view order: per_joint, n_used.
//   pass 3: lane v takes view v (V <= 64) and adds its kept joints in ascending joint order: S_v, C_v, per_view = S_v / C_v; every
//           lane then adds S_0 .. S_{V-1} and C_0 .. C_{V-1} in ascending view order, read by shuffles: per_frame = S / C, the
//           mean over the kept pairs view-major, grouped by view.
//   Passes 2 and 3 RECOMPUTE a pair's error instead of parking it in LDS: the same routine gives the same bits, a pair is some
//   thirty flops against a frame that is bound by launch latency, and V x J has no bound that an LDS array would need.  A pass
//   whose outputs are all NULL is skipped.  No LDS, no atomics, no scratch; a frame's outputs depend on its own inputs, V and J.
//
// k_eval_reprojection.  Layout: one workgroup of 256 threads per output row (0: all frames, 1 + g: group g), as k_eval_sequence.
//   The row's 1 + V + J columns are made one after the other: thread t takes frames t, t + 256, ... in index order, adds the
//   column's non-NaN entries of each frame in index order (all of them view-major / the view's joints / the joint's views), and
//   the 256 partial sums and counts meet in the same fixed tree.  mean = sum / count, NaN over nothing.
//
// k_refine.  Layout: k_triangulate's, lane = view.  A system (one joint of one frame) takes W = the next power of two >= V
//   adjacent lanes (64 / W systems per wavefront, 4 wavefronts per workgroup).  A lane holds its view's P, its detection and a
//   replica of X, the cost, lambda and the flags.  One trip needs 10 sums -- 6 of A = sum_v w_v J_v^T J_v, 3 of g = sum_v w_v J_v^T
//   r_v, and the cost at the trial point -- as butterflies over the W lanes: every lane of a system ends with the same bits and the
//   order of additions depends on V alone.  (Lanes >= V and left-out views add zeros.)  The 3 x 3 system
//   (A + lambda diag A) delta = -g is solved replicated in every lane by CHOLESKY (A is a Gram matrix; a pivot that is not > 0
//   rejects the trip).  A view with u2 <= 0 at the trial point adds +inf to the trial cost, so "every kept view in front" is
//   part of the one comparison trial < cost and needs no sum of its own.
//   Constants: lambda starts at REFINE_LAMBDA0 = 1e-3, is multiplied by REFINE_LAMBDA_DOWN = 0.1 when a trial is accepted and by
//   REFINE_LAMBDA_UP = 10 when it is rejected; a joint stops after an accepted trip with cost - trial < REFINE_STOP_FRACTION =
//   1e-6 x cost (scale-free: stated in the cost, not in world units; the step that fires it has been taken, so the result sits one
//   Gauss-Newton contraction beyond it), or at max_iters.  iters counts a joint's trips, accepted or not.  A stopped joint's
//   later trips (its wavefront runs until none of its systems is active) compute and commit nothing, so its result does not
//   depend on its neighbours in the wavefront.  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"

namespace {

constexpr int REPROJ_WAVES = 4;             // wavefronts per workgroup (k_reproject, k_refine)
constexpr int EVAL_THREADS = 256;
constexpr double REFINE_LAMBDA0 = 1e-3;
constexpr double REFINE_LAMBDA_DOWN = 0.1;
constexpr double REFINE_LAMBDA_UP = 10.0;
constexpr double REFINE_STOP_FRACTION = 1e-6;

struct Pixel { double x, y, depth; };

// the one projection routine: P (3,4) row-major, [X; 1]
__device__ __forceinline__ Pixel project(const double* __restrict__ P, double X0, double X1, double X2)
{
    const double u0 = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3];
    const double u1 = ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7];
    const double u2 = ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11];
    Pixel p;
    p.x = u0 / u2; p.y = u1 / u2; p.depth = u2;
    return p;
}

__device__ __forceinline__ double pixel_error(const Pixel& p, double dx_, double dy_)
{
    const double dx = p.x - dx_, dy = p.y - dy_;
    return sqrt(dx * dx + dy * dy);
}

// Pair (v, j) of one frame (every pointer is the frame's): the pixel, and the error or NaN when the pair is left out.
template <typename T3D, typename T2D>
__device__ __forceinline__ double pair_error(const double* __restrict__ Pn, const T3D* __restrict__ X, const T2D* __restrict__ det,
                                             const unsigned char* __restrict__ valid, int J, int v, int j, Pixel& px)
{
    const double X0 = (double)X[3 * j], X1 = (double)X[3 * j + 1], X2 = (double)X[3 * j + 2];
    px = project(Pn + (size_t)v * 12, X0, X1, X2);
    const size_t at = (size_t)v * J + j;
    if (!det || (valid && valid[at] == 0) || isnan(X0) || isnan(X1) || isnan(X2)) return (double)NAN;
    const double dx = (double)det[2 * at], dy = (double)det[2 * at + 1];
    if (!isfinite(dx) || !isfinite(dy)) return (double)NAN;
    return pixel_error(px, dx, dy);
}

template <typename T3D, typename T2D>
__global__ void __launch_bounds__(64 * REPROJ_WAVES)
k_reproject(int N, int V, int J, const double* __restrict__ proj, size_t rig_stride, const T3D* __restrict__ xyz,
            const T2D* __restrict__ poses_2d, const unsigned char* __restrict__ valid, double* __restrict__ uv,
            double* __restrict__ err, unsigned char* __restrict__ in_front, double* __restrict__ per_joint,
            double* __restrict__ per_view, double* __restrict__ per_frame, int* __restrict__ n_used)
{
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * REPROJ_WAVES + (threadIdx.x >> 6);
    if (f >= N) return;                                     // (a whole wavefront: nothing below waits for another one)
    const size_t pairs = (size_t)V * J;
    const double* Pn = proj + (size_t)f * rig_stride;
    const T3D* X = xyz + (size_t)f * J * 3;
    const T2D* det = poses_2d ? poses_2d + (size_t)f * pairs * 2 : nullptr;
    const unsigned char* ok = valid ? valid + (size_t)f * pairs : nullptr;
    Pixel px;
    if (uv || err || in_front) {
        for (int i = lane; i < (int)pairs; i += 64) {
            const int v = i / J, j = i - v * J;
            const double e = pair_error(Pn, X, det, ok, J, v, j, px);
            const size_t at = (size_t)f * pairs + i;
            if (uv) { uv[2 * at] = px.x; uv[2 * at + 1] = px.y; }
            if (err) err[at] = e;
            if (in_front) in_front[at] = px.depth > 0.0 ? 1 : 0;
        }
    }
    if (per_joint || n_used) {
        for (int j = lane; j < J; j += 64) {
            double s = 0.0;
            int c = 0;
            for (int v = 0; v < V; v++) {
                const double e = pair_error(Pn, X, det, ok, J, v, j, px);
                if (e == e) { s += e; c++; }
            }
            if (per_joint) per_joint[(size_t)f * J + j] = s / (double)c;        // (nothing kept: 0 / 0 = NaN)
            if (n_used) n_used[(size_t)f * J + j] = c;
        }
    }
    if (per_view || per_frame) {
        double s = 0.0;
        int c = 0;
        if (lane < V) {
            for (int j = 0; j < J; j++) {
                const double e = pair_error(Pn, X, det, ok, J, lane, j, px);
                if (e == e) { s += e; c++; }
            }
            if (per_view) per_view[(size_t)f * V + lane] = s / (double)c;
        }
        double S = 0.0;
        int C = 0;
        for (int v = 0; v < V; v++) {
            S += __shfl(s, v, 64);
            C += __shfl(c, v, 64);
        }
        if (lane == 0 && per_frame) per_frame[f] = S / (double)C;
    }
}

__global__ void __launch_bounds__(EVAL_THREADS)
k_eval_reprojection(int N, int V, int J, const double* __restrict__ err, const int* __restrict__ group_ids,
                    double* __restrict__ out)
{
    __shared__ double s_sum[EVAL_THREADS];
    __shared__ long long s_cnt[EVAL_THREADS];
    const int tid = threadIdx.x, g = (int)blockIdx.x - 1;
    const int cols = 1 + V + J;
    const size_t pairs = (size_t)V * J;
    for (int col = 0; col < cols; col++) {
        // the column's entries of a frame: first, count, stride
        const size_t first = col == 0 ? 0 : col <= V ? (size_t)(col - 1) * J : (size_t)(col - 1 - V);
        const size_t count = col == 0 ? pairs : col <= V ? (size_t)J : (size_t)V;
        const size_t stride = col > V ? (size_t)J : 1;
        double s = 0.0;
        long long c = 0;
        for (int i = tid; i < N; i += EVAL_THREADS) {
            if (g >= 0 && group_ids[i] != g) continue;
            const double* e = err + (size_t)i * pairs + first;
            for (size_t k = 0; k < count; k++) {
                const double x = e[k * stride];
                if (x == x) { s += x; c++; }
            }
        }
        s_sum[tid] = s; s_cnt[tid] = c;
        for (int o = EVAL_THREADS / 2; o > 0; o >>= 1) {
            __syncthreads();
            if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_cnt[tid] += s_cnt[tid + o]; }
        }
        if (tid == 0) out[(size_t)blockIdx.x * cols + col] = s_sum[0] / (double)s_cnt[0];      // (an empty row: 0 / 0 = NaN)
        __syncthreads();
    }
}

__device__ __forceinline__ double group_sum(double x, int W)
{
    for (int m = 1; m < W; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// what a lane keeps of its view at a point: the pixel, the residual, its norm
struct ViewAt { Pixel px; double dx, dy, e; };

__device__ __forceinline__ ViewAt view_at(const double* P, double x, double y, double X0, double X1, double X2)
{
    ViewAt a;
    a.px = project(P, X0, X1, X2);
    a.dx = a.px.x - x; a.dy = a.px.y - y;
    a.e = sqrt(a.dx * a.dx + a.dy * a.dy);
    return a;
}

__device__ __forceinline__ double rho(double e, double huber)
{
    return huber > 0.0 && !(e <= huber) ? 2.0 * huber * e - huber * huber : e * e;
}

template <typename T3D, typename T2D>
__global__ void __launch_bounds__(64 * REPROJ_WAVES)
k_refine(int total /* N * J */, int V, int J, int W, const double* __restrict__ proj, size_t rig_stride,
         const T2D* __restrict__ poses_2d, const unsigned char* __restrict__ valid, const T3D* xyz0 /* may alias xyz */,
         double huber, int max_iters, float* xyz, double* xyz_f64, double* __restrict__ cost_out, int* __restrict__ iters_out)
{
    const int lane = threadIdx.x & 63;
    const int per_wave = 64 / W;
    const int sys = (blockIdx.x * REPROJ_WAVES + (threadIdx.x >> 6)) * per_wave + lane / W;
    const int v = lane & (W - 1);
    const bool live = sys < total && v < V;
    const int n = live ? sys / J : 0, j = live ? sys - n * J : 0;
    double P[12], x = 0.0, y = 0.0;
#pragma unroll
    for (int k = 0; k < 12; k++) P[k] = 0.0;
    bool use = live;
    if (live) {
        const size_t at = ((size_t)n * V + v) * J + j;
        const double* Pv = proj + (size_t)n * rig_stride + (size_t)v * 12;
#pragma unroll
        for (int k = 0; k < 12; k++) P[k] = Pv[k];
        x = (double)poses_2d[2 * at]; y = (double)poses_2d[2 * at + 1];
        use = (!valid || valid[at] != 0) && isfinite(x) && isfinite(y);
    }
    double X[3] = {0.0, 0.0, 0.0};
    if (sys < total) {
        const T3D* s = xyz0 + (size_t)sys * 3;
        X[0] = (double)s[0]; X[1] = (double)s[1]; X[2] = (double)s[2];
    }
    const int kept = (int)group_sum(use ? 1.0 : 0.0, W);          // (exact: a count <= 64)
    ViewAt at = view_at(P, x, y, X[0], X[1], X[2]);
    const int behind = (int)group_sum(use && !(at.px.depth > 0.0) ? 1.0 : 0.0, W);
    double cost = group_sum(use ? rho(at.e, huber) : 0.0, W);
    const double cost0 = cost;
    bool active = sys < total && kept >= 2 && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && behind == 0;
    double lambda = REFINE_LAMBDA0;
    int iters = 0;
    for (int trip = 0; trip < max_iters; trip++) {
        if (!__any(active)) break;
        // this view's share of the normal equations at X
        const double w = use ? (huber > 0.0 && !(at.e <= huber) ? huber / at.e : 1.0) : 0.0;
        double Jx[3], Jy[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Jx[k] = (P[k] - at.px.x * P[8 + k]) / at.px.depth;
            Jy[k] = (P[4 + k] - at.px.y * P[8 + k]) / at.px.depth;
        }
        double a[6], g[3];          // a: 00 10 11 20 21 22
        {
            int t = 0;
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c <= r; c++) a[t++] = group_sum(use ? w * (Jx[r] * Jx[c] + Jy[r] * Jy[c]) : 0.0, W);
                g[r] = group_sum(use ? w * (Jx[r] * at.dx + Jy[r] * at.dy) : 0.0, W);
            }
        }
        // (A + lambda diag A) delta = -g by Cholesky, replicated in every lane
        const double m00 = a[0] + lambda * a[0], m11 = a[2] + lambda * a[2], m22 = a[5] + lambda * a[5];
        const double l00 = sqrt(m00), l10 = a[1] / l00, l20 = a[3] / l00;
        const double d1 = m11 - l10 * l10, l11 = sqrt(d1), l21 = (a[4] - l20 * l10) / l11;
        const double d2 = (m22 - l20 * l20) - l21 * l21, l22 = sqrt(d2);
        const bool solved = m00 > 0.0 && d1 > 0.0 && d2 > 0.0;
        const double y0 = -g[0] / l00, y1 = (-g[1] - l10 * y0) / l11, y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22;
        const double e2 = y2 / l22, e1 = (y1 - l21 * e2) / l11, e0 = ((y0 - l10 * e1) - l20 * e2) / l00;
        const double T0 = X[0] + e0, T1 = X[1] + e1, T2 = X[2] + e2;
        const ViewAt trial = view_at(P, x, y, T0, T1, T2);
        // a kept view behind its camera at the trial point makes the trial cost +inf: never strictly smaller
        const double tcost = group_sum(use ? (trial.px.depth > 0.0 ? rho(trial.e, huber) : (double)INFINITY) : 0.0, W);
        if (active) {
            iters++;
            if (solved && tcost < cost) {
                if (cost - tcost < REFINE_STOP_FRACTION * cost) active = false;
                X[0] = T0; X[1] = T1; X[2] = T2;
                at = trial;
                cost = tcost;
                lambda *= REFINE_LAMBDA_DOWN;
            } else {
                lambda *= REFINE_LAMBDA_UP;
            }
        }
    }
    if (sys >= total || v != 0) return;
    if (xyz) {
        float* d = xyz + (size_t)sys * 3;
        d[0] = (float)X[0]; d[1] = (float)X[1]; d[2] = (float)X[2];
    }
    if (xyz_f64) {
        double* d = xyz_f64 + (size_t)sys * 3;
        d[0] = X[0]; d[1] = X[1]; d[2] = X[2];
    }
    if (cost_out) { cost_out[2 * (size_t)sys] = cost0; cost_out[2 * (size_t)sys + 1] = cost; }
    if (iters_out) iters_out[sys] = iters;
}

int check_rig(const char* who, int N, int V, int J, const double* proj, size_t rig_stride)
{
    if (N < 1 || J < 1) return fail2(-1, "%s: N and J must be at least 1", who);
    if (V < 1 || V > SKS_MAX_VIEWS) return fail2(-1, "%s: %d views, a joint takes 1 .. %d (SKS_MAX_VIEWS)", who, V, SKS_MAX_VIEWS);
    if ((long long)N * J > 0x7fffffffLL - 64 * REPROJ_WAVES || (long long)V * J > 0x7fffffffLL / 2)
        return fail2(-1, "%s: N x J = %lld joints (V x J = %lld pairs a frame) are too many for one call", who, (long long)N * J, (long long)V * J);
    if (rig_stride != 0 && rig_stride != (size_t)V * 12) return fail2(-1, "%s: rig_stride must be 0 (one rig) or V * 12 (one per frame)", who);
    if (!proj) return fail2(-2, "%s: missing projection matrices", who);
    return 0;
}

template <typename T3D, typename T2D>
void launch_reproject(int N, int V, int J, const double* proj, size_t rig_stride, const T3D* xyz, const T2D* poses_2d,
                      const unsigned char* valid, double* uv, double* err, unsigned char* in_front, double* per_joint,
                      double* per_view, double* per_frame, int* n_used, hipStream_t stream)
{
    hipLaunchKernelGGL((k_reproject<T3D, T2D>), dim3((N + REPROJ_WAVES - 1) / REPROJ_WAVES), dim3(64 * REPROJ_WAVES), 0, stream, N, V,
                       J, proj, rig_stride, xyz, poses_2d, valid, uv, err, in_front, per_joint, per_view, per_frame, n_used);
}

template <typename T3D, typename T2D>
void launch_refine(dim3 grid, hipStream_t stream, int total, int V, int J, int W, const double* proj, size_t rig_stride,
                   const T2D* poses_2d, const unsigned char* valid, const T3D* xyz0, double huber, int max_iters, float* xyz,
                   double* xyz_f64, double* cost, int* iters)
{
    hipLaunchKernelGGL((k_refine<T3D, T2D>), grid, dim3(64 * REPROJ_WAVES), 0, stream, total, V, J, W, proj, rig_stride, poses_2d,
                       valid, xyz0, huber, max_iters, xyz, xyz_f64, cost, iters);
}

}  // namespace

extern "C" int sks_reproject(int N, int V, int J, const double* proj, size_t rig_stride, const float* xyz, const double* xyz_f64,
                             const float* poses_2d, const double* poses_2d_f64, const unsigned char* valid, double* uv,
                             double* err, unsigned char* in_front, double* per_joint, double* per_view, double* per_frame,
                             int* n_used, void* stream)
{
    if (int rc = check_rig("reproject", N, V, J, proj, rig_stride)) return rc;
    if (!xyz == !xyz_f64) return fail2(-2, "reproject: give the joints as float (xyz) or as double (xyz_f64), exactly one of the two");
    if (poses_2d && poses_2d_f64) return fail2(-2, "reproject: give the detections as float (poses_2d) or as double (poses_2d_f64), not both (neither: project only)");
    if (!uv && !err && !in_front && !per_joint && !per_view && !per_frame && !n_used) return fail2(-2, "reproject: no output asked for");
    const hipStream_t st = (hipStream_t)stream;
    if (xyz && poses_2d_f64)
        launch_reproject(N, V, J, proj, rig_stride, xyz, poses_2d_f64, valid, uv, err, in_front, per_joint, per_view, per_frame, n_used, st);
    else if (xyz)
        launch_reproject(N, V, J, proj, rig_stride, xyz, poses_2d, valid, uv, err, in_front, per_joint, per_view, per_frame, n_used, st);
    else if (poses_2d_f64)
        launch_reproject(N, V, J, proj, rig_stride, xyz_f64, poses_2d_f64, valid, uv, err, in_front, per_joint, per_view, per_frame, n_used, st);
    else
        launch_reproject(N, V, J, proj, rig_stride, xyz_f64, poses_2d, valid, uv, err, in_front, per_joint, per_view, per_frame, n_used, st);
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" int sks_eval_reprojection(int N, int V, int J, const double* err, const int* group_ids, int n_groups, double* out,
                                     void* stream)
{
    if (N < 1 || J < 1) return fail2(-1, "eval_reprojection: N = %d frames of J = %d joints; both must be at least 1", N, J);
    if (V < 1 || V > SKS_MAX_VIEWS) return fail2(-1, "eval_reprojection: %d views, 1 .. %d (SKS_MAX_VIEWS)", V, SKS_MAX_VIEWS);
    if ((long long)V * J > 0x7fffffffLL) return fail2(-1, "eval_reprojection: V x J = %lld pairs a frame are too many", (long long)V * J);
    if (n_groups < 0 || n_groups > SKS_EVAL_MAX_GROUPS) return fail2(-1, "eval_reprojection: n_groups = %d, 0 .. %d (SKS_EVAL_MAX_GROUPS)", n_groups, SKS_EVAL_MAX_GROUPS);
    if (!err) return fail2(-2, "eval_reprojection: missing err (N,V,J) doubles");
    if (!out) return fail2(-2, "eval_reprojection: missing out (1 + n_groups, 1 + V + J) doubles");
    if (n_groups > 0 && !group_ids) return fail2(-2, "eval_reprojection: n_groups = %d without group_ids", n_groups);
    hipLaunchKernelGGL(k_eval_reprojection, dim3(1 + n_groups), dim3(EVAL_THREADS), 0, (hipStream_t)stream, N, V, J, err, group_ids, out);
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" int sks_triangulate_refine(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_2d,
                                      const double* poses_2d_f64, const unsigned char* valid, const float* xyz0,
                                      const double* xyz0_f64, double huber_px, int max_iters, float* xyz, double* xyz_f64,
                                      double* cost, int* iters, void* stream)
{
    if (int rc = check_rig("triangulate_refine", N, V, J, proj, rig_stride)) return rc;
    if (!poses_2d == !poses_2d_f64) return fail2(-2, "triangulate_refine: give the detections as float (poses_2d) or as double (poses_2d_f64), exactly one of the two");
    if (!xyz0 == !xyz0_f64) return fail2(-2, "triangulate_refine: give the start as float (xyz0) or as double (xyz0_f64), exactly one of the two");
    if (!xyz && !xyz_f64) return fail2(-2, "triangulate_refine: at least one of xyz / xyz_f64");
    if (!(huber_px >= 0.0) || !isfinite(huber_px)) return fail2(-1, "triangulate_refine: huber_px must be finite and >= 0 pixels (0: plain squares), got %g", huber_px);
    if (max_iters < 1 || max_iters > SKS_REFINE_MAX_ITERS) return fail2(-1, "triangulate_refine: max_iters = %d, 1 .. %d (SKS_REFINE_MAX_ITERS)", max_iters, SKS_REFINE_MAX_ITERS);
    int W = 1;
    while (W < V) W <<= 1;
    const int total = N * J, per_block = REPROJ_WAVES * (64 / W);
    const dim3 grid((total + per_block - 1) / per_block);
    const hipStream_t st = (hipStream_t)stream;
    if (xyz0 && poses_2d)
        launch_refine(grid, st, total, V, J, W, proj, rig_stride, poses_2d, valid, xyz0, huber_px, max_iters, xyz, xyz_f64, cost, iters);
    else if (xyz0)
        launch_refine(grid, st, total, V, J, W, proj, rig_stride, poses_2d_f64, valid, xyz0, huber_px, max_iters, xyz, xyz_f64, cost, iters);
    else if (poses_2d)
        launch_refine(grid, st, total, V, J, W, proj, rig_stride, poses_2d, valid, xyz0_f64, huber_px, max_iters, xyz, xyz_f64, cost, iters);
    else
        launch_refine(grid, st, total, V, J, W, proj, rig_stride, poses_2d_f64, valid, xyz0_f64, huber_px, max_iters, xyz, xyz_f64, cost, iters);
    HIP_TRY2(hipGetLastError());
    return 0;
}
