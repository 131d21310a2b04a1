// sks_fuse.hip -- initial joints as the reprojection-error-weighted mean of the views' monocular 3D predictions
// (reference: dataset_tools/h36m/compute_initial_guess.py:23-116, dataset_tools/panoptic/compute_initial_guess_panoptic.py:
// 23-117; configs' initial_guess "metrabs" / "metrabs_occ_3") for MI355X.
//
// Per (frame, joint): candidate i (view i's prediction X_i) is projected into every camera c, e_ic = |u_ic - x_c|,
// ebar_i = mean over c, w_i = (1 / ebar_i) / sum_k (1 / ebar_k), result = sum_i w_i X_i / sum_i w_i.  Everything is float64, or,
// with norm_f32 (the Panoptic script), u - x is rounded to float32 and the norm, the mean, the reciprocal and the normalisation are
// float32, the average float64 again.
//
// Layout: lane = CANDIDATE.  A problem takes W = the next power of two >= V adjacent lanes of a wavefront (64 / W problems per
// wavefront, 4 wavefronts per workgroup), as sks_triangulate.hip does with lane = view.  Lane i walks the cameras c = 0 .. V-1 in
// index order and adds e_ic to its own running sum: the sum over cameras is numpy's, sequential in c, and needs no exchange
// between lanes (the V lanes of a problem read the same P_c and x_c in the same trip: one fetch, broadcast by the memory
// pipeline).  The two sums over candidates -- the weight sum and the average -- then walk i = 0 .. V-1 in index order as well, every
// lane of the problem reading lane i's value by a shuffle, so every lane ends with the same bits and the order of additions
// depends on V alone: never on N, on where the problem sits in the batch, on the launch geometry or on the stream.  A butterfly
// over the W lanes would be log2 W steps instead of V, but its order is not numpy's, and at V <= 64 the whole kernel is a few
// microseconds of latency either way.  Padding lanes and masked views are SKIPPED by the sums (never added as zeros: 0 * inf and
// -0 + 0 stay out of the picture).  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"

namespace {

constexpr int FUSE_WAVES = 4;            // wavefronts per workgroup

template <typename T3D, typename T2D, bool NORM_F32>
__global__ void __launch_bounds__(64 * FUSE_WAVES)
k_fuse(int total /* N * J */, int V, int J, int W, const double* __restrict__ proj, size_t rig_stride,
       const T3D* __restrict__ poses_3d, const T2D* __restrict__ poses_2d, const unsigned char* __restrict__ valid,
       float* __restrict__ xyz, double* __restrict__ xyz_f64, double* __restrict__ reproj_err, int* __restrict__ n_used)
{
    const int lane = threadIdx.x & 63;
    const int per_wave = 64 / W;
    const int sys = (blockIdx.x * FUSE_WAVES + (threadIdx.x >> 6)) * per_wave + lane / W;
    const int v = lane & (W - 1), base = lane - v;
    const bool live = sys < total && v < V;
    const int n = live ? sys / J : 0, j = live ? sys - n * J : 0;
    const size_t row = (size_t)n * V;                       // (frame n's first view in the (N,V,J,..) arrays)
    bool use = live;
    if (live && valid) use = valid[(row + v) * J + j] != 0;
    double X[3] = {0.0, 0.0, 0.0};
    if (use) {
        const T3D* p = poses_3d + ((row + v) * J + j) * 3;
        X[0] = (double)p[0]; X[1] = (double)p[1]; X[2] = (double)p[2];
    }
    // ebar of this lane's candidate: the cameras in index order, the left-out ones skipped
    double sum = 0.0;
    float sum_f = 0.0f;
    int used = 0;
    if (use) {
        const double* Pn = proj + (size_t)n * rig_stride;
        for (int c = 0; c < V; c++) {
            if (valid && valid[(row + c) * J + j] == 0) continue;
            const double* P = Pn + (size_t)c * 12;
            const T2D* d = poses_2d + ((row + c) * J + j) * 2;
            const double h0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
            const double h1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
            const double h2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
            const double dx = h0 / h2 - (double)d[0], dy = h1 / h2 - (double)d[1];
            if (NORM_F32) {
                const float fx = (float)dx, fy = (float)dy;
                sum_f += sqrtf(fx * fx + fy * fy);
            } else {
                sum += sqrt(dx * dx + dy * dy);
            }
            used++;
        }
    }
    // (a lane that is left out divides 0 by 0 here: its NaN is never read by the sums below)
    const double ebar = NORM_F32 ? (double)(sum_f / (float)used) : sum / (double)used;
    const float wf = 1.0f / (sum_f / (float)used);
    const double wd = NORM_F32 ? (double)wf : 1.0 / ebar;          // 1 / ebar_i, not yet normalised
    // the weight sum over the kept candidates, in index order; every lane of the problem walks the same lanes
    const unsigned long long kept = __ballot(use);
    double wsum = 0.0;
    float wsum_f = 0.0f;
    int count = 0;
    for (int i = 0; i < V; i++) {
        const double wi = __shfl(wd, base + i, 64);
        if ((kept >> (base + i)) & 1ull) {
            if (NORM_F32) wsum_f += (float)wi; else wsum += wi;
            count++;
        }
    }
    const double w = NORM_F32 ? (double)(wf / wsum_f) : wd / wsum;
    // the average: sum_i w_i X_i / sum_i w_i in float64, in index order
    double acc[3] = {0.0, 0.0, 0.0}, scl = 0.0;
    for (int i = 0; i < V; i++) {
        const double wi = __shfl(w, base + i, 64);
        const double x0 = __shfl(X[0], base + i, 64), x1 = __shfl(X[1], base + i, 64), x2 = __shfl(X[2], base + i, 64);
        if ((kept >> (base + i)) & 1ull) {
            acc[0] += x0 * wi; acc[1] += x1 * wi; acc[2] += x2 * wi;
            scl += wi;
        }
    }
    if (!live) return;
    if (reproj_err) reproj_err[(row + v) * J + j] = use ? ebar : (double)NAN;
    if (v != 0) return;
    double o[3];
    if (count == 0) {
        o[0] = o[1] = o[2] = (double)NAN;      // no view kept: nothing to average
    } else {
        o[0] = acc[0] / scl; o[1] = acc[1] / scl; o[2] = acc[2] / scl;
    }
    if (xyz) {
        float* d = xyz + (size_t)sys * 3;
        d[0] = (float)o[0]; d[1] = (float)o[1]; d[2] = (float)o[2];
    }
    if (xyz_f64) {
        double* d = xyz_f64 + (size_t)sys * 3;
        d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    }
    if (n_used) n_used[sys] = count;
}

template <typename T3D, typename T2D>
void launch(bool norm_f32, dim3 grid, dim3 block, hipStream_t stream, int total, int V, int J, int W, const double* proj,
            size_t rig_stride, const T3D* p3, const T2D* p2, const unsigned char* valid, float* xyz, double* xyz_f64,
            double* reproj_err, int* n_used)
{
    if (norm_f32)
        hipLaunchKernelGGL((k_fuse<T3D, T2D, true>), grid, block, 0, stream, total, V, J, W, proj, rig_stride, p3, p2, valid, xyz,
                           xyz_f64, reproj_err, n_used);
    else
        hipLaunchKernelGGL((k_fuse<T3D, T2D, false>), grid, block, 0, stream, total, V, J, W, proj, rig_stride, p3, p2, valid, xyz,
                           xyz_f64, reproj_err, n_used);
}

}  // namespace

extern "C" int sks_fuse_predictions(int N, int V, int J, const double* proj, size_t rig_stride, const float* poses_3d,
                                    const double* poses_3d_f64, const float* poses_2d, const double* poses_2d_f64,
                                    const unsigned char* valid, int norm_f32, float* xyz, double* xyz_f64, double* reproj_err,
                                    int* n_used, void* stream)
{
    if (N < 1 || J < 1) return fail2(-1, "fuse_predictions: N and J must be at least 1");
    if (V < 1 || V > SKS_MAX_VIEWS) return fail2(-1, "fuse_predictions: %d views, a joint takes 1 .. %d (SKS_MAX_VIEWS)", V, SKS_MAX_VIEWS);
    if ((long long)N * J > 0x7fffffffLL - 64 * FUSE_WAVES) return fail2(-1, "fuse_predictions: N x J = %lld joints are too many for one call", (long long)N * J);
    if (rig_stride != 0 && rig_stride != (size_t)V * 12) return fail2(-1, "fuse_predictions: rig_stride must be 0 (one rig) or V * 12 (one per frame)");
    if (!proj) return fail2(-2, "fuse_predictions: missing projection matrices");
    if (!poses_3d == !poses_3d_f64) return fail2(-2, "fuse_predictions: give the predictions as float (poses_3d) or as double (poses_3d_f64), not both");
    if (!poses_2d == !poses_2d_f64) return fail2(-2, "fuse_predictions: give the detections as float (poses_2d) or as double (poses_2d_f64), not both");
    if (!xyz && !xyz_f64) return fail2(-2, "fuse_predictions: at least one of xyz / xyz_f64");
    int W = 1;
    while (W < V) W <<= 1;
    const int total = N * J, per_block = FUSE_WAVES * (64 / W);
    const dim3 grid((total + per_block - 1) / per_block), block(64 * FUSE_WAVES);
    const hipStream_t st = (hipStream_t)stream;
    const bool f32 = norm_f32 != 0;
    if (poses_3d && poses_2d)
        launch(f32, grid, block, st, total, V, J, W, proj, rig_stride, poses_3d, poses_2d, valid, xyz, xyz_f64, reproj_err, n_used);
    else if (poses_3d)
        launch(f32, grid, block, st, total, V, J, W, proj, rig_stride, poses_3d, poses_2d_f64, valid, xyz, xyz_f64, reproj_err, n_used);
    else if (poses_2d)
        launch(f32, grid, block, st, total, V, J, W, proj, rig_stride, poses_3d_f64, poses_2d, valid, xyz, xyz_f64, reproj_err, n_used);
    else
        launch(f32, grid, block, st, total, V, J, W, proj, rig_stride, poses_3d_f64, poses_2d_f64, valid, xyz, xyz_f64, reproj_err, n_used);
    HIP_TRY2(hipGetLastError());
    return 0;
}
