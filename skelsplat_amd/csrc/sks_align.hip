// sks_align.hip -- pose errors after the best per-frame alignment of the prediction onto the ground truth, for MI355X: rigid
// (R, t), similarity (s, R, t: PA-MPJPE, "Protocol #2") and scale only on root-relative poses (N-MPJPE).  The reference reports
// MPJPE alone (eval.py), so these are held to two textbook float64 solutions (tests/procrustes_ref.py), not to reference output.
//
// Like sks_report.hip's kernels these are bound by launch latency: one wavefront per frame, nothing handed from one workgroup to
// another, no LDS, no atomics, no scratch.  Everything is computed in double from the float inputs and every output is rounded to
// its type once.  Every sum has a fixed order: lane l adds its joints l, l + 64, ... in index order and the 64 partial sums meet
// in a butterfly, after which every lane holds the same totals and runs the same 3x3 fit (csrc/sks_procrustes.h), so nothing is
// broadcast.  A frame's results depend on P and its own numbers only -- never on N, on where the frame sits or on the stream.
// Every loop's trip count is fixed by P or by PROCRUSTES_SWEEPS; a frame with a NaN or inf in a valid joint skips the fit.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"
#include "sks_procrustes.h"

namespace {

constexpr int EVAL_THREADS = 256;

__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One frame by one wavefront.  aligned (P,3), transform (13), per_joint (P), mean (1): each may be nullptr.
__global__ void __launch_bounds__(64)
k_align_poses(int P, int mode, const float* __restrict__ pred_all, const float* __restrict__ gt_all,
              const unsigned char* __restrict__ valid_all, float* __restrict__ aligned_all, double* __restrict__ transform_all,
              float* __restrict__ per_joint_all, float* __restrict__ mean_all)
{
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x;
    const float* __restrict__ pred = pred_all + f * P * 3;
    const float* __restrict__ gt = gt_all + f * P * 3;
    const unsigned char* __restrict__ valid = valid_all ? valid_all + f * P : nullptr;

    // the two origins: the centroids of the valid joints, or joint 0 (SKS_ALIGN_SCALE)
    double cnt = 0.0, mx[3] = { 0.0, 0.0, 0.0 }, my[3] = { 0.0, 0.0, 0.0 };
    for (int p = lane; p < P; p += 64) {
        if (valid && !valid[p]) continue;
        cnt += 1.0;
        _Pragma("unroll") for (int k = 0; k < 3; k++) { mx[k] += (double)pred[3 * p + k]; my[k] += (double)gt[3 * p + k]; }
    }
    cnt = wave_sum(cnt);
    const bool empty = cnt == 0.0;
    bool rootless = false;
    if (mode == SKS_ALIGN_SCALE) {
        rootless = valid && !valid[0];
        _Pragma("unroll") for (int k = 0; k < 3; k++) { mx[k] = (double)pred[k]; my[k] = (double)gt[k]; }
    } else {
        _Pragma("unroll") for (int k = 0; k < 3; k++) { mx[k] = wave_sum(mx[k]) / cnt; my[k] = wave_sum(my[k]) / cnt; }
    }
    if (empty)      // no joint to fit: the identity
        _Pragma("unroll") for (int k = 0; k < 3; k++) mx[k] = my[k] = 0.0;

    // H = sum x y^T and sum |x|^2 over the valid joints
    double H[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, sxx = 0.0;
    for (int p = lane; p < P; p += 64) {
        if (valid && !valid[p]) continue;
        double x[3], y[3];
        _Pragma("unroll") for (int k = 0; k < 3; k++) { x[k] = (double)pred[3 * p + k] - mx[k]; y[k] = (double)gt[3 * p + k] - my[k]; }
        _Pragma("unroll") for (int a = 0; a < 3; a++)
            _Pragma("unroll") for (int b = 0; b < 3; b++) H[3 * a + b] += x[a] * y[b];
        sxx += (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    }
    double hsum = 0.0;
    _Pragma("unroll") for (int k = 0; k < 9; k++) { H[k] = wave_sum(H[k]); hsum += H[k]; }
    sxx = wave_sum(sxx);
    // 0 where every valid joint of the frame is finite, NaN otherwise (a NaN or inf joint leaves a NaN in H or in sxx)
    const double poison = (hsum + sxx) * 0.0;
    const bool bad = poison != 0.0 || (rootless && !empty);

    double s = 1.0, R[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 };
    const bool rotate = mode != SKS_ALIGN_SCALE && !empty && !bad;
    if (rotate) sks::procrustes_rotation(H, R);
    if (!empty && !bad) {
        if (mode == SKS_ALIGN_SIMILARITY) {     // trace(R H^T) = sum <R x, y>: the least-squares scale for this R
            const double num = ((R[0] * H[0] + R[1] * H[3]) + R[2] * H[6]) + ((R[3] * H[1] + R[4] * H[4]) + R[5] * H[7])
                               + ((R[6] * H[2] + R[7] * H[5]) + R[8] * H[8]);
            s = sxx == 0.0 ? 1.0 : num / sxx;
        } else if (mode == SKS_ALIGN_SCALE) {
            s = sxx == 0.0 ? 1.0 : ((H[0] + H[4]) + H[8]) / sxx;
        }
    }
    double t[3];
    _Pragma("unroll") for (int k = 0; k < 3; k++) t[k] = my[k] - s * ((R[3 * k] * mx[0] + R[3 * k + 1] * mx[1]) + R[3 * k + 2] * mx[2]);
    if (bad) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        s = nan;
        _Pragma("unroll") for (int k = 0; k < 9; k++) R[k] = nan;
        _Pragma("unroll") for (int k = 0; k < 3; k++) t[k] = nan;
    }
    if (transform_all && lane == 0) {
        double* tr = transform_all + f * 13;
        tr[0] = s;
        _Pragma("unroll") for (int k = 0; k < 9; k++) tr[1 + k] = R[k];
        _Pragma("unroll") for (int k = 0; k < 3; k++) tr[10 + k] = t[k];
    }

    // every joint, masked ones included: s R (pred - origin_x) + origin_y, the transform applied about the origins it was fitted
    // at (the same point as s R pred + t, without the cancellation of a pose far from the world's origin)
    float* __restrict__ aligned = aligned_all ? aligned_all + f * P * 3 : nullptr;
    float* __restrict__ per_joint = per_joint_all ? per_joint_all + f * P : nullptr;
    double esum = 0.0;
    for (int p = lane; p < P; p += 64) {
        double x[3], a[3], e[3];
        _Pragma("unroll") for (int k = 0; k < 3; k++) x[k] = (double)pred[3 * p + k] - mx[k];
        _Pragma("unroll") for (int k = 0; k < 3; k++) {
            const double rx = rotate ? (R[3 * k] * x[0] + R[3 * k + 1] * x[1]) + R[3 * k + 2] * x[2] : x[k];
            a[k] = bad ? s : s * rx + my[k];
            e[k] = (double)gt[3 * p + k] - a[k];
        }
        const double err = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        if (aligned)
            _Pragma("unroll") for (int k = 0; k < 3; k++) aligned[3 * p + k] = (float)a[k];
        if (per_joint) per_joint[p] = (float)err;
        if (!valid || valid[p]) esum += err;
    }
    esum = wave_sum(esum);
    if (mean_all && lane == 0) mean_all[f] = (float)(esum / cnt);       // (no valid joint: 0 / 0 = NaN)
}

// One workgroup per output row (0: all frames, 1 + g: group g).  Thread t takes frames t, t + 256, ... in index order, a frame's
// valid joints in index order, sums and counts in double; the 256 partial sums meet in a tree (k_eval_sequence's shape).
__global__ void __launch_bounds__(EVAL_THREADS)
k_eval_aligned(int N, int P, const float* __restrict__ err_pa, const float* __restrict__ err_n,
               const unsigned char* __restrict__ valid, const int* __restrict__ group_ids, double* __restrict__ out)
{
    __shared__ double s_sum[2][EVAL_THREADS];
    __shared__ double s_cnt[EVAL_THREADS];
    const int tid = threadIdx.x, g = (int)blockIdx.x - 1;
    double sp = 0.0, sn = 0.0, c = 0.0;
    for (int i = tid; i < N; i += EVAL_THREADS) {
        if (g >= 0 && group_ids[i] != g) continue;
        const size_t base = (size_t)i * P;
        double fp = 0.0, fn = 0.0, fc = 0.0;
        for (int p = 0; p < P; p++) {
            if (valid && !valid[base + p]) continue;
            fp += (double)err_pa[base + p]; fn += (double)err_n[base + p]; fc += 1.0;
        }
        sp += fp; sn += fn; c += fc;
    }
    s_sum[0][tid] = sp; s_sum[1][tid] = sn; s_cnt[tid] = c;
    for (int o = EVAL_THREADS / 2; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) { s_sum[0][tid] += s_sum[0][tid + o]; s_sum[1][tid] += s_sum[1][tid + o]; s_cnt[tid] += s_cnt[tid + o]; }
    }
    if (tid == 0) {     // (a row without valid joints: 0 / 0 = NaN)
        out[2 * (size_t)blockIdx.x] = s_sum[0][0] / s_cnt[0];
        out[2 * (size_t)blockIdx.x + 1] = s_sum[1][0] / s_cnt[0];
    }
}

void launch_align(int N, int P, const float* pred, const float* gt, const unsigned char* valid, int mode, float* aligned,
                  double* transform, float* per_joint, float* mean, hipStream_t stream)
{
    hipLaunchKernelGGL(k_align_poses, dim3(N), dim3(64), 0, stream, P, mode, pred, gt, valid, aligned, transform, per_joint, mean);
}

}  // namespace

extern "C" int sks_align_poses(int N, int P, const float* pred, const float* gt, const unsigned char* valid, int mode,
                               float* aligned, double* transform, float* per_joint, float* mean, void* stream)
{
    if (N < 1 || P < 1) return fail2(-1, "align_poses: N = %d frames of P = %d joints; both must be at least 1", N, P);
    if ((long long)P * 3 > 0x7fffffffLL) return fail2(-1, "align_poses: P = %d joints are too many", P);
    if (mode < SKS_ALIGN_RIGID || mode > SKS_ALIGN_SCALE)
        return fail2(-1, "align_poses: mode = %d, must be SKS_ALIGN_RIGID (0), SKS_ALIGN_SIMILARITY (1) or SKS_ALIGN_SCALE (2)", mode);
    if (!pred || !gt) return fail2(-2, "align_poses: missing %s", !pred ? "pred" : "gt");
    if (!aligned && !transform && !per_joint && !mean)
        return fail2(-2, "align_poses: no output requested (aligned, transform, per_joint and mean are all NULL)");
    launch_align(N, P, pred, gt, valid, mode, aligned, transform, per_joint, mean, (hipStream_t)stream);
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" size_t sks_eval_sequence_aligned_scratch_bytes(int N, int P)
{
    if (N < 1 || P < 1) return 0;
    return (size_t)2 * (size_t)N * (size_t)P * sizeof(float);
}

extern "C" int sks_eval_sequence_aligned(int N, int P, const float* pred, const float* gt, const unsigned char* valid,
                                         const int* group_ids, int n_groups, void* scratch, size_t scratch_bytes, double* out,
                                         void* stream)
{
    if (N < 1 || P < 1) return fail2(-1, "eval_sequence_aligned: N = %d frames of P = %d joints; both must be at least 1", N, P);
    if ((long long)P * 3 > 0x7fffffffLL) return fail2(-1, "eval_sequence_aligned: P = %d joints are too many", P);
    if (n_groups < 0 || n_groups > SKS_EVAL_MAX_GROUPS)
        return fail2(-1, "eval_sequence_aligned: n_groups = %d, 0 .. %d (SKS_EVAL_MAX_GROUPS)", n_groups, SKS_EVAL_MAX_GROUPS);
    if (!pred || !gt) return fail2(-2, "eval_sequence_aligned: missing %s", !pred ? "pred" : "gt");
    if (!out) return fail2(-2, "eval_sequence_aligned: missing out (1 + n_groups, 2) doubles");
    if (n_groups > 0 && !group_ids) return fail2(-2, "eval_sequence_aligned: n_groups = %d without group_ids", n_groups);
    const size_t need = sks_eval_sequence_aligned_scratch_bytes(N, P);
    if (!scratch || scratch_bytes < need)
        return fail2(-2, "eval_sequence_aligned: scratch of %zu bytes, %zu are needed (sks_eval_sequence_aligned_scratch_bytes)",
                     scratch ? scratch_bytes : (size_t)0, need);
    float* err_pa = (float*)scratch;
    float* err_n = err_pa + (size_t)N * P;
    launch_align(N, P, pred, gt, valid, SKS_ALIGN_SIMILARITY, nullptr, nullptr, err_pa, nullptr, (hipStream_t)stream);
    HIP_TRY2(hipGetLastError());
    launch_align(N, P, pred, gt, valid, SKS_ALIGN_SCALE, nullptr, nullptr, err_n, nullptr, (hipStream_t)stream);
    HIP_TRY2(hipGetLastError());
    hipLaunchKernelGGL(k_eval_aligned, dim3(1 + n_groups), dim3(EVAL_THREADS), 0, (hipStream_t)stream, N, P, err_pa, err_n, valid,
                       group_ids, out);
    HIP_TRY2(hipGetLastError());
    return 0;
}
