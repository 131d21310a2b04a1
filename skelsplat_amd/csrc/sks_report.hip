// sks_report.hip -- what the reference reports about a pose while and after it optimises it, for MI355X: the per-joint absolute
// and root-relative errors against the ground truth and their means at every optimiser step (train.py:184-213, 239-242), the
// parameters at debug.save_iterations and at the stopping iteration (train.py:227-229), and the MPJPE of a sequence, overall and
// per activity (eval.py:115-142).
//
// All three kernels are bound by launch latency: a frame is 17 joints.  One wavefront per frame (errors, report) or one workgroup
// per output row (evaluation), nothing handed from one workgroup to another, no atomics, no scratch.  Every sum has a fixed order:
// lane l adds its joints l, l + 64, ... in index order and the 64 partial sums meet in a butterfly, so a frame's means depend on
// P and its own numbers only -- never on N, on where the frame sits in the batch or on the stream -- and sks_loop_report's trace
// rows are sks_pose_errors' means bit for bit (both call frame_errors).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"

namespace {

constexpr int EVAL_THREADS = 256;

// joint p of one pose: ||pred - gt|| and ||(pred - pred[0]) - (gt - gt[0])||, the reference's order of operations
// (train.py:198-204), both as sqrt((x^2 + y^2) + z^2) in float
__device__ __forceinline__ void joint_errors(const float* __restrict__ pred, const float* __restrict__ gt, int p, float& e_abs,
                                             float& e_rel)
{
    const float px = pred[3 * p], py = pred[3 * p + 1], pz = pred[3 * p + 2];
    const float gx = gt[3 * p], gy = gt[3 * p + 1], gz = gt[3 * p + 2];
    const float dx = px - gx, dy = py - gy, dz = pz - gz;
    e_abs = sqrtf(dx * dx + dy * dy + dz * dz);
    const float rx = (px - pred[0]) - (gx - gt[0]), ry = (py - pred[1]) - (gy - gt[1]), rz = (pz - pred[2]) - (gz - gt[2]);
    e_rel = sqrtf(rx * rx + ry * ry + rz * rz);
}

// One frame by one wavefront (every lane must call): per_joint (P,2) or nullptr, mean (2) or nullptr.
__device__ __forceinline__ void frame_errors(const float* __restrict__ pred, const float* __restrict__ gt, int P,
                                             float* __restrict__ per_joint, float* __restrict__ mean)
{
    const int lane = threadIdx.x & 63;
    float sa = 0.0f, sr = 0.0f;
    for (int p = lane; p < P; p += 64) {
        float ea, er;
        joint_errors(pred, gt, p, ea, er);
        if (per_joint) { per_joint[2 * (size_t)p] = ea; per_joint[2 * (size_t)p + 1] = er; }
        sa += ea; sr += er;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_xor(sa, o, 64);
        sr += __shfl_xor(sr, o, 64);
    }
    if (lane == 0 && mean) { mean[0] = sa / (float)P; mean[1] = sr / (float)P; }
}

__global__ void __launch_bounds__(64)
k_pose_errors(int P, const float* __restrict__ pred, const float* __restrict__ gt, float* __restrict__ per_joint,
              float* __restrict__ mean)
{
    const size_t f = blockIdx.x;
    frame_errors(pred + f * P * 3, gt + f * P * 3, P, per_joint ? per_joint + f * P * 2 : nullptr, mean + f * 2);
}

struct SaveIterations { int K; int it[SKS_REPORT_MAX_SAVES]; };

// One wavefront per frame of a batch, behind the step's tail (or behind new_scenes: n = 0).  It reads what the tail left in
// memory and writes rows that depend on that alone, so a replay for a frame that has stopped rewrites what is there.
__global__ void __launch_bounds__(64)
k_loop_report(int V, int P, const int* __restrict__ counters, const int* __restrict__ es_state, int es_stride,
              const float* __restrict__ xyz, const float* __restrict__ gt, const double* __restrict__ loss_sums, int acc_steps,
              int capacity, float* __restrict__ trace_err, float* __restrict__ trace_loss, float* __restrict__ final_err,
              SaveIterations sv, float* __restrict__ snaps)
{
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x;
    const int n = counters[2 * f + 1];                                  // Adam steps this frame has made
    const int stop = es_state ? es_state[f * es_stride + 1] : 0;        // the iteration it stopped at, 0 = running
    const float* x = xyz + f * P * 3;
    const bool row = n >= 0 && n < capacity;                            // (rows past the capacity are dropped)
    if (gt)
        frame_errors(x, gt + f * P * 3, P, final_err ? final_err + f * P * 2 : nullptr,
                     row && trace_err ? trace_err + (f * capacity + n) * 2 : nullptr);
    if (loss_sums && trace_loss && row)
        for (int v = lane; v < V; v += 64) {        // the loss early_stop_decide forms from the view's {S, N}
            const double* sn = loss_sums + 2 * (f * V + v);
            const double cnt = sn[1] < 1.0 ? 1.0 : sn[1];
            trace_loss[(f * capacity + n) * V + v] = (float)(sn[0] / cnt);
        }
    // Slot k holds the parameters as they stood at the end of iteration s = it[k]: those after s / acc_steps steps while the frame
    // runs, and the final ones if it stopped at exactly s.  A frame that turns out to have stopped before s never got there
    // (train.py:231-233 leaves the loop): its slot goes back to NaN, what it was initialised with.
    for (int k = 0; k < sv.K; k++) {
        const int s = sv.it[k];
        float* d = snaps + (f * sv.K + k) * P * 3;
        if (stop == 0 ? s / acc_steps == n : s == stop) {
            for (int i = lane; i < 3 * P; i += 64) d[i] = x[i];
        } else if (stop != 0 && s > stop) {
            for (int i = lane; i < 3 * P; i += 64) d[i] = NAN;
        }
    }
}

// One workgroup per output row (0: all frames, 1 + g: group g).  Thread t takes frames t, t + 256, ... in index order, a frame's
// joints in index order, norms in float (frame_errors' arithmetic), every sum in double; the 256 partial sums meet in a tree.
__global__ void __launch_bounds__(EVAL_THREADS)
k_eval_sequence(int N, int P, const float* __restrict__ pred, const float* __restrict__ gt, const int* __restrict__ group_ids,
                const unsigned char* __restrict__ abs_valid, double* __restrict__ out)
{
    __shared__ double s_sum[2][EVAL_THREADS];
    __shared__ long long s_cnt[2][EVAL_THREADS];
    const int tid = threadIdx.x, g = (int)blockIdx.x - 1;
    double sa = 0.0, sr = 0.0;
    long long ca = 0, cr = 0;
    for (int i = tid; i < N; i += EVAL_THREADS) {
        if (g >= 0 && group_ids[i] != g) continue;
        const float* a = pred + (size_t)i * P * 3;
        const float* b = gt + (size_t)i * P * 3;
        double fa = 0.0, fr = 0.0;
        for (int p = 0; p < P; p++) {
            float ea, er;
            joint_errors(a, b, p, ea, er);
            fa += (double)ea; fr += (double)er;
        }
        if (!abs_valid || abs_valid[i]) { sa += fa; ca++; }
        sr += fr; cr++;
    }
    s_sum[0][tid] = sa; s_sum[1][tid] = sr; s_cnt[0][tid] = ca; s_cnt[1][tid] = cr;
    for (int o = EVAL_THREADS / 2; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) {
            s_sum[0][tid] += s_sum[0][tid + o]; s_sum[1][tid] += s_sum[1][tid + o];
            s_cnt[0][tid] += s_cnt[0][tid + o]; s_cnt[1][tid] += s_cnt[1][tid + o];
        }
    }
    if (tid == 0) {     // (an empty row: 0 / 0 = NaN, np.mean of nothing)
        out[2 * (size_t)blockIdx.x] = s_sum[0][0] / ((double)s_cnt[0][0] * (double)P);
        out[2 * (size_t)blockIdx.x + 1] = s_sum[1][0] / ((double)s_cnt[1][0] * (double)P);
    }
}

}  // namespace

extern "C" int sks_pose_errors(int N, int P, const float* pred, const float* gt, float* per_joint, float* mean, void* stream)
{
    if (N < 1 || P < 1) return fail2(-1, "pose_errors: N = %d frames of P = %d joints; both must be at least 1", N, P);
    if ((long long)P * 3 > 0x7fffffffLL) return fail2(-1, "pose_errors: P = %d joints are too many", P);
    if (!pred || !gt) return fail2(-2, "pose_errors: missing %s", !pred ? "pred" : "gt");
    if (!mean) return fail2(-2, "pose_errors: missing mean (N,2); per_joint may be NULL");
    hipLaunchKernelGGL(k_pose_errors, dim3(N), dim3(64), 0, (hipStream_t)stream, P, pred, gt, per_joint, mean);
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" int sks_loop_report(int frames, int V, int P, const int* counters, const int* es_state, int es_window, const float* xyz,
                               const float* gt, const double* loss_sums, int acc_steps, int capacity, float* trace_err,
                               float* trace_loss, float* final_err, int K, const int* save_iterations, float* snaps, void* stream)
{
    if (frames < 1 || V < 1 || P < 1) return fail2(-1, "loop_report: frames, V and P must be at least 1");
    if ((long long)P * 3 > 0x7fffffffLL) return fail2(-1, "loop_report: P = %d joints are too many", P);
    if (acc_steps < 1) return fail2(-1, "loop_report: acc_steps = %d, must be at least 1", acc_steps);
    if (capacity < 0) return fail2(-1, "loop_report: capacity = %d rows, must not be negative", capacity);
    if (K < 0 || K > SKS_REPORT_MAX_SAVES) return fail2(-1, "loop_report: K = %d save iterations, 0 .. %d (SKS_REPORT_MAX_SAVES)", K, SKS_REPORT_MAX_SAVES);
    if (!counters || !xyz) return fail2(-2, "loop_report: missing %s", !counters ? "counters" : "xyz");
    if (es_state && (es_window < 1 || es_window > 16)) return fail2(-1, "loop_report: es_window = %d with an es_state, 1 .. 16", es_window);
    if (gt && !final_err) return fail2(-2, "loop_report: gt is given, so final_err (frames,P,2) is required");
    if (gt && capacity > 0 && !trace_err) return fail2(-2, "loop_report: gt and a capacity are given, so trace_err (frames,capacity,2) is required");
    if (!gt && (final_err || trace_err)) return fail2(-2, "loop_report: final_err / trace_err are given without gt");
    if (!loss_sums != !trace_loss) return fail2(-2, "loop_report: loss_sums and trace_loss go together (both or neither)");
    if (K > 0 && (!save_iterations || !snaps)) return fail2(-2, "loop_report: K = %d, so save_iterations (HOST K) and snaps (frames,K,P,3) are required", K);
    SaveIterations sv;
    sv.K = K;
    for (int k = 0; k < SKS_REPORT_MAX_SAVES; k++) {
        sv.it[k] = k < K ? save_iterations[k] : 0;
        if (sv.it[k] < 0) return fail2(-1, "loop_report: save_iterations[%d] = %d is negative", k, sv.it[k]);
    }
    hipLaunchKernelGGL(k_loop_report, dim3(frames), dim3(64), 0, (hipStream_t)stream, V, P, counters, es_state,
                       2 + 2 * es_window, xyz, gt, loss_sums, acc_steps, capacity, trace_err, trace_loss, final_err, sv, snaps);
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" int sks_eval_sequence(int N, int P, const float* pred, const float* gt, const int* group_ids, int n_groups,
                                 const unsigned char* abs_valid, double* out, void* stream)
{
    if (N < 1 || P < 1) return fail2(-1, "eval_sequence: N = %d frames of P = %d joints; both must be at least 1", N, P);
    if ((long long)P * 3 > 0x7fffffffLL) return fail2(-1, "eval_sequence: P = %d joints are too many", P);
    if (n_groups < 0 || n_groups > SKS_EVAL_MAX_GROUPS) return fail2(-1, "eval_sequence: n_groups = %d, 0 .. %d (SKS_EVAL_MAX_GROUPS)", n_groups, SKS_EVAL_MAX_GROUPS);
    if (!pred || !gt) return fail2(-2, "eval_sequence: missing %s", !pred ? "pred" : "gt");
    if (!out) return fail2(-2, "eval_sequence: missing out (1 + n_groups, 2) doubles");
    if (n_groups > 0 && !group_ids) return fail2(-2, "eval_sequence: n_groups = %d without group_ids", n_groups);
    hipLaunchKernelGGL(k_eval_sequence, dim3(1 + n_groups), dim3(EVAL_THREADS), 0, (hipStream_t)stream, N, P, pred, gt, group_ids,
                       abs_valid, out);
    HIP_TRY2(hipGetLastError());
    return 0;
}
