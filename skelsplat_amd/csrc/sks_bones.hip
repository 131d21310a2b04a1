// sks_bones.hip -- constant limb lengths over a sequence of poses, for MI355X: the length of every bone in every frame, the
// median and the median absolute deviation of a recording's lengths, and the pose of every frame moved onto those lengths by
// successive covariance-metric projections.  The three definitions, with the order of every sum, stand in
// include/skelsplat_hip.h above the prototypes; this file follows them op by op in float64 and is compiled without FMA
// contraction like the rest of the library, so a frame's bits are the same wherever it is computed.  No floating-point atomics:
// the medians are SELECTED by integer counts, which makes them exact, one of the inputs and free of any summation order.
//
// k_measure.  One lane per (frame, bone), 256 threads a workgroup.
// k_lengths.  One workgroup of 256 threads per (group, bone).  The k-th smallest of the group's usable measures by an
//   MSB-first radix select over the floats' bit patterns (a usable measure is finite with a clear sign bit, so the bit patterns
//   order like the values): four passes of eight bits, each a 256-bin histogram in LDS filled with INTEGER atomics by the threads
//   walking the frames f = t, t + 256, ..; thread 0 walks the bins to the one that holds rank k.  Then the same select over the
//   bit patterns of |l - median| (float32) for the MAD.  A group longer than 256 frames takes several trips per pass.
// k_project.  One wavefront (a workgroup of 64 threads) per frame; everything the trips share lives in LDS: the iterate x, the
//   joints' covariances, the bones' directions, S = A Sigma A^T (lower triangle, B x B doubles) and the right-hand side.  Lane b
//   owns bone b (norms, directions, row b of S and of the LDL^T update), lane j owns joint j (its covariance and its step).  The
//   exit test reads one LDS word every lane sees, so a frame leaves as a whole wave.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"

namespace {

constexpr int MEASURE_THREADS = 256;
constexpr int LENGTHS_THREADS = 256;
constexpr int PROJECT_THREADS = 64;
constexpr int MAXB = SKS_BONES_MAX_JOINTS - 1;

// the bones of a call, passed by value: parent and child joint of bone b
struct BoneTable { unsigned char p[MAXB + 1], c[MAXB + 1]; };

// index of entry (r, c) in xx, xy, xz, yy, yz, zz
__device__ constexpr int SYM[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};

__device__ __forceinline__ bool finite3(const float* x) { return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]); }

// u^T S v for the symmetric 3x3 S = {xx, xy, xz, yy, yz, zz}: w = S v row by row, then u . w, each (a + b) + c
__device__ __forceinline__ double quad3(const double* u, const double* S, const double* v)
{
    double w[3];
#pragma unroll
    for (int r = 0; r < 3; r++) w[r] = (S[SYM[r][0]] * v[0] + S[SYM[r][1]] * v[1]) + S[SYM[r][2]] * v[2];
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2];
}

// are the three pivots of the header's 3x3 LDL^T finite and > 0?
__device__ __forceinline__ bool positive3(double xx, double xy, double xz, double yy, double yz, double zz)
{
    const double d0 = xx;
    const double l10 = xy / d0;
    const double l20 = xz / d0;
    const double d1 = yy - l10 * xy;
    const double e = yz - l20 * xy;
    const double z1 = zz - l20 * xz;
    const double l21 = e / d1;
    const double d2 = z1 - l21 * e;
    return isfinite(d0) && isfinite(d1) && isfinite(d2) && d0 > 0.0 && d1 > 0.0 && d2 > 0.0;
}

__global__ void __launch_bounds__(MEASURE_THREADS)
k_measure(int N, int J, int B, BoneTable bones, const float* __restrict__ xyz, const float* __restrict__ cov6,
          const unsigned char* __restrict__ valid, double max_var, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * MEASURE_THREADS + threadIdx.x;
    if (i >= (long long)N * B) return;
    const long long f = i / B;
    const int b = (int)(i - f * B);
    const size_t ap = (size_t)f * J + bones.p[b], ac = (size_t)f * J + bones.c[b];
    const float* xp = xyz + 3 * ap;
    const float* xc = xyz + 3 * ac;
    float len = NAN;
    if (finite3(xp) && finite3(xc) && (!valid || (valid[ap] != 0 && valid[ac] != 0))) {
        double d[3];
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = (double)xc[k] - (double)xp[k];
        const double n = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        bool keep = true;
        if (cov6) {
            double u[3], S[6];
#pragma unroll
            for (int k = 0; k < 3; k++) u[k] = d[k] / n;
#pragma unroll
            for (int e = 0; e < 6; e++) S[e] = (double)cov6[6 * ap + e] + (double)cov6[6 * ac + e];
            keep = quad3(u, S, u) <= max_var;                       // (a NaN variance, n = 0 included: left out)
        }
        if (keep) len = (float)n;
    }
    out[i] = len;
}

// a usable measure: finite with a clear sign bit (0x7f800000 is +inf)
__device__ __forceinline__ bool usable_bits(uint32_t k) { return k < 0x7f800000u; }

// The bit pattern of the element of rank k = (n - 1) / 2 (0-based, ascending) among the group's n usable keys; MAD: the keys are
// |l - med|.  `n` receives the number of usable keys; with n == 0 the result is meaningless.
template <bool MAD>
__device__ uint32_t select_rank(int N, int B, int b, int g, const float* __restrict__ measured, const int* __restrict__ groups,
                                float med, int* s_hist, int* s_pick, int& n)
{
    const int tid = threadIdx.x;
    uint32_t prefix = 0;
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        s_hist[tid] = 0;
        __syncthreads();
        for (long long f = tid; f < N; f += LENGTHS_THREADS) {
            if (groups ? groups[f] != g : g != 0) continue;
            const float l = measured[(size_t)f * B + b];
            if (!usable_bits(__float_as_uint(l))) continue;
            const uint32_t key = MAD ? __float_as_uint(fabsf(l - med)) : __float_as_uint(l);
            if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int rank = s_pick[1];
            if (pass == 0) {
                int total = 0;
                for (int i = 0; i < 256; i++) total += s_hist[i];
                s_pick[2] = total;
                rank = (total - 1) / 2;
            }
            int bin = 0;
            for (int i = 0; i < 256; i++) {
                const int c = s_hist[i];
                if (rank < c) { bin = i; break; }
                rank -= c;
            }
            s_pick[0] = bin;
            s_pick[1] = rank;
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint32_t)s_pick[0];
        n = s_pick[2];
        if (n == 0) break;                                          // (read from LDS: the whole workgroup leaves together)
    }
    __syncthreads();                                                // s_pick is written again by the next select
    return prefix;
}

__global__ void __launch_bounds__(LENGTHS_THREADS)
k_lengths(int N, int B, const float* __restrict__ measured, const int* __restrict__ groups, float* __restrict__ length,
          float* __restrict__ mad, int* __restrict__ n_used)
{
    __shared__ int s_hist[256];
    __shared__ int s_pick[3];
    const int b = (int)blockIdx.x, g = (int)blockIdx.y;
    int n = 0;
    const uint32_t m = select_rank<false>(N, B, b, g, measured, groups, 0.0f, s_hist, s_pick, n);
    const size_t at = (size_t)g * B + b;
    if (n == 0) {
        if (threadIdx.x == 0) { length[at] = NAN; mad[at] = NAN; n_used[at] = 0; }
        return;
    }
    const float med = __uint_as_float(m);
    int n2 = 0;
    const uint32_t d = select_rank<true>(N, B, b, g, measured, groups, med, s_hist, s_pick, n2);
    if (threadIdx.x == 0) { length[at] = med; mad[at] = __uint_as_float(d); n_used[at] = n; }
}

// LDS of k_project, in doubles then ints: x [3 J], Sigma [6 J], u [3 B], lam [B] (right-hand side, then the multipliers),
// col [B], S [B B], res [64]; active [B], moved [J] ints
__host__ __device__ inline size_t project_lds(int J, int B)
{
    return ((size_t)3 * J + 6 * J + 3 * B + B + B + (size_t)B * B + 64) * sizeof(double) + ((size_t)B + J) * sizeof(int);
}

__global__ void __launch_bounds__(PROJECT_THREADS)
k_project(int N, int J, int B, int G, BoneTable bones, const float* __restrict__ xyz, const float* __restrict__ cov6,
          const unsigned char* __restrict__ valid, const int* __restrict__ groups, const float* __restrict__ lengths,
          double cov_floor, int max_iters, double tol, float* __restrict__ out_xyz, float* __restrict__ residual,
          int* __restrict__ n_trips, int* __restrict__ n_active)
{
    extern __shared__ double s_mem[];
    double* s_x = s_mem;                    // [J][3]
    double* s_sig = s_x + 3 * J;            // [J][6]
    double* s_u = s_sig + 6 * J;            // [B][3]
    double* s_lam = s_u + 3 * B;            // [B]
    double* s_col = s_lam + B;              // [B]
    double* s_S = s_col + B;                // [B][B], lower triangle
    double* s_res = s_S + B * B;            // [64]
    int* s_act = reinterpret_cast<int*>(s_res + 64);    // [B]
    int* s_moved = s_act + B;               // [J]
    const int lane = threadIdx.x;
    const long long f = blockIdx.x;
    const float* y = xyz + (size_t)f * J * 3;

    // joints: the iterate, the covariance and whether the joint may carry an active bone
    int joint_ok = 0;
    if (lane < J) {
        const float* yj = y + 3 * lane;
        bool ok = finite3(yj) && (!valid || valid[(size_t)f * J + lane] != 0);
        double S[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
        if (cov6) {
            const float* c = cov6 + ((size_t)f * J + lane) * 6;
            S[0] = (double)c[0] + cov_floor; S[1] = (double)c[1]; S[2] = (double)c[2];
            S[3] = (double)c[3] + cov_floor; S[4] = (double)c[4]; S[5] = (double)c[5] + cov_floor;
            bool fin = true;
#pragma unroll
            for (int e = 0; e < 6; e++) fin = fin && isfinite(S[e]);
            ok = ok && fin && positive3(S[0], S[1], S[2], S[3], S[4], S[5]);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) s_x[3 * lane + k] = (double)yj[k];
#pragma unroll
        for (int e = 0; e < 6; e++) s_sig[6 * lane + e] = S[e];
        s_moved[lane] = 0;
        joint_ok = ok ? 1 : 0;
    }
    // bit j: joint j is usable
    const unsigned long long ok_mask = __ballot(joint_ok);
    const int g = groups ? groups[f] : 0;
    const int bp = lane < B ? bones.p[lane] : 0, bc = lane < B ? bones.c[lane] : 0;
    double L = 0.0;
    bool active = false;
    if (lane < B && g >= 0 && g < G) {
        L = (double)lengths[(size_t)g * B + lane];
        active = ((ok_mask >> bp) & 1ull) && ((ok_mask >> bc) & 1ull) && isfinite(L) && L > 0.0;
    }
    __syncthreads();

    int trips = 0;
    double res = (double)NAN;
    int n_act = 0;
    for (;;) {
        // 1. the bones' lengths, directions and residuals at the iterate
        double r = 0.0;
        if (active) {
            double d[3];
#pragma unroll
            for (int k = 0; k < 3; k++) d[k] = s_x[3 * bc + k] - s_x[3 * bp + k];
            const double n = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            if (n == 0.0) active = false;                           // (from here on: the header's contract)
            else {
#pragma unroll
                for (int k = 0; k < 3; k++) s_u[3 * lane + k] = d[k] / n;
                r = n - L;
            }
        }
        if (lane < B) { s_act[lane] = active ? 1 : 0; s_lam[lane] = active ? r : 0.0; }
        s_res[lane] = active ? (isfinite(r) ? fabs(r) : (double)INFINITY) : 0.0;
        n_act = __popcll(__ballot(active ? 1 : 0));
        __syncthreads();
        if (n_act == 0) break;                                      // (a copy when it is the first trip)
        res = 0.0;
        for (int i = 0; i < B; i++) res = fmax(res, s_res[i]);      // (no NaN among them: exact, whatever the order)
        if (res <= tol || trips == max_iters) break;

        // 2. S = A Sigma A^T, lower triangle: lane b <= a makes S[a][b]
        for (int a = 0; a < B; a++) {
            if (lane > a) continue;
            double s = lane == a ? 1.0 : 0.0;
            const int pa = bones.p[a], ca = bones.c[a];
            if (s_act[a] && active) {
                const double* ua = s_u + 3 * a;
                const double* ub = s_u + 3 * lane;
                s = 0.0;
                if (pa == bp) s = s + quad3(ua, s_sig + 6 * pa, ub);
                if (pa == bc) s = s - quad3(ua, s_sig + 6 * pa, ub);
                if (ca == bp) s = s - quad3(ua, s_sig + 6 * ca, ub);
                if (ca == bc) s = s + quad3(ua, s_sig + 6 * ca, ub);
            } else if (lane == a) s = 1.0;
            else s = 0.0;
            s_S[a * B + lane] = s;
        }
        __syncthreads();

        // 3. LDL^T in place, right-looking, the right-hand side with it; lane i owns row i
        bool pivots = true;
        for (int j = 0; j < B; j++) {
            const double dj = s_S[j * B + j];
            pivots = pivots && isfinite(dj) && dj > 0.0;
            double li = 0.0;
            if (lane > j && lane < B) {
                li = s_S[lane * B + j] / dj;
                s_col[lane] = li;
                for (int c = j + 1; c <= lane; c++) s_S[lane * B + c] = s_S[lane * B + c] - li * s_S[c * B + j];
            }
            __syncthreads();                                        // column j is read undivided up to here
            if (lane > j && lane < B) {
                s_S[lane * B + j] = li;
                s_lam[lane] = s_lam[lane] - li * s_lam[j];
            }
            __syncthreads();
        }
        if (!pivots) break;                                         // (every lane read the same pivots: the wave leaves)
        if (lane < B) s_lam[lane] = s_lam[lane] / s_S[lane * B + lane];
        __syncthreads();
        for (int j = B - 1; j >= 1; j--) {
            if (lane < j) s_lam[lane] = s_lam[lane] - s_S[j * B + lane] * s_lam[j];
            __syncthreads();
        }

        // 4. x <- x - Sigma A^T lambda: lane j owns joint j, the bones in index order
        if (lane < J) {
            double gsum[3] = {0.0, 0.0, 0.0};
            bool touched = false;
            for (int b = 0; b < B; b++) {
                if (!s_act[b]) continue;
                const double lam = s_lam[b];
                if (bones.c[b] == lane) {
                    touched = true;
#pragma unroll
                    for (int k = 0; k < 3; k++) gsum[k] = gsum[k] + lam * s_u[3 * b + k];
                }
                if (bones.p[b] == lane) {
                    touched = true;
#pragma unroll
                    for (int k = 0; k < 3; k++) gsum[k] = gsum[k] - lam * s_u[3 * b + k];
                }
            }
            if (touched) {
                const double* S = s_sig + 6 * lane;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double step = (S[SYM[k][0]] * gsum[0] + S[SYM[k][1]] * gsum[1]) + S[SYM[k][2]] * gsum[2];
                    s_x[3 * lane + k] = s_x[3 * lane + k] - step;
                }
                s_moved[lane] = 1;
            }
        }
        trips++;
        __syncthreads();
    }

    if (lane < J) {
        float* o = out_xyz + ((size_t)f * J + lane) * 3;
        const float* yj = y + 3 * lane;
        if (s_moved[lane]) {
#pragma unroll
            for (int k = 0; k < 3; k++) o[k] = (float)s_x[3 * lane + k];
        } else {
            // every bit of the input, NaN payloads included: moved as integers
            const uint32_t* src = reinterpret_cast<const uint32_t*>(yj);
            uint32_t* dst = reinterpret_cast<uint32_t*>(o);
#pragma unroll
            for (int k = 0; k < 3; k++) dst[k] = src[k];
        }
    }
    if (lane == 0) {
        residual[f] = (float)res;
        n_trips[f] = trips;
        n_active[f] = n_act;
    }
}

// The checks the three entry points share; fills `t`.  bones: HOST (B,2) ints.
int check_bones(const char* who, int N, int J, int B, const int* bones, BoneTable* t)
{
    if (N < 1 || N > (1 << 26)) return fail2(-1, "%s: N = %d frames, 1 .. 2^26", who, N);
    if (J < 2 || J > SKS_BONES_MAX_JOINTS) return fail2(-1, "%s: J = %d joints, 2 .. %d (SKS_BONES_MAX_JOINTS)", who, J, SKS_BONES_MAX_JOINTS);
    if (B < 1 || B > SKS_BONES_MAX_JOINTS - 1) return fail2(-1, "%s: B = %d bones, 1 .. %d", who, B, SKS_BONES_MAX_JOINTS - 1);
    if (!bones) return fail2(-2, "%s: missing bones (HOST, (B,2) ints: parent, child)", who);
    int root[SKS_BONES_MAX_JOINTS];
    for (int j = 0; j < J; j++) root[j] = j;
    for (int b = 0; b < B; b++) {
        const int p = bones[2 * b], c = bones[2 * b + 1];
        if (p < 0 || p >= J || c < 0 || c >= J) return fail2(-1, "%s: bone %d = (%d, %d) names a joint outside 0 .. %d", who, b, p, c, J - 1);
        int rp = p, rc = c;
        while (root[rp] != rp) rp = root[rp];
        while (root[rc] != rc) rc = root[rc];
        if (rp == rc) return fail2(-1, "%s: bone %d = (%d, %d) closes a cycle: the bones must form a forest", who, b, p, c);
        root[rc] = rp;
        t->p[b] = (unsigned char)p;
        t->c[b] = (unsigned char)c;
    }
    return 0;
}

int check_groups(const char* who, const int* groups, int G)
{
    if (G < 1 || G > SKS_BONES_MAX_GROUPS) return fail2(-1, "%s: n_groups = %d, 1 .. %d (SKS_BONES_MAX_GROUPS)", who, G, SKS_BONES_MAX_GROUPS);
    if (!groups && G != 1) return fail2(-2, "%s: n_groups = %d without groups (NULL groups: one group)", who, G);
    return 0;
}

}  // namespace

extern "C" int sks_bones_launch(int N, int J, int B, int n_groups, int* out)
{
    if (N < 1 || N > (1 << 26) || J < 2 || J > SKS_BONES_MAX_JOINTS || B < 1 || B > SKS_BONES_MAX_JOINTS - 1 || n_groups < 1 ||
        n_groups > SKS_BONES_MAX_GROUPS)
        return fail2(-1, "bones_launch: N = %d (1 .. 2^26), J = %d (2 .. %d), B = %d (1 .. %d), n_groups = %d (1 .. %d)", N, J,
                     SKS_BONES_MAX_JOINTS, B, SKS_BONES_MAX_JOINTS - 1, n_groups, SKS_BONES_MAX_GROUPS);
    if (!out) return fail2(-2, "bones_launch: missing out (SKS_BONES_LAUNCH_INTS ints)");
    out[SKS_BONES_MEASURE_GROUPS] = (int)(((long long)N * B + MEASURE_THREADS - 1) / MEASURE_THREADS);
    out[SKS_BONES_MEASURE_THREADS] = MEASURE_THREADS;
    out[SKS_BONES_LENGTHS_GROUPS] = n_groups * B;
    out[SKS_BONES_LENGTHS_THREADS] = LENGTHS_THREADS;
    out[SKS_BONES_LENGTHS_LDS_BYTES] = (256 + 3) * (int)sizeof(int);
    out[SKS_BONES_PROJECT_GROUPS] = N;
    out[SKS_BONES_PROJECT_THREADS] = PROJECT_THREADS;
    out[SKS_BONES_PROJECT_LDS_BYTES] = (int)project_lds(J, B);
    return 0;
}

extern "C" int sks_bone_measure(int N, int J, int B, const int* bones, const float* xyz, const float* cov6,
                                const unsigned char* valid, double max_sigma_mm, float* measured, void* stream)
{
    BoneTable t = {};
    if (int rc = check_bones("bone_measure", N, J, B, bones, &t)) return rc;
    if (!xyz) return fail2(-2, "bone_measure: missing xyz (N,J,3) floats");
    if (!measured) return fail2(-2, "bone_measure: missing measured (N,B) floats");
    if (cov6 && (!(max_sigma_mm >= 0.0) || !isfinite(max_sigma_mm)))
        return fail2(-1, "bone_measure: max_sigma_mm must be finite and >= 0 with cov6, got %g", max_sigma_mm);
    const int groups = (int)(((long long)N * B + MEASURE_THREADS - 1) / MEASURE_THREADS);
    hipLaunchKernelGGL(k_measure, dim3(groups), dim3(MEASURE_THREADS), 0, (hipStream_t)stream, N, J, B, t, xyz, cov6, valid,
                       cov6 ? max_sigma_mm * max_sigma_mm : 0.0, measured);
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" int sks_bone_lengths(int N, int B, const float* measured, const int* groups, int n_groups, float* length, float* mad,
                                int* n_used, void* stream)
{
    if (N < 1 || N > (1 << 26)) return fail2(-1, "bone_lengths: N = %d frames, 1 .. 2^26", N);
    if (B < 1 || B > SKS_BONES_MAX_JOINTS - 1) return fail2(-1, "bone_lengths: B = %d bones, 1 .. %d", B, SKS_BONES_MAX_JOINTS - 1);
    if (int rc = check_groups("bone_lengths", groups, n_groups)) return rc;
    if (!measured) return fail2(-2, "bone_lengths: missing measured (N,B) floats");
    if (!length || !mad || !n_used) return fail2(-2, "bone_lengths: missing length / mad (G,B) floats or n_used (G,B) ints");
    hipLaunchKernelGGL(k_lengths, dim3(B, n_groups), dim3(LENGTHS_THREADS), 0, (hipStream_t)stream, N, B, measured, groups, length,
                       mad, n_used);
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" int sks_bone_project(int N, int J, int B, const int* bones, const float* xyz, const float* cov6,
                                const unsigned char* valid, const int* groups, int n_groups, const float* lengths,
                                double cov_floor, int max_iters, double tol_mm, float* out_xyz, float* residual, int* n_trips,
                                int* n_active, void* stream)
{
    BoneTable t = {};
    if (int rc = check_bones("bone_project", N, J, B, bones, &t)) return rc;
    if (int rc = check_groups("bone_project", groups, n_groups)) return rc;
    if (max_iters < 1 || max_iters > SKS_BONES_MAX_ITERS) return fail2(-1, "bone_project: max_iters = %d, 1 .. %d (SKS_BONES_MAX_ITERS)", max_iters, SKS_BONES_MAX_ITERS);
    if (!(cov_floor >= 0.0) || !isfinite(cov_floor)) return fail2(-1, "bone_project: cov_floor must be finite and >= 0 mm^2, got %g", cov_floor);
    if (!(tol_mm >= 0.0) || !isfinite(tol_mm)) return fail2(-1, "bone_project: tol_mm must be finite and >= 0, got %g", tol_mm);
    if (!xyz) return fail2(-2, "bone_project: missing xyz (N,J,3) floats");
    if (!lengths) return fail2(-2, "bone_project: missing lengths (n_groups,B) floats");
    if (!out_xyz || !residual || !n_trips || !n_active)
        return fail2(-2, "bone_project: missing out_xyz (N,J,3) / residual (N) floats or n_trips / n_active (N) ints");
    {
        const uintptr_t a = (uintptr_t)xyz, b = (uintptr_t)out_xyz, bytes = (uintptr_t)N * J * 3 * sizeof(float);
        if (a < b + bytes && b < a + bytes) return fail2(-2, "bone_project: out_xyz overlaps xyz (not in place)");
    }
    hipLaunchKernelGGL(k_project, dim3(N), dim3(PROJECT_THREADS), project_lds(J, B), (hipStream_t)stream, N, J, B, n_groups, t, xyz,
                       cov6, valid, groups, lengths, cov_floor, max_iters, tol_mm, out_xyz, residual, n_trips, n_active);
    HIP_TRY2(hipGetLastError());
    return 0;
}
