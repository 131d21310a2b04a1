// sks_smooth.hip -- covariance-weighted temporal smoothing of a sequence of poses, for MI355X: per (frame, joint) a local
// polynomial fit over the frames around it, every tap weighted by the inverse of its own 3x3 covariance (the optimised Gaussian
// of csrc/sks_uncertainty.hip), and the smoothness figures that go with it ("Accel", "Accel error").  The definition of the
// fit, with the order of every sum, stands in include/skelsplat_hip.h above the prototypes; this file follows it op by op in
// float64 and is compiled without FMA contraction like the rest of the library, so a (frame, joint)'s bits are the same wherever
// it is computed.  No square root: the whole fit is + - x / in IEEE float64.
//
// k_smooth<D>.  Layout: a workgroup of 256 threads owns a tile of T consecutive frames x Jc joints (Jc = J, all joints, whenever
//   the stage fits; plan() below), one (frame, joint) per lane.
//   stage:  the tile's frames and h halo frames on each side, S = T + 2h frames x Jc joints.  Neighbouring targets share 2h of
//           their 2h + 1 taps, so what a tap contributes to EVERY target is made once per staged (frame, joint) and parked in
//           LDS: usable?, its weight, its position and its information matrix Lambda = C^-1 (6 doubles).  A staged item is
//           48 + 12 + 4 = 64 bytes, struct-of-arrays (item-major inside every array: adjacent lanes read adjacent banks).
//           Nothing staged is relative to the tile (no tile-wide origin), so a tap's parked bits do not depend on the tile.
//   fit:    each lane walks ITS taps in ascending frame order whatever the tile, adds the moments and right-hand sides in
//           registers (5 x 6 + 3 x 3 = 39 doubles at D = 2), solves by LDL^T and writes its outputs.  A frame's result therefore
//           does not depend on N, on its position in a tile or on the launch shape.
//   The degree is a template argument, so the accumulators are arrays of constant size that stay in registers.
//
// k_eval_accel.  Layout: k_eval_reprojection's: one workgroup of 256 threads per output row (0: all frames, 1 + g: group g); the
//   row's 1 + J columns one after the other; thread t takes frames t + 1, t + 257, ... in index order and a frame's joints in
//   index order, and the 256 partial sums and counts meet in the same fixed tree.  mean = sum / count, NaN over nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"

namespace {

constexpr int SMOOTH_THREADS = 256;
constexpr int SMOOTH_MAX_ITEMS = 1000;      // staged (frame, joint) items per workgroup: 64 000 B + the frames' group ids <= 64 KiB
constexpr int EVAL_THREADS = 256;

// index of entry (r, c) in xx, xy, xz, yy, yz, zz
__device__ constexpr int SYM[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};

struct Ldl3 { double d0, d1, d2, l10, l20, l21; };

// LDL^T of the symmetric 3x3 {xx, xy, xz, yy, yz, zz}: the right-looking sequence of the header, the pivots in order
__device__ __forceinline__ Ldl3 ldl3(double xx, double xy, double xz, double yy, double yz, double zz)
{
    Ldl3 f;
    f.d0 = xx;
    f.l10 = xy / f.d0;
    f.l20 = xz / f.d0;
    f.d1 = yy - f.l10 * xy;
    const double e = yz - f.l20 * xy;
    const double z1 = zz - f.l20 * xz;
    f.l21 = e / f.d1;
    f.d2 = z1 - f.l21 * e;
    return f;
}

__device__ __forceinline__ bool positive(const Ldl3& f)
{
    return isfinite(f.d0) && isfinite(f.d1) && isfinite(f.d2) && f.d0 > 0.0 && f.d1 > 0.0 && f.d2 > 0.0;
}

// (L D L^T)^-1 = L^-T D^-1 L^-1 as xx, xy, xz, yy, yz, zz, with L^-1 = [1 0 0; -l10 1 0; m -l21 1], m = l21 l10 - l20
__device__ __forceinline__ void inverse3(const Ldl3& f, double* inv)
{
    const double i0 = 1.0 / f.d0, i1 = 1.0 / f.d1, i2 = 1.0 / f.d2;
    const double m = f.l21 * f.l10 - f.l20;
    inv[0] = (i0 + (f.l10 * f.l10) * i1) + (m * m) * i2;
    inv[1] = -(f.l10 * i1) - (m * f.l21) * i2;
    inv[2] = m * i2;
    inv[3] = i1 + (f.l21 * f.l21) * i2;
    inv[4] = -(f.l21 * i2);
    inv[5] = i2;
}

// The normal equations of effective degree DE, unknowns ordered c_DE, .., c_1, c_0 so that the position block is eliminated last:
// its 3x3 trailing factor is the Schur complement, whose inverse is the position's covariance.
template <int DE, int D>
__device__ __forceinline__ void solve(const double (&Mo)[2 * D + 1][6], const double (&R)[D + 1][3], double* c0, double* c1, double* cov)
{
    constexpr int M = 3 * (DE + 1);
    double B[M][M], y[M], col[M];
#pragma unroll
    for (int a = 0; a <= DE; a++)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            y[3 * a + r] = R[DE - a][r];
#pragma unroll
            for (int b = 0; b <= a; b++)
#pragma unroll
                for (int c = 0; c < 3; c++)
                    if (3 * b + c <= 3 * a + r) B[3 * a + r][3 * b + c] = Mo[(DE - a) + (DE - b)][SYM[r][c]];
        }
#pragma unroll
    for (int j = 0; j < M; j++) {
        const double dj = B[j][j];
#pragma unroll
        for (int i = j + 1; i < M; i++) col[i] = B[i][j] / dj;
#pragma unroll
        for (int i = j + 1; i < M; i++)
#pragma unroll
            for (int c = j + 1; c <= i; c++) B[i][c] = B[i][c] - col[i] * B[c][j];
#pragma unroll
        for (int i = j + 1; i < M; i++) {
            B[i][j] = col[i];
            y[i] = y[i] - col[i] * y[j];
        }
    }
#pragma unroll
    for (int j = 0; j < M; j++) y[j] = y[j] / B[j][j];
#pragma unroll
    for (int j = M - 1; j >= 1; j--)
#pragma unroll
        for (int i = 0; i < j; i++) y[i] = y[i] - B[j][i] * y[j];
    c0[0] = y[M - 3]; c0[1] = y[M - 2]; c0[2] = y[M - 1];
    if (DE >= 1) { c1[0] = y[M - 6]; c1[1] = y[M - 5]; c1[2] = y[M - 4]; }
    else { c1[0] = 0.0; c1[1] = 0.0; c1[2] = 0.0; }
    Ldl3 f;
    f.d0 = B[M - 3][M - 3]; f.l10 = B[M - 2][M - 3]; f.l20 = B[M - 1][M - 3];
    f.d1 = B[M - 2][M - 2]; f.l21 = B[M - 1][M - 2]; f.d2 = B[M - 1][M - 1];
    inverse3(f, cov);
}

struct SmoothPlan { int T, Jc, chunks, S, items; size_t lds; };

// The tile of one workgroup: all joints and T = 256 / J frames when T + 2h frames of them fit the stage, else the joints in
// `chunks` equal runs of Jc.  (Jc = 1: T = 256, 320 items at h = 32 -- the search always ends.)
SmoothPlan plan(int J, int h)
{
    SmoothPlan p;
    for (p.chunks = 1;; p.chunks++) {
        p.Jc = (J + p.chunks - 1) / p.chunks;
        p.T = SMOOTH_THREADS / p.Jc;
        p.S = p.T + 2 * h;
        p.items = p.S * p.Jc;
        if (p.items <= SMOOTH_MAX_ITEMS) break;
    }
    p.chunks = (J + p.Jc - 1) / p.Jc;
    p.lds = (size_t)p.items * 64 + (size_t)p.S * 4;
    return p;
}

template <int D>
__global__ void __launch_bounds__(SMOOTH_THREADS)
k_smooth(int N, int J, int T, int Jc, int h, int tricube, double cov_floor, const float* __restrict__ xyz,
         const float* __restrict__ cov6, const float* __restrict__ weights, const unsigned char* __restrict__ valid,
         const int* __restrict__ group_ids, float* __restrict__ out_xyz, float* __restrict__ out_vel, float* __restrict__ out_cov6,
         int* __restrict__ n_used)
{
    extern __shared__ double s_mem[];
    const int S = T + 2 * h, items = S * Jc;
    double* s_lam = s_mem;                                      // [6][items]
    float* s_x = reinterpret_cast<float*>(s_lam + 6 * (size_t)items);      // [3][items]
    float* s_w = s_x + 3 * (size_t)items;                       // [items]: the tap's weight, < 0 = not usable
    int* s_g = reinterpret_cast<int*>(s_w + items);             // [S]
    const int tid = threadIdx.x;
    const int j0 = (int)blockIdx.y * Jc;
    const int jc = min(Jc, J - j0);
    const long long first = (long long)blockIdx.x * T - h;      // the frame of staged row 0 (may lie in front of the sequence)

    for (int i = tid; i < items; i += SMOOTH_THREADS) {
        const int fs = i / Jc, jj = i - fs * Jc;
        const long long k = first + fs;
        float w = -1.0f;
        if (k >= 0 && k < N && jj < jc) {
            const size_t at = (size_t)k * J + (j0 + jj);
            const float x0 = xyz[3 * at], x1 = xyz[3 * at + 1], x2 = xyz[3 * at + 2];
            bool ok = (!valid || valid[at] != 0) && isfinite(x0) && isfinite(x1) && isfinite(x2);
            float wk = 1.0f;
            if (weights) { wk = weights[at]; ok = ok && isfinite(wk) && wk > 0.0f; }
            double lam[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
            if (cov6 && ok) {
                const float* c = cov6 + 6 * at;
                const Ldl3 f = ldl3((double)c[0] + cov_floor, (double)c[1], (double)c[2], (double)c[3] + cov_floor, (double)c[4],
                                    (double)c[5] + cov_floor);
                ok = positive(f);
                if (ok) inverse3(f, lam);
            }
            if (ok) {
                w = wk;
                s_x[i] = x0; s_x[items + i] = x1; s_x[2 * items + i] = x2;
#pragma unroll
                for (int e = 0; e < 6; e++) s_lam[e * items + i] = lam[e];
            }
        }
        s_w[i] = w;
    }
    for (int i = tid; i < S; i += SMOOTH_THREADS) {
        const long long k = first + i;
        s_g[i] = (group_ids && k >= 0 && k < N) ? group_ids[k] : 0;
    }
    __syncthreads();

    const int ft = tid / Jc, jj = tid - ft * Jc;
    const long long f = (long long)blockIdx.x * T + ft;
    if (ft >= T || f >= N || jj >= jc) return;                   // (behind the only barrier)
    double Mo[2 * D + 1][6], R[D + 1][3];
#pragma unroll
    for (int p = 0; p <= 2 * D; p++)
#pragma unroll
        for (int e = 0; e < 6; e++) Mo[p][e] = 0.0;
#pragma unroll
    for (int a = 0; a <= D; a++)
#pragma unroll
        for (int r = 0; r < 3; r++) R[a][r] = 0.0;
    double xo[3] = {0.0, 0.0, 0.0};
    int n = 0;
    const int g = s_g[ft + h];
    const int t_lo = (int)max((long long)-h, -f), t_hi = (int)min((long long)h, (long long)N - 1 - f);
    const double span = (double)(h + 1);
    for (int t = t_lo; t <= t_hi; t++) {
        const int fs = ft + h + t, i = fs * Jc + jj;
        const float w = s_w[i];
        if (!(w > 0.0f) || s_g[fs] != g) continue;
        const double x[3] = {(double)s_x[i], (double)s_x[items + i], (double)s_x[2 * items + i]};
        if (n == 0) { xo[0] = x[0]; xo[1] = x[1]; xo[2] = x[2]; }
        n++;
        double taper = 1.0;
        if (tricube) {
            const double u = fabs((double)t) / span;
            const double q = 1.0 - (u * u) * u;
            taper = (q * q) * q;
        }
        const double omega = (double)w * taper;
        double wl[6];
#pragma unroll
        for (int e = 0; e < 6; e++) wl[e] = omega * s_lam[e * items + i];
        const double dx[3] = {x[0] - xo[0], x[1] - xo[1], x[2] - xo[2]};
        double v[3];
#pragma unroll
        for (int r = 0; r < 3; r++) v[r] = (wl[SYM[r][0]] * dx[0] + wl[SYM[r][1]] * dx[1]) + wl[SYM[r][2]] * dx[2];
        double tp[5];
        tp[0] = 1.0; tp[1] = (double)t; tp[2] = tp[1] * tp[1]; tp[3] = tp[2] * tp[1]; tp[4] = tp[2] * tp[2];
#pragma unroll
        for (int p = 0; p <= 2 * D; p++)
#pragma unroll
            for (int e = 0; e < 6; e++) Mo[p][e] = Mo[p][e] + tp[p] * wl[e];
#pragma unroll
        for (int a = 0; a <= D; a++)
#pragma unroll
            for (int r = 0; r < 3; r++) R[a][r] = R[a][r] + tp[a] * v[r];
    }
    const double nan = (double)NAN;
    double c0[3] = {nan, nan, nan}, c1[3] = {nan, nan, nan}, cov[6] = {nan, nan, nan, nan, nan, nan};
    if (n > 0) {
        const int de = min(D, n - 1);
        if (D >= 2 && de == 2) solve<(D >= 2 ? 2 : D), D>(Mo, R, c0, c1, cov);
        else if (D >= 1 && de == 1) solve<(D >= 1 ? 1 : D), D>(Mo, R, c0, c1, cov);
        else solve<0, D>(Mo, R, c0, c1, cov);
#pragma unroll
        for (int r = 0; r < 3; r++) c0[r] = c0[r] + xo[r];
    }
    const size_t at = (size_t)f * J + (j0 + jj);
    out_xyz[3 * at] = (float)c0[0]; out_xyz[3 * at + 1] = (float)c0[1]; out_xyz[3 * at + 2] = (float)c0[2];
    if (out_vel) { out_vel[3 * at] = (float)c1[0]; out_vel[3 * at + 1] = (float)c1[1]; out_vel[3 * at + 2] = (float)c1[2]; }
    if (out_cov6) {
#pragma unroll
        for (int e = 0; e < 6; e++) out_cov6[6 * at + e] = (float)cov[e];
    }
    if (n_used) n_used[at] = n;
}

// ||x_{f-1} - 2 x_f + x_{f+1}|| of joint j (p: the joint's first float in frame f; stride: floats per frame), minus the ground
// truth's when q is given.  NaN or inf in any of the positions read: not finite, and the caller leaves the entry out.
__device__ __forceinline__ double accel_norm(const float* __restrict__ p, const float* __restrict__ q, size_t stride)
{
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double a = ((double)p[c] - 2.0 * (double)p[stride + c]) + (double)p[2 * stride + c];
        if (q) a = a - (((double)q[c] - 2.0 * (double)q[stride + c]) + (double)q[2 * stride + c]);
        s = c == 0 ? a * a : s + a * a;
    }
    return sqrt(s);
}

__global__ void __launch_bounds__(EVAL_THREADS)
k_eval_accel(int N, int J, const float* __restrict__ xyz, const float* __restrict__ gt, const int* __restrict__ group_ids,
             double* __restrict__ out)
{
    __shared__ double s_sum[2][EVAL_THREADS];
    __shared__ long long s_cnt[2][EVAL_THREADS];
    const int tid = threadIdx.x, g = (int)blockIdx.x - 1;
    const int cols = 1 + J;
    const size_t stride = (size_t)J * 3;
    for (int col = 0; col < cols; col++) {
        const int ja = col == 0 ? 0 : col - 1, jb = col == 0 ? J : col;
        double s[2] = {0.0, 0.0};
        long long c[2] = {0, 0};
        for (long long f = 1 + tid; f < (long long)N - 1; f += EVAL_THREADS) {
            if (group_ids) {
                const int gf = group_ids[f];
                if ((g >= 0 && gf != g) || group_ids[f - 1] != gf || group_ids[f + 1] != gf) continue;
            }
            for (int j = ja; j < jb; j++) {
                const float* p = xyz + (size_t)(f - 1) * stride + 3 * j;
                const double a = accel_norm(p, nullptr, stride);
                if (!isfinite(a)) continue;
                s[0] += a; c[0]++;
                if (!gt) continue;
                const float* q = gt + (size_t)(f - 1) * stride + 3 * j;
                if (!isfinite(accel_norm(q, nullptr, stride))) continue;
                s[1] += accel_norm(p, q, stride); c[1]++;
            }
        }
#pragma unroll
        for (int k = 0; k < 2; k++) { s_sum[k][tid] = s[k]; s_cnt[k][tid] = c[k]; }
        for (int o = EVAL_THREADS / 2; o > 0; o >>= 1) {
            __syncthreads();
            if (tid < o) {
#pragma unroll
                for (int k = 0; k < 2; k++) { s_sum[k][tid] += s_sum[k][tid + o]; s_cnt[k][tid] += s_cnt[k][tid + o]; }
            }
        }
        if (tid == 0) {
            double* row = out + (size_t)blockIdx.x * 2 * cols;
            row[col] = s_sum[0][0] / (double)s_cnt[0][0];              // (nothing entered: 0 / 0 = NaN)
            row[cols + col] = s_sum[1][0] / (double)s_cnt[1][0];
        }
        __syncthreads();
    }
}

int check_smooth_shape(const char* who, int N, int J, int h)
{
    if (N < 1 || N > (1 << 30)) return fail2(-1, "%s: N = %d frames, 1 .. 2^30", who, N);
    if (J < 1 || J > SKS_SMOOTH_MAX_JOINTS) return fail2(-1, "%s: J = %d joints, 1 .. %d (SKS_SMOOTH_MAX_JOINTS)", who, J, SKS_SMOOTH_MAX_JOINTS);
    if (h < 1 || h > SKS_SMOOTH_MAX_HALF_WINDOW)
        return fail2(-1, "%s: half_window = %d, 1 .. %d (SKS_SMOOTH_MAX_HALF_WINDOW)", who, h, SKS_SMOOTH_MAX_HALF_WINDOW);
    return 0;
}

template <int D>
void launch_smooth(const SmoothPlan& p, hipStream_t stream, int N, int J, int h, int taper, double cov_floor, const float* xyz,
                   const float* cov6, const float* weights, const unsigned char* valid, const int* group_ids, float* out_xyz,
                   float* out_vel, float* out_cov6, int* n_used)
{
    hipLaunchKernelGGL(k_smooth<D>, dim3((N + p.T - 1) / p.T, p.chunks), dim3(SMOOTH_THREADS), p.lds, stream, N, J, p.T, p.Jc, h,
                       taper == SKS_SMOOTH_TRICUBE ? 1 : 0, cov_floor, xyz, cov6, weights, valid, group_ids, out_xyz, out_vel,
                       out_cov6, n_used);
}

}  // namespace

extern "C" int sks_smooth_launch(int N, int J, int half_window, int* out)
{
    if (int rc = check_smooth_shape("smooth_launch", N, J, half_window)) return rc;
    if (!out) return fail2(-2, "smooth_launch: missing out (SKS_SMOOTH_LAUNCH_INTS ints)");
    const SmoothPlan p = plan(J, half_window);
    out[SKS_SMOOTH_TILE] = p.T;
    out[SKS_SMOOTH_GROUPS] = ((N + p.T - 1) / p.T) * p.chunks;
    out[SKS_SMOOTH_THREADS] = SMOOTH_THREADS;
    out[SKS_SMOOTH_LDS_BYTES] = (int)p.lds;
    return 0;
}

extern "C" int sks_smooth_sequence(int N, int J, const float* xyz, const float* cov6, const float* weights,
                                   const unsigned char* valid, const int* group_ids, int half_window, int degree, int taper,
                                   double cov_floor, float* out_xyz, float* out_vel, float* out_cov6, int* n_used, void* stream)
{
    if (int rc = check_smooth_shape("smooth_sequence", N, J, half_window)) return rc;
    if (degree < 0 || degree > 2) return fail2(-1, "smooth_sequence: degree = %d, 0 .. 2", degree);
    if (taper != SKS_SMOOTH_BOX && taper != SKS_SMOOTH_TRICUBE)
        return fail2(-1, "smooth_sequence: taper = %d, SKS_SMOOTH_BOX (0) or SKS_SMOOTH_TRICUBE (1)", taper);
    if (!(cov_floor >= 0.0) || !isfinite(cov_floor)) return fail2(-1, "smooth_sequence: cov_floor must be finite and >= 0 mm^2, got %g", cov_floor);
    if (!xyz) return fail2(-2, "smooth_sequence: missing xyz (N,J,3) floats");
    if (!out_xyz) return fail2(-2, "smooth_sequence: missing out_xyz (N,J,3) floats");
    {
        // a workgroup reads its halo frames, which another workgroup writes: in place is refused
        const uintptr_t a = (uintptr_t)xyz, b = (uintptr_t)out_xyz, bytes = (uintptr_t)N * J * 3 * sizeof(float);
        if (a < b + bytes && b < a + bytes) return fail2(-2, "smooth_sequence: out_xyz overlaps xyz (a tile reads its neighbours' frames: not in place)");
    }
    const SmoothPlan p = plan(J, half_window);
    const hipStream_t st = (hipStream_t)stream;
    if (degree == 0)
        launch_smooth<0>(p, st, N, J, half_window, taper, cov_floor, xyz, cov6, weights, valid, group_ids, out_xyz, out_vel, out_cov6, n_used);
    else if (degree == 1)
        launch_smooth<1>(p, st, N, J, half_window, taper, cov_floor, xyz, cov6, weights, valid, group_ids, out_xyz, out_vel, out_cov6, n_used);
    else
        launch_smooth<2>(p, st, N, J, half_window, taper, cov_floor, xyz, cov6, weights, valid, group_ids, out_xyz, out_vel, out_cov6, n_used);
    HIP_TRY2(hipGetLastError());
    return 0;
}

extern "C" int sks_eval_accel(int N, int J, const float* xyz, const float* gt, const int* group_ids, int n_groups, double* out,
                              void* stream)
{
    if (N < 1 || N > (1 << 30) || J < 1) return fail2(-1, "eval_accel: N = %d frames (1 .. 2^30) of J = %d joints (at least 1)", N, J);
    if (n_groups < 0 || n_groups > SKS_EVAL_MAX_GROUPS) return fail2(-1, "eval_accel: n_groups = %d, 0 .. %d (SKS_EVAL_MAX_GROUPS)", n_groups, SKS_EVAL_MAX_GROUPS);
    if (!xyz) return fail2(-2, "eval_accel: missing xyz (N,J,3) floats");
    if (!out) return fail2(-2, "eval_accel: missing out (1 + n_groups, 2, 1 + J) doubles");
    if (n_groups > 0 && !group_ids) return fail2(-2, "eval_accel: n_groups = %d without group_ids", n_groups);
    hipLaunchKernelGGL(k_eval_accel, dim3(1 + n_groups), dim3(EVAL_THREADS), 0, (hipStream_t)stream, N, J, xyz, gt, group_ids, out);
    HIP_TRY2(hipGetLastError());
    return 0;
}
