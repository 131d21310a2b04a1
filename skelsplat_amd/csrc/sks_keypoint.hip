// sks_keypoint.hip -- the keypoint read out of heat-map planes (reference: utils/loss_utils.py:41-64 `softargmax2d`) for
// MI355X (gfx950, wave64), forward and backward.
//
// A "plane" is one (H, W) channel of one view; a call takes `planes` contiguous planes of one size.  Per plane
//     p = softmax(beta * x)  over the H * W pixels,    xy = (sum p * col, sum p * row)          [pixels]
// (the reference weights with linspace(0, 1, w) and multiplies by w - 1 afterwards: the same number, also for w == 1).
//
// Forward, two launches:
//   k_softargmax_partial  grid (chunk, plane): a workgroup streams SA_CHUNK consecutive elements of its plane ONCE.  Every thread
//       keeps an online-softmax quadruple {m, s = sum e, s_c = sum e * col, s_r = sum e * row}, e = exp(beta * (x - m)), which it
//       rescales when m rises; the four terms of a 16-byte group are added in fp32 and every group's sums go into DOUBLE
//       accumulators (as k_masked_l2 does).  The workgroup agrees on its maximum through LDS, every thread rescales once to it in
//       fp64, the sums are reduced over the wave (fixed butterfly) and over the waves in wave order, and ONE quadruple per
//       (plane, chunk) goes to scratch.
//   k_softargmax_merge    one wave per plane: the plane's maximum over its chunk quadruples, every quadruple rescaled to it in fp64,
//       lane L adds chunks L, L + 64, ... in ascending order, then the fixed butterfly.  Writes xy and the stats record
//       {m, 1 / s, E[col], E[row], and the parts of E[col], E[row] their floats miss} the backward needs: col - E[col] cancels
//       next to the peak, where p is largest, and half an ulp of a coordinate near 1000 (3e-5 px) times beta * p is 100 times
//       the standing gradient tolerance; (col - hi) is exact in fp32, so (col - hi) - lo carries the fp64 expectation.
// Two launches on purpose: a "last workgroup to finish" tail needs device-scope atomics and fences.  No atomics anywhere; the order
// of every addition is fixed by (W, H) alone, so results are bit-identical from run to run and do not depend on `planes` or on
// where a plane sits in the batch -- EXCEPT through the plane's alignment: plane starts are only 4-byte aligned when H * W is no
// multiple of 4, so a chunk is a scalar head up to the first 16-byte boundary, 16-byte groups, and a scalar tail.  (The head's
// length depends on the plane's address; it moves elements between a thread's fp32 group sums, i.e. the last bits.)
//
// Backward, one launch, one read and one write of the image:
//   k_softargmax_bwd      dL/dx = beta * p * (g_c * (col - E[col]) + g_r * (row - E[row])),  p = exp(beta * (x - m)) * (1 / s),
//       same chunks, same head / groups / tail.
// All element offsets are size_t (31 x 19 x 1920 x 1080 floats exceed 2^32 bytes); an index INSIDE a plane fits an int.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"
#include "sks_math.h"

namespace {

using sks::wave_sum_d;
typedef float kp_v4f __attribute__((ext_vector_type(4)));

constexpr int SA_THREADS = 256;
constexpr int SA_WAVES = SA_THREADS / 64;
constexpr int SA_CHUNK = 16384;                 // elements per workgroup: 16 groups of 16 bytes per thread
constexpr int SA_UNROLL = 4;                    // 16-byte loads in flight per thread
static_assert(SA_CHUNK % 4 == 0, "every chunk of a plane starts at the same offset from a 16-byte boundary");

// where a chunk's scalar head, 16-byte groups and scalar tail lie
struct Span {
    int begin, len, head, nvec, tail;           // elements, relative to the plane
};

__device__ __forceinline__ Span chunk_span(const float* plane, int n, int chunk)
{
    Span s;
    s.begin = chunk * SA_CHUNK;
    s.len = min(SA_CHUNK, n - s.begin);
    const int mis = (int)((reinterpret_cast<uintptr_t>(plane + s.begin) >> 2) & 3);    // floats past a 16-byte boundary
    s.head = min(s.len, (4 - mis) & 3);
    s.nvec = (s.len - s.head) >> 2;
    s.tail = s.len - s.head - 4 * s.nvec;
    return s;
}

// (col, row) of a thread's current element and the constant step between its 16-byte groups
struct Walk {
    int col, row, dcol, drow, W;
    __device__ __forceinline__ void start(int idx, int step, int W_)
    {
        W = W_;
        row = idx / W; col = idx - row * W;
        drow = step / W; dcol = step - drow * W;
    }
    __device__ __forceinline__ void advance()
    {
        col += dcol; row += drow;
        if (col >= W) { col -= W; row++; }
    }
};

// the next element of a run: one column on, wrapping into the next row (any W >= 1)
__device__ __forceinline__ void next_pixel(int& c, int& r, int W)
{
    if (++c == W) { c = 0; r++; }
}

struct Online {
    float m;
    double s, sc, sr;
    __device__ __forceinline__ void raise(float gm, float beta)
    {
        if (gm > m) {
            const double f = (double)__expf(beta * (m - gm));    // m == -inf: 0 times sums that are still 0
            s *= f; sc *= f; sr *= f;
            m = gm;
        }
    }
    __device__ __forceinline__ void one(float x, int c, int r, float beta)
    {
        raise(x, beta);
        const float e = __expf(beta * (x - m));
        s += (double)e; sc += (double)(e * (float)c); sr += (double)(e * (float)r);
    }
    __device__ __forceinline__ void four(const float4& v, int c, int r, int W, float beta)
    {
        raise(fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)), beta);
        const float x[4] = {v.x, v.y, v.z, v.w};
        float e4 = 0.0f, c4 = 0.0f, r4 = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float e = __expf(beta * (x[k] - m));
            e4 += e;
            c4 = __builtin_fmaf(e, (float)c, c4);
            r4 = __builtin_fmaf(e, (float)r, r4);
            next_pixel(c, r, W);
        }
        s += (double)e4; sc += (double)c4; sr += (double)r4;
    }
};

__global__ __launch_bounds__(SA_THREADS) void k_softargmax_partial(int n /* H * W */, int W, float beta,
                                                                  const float* __restrict__ img, double* __restrict__ scratch)
{
    __shared__ float s_max[SA_WAVES];
    __shared__ double s_red[3][SA_WAVES];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const size_t plane = blockIdx.y;
    const float* base = img + plane * (size_t)n;
    const Span sp = chunk_span(base, n, chunk);
    const float* p = base + sp.begin;
    Online q = {-__builtin_huge_valf(), 0.0, 0.0, 0.0};

    if (tid < sp.head) {
        const int idx = sp.begin + tid, r = idx / W;
        q.one(p[tid], idx - r * W, r, beta);
    }
    const float4* pv = reinterpret_cast<const float4*>(p + sp.head);
    Walk w;
    w.start(sp.begin + sp.head + 4 * tid, 4 * SA_THREADS, W);
    int g = tid;
    for (; g + (SA_UNROLL - 1) * SA_THREADS < sp.nvec; g += SA_UNROLL * SA_THREADS) {
        float4 v[SA_UNROLL];
#pragma unroll
        for (int u = 0; u < SA_UNROLL; u++) v[u] = pv[g + u * SA_THREADS];
#pragma unroll
        for (int u = 0; u < SA_UNROLL; u++) {
            q.four(v[u], w.col, w.row, W, beta);
            w.advance();
        }
    }
    for (; g < sp.nvec; g += SA_THREADS) {
        q.four(pv[g], w.col, w.row, W, beta);
        w.advance();
    }
    if (tid < sp.tail) {
        const int off = sp.head + 4 * sp.nvec + tid, idx = sp.begin + off, r = idx / W;
        q.one(p[off], idx - r * W, r, beta);
    }

    // the workgroup's maximum, then every thread's sums on that scale (fp64), then the sums in a fixed order
    float wm = q.m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) wm = fmaxf(wm, __shfl_xor(wm, o, 64));
    if ((tid & 63) == 0) s_max[tid >> 6] = wm;
    __syncthreads();
    float M = s_max[0];
#pragma unroll
    for (int k = 1; k < SA_WAVES; k++) M = fmaxf(M, s_max[k]);
    const double f = q.s > 0.0 ? exp((double)beta * ((double)q.m - (double)M)) : 0.0;    // (a thread without elements: 0)
    const double S = wave_sum_d(q.s * f), Sc = wave_sum_d(q.sc * f), Sr = wave_sum_d(q.sr * f);
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = S; s_red[1][tid >> 6] = Sc; s_red[2][tid >> 6] = Sr; }
    __syncthreads();
    if (tid == 0) {
        double t[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < SA_WAVES; k++) { t[0] += s_red[0][k]; t[1] += s_red[1][k]; t[2] += s_red[2][k]; }
        double* o = scratch + (plane * gridDim.x + chunk) * 4;
        o[0] = (double)M; o[1] = t[0]; o[2] = t[1]; o[3] = t[2];
    }
}

__global__ __launch_bounds__(64) void k_softargmax_merge(int nchunks, float beta, const double* __restrict__ scratch,
                                                        float* __restrict__ xy, float* __restrict__ stats)
{
    const size_t plane = blockIdx.x;
    const int lane = threadIdx.x;
    const double* q = scratch + plane * (size_t)nchunks * 4;
    double M = -__builtin_huge_val();
    for (int k = lane; k < nchunks; k += 64) M = fmax(M, q[4 * k]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) M = fmax(M, __shfl_xor(M, o, 64));
    double s = 0.0, sc = 0.0, sr = 0.0;
    for (int k = lane; k < nchunks; k += 64) {
        const double f = exp((double)beta * (q[4 * k] - M));
        s += q[4 * k + 1] * f; sc += q[4 * k + 2] * f; sr += q[4 * k + 3] * f;
    }
    s = wave_sum_d(s); sc = wave_sum_d(sc); sr = wave_sum_d(sr);
    if (lane == 0) {
        const float ec = (float)(sc / s), er = (float)(sr / s);
        xy[plane * 2] = ec; xy[plane * 2 + 1] = er;
        float* st = stats + plane * SKS_SOFTARGMAX_STATS;
        st[0] = (float)M; st[1] = (float)(1.0 / s); st[2] = ec; st[3] = er;
        st[4] = (float)(sc / s - (double)ec); st[5] = (float)(sr / s - (double)er);
    }
}

__global__ __launch_bounds__(SA_THREADS) void k_softargmax_bwd(int n, int W, float beta, const float* __restrict__ img,
                                                              const float* __restrict__ stats, const float* __restrict__ dL_dxy,
                                                              float* __restrict__ dL_dimg)
{
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const size_t plane = blockIdx.y;
    const float* base = img + plane * (size_t)n;
    const Span sp = chunk_span(base, n, chunk);
    const float* p = base + sp.begin;
    float* d = dL_dimg + plane * (size_t)n + sp.begin;      // (the same offset from `dL_dimg` as `p` from `img`)
    const float* st = stats + plane * SKS_SOFTARGMAX_STATS;
    const float m = st[0], inv_s = st[1], ec = st[2], er = st[3], ec_lo = st[4], er_lo = st[5];
    const float gc = dL_dxy[plane * 2], gr = dL_dxy[plane * 2 + 1];
    auto one = [&](float x, int c, int r) -> float {
        const float pr = __expf(beta * (x - m)) * inv_s;
        return beta * pr * (gc * (((float)c - ec) - ec_lo) + gr * (((float)r - er) - er_lo));
    };
    if (tid < sp.head) {
        const int idx = sp.begin + tid, r = idx / W;
        d[tid] = one(p[tid], idx - r * W, r);
    }
    const float4* pv = reinterpret_cast<const float4*>(p + sp.head);
    // the gradient is stored 16 bytes at a time only where it is as aligned as the image; else element by element
    const bool vec_store = ((reinterpret_cast<uintptr_t>(d + sp.head) & 15) == 0);
    kp_v4f* dv = reinterpret_cast<kp_v4f*>(d + sp.head);
    Walk w;
    w.start(sp.begin + sp.head + 4 * tid, 4 * SA_THREADS, W);
    auto four = [&](const float4& v, int g) {
        int c = w.col, r = w.row;
        kp_v4f o;
        o.x = one(v.x, c, r); next_pixel(c, r, W);
        o.y = one(v.y, c, r); next_pixel(c, r, W);
        o.z = one(v.z, c, r); next_pixel(c, r, W);
        o.w = one(v.w, c, r);
        if (vec_store) {
            __builtin_nontemporal_store(o, dv + g);
        } else {
            float* ds = d + sp.head + 4 * (size_t)g;
            ds[0] = o.x; ds[1] = o.y; ds[2] = o.z; ds[3] = o.w;
        }
        w.advance();
    };
    int g = tid;
    for (; g + (SA_UNROLL - 1) * SA_THREADS < sp.nvec; g += SA_UNROLL * SA_THREADS) {
        float4 v[SA_UNROLL];
#pragma unroll
        for (int u = 0; u < SA_UNROLL; u++) v[u] = pv[g + u * SA_THREADS];
#pragma unroll
        for (int u = 0; u < SA_UNROLL; u++) four(v[u], g + u * SA_THREADS);
    }
    for (; g < sp.nvec; g += SA_THREADS) four(pv[g], g);
    if (tid < sp.tail) {
        const int off = sp.head + 4 * sp.nvec + tid, idx = sp.begin + off, r = idx / W;
        d[off] = one(p[off], idx - r * W, r);
    }
}

// planes, W, H >= 1, a plane's element count fits an int, and both grid dimensions fit
int check_sizes(const char* what, long long planes, int W, int H, int* n, int* nchunks)
{
    if (planes < 1 || W < 1 || H < 1) return fail2(-1, "%s: planes, W and H must be at least 1 (got %lld, %d, %d)", what, planes, W, H);
    const long long nn = (long long)W * H;
    if (nn > 0x7fffffffLL - SA_CHUNK) return fail2(-1, "%s: a plane of %d x %d elements is too large", what, W, H);
    if (planes > 65535) return fail2(-1, "%s: %lld planes, one call takes at most 65535", what, planes);
    *n = (int)nn;
    *nchunks = (int)((nn + SA_CHUNK - 1) / SA_CHUNK);
    return 0;
}

}  // namespace

extern "C" {

size_t sks_softargmax_scratch_bytes(int planes, int W, int H)
{
    int n, nchunks;
    if (check_sizes("softargmax_scratch_bytes", planes, W, H, &n, &nchunks)) return 0;
    return (size_t)planes * (size_t)nchunks * 4 * sizeof(double);
}

int sks_softargmax_fwd(int planes, int W, int H, float beta, const float* img, float* xy, float* stats, void* scratch,
                       size_t scratch_bytes, void* stream)
{
    int n, nchunks;
    if (int rc = check_sizes("softargmax_fwd", planes, W, H, &n, &nchunks)) return rc;
    const size_t need = (size_t)planes * (size_t)nchunks * 4 * sizeof(double);
    if (scratch_bytes < need) return fail2(-1, "softargmax_fwd: scratch of %zu bytes, %d planes of %d x %d need %zu (sks_softargmax_scratch_bytes)", scratch_bytes, planes, W, H, need);
    if (!img || !xy || !stats || !scratch) return fail2(-2, "softargmax_fwd: missing pointer");
    if ((reinterpret_cast<uintptr_t>(img) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 7)) return fail2(-2, "softargmax_fwd: img must be 4-byte and scratch 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_softargmax_partial, dim3(nchunks, planes), dim3(SA_THREADS), 0, st, n, W, beta, img, (double*)scratch);
    HIP_TRY2(hipGetLastError());
    hipLaunchKernelGGL(k_softargmax_merge, dim3(planes), dim3(64), 0, st, nchunks, beta, (const double*)scratch, xy, stats);
    HIP_TRY2(hipGetLastError());
    return 0;
}

int sks_softargmax_bwd(int planes, int W, int H, float beta, const float* img, const float* stats, const float* dL_dxy,
                       float* dL_dimg, void* stream)
{
    int n, nchunks;
    if (int rc = check_sizes("softargmax_bwd", planes, W, H, &n, &nchunks)) return rc;
    if (!img || !stats || !dL_dxy || !dL_dimg) return fail2(-2, "softargmax_bwd: missing pointer");
    if ((reinterpret_cast<uintptr_t>(img) & 3) || (reinterpret_cast<uintptr_t>(dL_dimg) & 3)) return fail2(-2, "softargmax_bwd: img and dL_dimg must be 4-byte aligned");
    hipLaunchKernelGGL(k_softargmax_bwd, dim3(nchunks, planes), dim3(SA_THREADS), 0, (hipStream_t)stream, n, W, beta, img, stats,
                       dL_dxy, dL_dimg);
    HIP_TRY2(hipGetLastError());
    return 0;
}

}  // extern "C"
