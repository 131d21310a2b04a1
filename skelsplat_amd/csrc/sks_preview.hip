// sks_preview.hip -- 8-bit grey previews of renders and heat-maps for MI355X (gfx950): the reference's debug pictures
// (train.py:279-304, save_heatmaps / save_images: sum a view's channels, min-max normalise, write 8 bits), on the device.
//
// The fixed sequence of one view, all fp32, one rounding per operation (include/skelsplat_hip.h):
//   1. s = p[0]; s += p[1]; ...; s += p[C-1]          channels in ascending order, per pixel
//   2. lo = min(s), hi = max(s) over the view's pixels  (a NaN pixel makes both NaN, as torch.min does)
//   3. t = ((s - lo) / (hi - lo)) * 255.0f
//   4. q = (t >= 0 && t <= 255) ? (uint8)trunc(t) : 0
// Two launches per call.  Pass A streams the planes once, writes the sum plane into scratch with plain stores (it is re-read at
// once and sits in the Infinity Cache) and one {min, max} partial per workgroup; pass B reduces a view's partials (at most
// PV_GROUPS of them), normalises and packs.  No atomics: min / max are exact in any order, so every byte is reproducible.
// The factor path's pass A evaluates the sum plane from the separable heat-map factors -- the very expression k_heatmaps stores
// (sks_ops.hip) -- and never sees a plane.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"
#include "sks_math.h"

namespace {

using sks::dpp_move;

constexpr int PV_THREADS = 256;
constexpr int PV_GROUPS = 256;      // most workgroups per view of either pass: pass B reduces the partials with one thread each
static_assert(PV_GROUPS <= PV_THREADS, "pass B reads one partial per thread");

struct PvSizes {                    // the factor path's per-view image sizes, by value in the kernel's argument segment
    int w[SKS_MAX_VIEWS], h[SKS_MAX_VIEWS];
};

// min and max over the 64 lanes, in every lane (the DPP scheme of sks::wave_sum); NaNs are carried by the caller's flag, fminf
// and fmaxf skip them
__device__ __forceinline__ float wave_min(float v)
{
    v = fminf(v, dpp_move<0xB1>(v));
    v = fminf(v, dpp_move<0x4E>(v));
    v = fminf(v, dpp_move<0x124>(v));
    v = fminf(v, dpp_move<0x128>(v));
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
__device__ __forceinline__ float wave_max(float v) { return -wave_min(-v); }

// The workgroup's {lo, hi, any NaN} from every thread's; the result in every thread.  s_red: 3 x 4 floats.
__device__ __forceinline__ void block_minmax(float& lo, float& hi, bool& nan, float (*s_red)[PV_THREADS / 64])
{
    lo = wave_min(lo);
    hi = wave_max(hi);
    const float n = wave_max(nan ? 1.0f : 0.0f);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = lo; s_red[1][tid >> 6] = hi; s_red[2][tid >> 6] = n; }
    __syncthreads();
    lo = fminf(fminf(s_red[0][0], s_red[0][1]), fminf(s_red[0][2], s_red[0][3]));
    hi = fmaxf(fmaxf(s_red[1][0], s_red[1][1]), fmaxf(s_red[1][2], s_red[1][3]));
    nan = fmaxf(fmaxf(s_red[2][0], s_red[2][1]), fmaxf(s_red[2][2], s_red[2][3])) != 0.0f;
}

__device__ __forceinline__ void see(float s, float& lo, float& hi, bool& nan)
{
    lo = fminf(lo, s);
    hi = fmaxf(hi, s);
    nan |= s != s;
}

// one workgroup's partial: NaN in both slots stands for "saw a NaN"
__device__ __forceinline__ void write_partial(float* __restrict__ part, float lo, float hi, bool nan)
{
    if (threadIdx.x == 0) {
        part[0] = nan ? __builtin_nanf("") : lo;
        part[1] = nan ? __builtin_nanf("") : hi;
    }
}

// ------------------------------------------------------------------------------------------------------------
// Pass A, plane path.  grid (groups, V).  VEC: n % 4 == 0 and 16-byte aligned bases -> one unit = a float4 of every plane;
// otherwise one unit = one pixel.  Workgroup-strided like k_masked_l2; the channel loop keeps four planes' loads in flight and
// adds them in ascending order.
// ------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(PV_THREADS) void k_preview_sum(int C, size_t n, const float* __restrict__ planes,
                                                            float* __restrict__ sum, float* __restrict__ partials)
{
    __shared__ float s_red[3][PV_THREADS / 64];
    const int v = blockIdx.y, tid = threadIdx.x;
    const float* p = planes + (size_t)v * C * n;
    float* o = sum + (size_t)v * n;
    float lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    const size_t stride = (size_t)gridDim.x * PV_THREADS;
    if (VEC) {
        const size_t n4 = n / 4;
        for (size_t i = (size_t)blockIdx.x * PV_THREADS + tid; i < n4; i += stride) {
            float4 s = reinterpret_cast<const float4*>(p)[i];
            int c = 1;
            for (; c + 4 <= C; c += 4) {
                float4 a[4];
#pragma unroll
                for (int u = 0; u < 4; u++) a[u] = reinterpret_cast<const float4*>(p + (size_t)(c + u) * n)[i];
#pragma unroll
                for (int u = 0; u < 4; u++) { s.x += a[u].x; s.y += a[u].y; s.z += a[u].z; s.w += a[u].w; }
            }
            for (; c < C; c++) {
                const float4 a = reinterpret_cast<const float4*>(p + (size_t)c * n)[i];
                s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
            }
            reinterpret_cast<float4*>(o)[i] = s;
            see(s.x, lo, hi, nan); see(s.y, lo, hi, nan); see(s.z, lo, hi, nan); see(s.w, lo, hi, nan);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * PV_THREADS + tid; i < n; i += stride) {
            float s = p[i];
            int c = 1;
            for (; c + 4 <= C; c += 4) {
                float a[4];
#pragma unroll
                for (int u = 0; u < 4; u++) a[u] = p[(size_t)(c + u) * n + i];
#pragma unroll
                for (int u = 0; u < 4; u++) s += a[u];
            }
            for (; c < C; c++) s += p[(size_t)c * n + i];
            o[i] = s;
            see(s, lo, hi, nan);
        }
    }
    block_minmax(lo, hi, nan, s_red);
    write_partial(partials + 2 * ((size_t)v * gridDim.x + blockIdx.x), lo, hi, nan);
}

// ------------------------------------------------------------------------------------------------------------
// Pass A, factor path.  grid (row bands, V): a workgroup walks `band` rows of its view, a thread the columns tid, tid + 256, ..;
// per pixel  s = 0; s += (row[j][y] * col[j][x] - cmin[j]) / den[j]  for j = 0 .. J-1.  The first addition is 0 + t = t exactly
// (t >= +0: the factors are non-negative and cmin is the product of their minima), so this is the plane path's p[0] + p[1] + ..
// Where row[j][y] and cmin[j] are both zero the term is (0 * col - 0) / den = +0 and adding it is the identity: the joint is
// skipped (wave-uniform: every lane of a workgroup is on the same row).  Ws, Hs: the strides (the largest view).
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PV_THREADS) void k_preview_factor_sum(int J, int Ws, int Hs, int band, PvSizes sz,
                                                                   const float* __restrict__ row, const float* __restrict__ col,
                                                                   const float* __restrict__ cmin, const float* __restrict__ den,
                                                                   float* __restrict__ sum, float* __restrict__ partials)
{
    __shared__ float s_red[3][PV_THREADS / 64];
    const int v = blockIdx.y, tid = threadIdx.x;
    const int w = sz.w[v], h = sz.h[v];
    const int y0 = blockIdx.x * band, y1 = min(y0 + band, h);
    float lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    float* o = sum + (size_t)v * Hs * Ws;
    for (int y = y0; y < y1; y++) {
        for (int x = tid; x < w; x += PV_THREADS) {
            float s = 0.0f;
            for (int j = 0; j < J; j++) {
                const int vj = v * J + j;
                const float a = row[(size_t)vj * Hs + y], m = cmin[vj];
                if (a == 0.0f && m == 0.0f) continue;
                s += (a * col[(size_t)vj * Ws + x] - m) / den[vj];
            }
            o[(size_t)y * Ws + x] = s;
            see(s, lo, hi, nan);
        }
    }
    block_minmax(lo, hi, nan, s_red);
    write_partial(partials + 2 * ((size_t)v * gridDim.x + blockIdx.x), lo, hi, nan);
}

__device__ __forceinline__ unsigned quantise(float s, float lo, float range)
{
    const float t = ((s - lo) / range) * 255.0f;
    return (t >= 0.0f && t <= 255.0f) ? (unsigned)truncf(t) : 0u;     // (NaN fails both comparisons)
}

// ------------------------------------------------------------------------------------------------------------
// Pass B.  grid (groups, V).  Every workgroup reduces its view's `parts` partials itself (one per thread), then walks the
// view's Ws x Hs pixels: WIDE: Ws % 16 == 0 and aligned bases -> a lane turns four float4 of the sum plane into one 16-byte
// store; otherwise bytes.  SIZED (factor path): pixels outside the view's own w x h are written 0 and the sum plane is not
// read there.  Workgroup 0 of a view writes its {lo, hi} to minmax (if given).
// ------------------------------------------------------------------------------------------------------------
template <bool WIDE, bool SIZED>
__global__ __launch_bounds__(PV_THREADS) void k_preview_pack(int Ws, int Hs, PvSizes sz, int parts, const float* __restrict__ sum,
                                                             const float* __restrict__ partials, float* __restrict__ minmax,
                                                             unsigned char* __restrict__ out)
{
    __shared__ float s_red[3][PV_THREADS / 64];
    const int v = blockIdx.y, tid = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    if (tid < parts) {
        const float a = partials[2 * ((size_t)v * parts + tid)], b = partials[2 * ((size_t)v * parts + tid) + 1];
        // a partial's first slot is a minimum, its second a maximum: a workgroup that saw no pixel (the factor path's bands past a
        // shorter view's own height) wrote the identity {+inf, -inf}, and neither half of it may reach the other bound
        lo = fminf(lo, a);
        hi = fmaxf(hi, b);
        nan = a != a || b != b;
    }
    block_minmax(lo, hi, nan, s_red);
    if (nan) lo = hi = __builtin_nanf("");
    if (minmax && blockIdx.x == 0 && tid == 0) { minmax[2 * v] = lo; minmax[2 * v + 1] = hi; }
    const float range = hi - lo;
    const int w = SIZED ? sz.w[v] : Ws, h = SIZED ? sz.h[v] : Hs;
    const size_t n = (size_t)Ws * Hs;
    const float* s = sum + (size_t)v * n;
    unsigned char* o = out + (size_t)v * n;
    const size_t stride = (size_t)gridDim.x * PV_THREADS;
    if (WIDE) {
        const size_t n16 = n / 16;
        for (size_t i = (size_t)blockIdx.x * PV_THREADS + tid; i < n16; i += stride) {
            const int y = (int)((i * 16) / Ws), x = (int)((i * 16) % Ws);      // (16 | Ws: the group lies in one row)
            unsigned q[4] = { 0u, 0u, 0u, 0u };
            if (!SIZED || (y < h && x < w)) {
                float4 a[4];
#pragma unroll
                for (int u = 0; u < 4; u++) a[u] = reinterpret_cast<const float4*>(s)[i * 4 + u];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const float e[4] = { a[u].x, a[u].y, a[u].z, a[u].w };
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (!SIZED || x + 4 * u + k < w) q[u] |= quantise(e[k], lo, range) << (8 * k);
                }
            }
            reinterpret_cast<uint4*>(o)[i] = make_uint4(q[0], q[1], q[2], q[3]);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * PV_THREADS + tid; i < n; i += stride) {
            bool inside = true;
            if (SIZED) inside = (int)(i / Ws) < h && (int)(i % Ws) < w;
            o[i] = inside ? (unsigned char)quantise(s[i], lo, range) : (unsigned char)0;
        }
    }
}

int groups_of(size_t units)
{
    size_t g = (units + PV_THREADS - 1) / PV_THREADS;
    return (int)(g < 1 ? 1 : g > PV_GROUPS ? PV_GROUPS : g);
}

struct PvLaunch {
    int load_bytes, store_bytes, groups_a, groups_b;
};

// the launch forms of a plane-path call: `aligned`: every base pointer is a multiple of 16
PvLaunch plane_launch(int W, int H, bool aligned)
{
    const size_t n = (size_t)W * H;
    PvLaunch L;
    L.load_bytes = (W % 4 == 0 && aligned) ? 16 : 4;
    L.store_bytes = (W % 16 == 0 && aligned) ? 16 : 1;
    L.groups_a = groups_of(L.load_bytes == 16 ? n / 4 : n);
    L.groups_b = groups_of(L.store_bytes == 16 ? n / 16 : n);
    return L;
}

size_t sum_bytes(int V, int W, int H) { return (((size_t)V * W * H * sizeof(float)) + 15) & ~(size_t)15; }

// the shape rules both entry points share
int check_shape(const char* who, int V, int C, const char* cname, int W, int H)
{
    if (V < 1 || C < 1 || W < 1 || H < 1)
        return fail2(-1, "%s: V = %d, %s = %d, W = %d, H = %d; all must be at least 1", who, V, cname, C, W, H);
    if ((long long)W * H > INT_MAX) return fail2(-1, "%s: W x H = %d x %d pixels do not fit an int", who, W, H);
    size_t total;
    if (__builtin_mul_overflow((size_t)V * (size_t)C, (size_t)W * (size_t)H * sizeof(float), &total))
        return fail2(-1, "%s: V x %s x H x W = %d x %d x %d x %d floats do not fit a size_t", who, cname, V, C, H, W);
    return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

size_t sks_preview_scratch_bytes(int V, int W, int H)
{
    if (V < 1 || W < 1 || H < 1 || (long long)W * H > INT_MAX) return 0;
    size_t planes;
    if (__builtin_mul_overflow((size_t)V, (size_t)W * (size_t)H * sizeof(float), &planes) || planes > SIZE_MAX / 2) return 0;
    return sum_bytes(V, W, H) + (size_t)V * PV_GROUPS * 2 * sizeof(float);
}

int sks_preview_launch(int W, int H, int aligned, int* out)
{
    if (!out) return fail2(-2, "preview_launch: missing out (SKS_PREVIEW_LAUNCH_INTS ints)");
    if (W < 1 || H < 1) return fail2(-1, "preview_launch: W = %d, H = %d; both must be at least 1", W, H);
    if ((long long)W * H > INT_MAX) return fail2(-1, "preview_launch: W x H = %d x %d pixels do not fit an int", W, H);
    const PvLaunch L = plane_launch(W, H, aligned != 0);
    out[0] = L.load_bytes;
    out[1] = L.store_bytes;
    out[2] = L.groups_a;
    out[3] = L.groups_b;
    return 0;
}

int sks_preview_planes(int V, int C, int W, int H, const float* planes, void* scratch, float* minmax, unsigned char* out,
                       void* stream)
{
    if (int rc = check_shape("preview_planes", V, C, "C", W, H)) return rc;
    if (V > 65535) return fail2(-1, "preview_planes: V = %d views, at most 65535 per call", V);
    if (C > SKS_MAX_CHANNELS) return fail2(-1, "preview_planes: C = %d channels, at most %d (SKS_MAX_CHANNELS)", C, SKS_MAX_CHANNELS);
    if (!planes) return fail2(-2, "preview_planes: missing planes");
    if (!scratch) return fail2(-2, "preview_planes: missing scratch (sks_preview_scratch_bytes)");
    if (!out) return fail2(-2, "preview_planes: missing out");
    if (!aligned16(scratch)) return fail2(-2, "preview_planes: scratch must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)W * H;
    float* sum = (float*)scratch;
    float* partials = (float*)((char*)scratch + sum_bytes(V, W, H));
    const PvLaunch L = plane_launch(W, H, aligned16(planes) && aligned16(out));
    if (L.load_bytes == 16)
        hipLaunchKernelGGL(k_preview_sum<true>, dim3(L.groups_a, V), dim3(PV_THREADS), 0, st, C, n, planes, sum, partials);
    else
        hipLaunchKernelGGL(k_preview_sum<false>, dim3(L.groups_a, V), dim3(PV_THREADS), 0, st, C, n, planes, sum, partials);
    const PvSizes none = {};
    if (L.store_bytes == 16)
        hipLaunchKernelGGL((k_preview_pack<true, false>), dim3(L.groups_b, V), dim3(PV_THREADS), 0, st, W, H, none, L.groups_a, sum,
                           partials, minmax, out);
    else
        hipLaunchKernelGGL((k_preview_pack<false, false>), dim3(L.groups_b, V), dim3(PV_THREADS), 0, st, W, H, none, L.groups_a, sum,
                           partials, minmax, out);
    HIP_TRY2(hipGetLastError());
    return 0;
}

int sks_preview_factors(int V, int J, int W, int H, const float* row, const float* col, const float* cmin, const float* den,
                        const int* view_wh, void* scratch, float* minmax, unsigned char* out, void* stream)
{
    if (int rc = check_shape("preview_factors", V, J, "J", W, H)) return rc;
    if (V > SKS_MAX_VIEWS) return fail2(-1, "preview_factors: V = %d views, at most %d (SKS_MAX_VIEWS)", V, SKS_MAX_VIEWS);
    if (!row || !col || !cmin || !den) return fail2(-2, "preview_factors: missing factors (row, col, cmin, den)");
    if (!scratch) return fail2(-2, "preview_factors: missing scratch (sks_preview_scratch_bytes)");
    if (!out) return fail2(-2, "preview_factors: missing out");
    if (!aligned16(scratch)) return fail2(-2, "preview_factors: scratch must be 16-byte aligned");
    PvSizes sz = {};
    for (int v = 0; v < V; v++) {
        sz.w[v] = view_wh ? view_wh[2 * v] : W;
        sz.h[v] = view_wh ? view_wh[2 * v + 1] : H;
        if (sz.w[v] < 1 || sz.w[v] > W || sz.h[v] < 1 || sz.h[v] > H)
            return fail2(-1, "preview_factors: view %d is %d x %d; every view's size must be within [1, %d] x [1, %d]", v, sz.w[v],
                         sz.h[v], W, H);
    }
    hipStream_t st = (hipStream_t)stream;
    float* sum = (float*)scratch;
    float* partials = (float*)((char*)scratch + sum_bytes(V, W, H));
    // row bands: the fewest rows per workgroup that keep the bands of the tallest view within PV_GROUPS.  A band past a view's
    // own height sees no pixel and writes the identity {+inf, -inf}.
    const int band = (H + PV_GROUPS - 1) / PV_GROUPS, bands = (H + band - 1) / band;
    hipLaunchKernelGGL(k_preview_factor_sum, dim3(bands, V), dim3(PV_THREADS), 0, st, J, W, H, band, sz, row, col, cmin, den, sum,
                       partials);
    const PvLaunch L = plane_launch(W, H, aligned16(out));
    if (L.store_bytes == 16)
        hipLaunchKernelGGL((k_preview_pack<true, true>), dim3(L.groups_b, V), dim3(PV_THREADS), 0, st, W, H, sz, bands, sum, partials,
                           minmax, out);
    else
        hipLaunchKernelGGL((k_preview_pack<false, true>), dim3(L.groups_b, V), dim3(PV_THREADS), 0, st, W, H, sz, bands, sum, partials,
                           minmax, out);
    HIP_TRY2(hipGetLastError());
    return 0;
}

}  // extern "C"
