/*
 * sks_ssim_oracle.c -- TEST INFRASTRUCTURE ONLY (never linked or imported by the product).
 *
 * Sequential CPU restatement of fused SSIM (laurabragagnolo/SkelSplat, submodules/fused-ssim/ssim.cu:100-185 the
 * separable 11-tap passes, 262-283 the map and its partial derivatives, 318-365 the backward), written from
 * skelsplat_amd/csrc/sks_ssim.hip: the operations that kernel performs on one output pixel, in the order it performs
 * them, one pixel at a time.  No tiles, no strips, no shared-memory picture of the kernel: whatever the kernel's
 * staging, halo, carried rows or swizzle get wrong shows as a difference from this file.
 *
 * One source, two builds (oracle/Makefile): -DSSIM_REAL=float is the oracle the GPU is held to bit for bit;
 * -DSSIM_REAL=double exists to prove that this text is SSIM (tests/test_ssim_oracle_cpu.py holds it to an independent
 * float64 conv2d SSIM with autograd).  Same text, other type.
 *
 * Floating-point contract (-ffp-contract=off, as for sks_oracle.c):
 *   - pixels outside the image are 0 and still pass through their tap;
 *   - the products u*u, v*v, u*v (forward) and dL*dm_* (backward) are rounded before they are filtered;
 *   - a filter is 11 taps acc = fma(g[t], value, acc) from acc = 0, t = 0..10 left to right, then the same top to
 *     bottom over the horizontally filtered rows;
 *   - every other operation rounds once, in the association written below; every quotient is the language's IEEE `/`.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#ifndef SSIM_REAL
#define SSIM_REAL float
#endif
typedef SSIM_REAL real;

#define FMA(a, b, c) _Generic((a), float: fmaf, double: fma)((a), (b), (c))
#define FABS(a) _Generic((a), float: fabsf, double: fabs)(a)
#define NEXTUP(a) _Generic((a), float: nextafterf, double: nextafter)((a), (real)INFINITY)

/* ssim.cu:9-19 */
static const float G11[11] = { 0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f,
                               0.21300552785396576f,  0.26601171493530273f,   0.21300552785396576f,  0.10936068743467331f,
                               0.036000773310661316f, 0.0075987582094967365f, 0.001028380123898387f };

int ssim_oracle_sizeof_real(void) { return (int)sizeof(real); }

/* ssim.cu:100-185 / 318-365: one plane, rows then columns; tmp holds the horizontally filtered rows */
static void blur_plane(const real* src, real* tmp, real* dst, int H, int W)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            real acc = 0;
            for (int t = 0; t < 11; t++) {
                const int xx = x + t - 5;
                const real v = (xx >= 0 && xx < W) ? src[(size_t)y * W + xx] : (real)0;
                acc = FMA((real)G11[t], v, acc);
            }
            tmp[(size_t)y * W + x] = acc;
        }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            real acc = 0;
            for (int t = 0; t < 11; t++) {
                const int yy = y + t - 5;
                const real v = (yy >= 0 && yy < H) ? tmp[(size_t)yy * W + x] : (real)0;
                acc = FMA((real)G11[t], v, acc);
            }
            dst[(size_t)y * W + x] = acc;
        }
}

/* distance from |q| to the next representable value above it (inf / nan for a non-finite q) */
static real ulp_of(real q)
{
    const real a = FABS(q);
    return NEXTUP(a) - a;
}

#define TWO_M100 ((real)7.888609052210118e-31)  /* 2^-100 */
#define TWO_P100 ((real)1.2676506002282294e30)  /* 2^100 */
#define TWO_M40 ((real)9.094947017729282e-13)   /* 2^-40 */
#define TWO_M60 ((real)8.673617379884035e-19)   /* 2^-60 */

typedef struct {
    int flagged;        /* a nonzero |n| < 2^-100, or d outside [2^-100, 2^100), behind this output */
    real ulps;          /* sum of ulp(q) */
    int64_t* outside;   /* quotients outside d in [2^-40, 2^8), |n| in [2^-60, 2^12) or n = 0 */
} QStat;

static real quot(real n, real d, QStat* s)
{
    const real q = n / d;
    const real an = FABS(n);
    if ((an != 0 && an < TWO_M100) || !(d >= TWO_M100 && d < TWO_P100)) s->flagged = 1;
    if (!(d >= TWO_M40 && d < (real)256 && (an == 0 || (an >= TWO_M60 && an < (real)4096)))) ++*s->outside;
    s->ulps += ulp_of(q);
    return q;
}

/*
 * ssim.cu:187-286.  flags: bit 0 the map's quotient, bit 1 any of dm_dmu1's four, bit 2 dm_dsigma1_sq's, bit 3
 * dm_dsigma12's was flagged (see QStat).  ulp_sum: sum of ulp(q_i) over dm_dmu1's four quotients.  dm_dmu1,
 * dm_dsigma1_sq, dm_dsigma12, flags, ulp_sum may be NULL (all three partial maps or none).
 */
int ssim_oracle_forward(int B, int CH, int H, int W, real C1, real C2, const real* img1, const real* img2, real* ssim_map,
                        real* dm_dmu1, real* dm_dsigma1_sq, real* dm_dsigma12, uint8_t* flags, real* ulp_sum,
                        int64_t* n_outside_documented)
{
    const size_t n = (size_t)H * W;
    real* buf = (real*)malloc(sizeof(real) * n * 7);
    int64_t outside = 0;
    if (!buf) return -1;
    real *prod = buf, *tmp = buf + n, *m1 = buf + 2 * n, *m2 = buf + 3 * n, *e11 = buf + 4 * n, *e22 = buf + 5 * n,
         *e12 = buf + 6 * n;
    for (int p = 0; p < B * CH; p++) {
        const real *u = img1 + p * n, *v = img2 + p * n;
        blur_plane(u, tmp, m1, H, W);
        blur_plane(v, tmp, m2, H, W);
        for (size_t i = 0; i < n; i++) prod[i] = u[i] * u[i];
        blur_plane(prod, tmp, e11, H, W);
        for (size_t i = 0; i < n; i++) prod[i] = v[i] * v[i];
        blur_plane(prod, tmp, e22, H, W);
        for (size_t i = 0; i < n; i++) prod[i] = u[i] * v[i];
        blur_plane(prod, tmp, e12, H, W);
        for (size_t i = 0; i < n; i++) {
            const real mu1 = m1[i], mu2 = m2[i];
            const real sigma1_sq = e11[i] - mu1 * mu1;
            const real sigma2_sq = e22[i] - mu2 * mu2;
            const real sigma12 = e12[i] - mu1 * mu2;
            /* ssim.cu:262-283 */
            const real mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
            const real Cn = (real)2 * mu1_mu2 + C1;
            const real D = (real)2 * sigma12 + C2;
            const real A = (mu1_sq + mu2_sq) + C1;
            const real Bd = (sigma1_sq + sigma2_sq) + C2;
            const real AB = A * Bd;
            QStat sm = { 0, 0, &outside }, s1 = { 0, 0, &outside }, s2 = { 0, 0, &outside }, s3 = { 0, 0, &outside };
            ssim_map[p * n + i] = quot(Cn * D, AB, &sm);
            if (dm_dmu1) {
                const real AAB = (A * A) * Bd, ABB = (A * Bd) * Bd;
                const real q1 = quot((mu2 * (real)2) * D, AB, &s1);
                const real q2 = quot((mu2 * (real)2) * Cn, AB, &s1);
                const real q3 = quot(((mu1 * (real)2) * Cn) * D, AAB, &s1);
                const real q4 = quot(((mu1 * (real)2) * Cn) * D, ABB, &s1);
                dm_dmu1[p * n + i] = ((q1 - q2) - q3) + q4;
                dm_dsigma1_sq[p * n + i] = quot((-Cn) * D, ABB, &s2);
                dm_dsigma12[p * n + i] = quot((real)2 * Cn, AB, &s3);
            }
            if (flags) flags[p * n + i] = (uint8_t)(sm.flagged | (s1.flagged << 1) | (s2.flagged << 2) | (s3.flagged << 3));
            if (ulp_sum) ulp_sum[p * n + i] = s1.ulps;
        }
    }
    if (n_outside_documented) *n_outside_documented = outside;
    free(buf);
    return 0;
}

/* ssim.cu:288-366: dL_dimg1 = G*(dL dm_dmu1) + 2 img1 G*(dL dm_dsigma1_sq) + img2 G*(dL dm_dsigma12).  No division. */
int ssim_oracle_backward(int B, int CH, int H, int W, const real* img1, const real* img2, const real* dL_dmap,
                         const real* dm_dmu1, const real* dm_dsigma1_sq, const real* dm_dsigma12, real* dL_dimg1)
{
    const size_t n = (size_t)H * W;
    real* buf = (real*)malloc(sizeof(real) * n * 5);
    if (!buf) return -1;
    real *prod = buf, *tmp = buf + n, *a = buf + 2 * n, *b = buf + 3 * n, *c = buf + 4 * n;
    for (int p = 0; p < B * CH; p++) {
        const real* dL = dL_dmap + p * n;
        for (size_t i = 0; i < n; i++) prod[i] = dm_dmu1[p * n + i] * dL[i];
        blur_plane(prod, tmp, a, H, W);
        for (size_t i = 0; i < n; i++) prod[i] = dm_dsigma1_sq[p * n + i] * dL[i];
        blur_plane(prod, tmp, b, H, W);
        for (size_t i = 0; i < n; i++) prod[i] = dm_dsigma12[p * n + i] * dL[i];
        blur_plane(prod, tmp, c, H, W);
        for (size_t i = 0; i < n; i++)
            dL_dimg1[p * n + i] = (a[i] + (img1[p * n + i] * (real)2) * b[i]) + img2[p * n + i] * c[i];
    }
    free(buf);
    return 0;
}

/* the backward under dL_dmap = (dL_value * dL_scale, rounded) inside the image shrunk by `crop` per side, 0 outside */
int ssim_oracle_backward_uniform(int B, int CH, int H, int W, const real* img1, const real* img2, real dL_value,
                                 real dL_scale, int crop, const real* dm_dmu1, const real* dm_dsigma1_sq,
                                 const real* dm_dsigma12, real* dL_dimg1)
{
    const size_t n = (size_t)H * W;
    const real dval = dL_value * dL_scale;
    real* dL = (real*)malloc(sizeof(real) * n * (size_t)(B * CH > 0 ? B * CH : 1));
    if (!dL) return -1;
    for (int p = 0; p < B * CH; p++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                dL[p * n + (size_t)y * W + x] = (y >= crop && y < H - crop && x >= crop && x < W - crop) ? dval : (real)0;
    const int rc = ssim_oracle_backward(B, CH, H, W, img1, img2, dL, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1);
    free(dL);
    return rc;
}

/* the mean of the map over the image shrunk by `crop` per side: a double sum times 1 / count, rounded to float (nan
 * for an empty map, like torch's) */
float ssim_oracle_mean(int B, int CH, int H, int W, const real* ssim_map, int crop)
{
    const size_t n = (size_t)H * W;
    const double count = (double)B * CH * (H > 2 * crop ? H - 2 * crop : 0) * (W > 2 * crop ? W - 2 * crop : 0);
    double sum = 0.0;
    if (!(count > 0.0)) return NAN;
    for (int p = 0; p < B * CH; p++)
        for (int y = crop; y < H - crop; y++)
            for (int x = crop; x < W - crop; x++) sum += (double)ssim_map[p * n + (size_t)y * W + x];
    return (float)(sum * (1.0 / count));
}
