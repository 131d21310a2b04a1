// sks_procrustes.h -- the rotation of the orthogonal Procrustes problem from the 3x3 cross-covariance, in double, for one thread:
// R = argmax over PROPER rotations of trace(R H), H = sum x_i y_i^T (x onto y).  Used by sks_align.hip; plain C++ (no HIP
// runtime call), so the same sequence of operations can be compiled for the host and held against a textbook solution there.
//
// Horn's closed form (J. Opt. Soc. Am. A 4, 1987): trace(R H) = q^T N q for the unit quaternion q of R and a symmetric
// traceless 4x4 N built from H, so q is the eigenvector of N's largest eigenvalue.  What that buys over an SVD of H:
//   - every unit quaternion is a proper rotation, so there is no reflection case to repair and no rank-deficient basis to
//     complete: planar (rank 2), collinear (rank 1) and mirrored inputs go through the same arithmetic as any other;
//   - H = 0 (one joint, coincident joints) leaves N = 0, the sweeps rotate nothing, the first eigenvector is (1,0,0,0): R = I.
// The eigenvector comes from cyclic Jacobi sweeps (Rutishauser's form: t = sgn / (|theta| + sqrt(theta^2 + 1)), updates through
// tau = s / (1 + c)), at most PROCRUSTES_SWEEPS of them; a sweep that finds every off-diagonal entry exactly zero ends the loop.
// The ten entries of N's upper triangle and the sixteen of the eigenvector matrix are named scalars and the six rotations of a
// sweep are written out, so all of it lives in registers (arrays picked from by the final argmax ended up in private memory).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SKS_HD __host__ __device__ __forceinline__
#else
#define SKS_HD inline
#endif

namespace sks {

constexpr int PROCRUSTES_SWEEPS = 12;   // random and degenerate H need 4 .. 7 (DESIGN.md "Aligned errors")

// One Jacobi rotation in the (p, q) plane of the symmetric matrix a (upper triangle a01 .. a33) and of the eigenvectors v; r1p .. r2q
// name the entries (r, p), (r, q) of the two other rows r as the upper triangle stores them.
#define SKS_JACOBI(p, q, r1p, r1q, r2p, r2q)                                                                                \
    do {                                                                                                                    \
        const double apq = a##p##q, g = 100.0 * fabs(apq);                                                                  \
        /* after the first sweeps an entry that no longer registers against either diagonal neighbour is set to zero */     \
        if (late && fabs(a##p##p) + g == fabs(a##p##p) && fabs(a##q##q) + g == fabs(a##q##q)) { a##p##q = 0.0; break; }     \
        if (apq == 0.0) break;                                                                                              \
        const double h = a##q##q - a##p##p;                                                                                 \
        double t;                                                                                                           \
        if (fabs(h) + g == fabs(h)) {                                                                                       \
            t = apq / h;                                                                                                    \
        } else {                                                                                                            \
            const double theta = 0.5 * h / apq;                                                                             \
            t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));                                                            \
            if (theta < 0.0) t = -t;                                                                                        \
        }                                                                                                                   \
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c), d = t * apq;                              \
        a##p##p -= d; a##q##q += d; a##p##q = 0.0;                                                                          \
        SKS_ROT(r1p, r1q) SKS_ROT(r2p, r2q)                                                                                 \
        SKS_ROT(v0##p, v0##q) SKS_ROT(v1##p, v1##q) SKS_ROT(v2##p, v2##q) SKS_ROT(v3##p, v3##q)                             \
    } while (0)
#define SKS_ROT(x, y) { const double x_ = x, y_ = y; x = x_ - s * (y_ + x_ * tau); y = y_ + s * (x_ - y_ * tau); }

// H row-major: H[3 a + b] = sum x_a y_b.  R row-major, R x ~ y.  Any finite H gives a rotation with |det R - 1| and
// |R^T R - I| of a few 1e-16.
SKS_HD void procrustes_rotation(const double* H, double* R)
{
    const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
    double a00 = (Sxx + Syy) + Szz, a01 = Syz - Szy, a02 = Szx - Sxz, a03 = Sxy - Syx;
    double a11 = (Sxx - Syy) - Szz, a12 = Sxy + Syx, a13 = Szx + Sxz;
    double a22 = (Syy - Sxx) - Szz, a23 = Syz + Szy;
    double a33 = (Szz - Sxx) - Syy;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v03 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v13 = 0.0;
    double v20 = 0.0, v21 = 0.0, v22 = 1.0, v23 = 0.0, v30 = 0.0, v31 = 0.0, v32 = 0.0, v33 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < PROCRUSTES_SWEEPS; sweep++) {
        const double off = ((fabs(a01) + fabs(a02)) + (fabs(a03) + fabs(a12))) + (fabs(a13) + fabs(a23));
        if (off == 0.0) break;
        const bool late = sweep > 2;
        SKS_JACOBI(0, 1, a02, a12, a03, a13);
        SKS_JACOBI(0, 2, a01, a12, a03, a23);
        SKS_JACOBI(0, 3, a01, a13, a02, a23);
        SKS_JACOBI(1, 2, a01, a02, a13, a23);
        SKS_JACOBI(1, 3, a01, a03, a12, a23);
        SKS_JACOBI(2, 3, a02, a03, a12, a13);
    }
    double lam = a00, qw = v00, qx = v10, qy = v20, qz = v30;
#define SKS_PICK(j) if (a##j##j > lam) { lam = a##j##j; qw = v0##j; qx = v1##j; qy = v2##j; qz = v3##j; }
    SKS_PICK(1) SKS_PICK(2) SKS_PICK(3)
#undef SKS_PICK
    const double n = sqrt((qw * qw + qx * qx) + (qy * qy + qz * qz));
    qw /= n; qx /= n; qy /= n; qz /= n;
    const double ww = qw * qw, xx = qx * qx, yy = qy * qy, zz = qz * qz;
    const double xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
    R[0] = (ww + xx) - (yy + zz); R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);       R[4] = (ww + yy) - (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = (ww + zz) - (xx + yy);
}

#undef SKS_ROT
#undef SKS_JACOBI

}  // namespace sks
