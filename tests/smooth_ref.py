"""Two independent float64 references of the temporal fit of include/skelsplat_hip.h (sks_smooth_sequence), and of sks_eval_accel.

fit_lstsq  (a) the textbook form: per target a weighted least-squares solve by np.linalg.lstsq on the WHITENED design matrix -- rows
           sqrt(omega_k) G_k^T [I, t I, t^2 I] with Lambda_k = G_k G_k^T from np.linalg.inv and np.linalg.cholesky -- and the
           covariance from the design's SVD.  No normal equations are formed.  Also returns the condition number of every normal
           matrix (the square of the design's).
fit_ldl    (b) the header's fixed sequence restated op by op on Python floats (IEEE float64, one rounding per operation), one
           target at a time: what the kernel is designed to equal bit for bit before the final rounding to float32.
accel_ref  the acceleration figures, entry by entry, with the counts.

A case is a dict of tests/smooth_cases.py: xyz (N,J,3) float32, cov6 / weights / valid / groups or None, h, d, taper, floor."""
import numpy as np


def _taper(kind, t, h):
    if kind == "box":
        return 1.0
    u = abs(float(t)) / float(h + 1)
    q = 1.0 - (u * u) * u
    return (q * q) * q


def _mat(c):
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], dtype=np.float64)


def _taps(case, f, j, cov_ok):
    """The usable taps of target (f, j), ascending: [(t, k)]."""
    xyz, N, h = case["xyz"], case["xyz"].shape[0], case["h"]
    out = []
    for k in range(max(0, f - h), min(N - 1, f + h) + 1):
        if case["groups"] is not None and case["groups"][k] != case["groups"][f]:
            continue
        if case["valid"] is not None and not case["valid"][k, j]:
            continue
        if not np.all(np.isfinite(xyz[k, j])):
            continue
        if case["weights"] is not None and not (np.isfinite(case["weights"][k, j]) and case["weights"][k, j] > 0):
            continue
        if not cov_ok(k, j):
            continue
        out.append((k - f, k))
    return out


def fit_lstsq(case):
    """(a): dict of joints, velocity (N,J,3), cov6 (N,J,6) float64, n_used (N,J) int, cond (N,J) (NaN where n = 0)."""
    xyz = case["xyz"].astype(np.float64)
    N, J = xyz.shape[:2]
    C = None
    if case["cov6"] is not None:
        C = case["cov6"].astype(np.float64).copy()
        C[..., [0, 3, 5]] += case["floor"]

    def cov_ok(k, j):      # (the cases hold nothing borderline: clearly positive definite, or clearly not)
        return C is None or (np.all(np.isfinite(C[k, j])) and np.linalg.eigvalsh(_mat(C[k, j])).min() > 0)

    out = dict(joints=np.full((N, J, 3), np.nan), velocity=np.full((N, J, 3), np.nan), cov6=np.full((N, J, 6), np.nan),
               n_used=np.zeros((N, J), dtype=np.int64), cond=np.full((N, J), np.nan))
    for f in range(N):
        for j in range(J):
            taps = _taps(case, f, j, cov_ok)
            n = len(taps)
            out["n_used"][f, j] = n
            if n == 0:
                continue
            de = min(case["d"], n - 1)
            x0 = xyz[taps[0][1], j]
            A, b = [], []
            for t, k in taps:
                w = 1.0 if case["weights"] is None else float(case["weights"][k, j])
                Gt = np.eye(3) if C is None else np.linalg.cholesky(np.linalg.inv(_mat(C[k, j]))).T
                Gt = np.sqrt(w * _taper(case["taper"], t, case["h"])) * Gt
                A.append(np.hstack([Gt * float(t) ** i for i in range(de + 1)]))
                b.append(Gt @ (xyz[k, j] - x0))
            A, b = np.vstack(A), np.concatenate(b)
            c = np.linalg.lstsq(A, b, rcond=None)[0]
            _, s, Vt = np.linalg.svd(A, full_matrices=False)
            cov = (Vt.T / (s * s)) @ Vt
            out["joints"][f, j] = c[:3] + x0
            out["velocity"][f, j] = c[3:6] if de >= 1 else 0.0
            out["cov6"][f, j] = cov[:3, :3][np.triu_indices(3)]
            out["cond"][f, j] = (s[0] / s[-1]) ** 2
    return out


def _ldl3(xx, xy, xz, yy, yz, zz):
    d0 = xx
    l10 = xy / d0
    l20 = xz / d0
    d1 = yy - l10 * xy
    e = yz - l20 * xy
    z1 = zz - l20 * xz
    l21 = e / d1
    d2 = z1 - l21 * e
    return d0, d1, d2, l10, l20, l21


def _inverse3(d0, d1, d2, l10, l20, l21):
    i0, i1, i2 = 1.0 / d0, 1.0 / d1, 1.0 / d2
    m = l21 * l10 - l20
    return [(i0 + (l10 * l10) * i1) + (m * m) * i2, -(l10 * i1) - (m * l21) * i2, m * i2, i1 + (l21 * l21) * i2, -(l21 * i2), i2]


_SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))


def fit_ldl(case):
    """(b): dict of joints, velocity (N,J,3), cov6 (N,J,6) float64 BEFORE the rounding to float32, n_used (N,J) int, and deff (N,J)
    the effective degree (-1 where n = 0)."""
    xyz = case["xyz"]
    N, J = xyz.shape[:2]
    d, h, floor = case["d"], case["h"], np.float64(case["floor"])
    lam = {}
    with np.errstate(all="ignore"):
        if case["cov6"] is not None:
            for k in range(N):
                for j in range(J):
                    c = [np.float64(v) for v in case["cov6"][k, j]]          # (np.float64: x / 0 is inf or NaN, not an exception)
                    f = _ldl3(c[0] + floor, c[1], c[2], c[3] + floor, c[4], c[5] + floor)
                    if all(np.isfinite(p) and p > 0 for p in f[:3]):
                        lam[k, j] = [float(v) for v in _inverse3(*f)]
    cov_ok = lambda k, j: case["cov6"] is None or (k, j) in lam
    out = dict(joints=np.full((N, J, 3), np.nan), velocity=np.full((N, J, 3), np.nan), cov6=np.full((N, J, 6), np.nan),
               n_used=np.zeros((N, J), dtype=np.int64), deff=np.full((N, J), -1, dtype=np.int64))
    for f in range(N):
        for j in range(J):
            taps = _taps(case, f, j, cov_ok)
            n = len(taps)
            out["n_used"][f, j] = n
            if n == 0:
                continue
            de = min(d, n - 1)
            out["deff"][f, j] = de
            x0 = [float(v) for v in xyz[taps[0][1], j]]
            Mo = [[0.0] * 6 for _ in range(2 * d + 1)]
            R = [[0.0] * 3 for _ in range(d + 1)]
            for t, k in taps:
                w = 1.0 if case["weights"] is None else float(case["weights"][k, j])
                omega = w * _taper(case["taper"], t, h)
                L = lam[k, j] if case["cov6"] is not None else [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
                W = [omega * L[e] for e in range(6)]
                dx = [float(xyz[k, j, r]) - x0[r] for r in range(3)]
                v = [(W[s[0]] * dx[0] + W[s[1]] * dx[1]) + W[s[2]] * dx[2] for s in _SYM]
                t1 = float(t)
                tp = [1.0, t1, t1 * t1, (t1 * t1) * t1, (t1 * t1) * (t1 * t1)]
                for p in range(2 * d + 1):
                    for e in range(6):
                        Mo[p][e] = Mo[p][e] + tp[p] * W[e]
                for a in range(d + 1):
                    for r in range(3):
                        R[a][r] = R[a][r] + tp[a] * v[r]
            m = 3 * (de + 1)
            B = [[0.0] * m for _ in range(m)]
            y = [0.0] * m
            for a in range(de + 1):
                for r in range(3):
                    y[3 * a + r] = R[de - a][r]
                    for b in range(de + 1):
                        for c in range(3):
                            B[3 * a + r][3 * b + c] = Mo[(de - a) + (de - b)][_SYM[r][c]]
            for q in range(m):
                col = [B[i][q] / B[q][q] if i > q else None for i in range(m)]
                for i in range(q + 1, m):
                    for c in range(q + 1, i + 1):
                        B[i][c] = B[i][c] - col[i] * B[c][q]
                for i in range(q + 1, m):
                    B[i][q] = col[i]
                    y[i] = y[i] - col[i] * y[q]
            for q in range(m):
                y[q] = y[q] / B[q][q]
            for q in range(m - 1, 0, -1):
                for i in range(q):
                    y[i] = y[i] - B[q][i] * y[q]
            out["joints"][f, j] = [y[m - 3 + r] + x0[r] for r in range(3)]
            out["velocity"][f, j] = [y[m - 6 + r] for r in range(3)] if de >= 1 else 0.0
            out["cov6"][f, j] = _inverse3(B[m - 3][m - 3], B[m - 2][m - 2], B[m - 1][m - 1], B[m - 2][m - 3], B[m - 1][m - 3], B[m - 1][m - 2])
    return out


def accel_ref(xyz, gt=None, groups=None, n_groups=0):
    """sks_eval_accel: (table (1 + n_groups, 2, 1 + J) float64, counts of the same shape), summed entry by entry in frame-major
    order with math.fsum-free plain additions (the allowance of the test counts the terms)."""
    X = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    Y = None if gt is None else np.asarray(gt, dtype=np.float32).astype(np.float64)
    N, J = X.shape[:2]
    sums = np.zeros((1 + n_groups, 2, 1 + J))
    cnt = np.zeros((1 + n_groups, 2, 1 + J), dtype=np.int64)
    for f in range(1, N - 1):
        if groups is not None and not (groups[f - 1] == groups[f] == groups[f + 1]):
            continue
        rows = [0] + ([1 + int(groups[f])] if groups is not None and 0 <= groups[f] < n_groups else [])
        for j in range(J):
            if not np.all(np.isfinite(X[f - 1:f + 2, j])):
                continue
            a = X[f - 1, j] - 2.0 * X[f, j] + X[f + 1, j]
            figs = [np.sqrt(np.sum(a * a))]
            if Y is not None and np.all(np.isfinite(Y[f - 1:f + 2, j])):
                figs.append(np.sqrt(np.sum((a - (Y[f - 1, j] - 2.0 * Y[f, j] + Y[f + 1, j])) ** 2)))
            for row in rows:
                for k, v in enumerate(figs):
                    for col in (0, 1 + j):
                        sums[row, k, col] += v
                        cnt[row, k, col] += 1
    with np.errstate(all="ignore"):
        return sums / cnt, cnt
