"""The three definitions of include/skelsplat_hip.h "Constant limb lengths" restated op by op on Python floats (IEEE float64, one
rounding per operation, math.sqrt correctly rounded), a frame and a bone at a time, in the header's loop orders -- what
csrc/sks_bones.hip must equal bit for bit; the select is np.sort plus the index.  Written from the header, not from the kernel or
from skeleton.py's vectorised host functions, which tests/test_bones_cpu.py holds to it."""
import math

import numpy as np

SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
INF, NAN = float("inf"), float("nan")


def f32(x):
    return np.float32(x)


def quad(a, M, b):
    w = [(M[s[0]] * b[0] + M[s[1]] * b[1]) + M[s[2]] * b[2] for s in SYM]
    return (a[0] * w[0] + a[1] * w[1]) + a[2] * w[2]


def div(a, b):
    """IEEE division on Python floats (Python raises where IEEE gives inf or NaN)."""
    return float(np.float64(a) / np.float64(b))


def norm3(d):
    s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return math.sqrt(s) if s >= 0 and s != INF else (INF if s == INF else NAN)


def usable_end(xyz, valid, f, j):
    return bool(np.isfinite(xyz[f, j]).all()) and (valid is None or bool(valid[f, j]))


def measure(xyz, bones, cov6=None, valid=None, max_sigma_mm=None):
    """sks_bone_measure: (N,B) float32."""
    xyz = np.asarray(xyz, dtype=np.float32)
    N, B = xyz.shape[0], len(bones)
    out = np.full((N, B), np.nan, dtype=np.float32)
    with np.errstate(all="ignore"):
        for f in range(N):
            for b, (p, c) in enumerate(bones):
                if not (usable_end(xyz, valid, f, p) and usable_end(xyz, valid, f, c)):
                    continue
                d = [float(xyz[f, c, k]) - float(xyz[f, p, k]) for k in range(3)]
                n = norm3(d)
                if max_sigma_mm is not None:
                    u = [div(d[k], n) for k in range(3)]
                    S = [float(cov6[f, p, e]) + float(cov6[f, c, e]) for e in range(6)]
                    if not quad(u, S, u) <= float(max_sigma_mm) * float(max_sigma_mm):
                        continue
                out[f, b] = f32(n)
    return out


def lengths(measured, groups=None, n_groups=1):
    """sks_bone_lengths: length, mad (G,B) float32 and n_used (G,B) int32."""
    M = np.asarray(measured, dtype=np.float32)
    N, B = M.shape
    G = int(n_groups)
    length, mad = np.full((G, B), np.nan, dtype=np.float32), np.full((G, B), np.nan, dtype=np.float32)
    n_used = np.zeros((G, B), dtype=np.int32)
    for g in range(G):
        for b in range(B):
            l = np.array([M[f, b] for f in range(N) if (0 if groups is None else int(groups[f])) == g
                          and np.isfinite(M[f, b]) and not np.signbit(M[f, b])], dtype=np.float32)
            n = len(l)
            if n == 0:
                continue
            k = (n - 1) // 2
            m = np.sort(l)[k]
            dev = np.abs((l - m).astype(np.float32))             # float32 - float32, rounded once
            length[g, b], mad[g, b], n_used[g, b] = m, np.sort(dev)[k], n
    return length, mad, n_used


def pivots_positive(S):
    xx, xy, xz, yy, yz, zz = S
    d0 = xx
    l10 = div(xy, d0)
    l20 = div(xz, d0)
    d1 = yy - l10 * xy
    e = yz - l20 * xy
    z1 = zz - l20 * xz
    l21 = div(e, d1)
    d2 = z1 - l21 * e
    return all(math.isfinite(q) and q > 0 for q in (d0, d1, d2))


def project_frame(y32, bones, L32, in_range, cov6=None, valid=None, cov_floor=0.0, max_iters=16, tol_mm=1e-3, trace=None):
    """One frame of sks_bone_project.  y32 (J,3) float32, L32 (B,) float32: the frame's group's lengths, in_range: is its group
    id one of the rows.  Returns joints (J,3) float32, residual float32, n_trips, n_active.  trace: a list that receives x (J,3)
    float64 after every trip."""
    J, B = y32.shape[0], len(bones)
    x = [[float(y32[j, k]) for k in range(3)] for j in range(J)]
    Sig, fit = [], []
    for j in range(J):
        ok = bool(np.isfinite(y32[j]).all()) and (valid is None or bool(valid[j]))
        S = [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
        if cov6 is not None:
            S = [float(cov6[j, e]) for e in range(6)]
            for e in (0, 3, 5):
                S[e] = S[e] + float(cov_floor)
            ok = ok and all(math.isfinite(s) for s in S) and pivots_positive(S)
        Sig.append(S)
        fit.append(ok)
    L = [float(L32[b]) for b in range(B)]
    active = [in_range and fit[p] and fit[c] and math.isfinite(L[b]) and L[b] > 0 for b, (p, c) in enumerate(bones)]
    moved = [False] * J
    trips, rho, n_act = 0, NAN, 0
    while True:
        u, r = [None] * B, [0.0] * B
        for b, (p, c) in enumerate(bones):
            if not active[b]:
                continue
            d = [x[c][k] - x[p][k] for k in range(3)]
            n = norm3(d)
            if n == 0.0:
                active[b] = False
                continue
            u[b] = [div(d[k], n) for k in range(3)]
            r[b] = n - L[b]
        n_act = sum(active)
        if n_act == 0:
            break
        rho = max((abs(r[b]) if math.isfinite(r[b]) else INF) for b in range(B) if active[b])
        if rho <= tol_mm or trips == max_iters:
            break
        S = [[0.0] * B for _ in range(B)]
        yv = [r[b] if active[b] else 0.0 for b in range(B)]
        for a, (pa, ca) in enumerate(bones):
            for b in range(a + 1):
                pb, cb = bones[b]
                if not (active[a] and active[b]):
                    S[a][b] = 1.0 if a == b else 0.0
                    continue
                s = 0.0
                if pa == pb:
                    s = s + quad(u[a], Sig[pa], u[b])
                if pa == cb:
                    s = s - quad(u[a], Sig[pa], u[b])
                if ca == pb:
                    s = s - quad(u[a], Sig[ca], u[b])
                if ca == cb:
                    s = s + quad(u[a], Sig[ca], u[b])
                S[a][b] = s
        ok = True
        for j in range(B):
            dj = S[j][j]
            ok = ok and math.isfinite(dj) and dj > 0
            col = {i: div(S[i][j], dj) for i in range(j + 1, B)}
            for i in range(j + 1, B):
                for c in range(j + 1, i + 1):
                    S[i][c] = S[i][c] - col[i] * S[c][j]
            for i in range(j + 1, B):
                S[i][j] = col[i]
                yv[i] = yv[i] - col[i] * yv[j]
        if not ok:
            break
        for j in range(B):
            yv[j] = div(yv[j], S[j][j])
        for j in range(B - 1, 0, -1):
            for i in range(j):
                yv[i] = yv[i] - S[j][i] * yv[j]
        for j in range(J):
            g, touched = [0.0, 0.0, 0.0], False
            for b, (p, c) in enumerate(bones):
                if not active[b]:
                    continue
                if c == j:
                    touched = True
                    g = [g[k] + yv[b] * u[b][k] for k in range(3)]
                if p == j:
                    touched = True
                    g = [g[k] - yv[b] * u[b][k] for k in range(3)]
            if touched:
                Sj = Sig[j]
                x[j] = [x[j][k] - ((Sj[SYM[k][0]] * g[0] + Sj[SYM[k][1]] * g[1]) + Sj[SYM[k][2]] * g[2]) for k in range(3)]
                moved[j] = True
        trips += 1
        if trace is not None:
            trace.append(np.array(x))
    out = np.array(y32, dtype=np.float32, copy=True)
    for j in range(J):
        if moved[j]:
            out[j] = np.array(x[j]).astype(np.float32)
    return out, f32(rho), trips, n_act


def project(xyz, bones, lengths_, cov6=None, valid=None, groups=None, cov_floor=0.0, max_iters=16, tol_mm=1e-3):
    """sks_bone_project: joints (N,J,3) float32, residual (N,) float32, n_trips, n_active (N,) int32."""
    xyz = np.asarray(xyz, dtype=np.float32)
    Lt = np.asarray(lengths_, dtype=np.float32)
    Lt = Lt[None] if Lt.ndim == 1 else Lt
    N, G = xyz.shape[0], Lt.shape[0]
    bones = [(int(p), int(c)) for p, c in bones]
    joints = np.empty_like(xyz)
    res, trips, nact = np.empty(N, np.float32), np.empty(N, np.int32), np.empty(N, np.int32)
    with np.errstate(all="ignore"):
        for f in range(N):
            g = 0 if groups is None else int(groups[f])
            inr = 0 <= g < G
            joints[f], res[f], trips[f], nact[f] = project_frame(
                xyz[f], bones, Lt[g] if inr else Lt[0], inr, None if cov6 is None else cov6[f], None if valid is None else valid[f],
                cov_floor, max_iters, tol_mm)
    return joints, res, trips, nact


def sigma_cost(x, y, cov6=None, cov_floor=0.0):
    """sum_j (x_j - y_j)^T Sigma_j^-1 (x_j - y_j) of one frame (float64, numpy's solve): what the Sigma-closest pose minimises."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    total = 0.0
    for j in range(x.shape[0]):
        d = x[j] - y[j]
        if cov6 is None:
            total += float(d @ d)
        else:
            c = np.asarray(cov6[j], np.float64)
            S = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]) + cov_floor * np.eye(3)
            total += float(d @ np.linalg.solve(S, d))
    return total
