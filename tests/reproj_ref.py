"""The float64 numpy restatement of csrc/sks_reproject.hip in the kernels' own order of operations -- what the GPU tests hold the
device to -- and an independent check of the refinement: scipy's Levenberg-Marquardt run to its limits on the same residuals.

Restated constants of k_refine: lambda starts at 1e-3, x 0.1 when a trial is accepted, x 10 when it is rejected; a joint stops
after an accepted trip with cost - trial < 1e-6 x cost, or at max_iters (<= 16).  The 3 x 3 solve is Cholesky."""
import numpy as np

from tests.tri_cases import _butterfly

LAMBDA0, LAMBDA_DOWN, LAMBDA_UP, STOP_FRACTION, MAX_ITERS = 1e-3, 0.1, 10.0, 1e-6, 16
EPS = np.finfo(np.float64).eps


def _rigs(P, N):
    return np.broadcast_to(P, (N,) + P.shape) if P.ndim == 3 else P


def project(P, X):
    """One frame: P (V,3,4), X (J,3) float64 -> u (V,J,3) with u = P_v [X; 1] added in column order 0..3, and mag (V,J,3) =
    sum_k |P_vk X_k|, the scale the device's rounding allowance is counted from."""
    Pb, Xb = P[:, None], X[None]
    u = np.stack([((Pb[..., r, 0] * Xb[..., 0] + Pb[..., r, 1] * Xb[..., 1]) + Pb[..., r, 2] * Xb[..., 2]) + Pb[..., r, 3]
                  for r in range(3)], axis=-1)
    mag = np.stack([np.abs(Pb[..., r, 0] * Xb[..., 0]) + np.abs(Pb[..., r, 1] * Xb[..., 1]) + np.abs(Pb[..., r, 2] * Xb[..., 2])
                    + np.abs(Pb[..., r, 3]) for r in range(3)], axis=-1)
    return u, mag


def reproject(P, X, det=None, valid=None):
    """sks_reproject: P (V,3,4) or (N,V,3,4), X (N,J,3), det (N,V,J,2) or None, valid (N,V,J) bool or None, everything widened
    to float64 -> dict(uv, err, in_front, per_joint, per_view, per_frame, n_used, u, mag)."""
    X = np.asarray(X, dtype=np.float64)
    N, J = X.shape[:2]
    P = _rigs(np.asarray(P, dtype=np.float64), N)
    V = P.shape[1]
    out = dict(uv=np.empty((N, V, J, 2)), err=np.full((N, V, J), np.nan), in_front=np.empty((N, V, J), bool),
               per_joint=np.empty((N, J)), per_view=np.empty((N, V)), per_frame=np.empty(N), n_used=np.empty((N, J), np.int32),
               u=np.empty((N, V, J, 3)), mag=np.empty((N, V, J, 3)))
    with np.errstate(all="ignore"):
        for n in range(N):
            u, mag = project(P[n], X[n])
            out["u"][n], out["mag"][n] = u, mag
            uv = np.stack([u[..., 0] / u[..., 2], u[..., 1] / u[..., 2]], axis=-1)
            out["uv"][n], out["in_front"][n] = uv, u[..., 2] > 0
            if det is not None:
                d = np.asarray(det[n], dtype=np.float64)
                keep = np.isfinite(d).all(axis=-1) & ~np.isnan(X[n]).any(axis=-1)[None]
                if valid is not None:
                    keep &= np.asarray(valid[n], dtype=bool)
                dx, dy = uv[..., 0] - d[..., 0], uv[..., 1] - d[..., 1]
                out["err"][n] = np.where(keep, np.sqrt(dx * dx + dy * dy), np.nan)
            e = out["err"][n]
            for j in range(J):                  # pass 2: a joint's views in ascending order
                s, c = 0.0, 0
                for v in range(V):
                    if e[v, j] == e[v, j]:
                        s, c = s + e[v, j], c + 1
                out["per_joint"][n, j], out["n_used"][n, j] = np.float64(s) / np.float64(c), c
            S, C = 0.0, 0                       # pass 3: a view's joints in ascending order, then the views
            for v in range(V):
                s, c = 0.0, 0
                for j in range(J):
                    if e[v, j] == e[v, j]:
                        s, c = s + e[v, j], c + 1
                out["per_view"][n, v] = np.float64(s) / np.float64(c)
                S, C = S + s, C + c
            out["per_frame"][n] = np.float64(S) / np.float64(C)
    return out


def eval_reprojection(err, groups=None, n_groups=0):
    """sks_eval_reprojection: (table (1 + n_groups, 1 + V + J), counts of the same shape).  Thread t adds frames t, t + 256, ...
    in index order, a frame's entries of the column in index order; the 256 partial sums meet in the kernel's tree."""
    N, V, J = err.shape
    out = np.full((1 + n_groups, 1 + V + J), np.nan)
    cnt = np.zeros(out.shape, dtype=np.int64)
    cols = [err.reshape(N, -1)] + [err[:, v, :] for v in range(V)] + [err[:, :, j] for j in range(J)]
    with np.errstate(all="ignore"):
        for r in range(1 + n_groups):
            rows = np.arange(N) if r == 0 else np.flatnonzero(np.asarray(groups) == r - 1)
            for c, col in enumerate(cols):
                part, k = np.zeros(256), 0
                for i in rows:
                    for x in col[i]:
                        if x == x:
                            part[i % 256] += x
                            k += 1
                o = 128
                while o > 0:
                    part[:o] = part[:o] + part[o:2 * o]
                    o >>= 1
                out[r, c], cnt[r, c] = part[0] / np.float64(k), k
    return out, cnt


def _rho(e, huber):
    return np.where(e <= huber, e * e, 2.0 * huber * e - huber * huber) if huber > 0 else e * e


def refine(P, det, valid, X0, huber=0.0, max_iters=MAX_ITERS, tie_ulps=64):
    """sks_triangulate_refine, every joint at once as (N,J,W) lanes with W = the next power of two >= V; the ten sums of a trip
    are tri_cases._butterfly over the lanes, padding lanes and left-out views adding zeros.
    -> X (N,J,3), cost (N,J,2), iters (N,J) int32, near_tie (N,J) bool: some accept or stop comparison of the joint was within
    `tie_ulps` roundings of its larger side of a tie (there the device may decide the other way)."""
    det = np.asarray(det, dtype=np.float64)
    N, V, J = det.shape[:3]
    W = 1
    while W < V:
        W <<= 1
    Pl = np.zeros((N, 1, W, 3, 4))
    Pl[:, 0, :V] = _rigs(np.asarray(P, dtype=np.float64), N)
    x, y = np.zeros((N, J, W)), np.zeros((N, J, W))
    x[..., :V], y[..., :V] = det[..., 0].transpose(0, 2, 1), det[..., 1].transpose(0, 2, 1)
    use = np.zeros((N, J, W), dtype=bool)
    use[..., :V] = np.isfinite(x[..., :V]) & np.isfinite(y[..., :V])
    if valid is not None:
        use[..., :V] &= np.asarray(valid, dtype=bool).transpose(0, 2, 1)

    def at(X):
        Xb = X[:, :, None]
        row = lambda r: ((Pl[..., r, 0] * Xb[..., 0] + Pl[..., r, 1] * Xb[..., 1]) + Pl[..., r, 2] * Xb[..., 2]) + Pl[..., r, 3]
        u2 = row(2)
        px, py = row(0) / u2, row(1) / u2
        dx, dy = px - x, py - y
        return px, py, u2, dx, dy, np.sqrt(dx * dx + dy * dy)

    lanes = lambda t: _butterfly(np.where(use, t, 0.0))
    with np.errstate(all="ignore"):
        X = np.asarray(X0, dtype=np.float64).copy()
        cur = at(X)
        cost = lanes(_rho(cur[5], huber))
        cost0 = cost.copy()
        active = (use.sum(axis=-1) >= 2) & np.isfinite(X).all(axis=-1) & ~(use & ~(cur[2] > 0)).any(axis=-1)
        lam = np.full(cost.shape, LAMBDA0)
        iters = np.zeros(cost.shape, dtype=np.int32)
        near = np.zeros(cost.shape, dtype=bool)
        for _ in range(max_iters):
            if not active.any():
                break
            px, py, u2, dx, dy, e = cur
            w = np.where(e <= huber, 1.0, huber / e) if huber > 0 else np.ones_like(e)
            Jx = [(Pl[..., 0, k] - px * Pl[..., 2, k]) / u2 for k in range(3)]
            Jy = [(Pl[..., 1, k] - py * Pl[..., 2, k]) / u2 for k in range(3)]
            a = {(r, c): lanes(w * (Jx[r] * Jx[c] + Jy[r] * Jy[c])) for r in range(3) for c in range(r + 1)}
            g = [lanes(w * (Jx[r] * dx + Jy[r] * dy)) for r in range(3)]
            m00, m11, m22 = a[0, 0] + lam * a[0, 0], a[1, 1] + lam * a[1, 1], a[2, 2] + lam * a[2, 2]
            l00 = np.sqrt(m00)
            l10, l20 = a[1, 0] / l00, a[2, 0] / l00
            d1 = m11 - l10 * l10
            l11 = np.sqrt(d1)
            l21 = (a[2, 1] - l20 * l10) / l11
            d2 = (m22 - l20 * l20) - l21 * l21
            l22 = np.sqrt(d2)
            solved = (m00 > 0) & (d1 > 0) & (d2 > 0)
            y0 = -g[0] / l00
            y1 = (-g[1] - l10 * y0) / l11
            y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22
            e2 = y2 / l22
            e1 = (y1 - l21 * e2) / l11
            e0 = ((y0 - l10 * e1) - l20 * e2) / l00
            T = X + np.stack([e0, e1, e2], axis=-1)
            trial = at(T)
            tcost = lanes(np.where(trial[2] > 0, _rho(trial[5], huber), np.inf))
            accept = active & solved & (tcost < cost)
            drop = cost - tcost
            stop = accept & (drop < STOP_FRACTION * cost)
            # a tie of the accept comparison (trial against cost) or of the stop comparison (drop against fraction x cost)
            slack = tie_ulps * EPS * cost
            near |= active & solved & np.isfinite(tcost) & ((np.abs(drop) <= slack) | (np.abs(drop - STOP_FRACTION * cost) <= slack))
            iters += active
            lam = np.where(accept, lam * LAMBDA_DOWN, np.where(active, lam * LAMBDA_UP, lam))
            X = np.where(accept[..., None], T, X)
            cur = tuple(np.where(accept[..., None], t, c) for t, c in zip(trial, cur))
            cost = np.where(accept, tcost, cost)
            active &= ~stop
    return X, np.stack([cost0, cost], axis=-1), iters, near


def scipy_lm(P, det, valid, X0):
    """Each joint's plain-squares minimum by scipy.optimize.least_squares(method="lm") run to its limits (tolerances at the
    float64 floor, restarted once from its own result): P (V,3,4), det (V,J,2), valid (V,J) bool or None, X0 (J,3) -> (J,3)."""
    from scipy.optimize import least_squares
    P, det = np.asarray(P, dtype=np.float64), np.asarray(det, dtype=np.float64)
    V, J = det.shape[:2]
    out = np.array(X0, dtype=np.float64)
    for j in range(J):
        keep = np.arange(V) if valid is None else np.flatnonzero(np.asarray(valid)[:, j])

        def residuals(X):
            u = P[keep] @ np.append(X, 1.0)
            return (u[:, :2] / u[:, 2:3] - det[keep, j]).ravel()
        sol = out[j]
        for _ in range(2):
            sol = least_squares(residuals, sol, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000).x
        out[j] = sol
    return out
