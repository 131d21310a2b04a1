"""Float64 textbook solutions of the per-frame alignment sks_align_poses computes (csrc/sks_align.hip), numpy only:

umeyama   S. Umeyama, "Least-squares estimation of transformation parameters between two point patterns", PAMI 13(4), 1991:
          SVD of the cross-covariance, the smallest singular direction flipped where the best orthogonal matrix is a reflection;
horn      B. K. P. Horn, "Closed-form solution of absolute orientation using unit quaternions", JOSA A 4(4), 1987: the
          eigenvector of the largest eigenvalue of a symmetric 4x4 matrix (np.linalg.eigh).

They share the conventions of include/skelsplat_hip.h (pred onto gt over the joints with valid != 0; modes rigid, similarity,
scale) and nothing else: neither calls the other, and neither uses the product."""
import numpy as np

MODES = ("rigid", "similarity", "scale")
U32 = 2.0 ** -24        # half an ulp of float32, relative


def _select(pred, gt, valid):
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    assert pred.shape == gt.shape and pred.ndim == 2 and pred.shape[1] == 3, (pred.shape, gt.shape)
    v = np.ones(len(pred), dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    assert v.shape == (len(pred),)
    return pred, gt, v


_IDENTITY = (1.0, np.eye(3), np.zeros(3))
_NAN = (np.nan, np.full((3, 3), np.nan), np.full(3, np.nan))


def _scale_only(pred, gt, v, dot):
    """mode "scale": both poses relative to joint 0, s = sum <x, y> / sum <x, x> over the valid joints."""
    if not v[0]:
        return _NAN
    x, y = pred[v] - pred[0], gt[v] - gt[0]
    den = dot(x, x)
    s = dot(x, y) / den if den != 0 else 1.0
    if not np.isfinite(s):
        return _NAN
    return float(s), np.eye(3), gt[0] - s * pred[0]


def umeyama(pred, gt, valid=None, mode="similarity"):
    """(s, R (3,3), t (3,)) with s R pred_i + t ~ gt_i, from the SVD of H = sum x_i y_i^T."""
    assert mode in MODES
    pred, gt, v = _select(pred, gt, valid)
    if not v.any():
        return _IDENTITY
    if mode == "scale":
        return _scale_only(pred, gt, v, lambda a, b: float(np.sum(a * b)))
    mx, my = pred[v].mean(axis=0), gt[v].mean(axis=0)
    x, y = pred[v] - mx, gt[v] - my
    H = x.T @ y
    if not np.isfinite(H).all():
        return _NAN
    U, S, Vt = np.linalg.svd(H)
    d = np.array([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ np.diag(d) @ U.T
    sxx = float(np.sum(x * x))
    s = float(np.sum(S * d)) / sxx if mode == "similarity" and sxx != 0 else 1.0
    return s, R, my - s * (R @ mx)


def horn(pred, gt, valid=None, mode="similarity"):
    """The same transform from the unit quaternion that maximises q^T N q."""
    assert mode in MODES
    pred, gt, v = _select(pred, gt, valid)
    if not v.any():
        return _IDENTITY
    if mode == "scale":
        return _scale_only(pred, gt, v, lambda a, b: float(np.einsum("ij,ij->", a, b)))
    mx, my = np.sum(pred[v], axis=0) / v.sum(), np.sum(gt[v], axis=0) / v.sum()
    x, y = pred[v] - mx, gt[v] - my
    M = np.einsum("ia,ib->ab", x, y)
    if not np.isfinite(M).all():
        return _NAN
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    lam, vec = np.linalg.eigh(N)
    w, a, b, c = vec[:, -1] / np.linalg.norm(vec[:, -1])
    R = np.array([[w * w + a * a - b * b - c * c, 2 * (a * b - w * c), 2 * (a * c + w * b)],
                  [2 * (a * b + w * c), w * w - a * a + b * b - c * c, 2 * (b * c - w * a)],
                  [2 * (a * c - w * b), 2 * (b * c + w * a), w * w - a * a - b * b + c * c]])
    sxx = float(np.einsum("ij,ij->", x, x))
    # (the largest eigenvalue is the sum of <R x_i, y_i> at the optimum: Horn's eq. for the scale with the asymmetry of Umeyama's)
    s = float(lam[-1]) / sxx if mode == "similarity" and sxx != 0 else 1.0
    return s, R, my - s * (R @ mx)


def apply(transform, pred):
    s, R, t = transform
    return s * (np.asarray(pred, dtype=np.float64) @ np.asarray(R).T) + t


def errors(pred, gt, valid=None, mode="similarity", solver=umeyama):
    """One frame: (aligned (P,3), per_joint (P,), mean) -- aligned and per_joint for ALL joints with the transform fitted on the
    valid ones, the mean over the valid ones (NaN without any)."""
    pred, gt, v = _select(pred, gt, valid)
    aligned = apply(solver(pred, gt, v, mode), pred)
    per_joint = np.linalg.norm(gt - aligned, axis=-1)
    return aligned, per_joint, float(per_joint[v].mean()) if v.any() else float("nan")


def batch_errors(pred, gt, valid=None, mode="similarity", solver=umeyama):
    """(N,P,3) poses: (aligned (N,P,3), per_joint (N,P), mean (N,), transforms: s (N,), R (N,3,3), t (N,3))."""
    out = [errors(pred[f], gt[f], None if valid is None else valid[f], mode, solver) for f in range(len(pred))]
    tr = [solver(pred[f], gt[f], None if valid is None else valid[f], mode) for f in range(len(pred))]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out]),
            (np.array([t[0] for t in tr]), np.stack([t[1] for t in tr]), np.stack([t[2] for t in tr])))


def objective(transform, pred, gt, valid=None):
    """sum over the valid joints of ||gt - (s R pred + t)||^2."""
    pred, gt, v = _select(pred, gt, valid)
    return float(np.sum((gt[v] - apply(transform, pred[v])) ** 2))


def extent(gt, valid=None):
    """The largest |gt - centroid| coordinate over the valid joints (0 without any): the length the allowances scale with."""
    gt = np.asarray(gt, dtype=np.float64)
    v = np.ones(len(gt), dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    if not v.any() or not np.isfinite(gt[v]).all():
        return 0.0
    return float(np.abs(gt[v] - gt[v].mean(axis=0)).max())


def conditioning(pred, gt, valid=None, mode="similarity"):
    """How well the data determine the transform, in [0, 1]; the tests compare s, R and t where this is >= 1e-3.
    rigid / similarity: sigma_2 / sigma_1 of H (below it the rotation about the dominant direction is decided by rounding);
    scale: |sum <x, y>| / sqrt(sum <x, x> sum <y, y>) (below it s is the remainder of a cancellation)."""
    pred, gt, v = _select(pred, gt, valid)
    if not v.any() or not (np.isfinite(pred[v]).all() and np.isfinite(gt[v]).all()):
        return 0.0
    if mode == "scale":
        if not v[0]:
            return 0.0
        x, y = pred[v] - pred[0], gt[v] - gt[0]
        den = np.sqrt(np.sum(x * x) * np.sum(y * y))
        return float(abs(np.sum(x * y)) / den) if den > 0 else 0.0
    x, y = pred[v] - pred[v].mean(axis=0), gt[v] - gt[v].mean(axis=0)
    S = np.linalg.svd(x.T @ y, compute_uv=False)
    return float(S[1] / S[0]) if S[0] > 0 else 0.0


def allowance(ref, ext):
    """|device - ref| for an error, a mean or an aligned coordinate `ref` of a frame of extent `ext`:
    2^-23 |ref| for the one rounding of the float64 result to float32 (half an ulp, and one spare unit), plus 1e-10 ext for the
    float64 fit itself -- about 180 x what the two solutions above differ by over the case table (5.5e-13 ext)."""
    return 2.0 ** -23 * np.abs(ref) + 1e-10 * np.asarray(ext, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ sequences
def eval_sequence_ref(per_joint_pa, per_joint_n, valid, groups, n_groups):
    """(1 + n_groups, 2) float64: row 0 the mean over all valid joints of all frames of the two (N,P) per-joint errors, row 1 + g
    over the frames of group g; NaN for a row without valid joints."""
    N, P = per_joint_pa.shape
    v = np.ones((N, P), dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    rows = [np.ones(N, dtype=bool)] + [np.asarray(groups) == g for g in range(n_groups)]
    out = np.full((len(rows), 2), np.nan)
    for r, sel in enumerate(rows):
        m = v & sel[:, None]
        if m.any():
            out[r] = [np.asarray(per_joint_pa, dtype=np.float64)[m].mean(), np.asarray(per_joint_n, dtype=np.float64)[m].mean()]
    return out
