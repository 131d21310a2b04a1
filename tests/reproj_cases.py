"""Shared by tests/test_reprojection_cpu.py and tests/test_reprojection_gpu.py: the seeded scenes of the reprojection kernels
(csrc/sks_reproject.hip), small on purpose -- N = 3 frames --, and the counted rounding allowances the device is held to."""
import numpy as np

from tests import tri_cases

EPS = np.finfo(np.float64).eps
N = 3
REPROJECT_VIEWS = (1, 2, 3, 4, 5, 31, 64)
REPROJECT_JOINTS = (1, 17, 19)
REFINE_VIEWS = (2, 3, 4, 5, 8, 31, 64)          # lane groups of 2, 4, 4, 8, 8, 32, 64
HUBER_PX, SHIFT_PX, SHIFT_VIEW = 10.0, 40.0, 1  # the Huber case: one view's x coordinates are off by 40 px
NEAR_TIE_SHARE = 0.01                            # at most this share of a case's joints may sit on a tie of the restatement
_cache = {}


def scene(V, J=17, frames=N, seed=0):
    """(P (V,3,4), joints to measure (frames,J,3) -- the ground truth off by 5 mm of noise --, detections (frames,V,J,2) with
    3 px of noise), float64.  J = 19 is the Panoptic skeleton, 17 H36M's, 1 its first joint."""
    key = (V, J, frames, seed)
    if key not in _cache:
        sc, P, gt, p2d = tri_cases.sequence("panoptic" if J == 19 else "h36m", V, frames=frames, seed=seed, dtype=np.float64)
        rng = np.random.default_rng(100 + seed)
        X = gt + rng.normal(0, 5.0, gt.shape)
        _cache[key] = (P, X[:, :J].copy(), p2d[:, :, :J].copy())
    return tuple(a.copy() for a in _cache[key])


def rigs_per_frame(P, frames=N):
    """(frames,V,3,4): frame n sees the rig with its views rotated by n places (its detections then belong to other cameras: the
    errors are large and as well defined as any)."""
    return np.stack([np.roll(P, n, axis=0) for n in range(frames)])


def hard_reproject_case(V, J):
    """P, X, det, valid with: a mask that empties joint J - 1 of frame 0, view V - 1 of frame 1 and the whole of frame 2; a NaN
    detection at (0, 0, 0); joint 0 of frame 1 mirrored behind camera 0.  -> (P, X, det, valid, behind = (1, 0, 0))."""
    P, X, det = scene(V, J, seed=4)
    valid = np.ones((N, V, J), dtype=bool)
    valid[0, :, J - 1] = False
    valid[1, V - 1, :] = False
    valid[2] = False
    det[0, 0, 0, 0] = np.nan
    r3 = P[0, 2, :3]                                   # (K's last row is 0 0 1: the unit viewing direction of camera 0)
    depth = r3 @ X[1, 0] + P[0, 2, 3]
    X[1, 0] = X[1, 0] - 2.0 * depth * r3               # the same point mirrored in camera 0's plane: depth -> -depth
    return P, X, det, valid, (1, 0, 0)


def pixel_allowances(ref):
    """From reproj_ref.reproject's own u and mag = sum_k |P_vk X_k|: how far a float64 evaluation of the same formulas in the same
    order may sit from it.  A component of u is four products and three additions: |du_r| <= 4 eps mag_r.  uv_k = u_k / u_2:
    |duv_k| <= (4 eps mag_k + |uv_k| 4 eps mag_2) / |u_2| + eps |uv_k|.  err = sqrt(dx^2 + dy^2) with dx = uv_x - x: |derr| <=
    |duv_x| + |duv_y| + 5 eps err (the subtractions eps (|dx| + |dy|) <= 2 eps err; two squares, an addition and the root: 2.5
    eps err, rounded up).  Both sides carry such an error, so the allowance is twice that.  -> (allow_uv (N,V,J,2), allow_err)."""
    u, mag, uv = ref["u"], ref["mag"], ref["uv"]
    with np.errstate(all="ignore"):
        a = [(4 * mag[..., k] + np.abs(uv[..., k]) * 4 * mag[..., 2]) / np.abs(u[..., 2]) + np.abs(uv[..., k]) for k in range(2)]
        allow_uv = 2 * EPS * np.stack(a, axis=-1)
        allow_err = allow_uv[..., 0] + allow_uv[..., 1] + 2 * 5 * EPS * np.nan_to_num(ref["err"])
    return allow_uv, allow_err


def mean_allowance(values, allow, axis):
    """A mean of n kept terms added one after the other and divided once: the terms' own allowances (their largest) plus
    2 (n + 1) eps of the mean of their magnitudes (n - 1 additions, a division, both sides)."""
    n = (~np.isnan(values)).sum(axis=axis)
    with np.errstate(all="ignore"):
        scale = np.nansum(np.abs(values), axis=axis) / np.maximum(n, 1)
    return np.nanmax(np.where(np.isnan(values), 0.0, allow), axis=axis) + 2 * (n + 1) * EPS * scale


def refine_case(V, kind="plain", seed=0):
    """(P, det (N,V,17,2), valid or None, start (N,17,3) = the DLT of the kept views, huber_px) for kind in plain / huber / masks."""
    from skelsplat_amd import triangulation
    P, _, det = scene(V, 17, seed=seed)
    valid, huber = None, 0.0
    if kind == "huber":
        det[:, SHIFT_VIEW % V, :, 0] += SHIFT_PX
        huber = HUBER_PX
    if kind == "masks":
        rng = np.random.default_rng(7 + seed)
        valid = np.ones((N, V, 17), dtype=bool)
        for f in range(N):
            for j in range(17):
                valid[f, rng.choice(V, size=rng.integers(0, max(V - 1, 1)), replace=False), j] = False       # 2 .. V views kept
        valid[0, :, 9] = True           # an intact joint beside ...
        valid[1, 0, 3], valid[1, 1:, 3] = True, False         # ... one kept in a single view
        valid[2, :, 5] = False          # ... and a fully masked one
        det[~valid] = np.nan            # a left-out detection is never read
    start = triangulation.triangulate_sequence(P, det, valid=valid, homogeneous=True)[..., :3]
    return P, det, valid, start, huber
