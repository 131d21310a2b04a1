"""Seeded cases for csrc/sks_uncertainty.hip, shared by the CPU tests (which hold their conditions on the references alone) and
the GPU tests.  numpy only."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_uncertainty.npz")

# (N, P): N x P = 1, 255, 256, 257 -- one thread, a block less one, a full block, a second block -- and the skeletons' sizes
JOINT_SHAPES = ((1, 1), (15, 17), (1, 255), (16, 16), (1, 256), (1, 257), (3, 17), (2, 19), (1, 65))
MODIFIERS = (1.0, 1.3)
CAL_N, CAL_P, CAL_K = (1, 255, 256, 257, 1000), (1, 17, 19), (1, 3, 8)
CAL_LEVELS = (1.0, 2.0, 3.0, 0.5, 1.5, 2.5, 3.5, 4.0)      # the first K are a case's sigma levels
GAP_FACTOR = 8.0            # no fixture joint's d2 may sit within this many allowances of a threshold


def joint_case(N, P, seed=0):
    """dict of float32 arrays xyz, scales (ACTIVATED), rot, gt, all (N,P,..).  Scales from 1e-3 to 1e4 with ratios up to 1e6 inside
    a joint (the first joints of the case are the corners: both ends isotropic, a needle and a disc at the full ratio); quaternion
    norms from 1e-3 to 1e3; the ground truth at a Mahalanobis distance in [0.05, 4] in a random direction."""
    rng = np.random.default_rng(1000 * N + P + 7919 * seed)
    n = N * P
    big = 10.0 ** rng.uniform(-3.0, 4.0, (n, 1))
    scales = np.maximum(big * 10.0 ** rng.uniform(-6.0, 0.0, (n, 3)), 1e-3)
    scales[np.arange(n), rng.integers(0, 3, n)] = big[:, 0]
    corners = np.array([[1e-3, 1e-3, 1e-3], [1e4, 1e4, 1e4], [1e4, 1e-2, 1e-2], [1e-2, 1e4, 1e4], [7.0, 7.0, 7.0]])
    scales[:min(n, len(corners))] = corners[:n]
    q = rng.normal(0.0, 1.0, (n, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * 10.0 ** rng.uniform(-3.0, 3.0, (n, 1))
    if n > 5:
        q[5] = [2.0, 0.0, 0.0, 0.0]                         # the identity, un-normalised
    xyz = rng.normal(0.0, 800.0, (n, 3))
    scales32, q32, xyz32 = scales.astype(np.float32), q.astype(np.float32), xyz.astype(np.float32)
    from tests import uncertainty_ref as ur
    u = rng.normal(0.0, 1.0, (n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    m = rng.uniform(0.05, 4.0, (n, 1))
    gt = xyz32.astype(np.float64) + np.einsum("nab,nb->na", ur.rotation_ref(q32), scales32.astype(np.float64) * u * m)
    sh = lambda a, k: np.ascontiguousarray(a.reshape(N, P, k))
    return dict(xyz=sh(xyz32, 3), scales=sh(scales32, 3), rot=sh(q32, 4), gt=sh(gt.astype(np.float32), 3))


def calibration_case(N, P, seed=0):
    """(d2 (N,P) float32, valid (N,) bool): distances m^2 with m uniform in [0.05, 4.2], and planted among them every level's
    threshold itself (fl(k x k): inside), the float just above it (outside), +inf (counted, inside nothing), NaN (not counted) and
    frames that are not valid."""
    rng = np.random.default_rng(77 * N + P + 7919 * seed)
    d2 = (rng.uniform(0.05, 4.2, (N, P)) ** 2).astype(np.float32)
    flat = d2.reshape(-1)
    plant = []
    for k in CAL_LEVELS:
        t = np.float32(k) * np.float32(k)
        plant += [t, np.nextafter(t, np.float32(np.inf))]
    plant += [np.float32(np.inf), np.float32(np.nan), np.float32(np.nan)]
    where = rng.permutation(flat.size)[:len(plant)]
    flat[where] = np.array(plant, np.float32)[:len(where)]
    valid = rng.uniform(size=N) > 0.2
    if N > 2:
        valid[1], valid[N - 1] = False, True
    return d2, valid


def fixture():
    """tests/golden/reference_uncertainty.npz as a dict (see tests/golden/make_golden_uncertainty.py)."""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
