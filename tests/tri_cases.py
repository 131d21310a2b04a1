"""Shared by tests/test_triangulate_cpu.py and tests/test_triangulate_gpu.py: seeded synthetic sequences, the three golden
triangulation cases of tests/golden/reference_next.npz, and a numpy restatement of the device kernel's arithmetic."""
import os

import numpy as np

from skelsplat_amd import scene, triangulation

NEXT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_next.npz")
GOLDEN_TAGS = ("h36m4", "pan8", "two")
# the project's bars for this quantity (tests/test_cpu.py): against the reference's golden X, and batched SVD against SVD
GOLDEN_TOL = dict(rtol=1e-8, atol=1e-6)
SVD_TOL = dict(rtol=1e-9, atol=1e-6)


def golden(tag):
    """(P (V,3,4), x2d (V,J,2), X (J,4)) float64: the reference's own inputs and output."""
    G = np.load(NEXT)
    return tuple(G[f"tri_{tag}_{k}"] for k in ("P", "x2d", "X"))


def sequence(dataset="h36m", n_views=4, frames=5, seed=0, device="cpu", dtype=np.float32):
    """A moving skeleton seen by `n_views` cameras: (SyntheticScene, P (V,3,4), gt (N,J,3), detections (N,V,J,2) with 3 px
    of noise)."""
    sc = scene.SyntheticScene(dataset, n_views=n_views, seed=seed, device=device)
    rng = np.random.default_rng(seed + 1)
    gt = np.stack([sc.pose_3d_gt + np.array([8.0 * (f % 50), 3.0 * (f % 70), 0.0]) + rng.normal(0, 5.0, sc.pose_3d_gt.shape)
                   for f in range(frames)])
    p2d = np.stack([np.stack([scene.project_points(c, gt[f]) + rng.normal(0, 3.0, (sc.n_points, 2)) for c in sc.cameras])
                    for f in range(frames)]).astype(dtype)
    return sc, triangulation.projection_matrices(sc.cameras), gt, p2d


def kept_views_reference(P, x2d, valid):
    """triangulate_poses on each joint's kept views only: P (V,3,4), x2d (V,J,2), valid (V,J) -> (J,4), NaN where fewer
    than two views are kept."""
    V, J = x2d.shape[:2]
    out = np.full((J, 4), np.nan)
    for j in range(J):
        keep = np.flatnonzero(valid[:, j])
        if keep.size >= 2:
            out[j] = triangulation.triangulate_poses(P[keep], x2d[keep][:, j:j + 1])[0]
    return out


def _butterfly(x):
    """Sum over the last axis (a power of two wide) in the kernel's order: stage m adds lane i ^ m to lane i."""
    W, m = x.shape[-1], 1
    while m < W:
        x = x + x[..., np.arange(W) ^ m]
        m <<= 1
    return x[..., 0]


def jacobi_dlt(P, x2d, valid=None, max_sweeps=16):
    """One frame by the arithmetic of sks_triangulate (one-sided Jacobi on the columns of the system, float64, the sums as
    butterflies over the next power of two >= V lanes): ((J,4) homogeneous joints, sweeps of the slowest joint)."""
    V, J = x2d.shape[:2]
    W = 1
    while W < V:
        W <<= 1
    eps = np.finfo(np.float64).eps
    rows = np.zeros((J, W, 2, 4))
    for v in range(V):
        rows[:, v, 0] = x2d[v, :, 0:1].astype(np.float64) * P[v, 2] - P[v, 0]
        rows[:, v, 1] = x2d[v, :, 1:2].astype(np.float64) * P[v, 2] - P[v, 1]
    if valid is not None:
        rows[:, :V][~np.asarray(valid, dtype=bool).T] = 0.0
    out, slowest = np.zeros((J, 4)), 0
    norm2 = lambda A, k: _butterfly(A[:, 0, k] * A[:, 0, k] + A[:, 1, k] * A[:, 1, k])
    for j in range(J):
        A, R = rows[j].copy(), np.eye(4)
        for sweep in range(max_sweeps):
            rotated = False
            for p in range(3):
                for q in range(p + 1, 4):
                    a, b = norm2(A, p), norm2(A, q)
                    c = _butterfly(A[:, 0, p] * A[:, 0, q] + A[:, 1, p] * A[:, 1, q])
                    if abs(c) <= eps * np.sqrt(a * b):
                        continue
                    rotated = True
                    zeta = (b - a) / (2.0 * c)
                    t = np.copysign(1.0, zeta) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    cs = 1.0 / np.sqrt(1.0 + t * t)
                    sn = cs * t
                    for M in (A, R):
                        Mp, Mq = cs * M[..., p] - sn * M[..., q], sn * M[..., p] + cs * M[..., q]
                        M[..., p], M[..., q] = Mp, Mq
            if not rotated:
                break
        slowest = max(slowest, sweep + 1)
        k = int(np.argmin([norm2(A, k) for k in range(4)]))
        out[j] = R[:, k] / R[3, k]
    return out, slowest
