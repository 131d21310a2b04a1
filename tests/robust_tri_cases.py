"""Shared by tests/test_robust_triangulate_cpu.py and tests/test_robust_triangulate_gpu.py: sequences with corrupted
detections, hand-made edge cases, and a plain numpy oracle of the two-view consensus -- written from the rule (every pair of
kept views is a hypothesis, one np.linalg.svd each), not from the kernel -- that also says where its decisions are decisive."""
import functools
import itertools

import numpy as np

from tests import tri_cases as TC

TAU = 20.0              # reject_px of the generated cases: 3 px of noise against corruptions of 80 .. 300 px
MARGIN = 1e-3           # px: a decision closer than this to its threshold is not compared
DEPTH_MARGIN = 1e-6
MAX_UNDECIDED = 0.05    # of a case's joints
# (dataset, views, frames, joints or None for all): the smallest shapes at which the kernel takes another path -- nothing to
# test (2), 4 / 8 / 16 lanes per system (3, 4, 5), more pairs than lanes (12: 66, 31: 465, 64: 2 016)
SHAPES = (("h36m", 2, 4, None), ("h36m", 3, 5, None), ("h36m", 4, 8, None), ("h36m", 5, 7, None), ("panoptic", 12, 3, None),
          ("panoptic", 31, 2, None), ("panoptic", 64, 1, 4))
SHAPE_IDS = [f"{ds}-{v}" for ds, v, _, _ in SHAPES]


def corrupt(p2d, rng):
    """Per joint, k views drawn uniformly from 0 .. (V - 2) // 2 are moved by 80 .. 300 px in a random direction:
    (detections, corrupted (N,V,J) bool)."""
    N, V, J = p2d.shape[:3]
    x, bad = p2d.copy(), np.zeros((N, V, J), dtype=bool)
    for n in range(N):
        for j in range(J):
            k = int(rng.integers(0, (V - 2) // 2 + 1))
            for v in rng.choice(V, size=k, replace=False):
                r, th = rng.uniform(80.0, 300.0), rng.uniform(0.0, 2.0 * np.pi)
                x[n, v, j] += r * np.array([np.cos(th), np.sin(th)])
                bad[n, v, j] = True
    return x, bad


@functools.lru_cache(maxsize=None)
def generated(ds, V, frames, joints, seed=5, corruption_seed=17):
    """(P (V,3,4), detections (N,V,J,2) float64, corrupted (N,V,J)) of TC.sequence with its 3 px of noise."""
    sc, P, gt, p2d = TC.sequence(ds, V, frames, seed, dtype=np.float64)
    if joints is not None:
        p2d = p2d[:, :, :joints]
    x, bad = corrupt(p2d, np.random.default_rng(corruption_seed))
    return P, x, bad


def _dlt(rows):
    Vt = np.linalg.svd(rows)[2]
    return Vt[-1] / Vt[-1, 3]


def _rows(P, xy):
    return np.stack([xy[0] * P[2] - P[0], xy[1] * P[2] - P[1]])


def consensus_of_joint(P, xy, keep, tau, m):
    """One joint by the rule: P (V,3,4), xy (V,2), keep (V,) bool -> (inliers (V,) bool, n_consensus, decisive,
    a rival set of equal count was decided by the sum)."""
    K = np.flatnonzero(keep)
    if K.size < 3:
        return keep.copy(), K.size, True, False
    hyps = []               # (count, sum, set, borderline views)
    with np.errstate(all="ignore"):
        for a, b in itertools.combinations(K, 2):
            rows = np.concatenate([_rows(P[a], xy[a]), _rows(P[b], xy[b])])
            inl, s, c, edge = np.zeros(len(keep), dtype=bool), 0.0, 0, 0
            if np.isfinite(rows).all():
                X = _dlt(rows)
                for v in K:             # (ascending: the order the sum is taken in)
                    u = P[v] @ X
                    d = u[2]
                    e = np.hypot(u[0] / d - xy[v, 0], u[1] / d - xy[v, 1])
                    edge += bool(abs(e - tau) < MARGIN or abs(d) < DEPTH_MARGIN)
                    if d > 0 and e <= tau:
                        inl[v], c, s = True, c + 1, s + e
            hyps.append((c, s, inl, edge))
    w = min(range(len(hyps)), key=lambda h: (-hyps[h][0], hyps[h][1], h))
    cw, sw, setw, edgew = hyps[w]
    decisive, tie = edgew == 0, False
    for h, (c, s, inl, edge) in enumerate(hyps):
        if h == w:
            continue
        same = np.array_equal(inl, setw) and edge == 0
        fewer = c + edge < cw
        later = edge == 0 and c == cw and s - sw >= MARGIN
        decisive &= same or fewer or later
        tie |= c == cw and not np.array_equal(inl, setw)
    return (setw if cw >= m else keep.copy()), cw, bool(decisive), bool(tie)


def oracle(P, x, valid=None, tau=TAU, m=3):
    """The rule over a sequence: P (V,3,4) or (N,V,3,4), x (N,V,J,2), valid (N,V,J) bool or None -> dict of inliers (N,V,J)
    bool, n_consensus (N,J), n_used (N,J), xyzw (N,J,4) -- the refit restated with TC.kept_views_reference --, decisive (N,J)
    and tie (N,J): an equal-count rival set lost by its larger sum."""
    N, V, J = x.shape[:3]
    keep = np.ones((N, V, J), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    out = dict(inliers=np.zeros((N, V, J), dtype=bool), n_consensus=np.zeros((N, J), dtype=np.int32),
               decisive=np.zeros((N, J), dtype=bool), tie=np.zeros((N, J), dtype=bool), xyzw=np.zeros((N, J, 4)))
    for n in range(N):
        Pn = P[n] if P.ndim == 4 else P
        for j in range(J):
            out["inliers"][n, :, j], out["n_consensus"][n, j], out["decisive"][n, j], out["tie"][n, j] = \
                consensus_of_joint(Pn, x[n, :, j], keep[n, :, j], tau, m)
        out["xyzw"][n] = _refit(Pn, x[n], out["inliers"][n])
    out["n_used"] = out["inliers"].sum(1).astype(np.int32)
    return out


def _refit(P, x, inl):
    """TC.kept_views_reference; a joint whose used views hold a NaN (a fallback over one) is NaN, which LAPACK would refuse."""
    nan = np.isnan(np.where(inl[..., None], x, 0.0)).any(axis=(0, 2))
    ref = TC.kept_views_reference(P, x, inl & ~nan[None])
    ref[nan] = np.nan
    return ref


@functools.lru_cache(maxsize=None)
def generated_oracle(ds, V, frames, joints):
    P, x, bad = generated(ds, V, frames, joints)
    return oracle(P, x)


# hand case: h36m, 4 views, 3 frames = 51 systems (no multiple of the 8 systems a wavefront packs at V = 4)
HAND = dict(nan=(0, 3), none=(0, 5), one=(0, 6), two=(0, 7), split=(1, 2), behind=(1, 8))


@functools.lru_cache(maxsize=None)
def hand():
    """(P, x (3,4,17,2), valid (3,4,17)): HAND names the (frame, joint) of a NaN detection (view 2); of joints whose `valid`
    keeps 0, 1 and exactly 2 views; of a joint with two of four views corrupted (no consensus: fallback); of a joint whose
    views 0 and 1 see the projections of a point BEHIND both of them (their hypothesis reprojects exactly, and only the depth
    test rejects it: with min_inliers = 2 the winner is (2, 3))."""
    sc, P, gt, p2d = TC.sequence("h36m", 4, 3, seed=5, dtype=np.float64)
    x, valid = p2d.copy(), np.ones(p2d.shape[:3], dtype=bool)
    f, j = HAND["nan"]
    x[f, 2, j] = np.nan
    f, j = HAND["none"]
    valid[f, :, j] = False
    f, j = HAND["one"]
    valid[f, 1:, j] = False
    f, j = HAND["two"]
    valid[f, 2:, j] = False
    f, j = HAND["split"]
    x[f, 1, j] += (200.0, 0.0)
    x[f, 3, j] += (0.0, -200.0)
    f, j = HAND["behind"]
    centre = [-np.asarray(c.R) @ np.asarray(c.T).reshape(3) for c in sc.cameras[:2]]
    X = np.append(gt[f, j] + 5.0 * ((centre[0] - gt[f, j]) + (centre[1] - gt[f, j])), 1.0)
    for v in (0, 1):
        u = P[v] @ X
        assert u[2] < 0
        x[f, v, j] = u[:2] / u[2]
    return P, x, valid


@functools.lru_cache(maxsize=None)
def hand_oracle(m):
    P, x, valid = hand()
    return oracle(P, x, valid, TAU, m)
