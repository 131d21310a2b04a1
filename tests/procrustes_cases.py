"""The seeded case table the CPU and GPU tests of the aligned errors share (csrc/sks_align.hip): float32 poses of every joint
count at which the kernel's loops change their trip count, crossed with the kinds of pose at which a 3x3 fit goes wrong.  numpy
only; the same call gives the same bytes everywhere (PCG64 streams keyed by joint count and kind)."""
import numpy as np

# 65: lane 0 makes a second trip; 130: lanes 0 and 1 a third
JOINTS = (1, 2, 3, 4, 17, 19, 64, 65, 130)
KINDS = ("noise", "similarity", "mirrored", "planar", "collinear_gt", "collinear_pred", "collinear_both", "coincident",
         "coincident_gt", "far", "tiny", "mask_0", "mask_1", "mask_2", "mask_3", "mask_all_but_one", "mask_no_root", "nan_valid",
         "nan_masked")
# kinds with a NaN in a valid joint: every output of the frame is NaN
POISONED = ("nan_valid",)


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _pose(rng, P, spread=1000.0, centre=2000.0):
    return rng.uniform(-centre, centre, 3) + rng.uniform(-spread, spread, (P, 3))


def _line(rng, P, spread=1000.0):
    d = rng.normal(size=3)
    return rng.uniform(-2000.0, 2000.0, 3) + rng.uniform(-spread, spread, (P, 1)) * (d / np.linalg.norm(d))


def make_case(P, kind):
    """-> pred (P,3) float32, gt (P,3) float32, valid (P,) bool."""
    rng = np.random.default_rng([P, KINDS.index(kind), 20240229])
    gt = _pose(rng, P)
    pred = gt + rng.normal(0.0, 40.0, (P, 3))
    valid = np.ones(P, dtype=bool)
    if kind == "similarity":
        pred = _pose(rng, P)
        gt = rng.uniform(0.5, 2.0) * pred @ _rotation(rng).T + rng.uniform(-3000.0, 3000.0, 3)
    elif kind == "mirrored":
        pred = gt * np.array([-1.0, 1.0, 1.0]) + rng.normal(0.0, 40.0, (P, 3))
    elif kind == "planar":
        gt[:, 2] = gt[0, 2]
        pred[:, 2] = pred[0, 2]
    elif kind == "collinear_gt":
        gt = _line(rng, P)
    elif kind == "collinear_pred":
        pred = _line(rng, P)
    elif kind == "collinear_both":
        gt, pred = _line(rng, P), _line(rng, P)
    elif kind == "coincident":
        gt, pred = np.repeat(gt[:1], P, axis=0), np.repeat(pred[:1], P, axis=0)
    elif kind == "coincident_gt":
        gt = np.repeat(gt[:1], P, axis=0)
    elif kind == "far":
        d = rng.normal(size=3)
        gt = 5000.0 * d / np.linalg.norm(d) + rng.uniform(-10.0, 10.0, (P, 3))
        pred = gt + rng.normal(0.0, 1.0, (P, 3))
    elif kind == "tiny":
        gt = rng.uniform(-1e-3, 1e-3, (P, 3))
        pred = gt + rng.normal(0.0, 1e-4, (P, 3))
    elif kind.startswith("mask_") and kind[5:].isdigit():       # the root and k - 1 others stay
        k = min(int(kind[5:]), P)
        valid[:] = False
        if k:
            valid[0] = True
            valid[1 + rng.permutation(P - 1)[:k - 1]] = True
    elif kind == "mask_all_but_one":
        valid[P - 1] = False
    elif kind == "mask_no_root":
        valid[0] = False
    elif kind == "nan_valid":
        pred[P // 2, 1] = np.nan
    elif kind == "nan_masked":
        valid[P - 1] = False
        pred[P - 1, 2] = np.nan
    return pred.astype(np.float32), gt.astype(np.float32), valid


def batch(P):
    """Every kind at one joint count as one batch: pred, gt (K,P,3) float32, valid (K,P) bool, in the order of KINDS."""
    cases = [make_case(P, kind) for kind in KINDS]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])


# ------------------------------------------------------------------------------------------------ sequences
SEQUENCE_FRAMES = (1, 3, 257, 513)      # 257: thread 0 of the reduction makes a second trip
SEQUENCE_GROUPS = (0, 1, 15, 64)
SEQUENCE_JOINTS = 17


def make_sequence(N, G):
    """-> pred, gt (N,17,3) float32, valid (N,17) bool (a tenth of the joints masked, never the root; frame N - 1 has none
    valid when N > 1), groups (N,) int32 in [0, G) that leave group G - 1 without frames when G > 1 (zeros when G == 0)."""
    P = SEQUENCE_JOINTS
    rng = np.random.default_rng([N, 977])           # (the poses depend on N alone: one reference per N serves every G)
    gt = rng.uniform(-2000.0, 2000.0, (N, 1, 3)) + rng.uniform(-1000.0, 1000.0, (N, P, 3))
    pred = gt + rng.normal(0.0, 40.0, (N, P, 3))
    valid = rng.uniform(size=(N, P)) > 0.1
    valid[:, 0] = True
    if N > 1:
        valid[N - 1] = False
    rng = np.random.default_rng([N, G, 978])
    groups = rng.integers(0, max(G - 1, 1), N).astype(np.int32) if G else np.zeros(N, dtype=np.int32)
    return pred.astype(np.float32), gt.astype(np.float32), valid, groups
