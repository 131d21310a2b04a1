"""Scenes with UNOBSERVED joints -- rows of the means that hold a NaN (DESIGN.md "Unobserved joints") -- shared by
tests/test_nan_joint_cpu.py (the references alone) and tests/test_nan_joint_gpu.py (the kernels).

A rasterizer case is a small H36M scene (util.make_case) in one of the launch regimes of REGIMES with the rows of one PLACEMENT
made NaN.  It comes in two forms that every test compares: `nan` (what the loops hand the kernels) and `cull` (the same rows
placed at a finite point behind every camera, `behind_every_camera`).  Only the `cull` form is ever given to the CPU oracle:
its C `(int)` of a NaN is undefined.  Host arrays only; nothing here needs a device.

The loop cases (loop_scene, loop_frames) are four frames of one 4-view scene of which one has an unobserved joint, obtained the
documented way: the joint is dropped in all views but one, so the DLT of new_scenes(None, ...) has no triangulation for it."""
import functools

import numpy as np

from skelsplat_amd import _lib
from tests import util

J = 17                                       # joints of an H36M skeleton; limb indices address the first skeleton
ARMS, LEGS = (12, 13, 15, 16), (5, 6, 2, 3)  # scene.DATASETS["h36m"]["limbs"]: (l_arm, r_arm), (l_leg, r_leg)
NO_LIMB = (0, 1, 4, 7, 8, 9, 10, 11, 14)

# name -> make_case keywords, forced path, and what the launch-regime query must answer for the shape (the compositing backward
# the regime is there for: wave-resident lists up to 64 Gaussians, lists in LDS up to 256, the binned path's tiles beyond)
REGIMES = {
    "p17": dict(kw=dict(W=96, H=80, n_views=4), binned=False, claims={"path": _lib.PATH_SMALL, "bwd": _lib.BWD_WAVE}),
    "p68": dict(kw=dict(W=128, H=96, n_views=4, n_skeletons=4, pitch=500.0), binned=False,
                claims={"path": _lib.PATH_SMALL, "bwd": _lib.BWD_GATHER}),
    "p272": dict(kw=dict(W=176, H=144, n_views=4, n_skeletons=16, pitch=400.0), binned=False,
                 claims={"path": _lib.PATH_BINNED, "bwd": _lib.BWD_TILE}),
    "p17-binned": dict(kw=dict(W=112, H=96, n_views=4), binned=True, claims={"path": _lib.PATH_BINNED, "bwd": _lib.BWD_TILE}),
    "p17-v9": dict(kw=dict(W=96, H=80, n_views=9), binned=False, claims={"path": _lib.PATH_SMALL, "bwd": _lib.BWD_WAVE}),
}


def placement(name, P):
    """(rows, coordinates made NaN, the limb pairs -- "arms" / "legs" -- the placement takes out of the limb-symmetry loss)."""
    xyz = (0, 1, 2)
    table = {
        "lowest": ((0,), xyz),                 # index 0 owns tile bookkeeping in several kernels
        "highest": ((P - 1,), xyz),
        "middle": ((P // 2,), xyz),
        "arm": ((12,), xyz),
        "leg": ((5,), xyz),
        "no-limb": ((9,), xyz),
        "same-pair": ((12, 16), xyz),          # left and right arm: two joints of the arm pair
        "y-only": ((6,), (1,)),                # one NaN coordinate makes every view coordinate NaN
        "all": (tuple(range(P)), xyz),
    }
    rows, coords = table[name]
    first = {r for r in rows if r < J}
    dropped = {n for n, idx in (("arms", ARMS), ("legs", LEGS)) if first & set(idx)}
    return rows, coords, dropped


PLACEMENTS = ("lowest", "highest", "middle", "arm", "leg", "no-limb", "same-pair", "y-only", "all")
NAMES = tuple(f"{r}-{p}" for r in REGIMES for p in PLACEMENTS)


def behind_every_camera(cams, around, margin=1000.0):
    """A finite point with view depth <= -margin in every camera: from `around`, against the mean viewing direction, as far as
    that takes.  (The ring cameras look down at the skeleton from above its head: the point is far above them.)"""
    R = [np.asarray(c.world_view_transform.cpu().numpy(), np.float64).T for c in cams]      # x_view = R[:3,:3] x + R[:3,3]
    fwd = np.stack([r[2, :3] for r in R])
    u = -fwd.sum(0)
    assert np.linalg.norm(u) > 1e-3, "the cameras' viewing directions cancel: no direction leaves all of them behind"
    u /= np.linalg.norm(u)
    L = 1000.0
    while L < 1e7:
        x = np.asarray(around, np.float64) + L * u
        z = np.array([r[2, :3] @ x + r[2, 3] for r in R])
        if z.max() <= -margin:
            return x.astype(np.float32)
        L *= 2.0
    raise AssertionError("no point behind every camera along the mean viewing direction")


class NanCase:
    """name, regime, rows / coords / dropped (placement), W H P C V, force_binned, `nan` and `cull`: two util cases that differ in
    the means of `rows` only; point: the replacement."""


def _rig(c0, name, regime, seed):
    """What tests/geometry_cases.Run reads of a case, on a util.make_case scene."""
    c0.name, c0.seed, c0.V = name, seed, len(c0.cams)
    c0.extras, c0.bg, c0.flags = True, None, 0
    c0.force_binned = REGIMES[regime]["binned"]
    c0.claims = dict(REGIMES[regime]["claims"])
    c0.gx, c0.gy = (c0.W + 15) // 16, (c0.H + 15) // 16
    return c0


def regime_of(name):
    return next(r for r in sorted(REGIMES, key=len, reverse=True) if name.startswith(r + "-") and name[len(r) + 1:] in PLACEMENTS)


@functools.lru_cache(maxsize=None)
def get(name):
    regime = regime_of(name)
    pl = name[len(regime) + 1:]
    seed = 300 + 10 * list(REGIMES).index(regime) + PLACEMENTS.index(pl)
    mk = lambda: _rig(util.make_case(seed=seed, with_dL=False, **REGIMES[regime]["kw"]), name, regime, seed)
    c = NanCase()
    c.name, c.regime, c.seed = name, regime, seed
    c.nan, c.cull = mk(), mk()
    c.W, c.H, c.P, c.C, c.V = c.nan.W, c.nan.H, c.nan.P, c.nan.C, c.nan.V
    c.force_binned = c.nan.force_binned
    c.rows, c.coords, c.dropped = placement(pl, c.P)
    c.point = behind_every_camera(c.nan.cams, c.nan.means.mean(0))
    c.nan.means = c.nan.means.copy()
    c.cull.means = c.cull.means.copy()
    for r in c.rows:
        c.nan.means[r, list(c.coords)] = np.nan
        c.cull.means[r] = c.point
    assert np.isfinite(c.cull.means).all() and int(np.isnan(c.nan.means).any(axis=1).sum()) == len(c.rows)
    return c


# ------------------------------------------------------------------------------------------------------------
# whole loops: F frames of one scene, one of them with an unobserved joint
# ------------------------------------------------------------------------------------------------------------
LOOP_W, LOOP_H, LOOP_V, LOOP_F = 160, 128, 4, 4
POISONED, MISSING = 2, 13         # frame 2 has no triangulation for joint 13 (left forearm: the arm pair leaves the loss)
KEPT_VIEW = 1


def loop_scene(device="cpu", V=LOOP_V, seed=9):
    """(scene, model factory): the scene of tests/test_frames_es_gpu.py."""
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    sc = SyntheticScene("h36m", n_views=V, seed=seed, W=LOOP_W, H=LOOP_H, ring=2500.0, fx=1145.0 * (LOOP_W / 1000) * 1.5,
                        device=device)

    def model(dev):
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9,
                                                scaling_modifier=1.0, device=dev)
        gm.training_setup()
        return gm
    return sc, model


def loop_frames(sc, n=LOOP_F, rng_seed=21):
    """(detections (n,V,J,2) float32, drop masks (n,V,J) bool with MISSING dropped in every view of frame POISONED but
    KEPT_VIEW, the same masks with that frame clean): frame f's detections carry f x 1.5 px of noise."""
    rng = np.random.default_rng(rng_seed)
    base = np.asarray(sc.poses_2d, np.float32)
    p2d = np.stack([base + rng.normal(0, 1.5 * f, base.shape) for f in range(n)]).astype(np.float32)
    clean = np.zeros((n,) + base.shape[:2], bool)
    drop = clean.copy()
    drop[POISONED, :, MISSING] = True
    drop[POISONED, KEPT_VIEW, MISSING] = False
    return p2d, drop, clean
