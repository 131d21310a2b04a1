"""Seeded cases for the constant-limb-length kernels (sks_bone_measure / sks_bone_lengths / sks_bone_project; the definitions:
include/skelsplat_hip.h), each a few hundred joints at most -- the long ones (N = 257, 1025: a group longer than a workgroup of
the select, several histogram trips) have three joints -- so that the op-by-op restatement of tests/bones_ref.py runs them in about
a second.

A case is a dict: name, xyz (N,J,3) float32, bones ((parent, child), ..), cov6 (N,J,6) float32 / valid (N,J) bool / groups (N,)
int32 or None, G, max_sigma (mm or None), target: None (project onto the case's own median lengths) or (G,B) float32, floor,
iters, tol.  Perturbations stay within what a numpy prototype of the trip found to converge: at most 30 mm, std ratio at most 10."""
import functools

import numpy as np

from skelsplat_amd.scene import DATASETS, skeleton_template

CHAIN3 = ((0, 1), (1, 2))
LONG_N = (1, 2, 3, 4, 5, 64, 65, 257, 1025)


def covariances(rng, shape, big, ratio):
    """Needles: std `big` mm along a random direction, big / ratio across it.  (.., 6) float32 and the float64 matrices."""
    v = rng.normal(size=shape + (3,))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    small = big / ratio
    C = small ** 2 * np.eye(3) + (big ** 2 - small ** 2) * v[..., :, None] * v[..., None, :]
    return C[..., [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]].astype(np.float32), C


def template_lengths(dataset):
    t, b = skeleton_template(dataset), np.asarray(DATASETS[dataset]["bones"])
    return np.linalg.norm(t[b[:, 1]] - t[b[:, 0]], axis=-1).astype(np.float32)[None]


def _case(name, xyz, bones, cov6=None, valid=None, groups=None, G=1, max_sigma=None, target=None, floor=0.0, iters=16, tol=1e-3):
    return dict(name=name, xyz=np.ascontiguousarray(xyz, dtype=np.float32), bones=tuple((int(p), int(c)) for p, c in bones),
                cov6=cov6, valid=valid, groups=None if groups is None else np.asarray(groups, dtype=np.int32), G=G,
                max_sigma=max_sigma, target=target, floor=floor, iters=iters, tol=tol)


def _poses(seed, dataset, N, noise, ratio=None):
    """Template poses, each somewhere in a room, perturbed by `noise` mm: isotropic, or drawn from needle covariances."""
    rng = np.random.default_rng(seed)
    t = skeleton_template(dataset)
    J = t.shape[0]
    x = t[None] + rng.uniform(-2000.0, 2000.0, (N, 1, 3))
    if ratio is None:
        cov6 = np.zeros((N, J, 6), dtype=np.float32)
        cov6[..., [0, 3, 5]] = noise ** 2
        return x + rng.normal(scale=noise, size=x.shape), cov6
    cov6, C = covariances(rng, (N, J), noise, ratio)
    return x + np.einsum("njab,njb->nja", np.linalg.cholesky(C), rng.normal(size=x.shape)), cov6


def _chain(seed, N, J, step=100.0, noise=5.0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(J - 1, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    base = np.concatenate([np.zeros((1, 3)), np.cumsum(step * d, axis=0)])
    return base[None] + rng.uniform(-500, 500, (N, 1, 3)) + rng.normal(scale=noise, size=(N, J, 3))


def _one_bone(lengths):
    """A bone from the origin along x whose length in frame f is exactly the float32 lengths[f]."""
    l = np.asarray(lengths, dtype=np.float32)
    xyz = np.zeros((l.size, 2, 3), dtype=np.float32)
    xyz[:, 1, 0] = l
    return xyz


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for N in LONG_N:
        out.append(_case(f"chain3_N{N}", _chain(100 + N, N, 3), CHAIN3))
    for ds in ("h36m", "panoptic", "occlusion-person"):
        x, cov6 = _poses(200 + len(ds), ds, 5, 10.0)
        out.append(_case(f"{ds}_isotropic", x, DATASETS[ds]["bones"], cov6=cov6, target=template_lengths(ds)))
        x, cov6 = _poses(210 + len(ds), ds, 5, 30.0, ratio=10.0)
        out.append(_case(f"{ds}_needles", x, DATASETS[ds]["bones"], cov6=cov6, target=template_lengths(ds)))
    x, _ = _poses(220, "h36m", 4, 20.0)
    out.append(_case("h36m_unit_sigma", x, DATASETS["h36m"]["bones"], target=template_lengths("h36m")))
    out.append(_case("h36m_own_medians", _poses(221, "h36m", 9, 8.0)[0], DATASETS["h36m"]["bones"]))
    out.append(_case("chain32", _chain(230, 3, 32), tuple((j, j + 1) for j in range(31))))
    out.append(_case("forest", _chain(231, 4, 7), ((0, 1), (1, 2), (3, 4), (5, 4))))           # joint 6: no bone
    out.append(_case("single_bone", _chain(232, 5, 2), ((1, 0),)))
    out.append(_case("ties", _one_bone([3, 3, 5, 5, 5, 7, 3, 5]), ((0, 1),)))
    rng = np.random.default_rng(233)
    low = (np.uint32(0x43000000) + rng.permutation(40).astype(np.uint32)).view(np.float32)
    out.append(_case("lowest_byte", _one_bone(low), ((0, 1),)))
    high = ((rng.permutation(np.arange(0x3c, 0x47)).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00345678)).view(np.float32)
    out.append(_case("highest_byte", _one_bone(high), ((0, 1),)))
    # groups: interleaved in frame order, one with every frame NaN, an id outside the range; and the most groups there can be
    x = _chain(240, 20, 3)
    g = np.arange(20) % 3
    x[g == 1] = np.nan
    g[6] = 5
    out.append(_case("groups_3", x, CHAIN3, groups=g, G=3))
    out.append(_case("groups_max", _chain(241, 300, 2), ((0, 1),), groups=(np.arange(300) * 7) % 256, G=256))
    # degenerate rows: a NaN joint, a masked joint, covariances that are not positive definite or not finite, coincident joints
    x, cov6 = _poses(250, "h36m", 6, 10.0, ratio=3.0)
    valid = np.ones(x.shape[:2], dtype=bool)
    x[0, 13] = np.nan
    x[1, 2, 1] = np.nan
    valid[2, 8] = False
    cov6[3, 5] = 0.0
    cov6[3, 15, 3] = -4.0
    cov6[4, 11, 4] = np.nan
    x[5, 6] = x[5, 5]
    out.append(_case("degenerate_rows", x, DATASETS["h36m"]["bones"], cov6=cov6, valid=valid, target=template_lengths("h36m")))
    # a floor makes the zero covariance usable again
    out.append(_case("cov_floor", x, DATASETS["h36m"]["bones"], cov6=cov6, valid=valid, target=template_lengths("h36m"), floor=4.0))
    # targets that are NaN, zero and negative
    x, cov6 = _poses(251, "occlusion-person", 3, 10.0)
    t = template_lengths("occlusion-person").copy()
    t[0, 3], t[0, 7], t[0, 9] = np.nan, 0.0, -50.0
    out.append(_case("bad_targets", x, DATASETS["occlusion-person"]["bones"], cov6=cov6, target=t))
    # the gate on the length's standard deviation: some frames out, all frames out
    x, cov6 = _poses(252, "h36m", 12, 10.0, ratio=10.0)
    out.append(_case("gate_some", x, DATASETS["h36m"]["bones"], cov6=cov6, max_sigma=8.0))
    out.append(_case("gate_all", x, DATASETS["h36m"]["bones"], cov6=cov6, max_sigma=0.01))
    # a trip limit that ends frames before they converge
    x, cov6 = _poses(253, "h36m", 3, 30.0, ratio=10.0)
    out.append(_case("two_trips", x, DATASETS["h36m"]["bones"], cov6=cov6, target=template_lengths("h36m"), iters=2))
    return {c["name"]: c for c in out}


NAMES = tuple(cases())
# the cases whose frames are allowed to stop short of tol_mm: the trip limit is what they are about
UNCONVERGED = ("two_trips",)


@functools.lru_cache(maxsize=None)
def reference(name):
    """tests/bones_ref.py's measure, lengths and projection of a case, computed once and shared; leave it unchanged.  A case
    without `target` is projected onto its own median lengths."""
    from tests import bones_ref as REF
    c = cases()[name]
    measured = REF.measure(c["xyz"], c["bones"], c["cov6"], c["valid"], c["max_sigma"])
    length, mad, n_used = REF.lengths(measured, c["groups"], c["G"])
    target = length if c["target"] is None else c["target"]
    joints, residual, n_trips, n_active = REF.project(c["xyz"], c["bones"], target, c["cov6"], c["valid"], c["groups"], c["floor"],
                                                      c["iters"], c["tol"])
    return dict(measured=measured, length=length, mad=mad, n_used=n_used, target=target, joints=joints, residual=residual,
                n_trips=n_trips, n_active=n_active)
