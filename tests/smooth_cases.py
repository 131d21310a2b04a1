"""Seeded cases for the temporal fit (sks_smooth_sequence; the definition: include/skelsplat_hip.h), small enough for the op-by-op
Python restatement of tests/smooth_ref.py: positions of a few thousand mm on a slow trajectory plus noise drawn from each tap's
own covariance, J in {1, 15, 17, 19}, N around the seams of the kernel's tiles -- the tile length T comes from the library's own
host-only answer, sks_smooth_launch, never from a constant here.

A case is a dict: name, xyz (N,J,3) float32, cov6 (N,J,6) float32 / weights (N,J) float32 / valid (N,J) bool / groups (N,) int32 or
None, h, d, taper, floor, and `expect`: what the case is there to reach (checked by tests/test_smooth_cpu.py).  Covariances are
clearly positive definite (anisotropy up to 1e4) or clearly not (a NaN entry, the zero matrix, a negative diagonal): nothing
borderline, where the header's pivot rule and a library's eigenvalues could disagree."""
import functools

import numpy as np

from skelsplat_amd import _lib


def tile(J, h, N=1):
    return _lib.smooth_launch(N, J, h)["tile"]


def covariances(rng, N, J, big=(1.0, 1e3), ratios=(1e2, 1e4)):
    """(N,J,6) float32: random orientation, largest eigenvalue log-uniform in `big` mm^2, the other two smaller by log-uniform
    factors of up to ratios[0] and ratios[1]; and the float64 matrices they were made from."""
    Q = np.linalg.qr(rng.normal(size=(N, J, 3, 3)))[0]
    l1 = np.exp(rng.uniform(np.log(big[0]), np.log(big[1]), (N, J)))
    lam = np.stack([l1, l1 / np.exp(rng.uniform(0, np.log(ratios[0]), (N, J))), l1 / np.exp(rng.uniform(0, np.log(ratios[1]), (N, J)))], -1)
    C = np.einsum("njab,njb,njcb->njac", Q, lam, Q)
    return C[..., [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]].astype(np.float32), C


def trajectory(rng, N, J, C=None, noise=5.0):
    """(N,J,3) float32: per joint a place within a few thousand mm, a slow sinusoid per coordinate, and noise -- drawn from each
    tap's covariance C (N,J,3,3), or isotropic with `noise` mm."""
    f = np.arange(N)[:, None, None]
    base = rng.uniform(-3000.0, 3000.0, (1, J, 3))
    amp, freq, phase = rng.uniform(20, 200, (1, J, 3)), rng.uniform(0.02, 0.15, (1, J, 3)), rng.uniform(0, 6.28, (1, J, 3))
    x = base + amp * np.sin(freq * f + phase)
    if C is None:
        return (x + rng.normal(scale=noise, size=x.shape)).astype(np.float32)
    L = np.linalg.cholesky(C)
    return (x + np.einsum("njab,njb->nja", L, rng.normal(size=x.shape))).astype(np.float32)


def _case(name, seed, N, J, h, d, taper, cov=True, floor=0.0, expect=(), **cov_kw):
    rng = np.random.default_rng(seed)
    cov6, C = covariances(rng, N, J, **cov_kw) if cov else (None, None)
    return dict(name=name, xyz=trajectory(rng, N, J, C), cov6=cov6, weights=None, valid=None, groups=None, h=h, d=d, taper=taper,
                floor=floor, expect=set(expect), rng=rng)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  (Built once: the references of tests/smooth_ref.py are cached per name next to them.)"""
    out = []
    # degrees x tapers; J = 19
    for d in (0, 1, 2):
        for taper in ("box", "tricube"):
            out.append(_case(f"d{d}_{taper}", 10 + d, 12, 19, 3, d, taper))
    # no covariances (Lambda = I), and h = 1
    out.append(_case("unit_weights", 20, 14, 15, 2, 2, "box", cov=False))
    out.append(_case("h1", 21, 9, 15, 1, 1, "tricube"))
    # h = 32: one joint across a tile's halo, and 17 joints, where the stage splits the joints into runs (mild anisotropy: t^4
    # reaches 1e6 and the normal matrix's condition number is to stay below 1e9)
    out.append(_case("h32_one_joint", 22, 70, 1, 32, 2, "tricube", ratios=(3.0, 10.0)))
    out.append(_case("h32_joint_runs", 23, 20, 17, 32, 2, "box", ratios=(3.0, 10.0)))
    # short sequences: N = 1, 2 and N < 2h + 1
    for N in (1, 2, 5):
        out.append(_case(f"short_N{N}", 30 + N, N, 15, 4, 2, "tricube", expect={"reduced"} if N < 3 else ()))
    # the tile seams, J = 17 and (256 frames a tile) J = 1
    T = tile(17, 2)
    for N in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
        out.append(_case(f"seam_N{N}", 40 + N, N, 17, 2, 2, "tricube"))
    T1 = tile(1, 1)
    out.append(_case(f"seam_one_joint_N{2 * T1 + 1}", 50, 2 * T1 + 1, 1, 1, 1, "box"))
    # group boundaries inside a tile, on a seam and one frame behind one
    c = _case("groups", 60, 2 * T + 4, 17, 2, 2, "tricube")
    c["groups"] = np.digitize(np.arange(c["xyz"].shape[0]), [T // 2, T, 2 * T + 1]).astype(np.int32)
    out.append(c)
    # a group of one frame and a group of two under d = 2: the degree comes down to 0 and to 1
    c = _case("degree_reduction", 61, 8, 15, 3, 2, "box", expect={"reduced"})
    c["groups"] = np.array([0, 0, 0, 1, 2, 2, 3, 3], dtype=np.int32)
    out.append(c)
    # valid: a gap shorter than the window is filled, a gap longer than it stays empty in its middle
    c = _case("gaps", 62, 24, 15, 3, 2, "tricube", expect={"filled", "empty"})
    c["valid"] = np.ones((24, 15), dtype=bool)
    c["valid"][8:11, 1] = False
    c["valid"][5:18, 2] = False
    out.append(c)
    # a NaN joint row (an unobserved joint) with finite neighbours; an inf coordinate
    c = _case("nan_rows", 63, 12, 17, 2, 2, "tricube", expect={"filled"})
    c["xyz"][5, 2] = np.nan
    c["xyz"][7, 3, 1] = np.nan
    c["xyz"][0, 4, 0] = np.inf
    out.append(c)
    # covariances that are clearly bad: a NaN entry, the zero matrix, a negative diagonal
    c = _case("bad_covariances", 64, 12, 15, 2, 2, "tricube", expect={"filled"})
    c["cov6"][3, 0, 4] = np.nan
    c["cov6"][4, 1] = 0.0
    c["cov6"][5, 2, 3] = -4.0
    c["cov6"][6, 3, 0] = -1.0
    c["bad"] = [(3, 0), (4, 1), (5, 2), (6, 3)]
    out.append(c)
    # a floor: the zero matrix becomes floor x I and is used
    c = _case("cov_floor", 65, 12, 15, 2, 2, "tricube", floor=4.0)
    c["cov6"][4, 1] = 0.0
    out.append(c)
    # weights, with zeros, a negative and a NaN
    c = _case("weights", 66, 14, 15, 2, 2, "box", expect={"filled"})
    c["weights"] = c["rng"].uniform(0.25, 4.0, (14, 15)).astype(np.float32)
    c["weights"][3:5, 0] = 0.0
    c["weights"][6, 1] = -1.0
    c["weights"][7, 2] = np.nan
    out.append(c)
    # everything at once
    c = _case("all_inputs", 67, T + 3, 19, 4, 2, "tricube", floor=0.5, expect={"filled"})
    n = c["xyz"].shape[0]
    c["weights"] = c["rng"].uniform(0.5, 2.0, (n, 19)).astype(np.float32)
    c["valid"] = c["rng"].uniform(size=(n, 19)) > 0.15
    c["groups"] = (np.arange(n) >= n // 2).astype(np.int32)
    out.append(c)
    for c in out:
        del c["rng"]
    return {c["name"]: c for c in out}


NAMES = tuple(cases())


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """tests/smooth_ref.py's fit_lstsq ("a") or fit_ldl ("b") of a case, computed once and shared; leave it unchanged."""
    from tests import smooth_ref
    return (smooth_ref.fit_lstsq if kind == "a" else smooth_ref.fit_ldl)(cases()[name])


def ulp32(x):
    """The float32 spacing at |x| (float64 array in, float64 out)."""
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def e64():
    """E64: the largest difference between references (a) and (b) over all cases -- positions in float32 ulps of the result,
    velocity in mm per frame and covariance in mm^2, absolute.  It bounds what float64 leaves of the fit before the last rounding."""
    worst = dict(joints=0.0, velocity=0.0, cov6=0.0)
    for name in NAMES:
        a, b = reference(name, "a"), reference(name, "b")
        with np.errstate(invalid="ignore"):
            worst["joints"] = max(worst["joints"], float(np.nanmax(np.abs(a["joints"] - b["joints"]) / ulp32(a["joints"]), initial=0.0)))
            for key in ("velocity", "cov6"):
                worst[key] = max(worst[key], float(np.nanmax(np.abs(a[key] - b[key]), initial=0.0)))
    return worst


def accel_case(N, J=17, seed=0):
    """xyz, gt (N,J,3) float32 and groups (N,) int32 for sks_eval_accel: NaN joints, a NaN in the ground truth alone, three groups
    of which id 1 is empty and id 7 lies outside the range."""
    rng = np.random.default_rng(1000 + N + seed)
    gt = trajectory(rng, N, J, noise=0.0)
    xyz = (gt + rng.normal(scale=4.0, size=gt.shape)).astype(np.float32)
    if N > 4:
        xyz[rng.uniform(size=(N, J)) < 0.05] = np.nan
        gt[rng.uniform(size=(N, J)) < 0.03] = np.nan
        xyz[:, 5] = np.nan                            # a joint that never enters
    groups = np.sort(rng.integers(0, 3, N)).astype(np.int32)
    groups[groups == 1] = 7
    return xyz, gt, groups
