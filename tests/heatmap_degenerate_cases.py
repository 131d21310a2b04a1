"""TEST INFRASTRUCTURE -- the cases of tests/test_heatmap_degenerate_{cpu,gpu}.py (DESIGN.md "Degenerate footprints"), CPU only:
inputs that put the heat-map factors' two variances at the truncation-radius cap, across the sign change of lambda2, and at
non-finite and huge values, with the rule that classifies a plane and the fp64 definition a kept plane is held to.

Nothing here loads the HIP library.  Scales are found by bisection on the twin's own fp32 lambdas (oracle/heatmaps_ref.py), as
tests/test_loop_tail_gpu._solve_scales does; the GPU tests take each plane's class from the KERNEL's lambdas (sks_view_footprints)
and this module's rule, and tests/test_heatmap_degenerate_cpu.py shows on the twin that the cases reach what they claim.
"""
import functools
import math

import numpy as np
import torch

from oracle import heatmaps_ref as HR
from tests import tail_ref

R_MAX = HR.HEATMAP_MAX_RADIUS
SHAPES = [(16, 16, False), (40, 24, False), (130, 1, False), (40, 24, True)]
SHAPE_IDS = ["16x16", "40x24", "130x1", "40x24+36x20"]
MODIFIER = 1.3
DEN0 = np.float32(1e-8)
TRIP_CAP = 1 << 20          # per-thread exp of any plane a GPU case draws (keeps the GPU tests short; not a measurement)
LONG = (1.0, 1.0 / 32, 1.0 / 32)      # a Gaussian 32 x longer along world x: sigma1 = 32 sigma2 in either view of the scenes below


# ------------------------------------------------------------------------------------------------ the rule and the definition
def radius_of(lam):
    """floor(4.0 * (double)sqrtf(lambda) + 0.5) as the kernel forms it (fp32 root, widened); NaN where lambda is not positive."""
    lam = np.asarray(lam, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.floor(4.0 * np.sqrt(lam).astype(np.float64) + 0.5)


def draws(lam, p2d):
    """The contract: lam (V,J,2) fp32 lambdas, p2d (V,J,2) detections -> (V,J) bool, True where the plane draws an impulse."""
    lam = np.asarray(lam, dtype=np.float32)
    ok = np.isfinite(lam).all(-1) & np.isfinite(np.asarray(p2d, dtype=np.float32)).all(-1)
    with np.errstate(invalid="ignore"):
        ok &= (lam[..., 0] > 0) & (lam[..., 1] > 0)
        ok &= (radius_of(lam[..., 0]) <= R_MAX) & (radius_of(lam[..., 1]) <= R_MAX)
    return ok


@functools.lru_cache(maxsize=None)
def _impulse(n, p, sigma):
    return tail_ref.impulse_ref(n, p, sigma)[0]


def trips(n, radius):
    """Per-thread exp count of impulse_response on an axis of n samples (the bound in k_heatmap_factors' comment, exactly):
    normalisation trips + ceil(n / 256) * (3 + 4 * bounces)."""
    radius = int(radius)
    return (radius + 255) // 256 + ((n + 255) // 256) * (3 + 4 * ((radius + n - 1) // (2 * n)))


def expected(lam, p2d, sizes):
    """What the contract asks of sks_heatmap_factors for lambdas `lam` (V,J,2) fp32 -- the kernel's own, or the twin's -- and
    detections p2d (V,J,2): (draw (V,J) bool, rows, cols) with rows[v][j] (h_v,) / cols[v][j] (w_v,) float64 by the fp64 definition
    (tests/tail_ref.impulse_ref, x 255 for rows) for a plane that draws, None for one that does not.  sizes: per view (w, h)."""
    lam = np.asarray(lam, dtype=np.float32)
    p2d = np.asarray(p2d, dtype=np.float32)
    draw = draws(lam, p2d)
    rows, cols = [], []
    for v, (w, h) in enumerate(sizes):
        rows.append([])
        cols.append([])
        for j in range(lam.shape[1]):
            if not draw[v, j]:
                rows[v].append(None)
                cols[v].append(None)
                continue
            xs, ys = min(max(int(p2d[v, j, 0]), 0), w - 1), min(max(int(p2d[v, j, 1]), 0), h - 1)
            s1, s2 = float(np.sqrt(lam[v, j, 0])), float(np.sqrt(lam[v, j, 1]))
            assert trips(h, radius_of(lam[v, j, 0])) <= TRIP_CAP and trips(w, radius_of(lam[v, j, 1])) <= TRIP_CAP
            rows[v].append(255.0 * _impulse(h, ys, s1))
            cols[v].append(_impulse(w, xs, s2))
    return draw, rows, cols


def hold(what, row, col, cmin, den, lam, p2d, sizes, assert_close):
    """row (V,J,H), col (V,J,W), cmin, den (V,J): fp32 torch tensors on the CPU whose buffers started as NaN, against `expected`:
    kept planes at rtol 2e-5 / atol_scale 1e-6 of the definition, no-impulse planes bit for bit (+0, cmin 0, den 1e-8f), nothing
    written beyond a view's own size, every written value finite, cmin / den bit for bit as functions of the rows written.
    Returns draw (V,J)."""
    draw, rows, cols = expected(lam, p2d, sizes)
    row, col, cmin, den = (t.detach().cpu() for t in (row, col, cmin, den))
    for v, (w, h) in enumerate(sizes):
        r_, c_ = row[v, :, :h], col[v, :, :w]
        assert bool(torch.isfinite(r_).all()) and bool(torch.isfinite(c_).all()), f"{what} view {v}: a non-finite factor"
        assert bool(torch.isfinite(cmin[v]).all()) and bool(torch.isfinite(den[v]).all()), f"{what} view {v}: non-finite cmin / den"
        assert bool(torch.isnan(row[v, :, h:]).all()) and bool(torch.isnan(col[v, :, w:]).all()), f"{what} view {v}: wrote beyond its size"
        for j in range(row.shape[1]):
            if draw[v, j]:
                assert_close(f"{what} row view {v} joint {j}", r_[j], rows[v][j], rtol=2e-5, atol_scale=1e-6)
                assert_close(f"{what} col view {v} joint {j}", c_[j], cols[v][j], rtol=2e-5, atol_scale=1e-6)
            else:
                for name, t in (("row", r_[j]), ("col", c_[j])):
                    assert not t.any() and not torch.signbit(t).any(), f"{what} view {v} joint {j}: {name} of a no-impulse plane is not +0"
                assert float(cmin[v, j]) == 0.0 and not bool(torch.signbit(cmin[v, j])), (what, v, j, float(cmin[v, j]))
                assert np.float32(den[v, j].item()) == DEN0, (what, v, j, float(den[v, j]))
        lo = r_.amin(dim=1) * c_.amin(dim=1)
        assert torch.equal(cmin[v], lo) and torch.equal(den[v], (r_.amax(dim=1) * c_.amax(dim=1) - lo) + 1e-8), f"{what} view {v}: cmin / den"
    return draw


# ------------------------------------------------------------------------------------------------ scenes and the twin's lambdas
@functools.lru_cache(maxsize=None)
def scene(W, H, mixed):
    """(scene, cameras, per-view (w, h)): the scene of test_heatmap_factors_at_any_radius, V = 2; `mixed`: view 1 is 4 px smaller."""
    from skelsplat_amd.scene import SyntheticScene
    sc = SyntheticScene("h36m", n_views=2, seed=4, W=W, H=H, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5)
    cams = list(sc.cameras)
    if mixed:
        small = SyntheticScene("h36m", n_views=2, seed=4, W=W - 4, H=H - 4, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5)
        cams[1] = small.cameras[1]
    return sc, cams, [(int(c.image_width), int(c.image_height)) for c in cams]


def twin_lambdas(cams, means, scales, rot, modifier=MODIFIER):
    """(V,J,2) fp32 numpy: the twin's lambda1, lambda2 of every joint in every view, each view at its own size."""
    cov = HR.covariance_from_scaling_rotation(scales, rot, modifier)
    out = []
    with np.errstate(all="ignore"):
        for cam in cams:
            l1, l2 = HR.ewa_lambdas_views(means, cov, [cam], int(cam.image_width), int(cam.image_height))
            out.append(torch.stack([l1[0], l2[0]], dim=-1))
    return torch.stack(out).numpy()


def _ident(J):
    return torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(J, 1)


def _next(x, k):
    """The fp32 k steps from positive fp32 x (k of either sign)."""
    return (np.asarray(x, dtype=np.float32).view(np.int32) + np.int32(k)).view(np.float32)


def solve_scales(cam, means, shapes, targets, modifier=MODIFIER):
    """Per joint a factor s such that, with scales s * shapes[j], floor(4 sigma + 0.5) of the targeted axis in `cam` is the wanted
    radius with 4 sigma + 0.5 in the middle of its integer interval: bisection on the twin's fp32 lambdas.  targets: [(axis, radius)];
    axis 2: the mean of the two lambdas (what both are when the root is absorbed)."""
    J = means.shape[0]
    shapes = torch.tensor(shapes, dtype=torch.float32)
    lo, hi = torch.full((J,), 1e-3), torch.full((J,), 1e9)
    want = torch.tensor([r / 4.0 if r else 0.0625 for _, r in targets], dtype=torch.float32)
    axis = torch.tensor([a for a, _ in targets])
    w, h = int(cam.image_width), int(cam.image_height)
    for _ in range(80):
        mid = torch.sqrt(lo * hi)
        cov = HR.covariance_from_scaling_rotation(mid[:, None] * shapes, _ident(J), modifier)
        l1, l2 = HR.ewa_lambdas_views(means, cov, [cam], w, h)
        sig = torch.where(axis == 0, l1[0], torch.where(axis == 1, l2[0], 0.5 * (l1[0] + l2[0]))).clamp_min(0).sqrt()
        small = sig < want
        lo, hi = torch.where(small, mid, lo), torch.where(small, hi, mid)
    return (torch.sqrt(lo * hi)[:, None] * shapes).contiguous()


def detections(V, J, W, H):
    """Detections at 0, at n - 1 and in the middle, by joint."""
    p2d = torch.zeros((V, J, 2))
    for j in range(J):
        p2d[:, j] = torch.tensor([[0.3, 0.7], [W - 0.5, H - 0.5], [W / 2.0, H / 2.0]][j % 3])
    return p2d


class Case:
    """V, J, W, H, cams, sizes, means, scales, rot, p2d (torch fp32), modifier, lam (the twin's lambdas), notes."""


def _case(W, H, mixed, means, scales, rot, p2d, modifier=MODIFIER, **notes):
    c = Case()
    sc, c.cams, c.sizes = scene(W, H, mixed)
    c.W, c.H, c.mixed, c.V, c.J = W, H, mixed, 2, means.shape[0]
    c.means, c.scales, c.rot, c.p2d, c.modifier = means.contiguous(), scales.contiguous(), rot.contiguous(), p2d.contiguous(), modifier
    c.lam = twin_lambdas(c.cams, c.means, c.scales, c.rot, modifier)
    c.__dict__.update(notes)
    return c


# ------------------------------------------------------------------------------------------------ 1: at the cap
CAP_RADII = (R_MAX - 1, R_MAX, R_MAX + 1, 2 * R_MAX, 16 * R_MAX)


@functools.lru_cache(maxsize=None)
def cap_case(W, H, mixed):
    """17 joints.  0-4: a LONG Gaussian, lambda1 (rows) at the radii CAP_RADII, lambda2's radius 32 x smaller -- axis 0
    alone crosses the cap.  5-9: an isotropic Gaussian, for which the reference's transcription gives lambda1 ~ lambda2, with
    lambda2 (columns) at CAP_RADII in view 0.  lambda1 >= lambda2 always, so axis 1 is never ALONE beyond the cap and its kept
    planes need lambda1's radius <= R_MAX too.  At these magnitudes mid^2 - det is rounding noise: at most fp32 scales the root
    is absorbed and lambda1 == lambda2, at the others the radii are 64 or more apart.  Joints 5 and 6 are searched among the
    neighbouring fp32 scales for radius1 == radius2 == R_MAX - 1 and == R_MAX; joints 7-9 have both radii beyond the cap.
    The radii are solved in view 0, those of 16 R_MAX (joints 4 and 9) in the view that sees the joint larger (`top_view`): no plane of the case has a radius beyond 16 R_MAX, so a kernel without the cap still makes a short launch of it
    (at most 2^23 exp per thread, on the one-sample axis of 130x1).  10-16: ordinary radii (1 .. about 2 n).  Detections at 0,
    n - 1, the middle."""
    sc, cams, sizes = scene(W, H, mixed)
    means = torch.tensor(sc.pose_3d_init, dtype=torch.float32)
    J = means.shape[0]
    assert J == 17
    ordinary = [(1, 1), (0, max(H, 4)), (1, W), (0, 4), (1, 2 * W), (0, max(2 * H, 4)), (1, 3)]
    targets = [(0, r) for r in CAP_RADII] + [(2, r) for r in CAP_RADII] + ordinary
    shapes = [LONG] * 5 + [(1.0, 1.0, 1.0)] * 12
    scales = solve_scales(cams[0], means, shapes, targets)
    other = solve_scales(cams[1], means, shapes, targets)
    top_view = {j: int(other[j, 0] < scales[j, 0]) for j in (4, 9)}           # the view in which a smaller Gaussian reaches 16 R_MAX
    for j, v in top_view.items():
        scales[j] = (scales, other)[v][j]
    # joints 0-9: walk the fp32 scales around the solution (a step moves 4 sigma by about 0.03 at the cap, 0.5 at 16 R_MAX) until
    # the radii in the view they are solved in are as wanted and no 4 sigma + 0.5, in either view, is an integer
    for j in range(10):
        r = CAP_RADII[j % 5]
        ok = (lambda r1, r2: r1 == r) if j < 5 else (lambda r1, r2: r1 == r2 == r) if j in (5, 6) else \
            (lambda r1, r2: r - 8 <= r1 == r2 <= r) if j == 9 else (lambda r1, r2: min(r1, r2) >= r)
        s0 = scales[j, 0].item()
        for k in sorted(range(-12, 13), key=abs):
            trial = scales.clone()          # (all joints at once, as the case is evaluated: a batched product may round differently)
            trial[j] = torch.tensor(shapes[j]) * float(_next(s0, k))
            lam = twin_lambdas(cams, means, trial, _ident(J))[:, j]
            x = 4.0 * np.sqrt(lam).astype(np.float64) + 0.5
            if ok(*np.floor(x[top_view.get(j, 0)])) and np.abs(x - np.round(x))[x < 4.0 * R_MAX].min(initial=1.0) > 1e-3:      # (see margins_ok)
                scales = trial
                break
        else:
            raise AssertionError(f"joint {j}: no fp32 scale near {s0} gives radius {r}")
    assert np.nanmax(radius_of(twin_lambdas(cams, means, scales, _ident(J)))) <= 16 * R_MAX
    return _case(W, H, mixed, means, scales, _ident(J), detections(2, J, W, H), targets=targets, top_view=top_view)


# ------------------------------------------------------------------------------------------------ 2: the zero crossing of lambda2
ZERO_J = 256


@functools.lru_cache(maxsize=None)
def zero_case(W, H, mixed):
    """256 copies of joint 0, identity rotation, isotropic scales that are CONSECUTIVE fp32 numbers centred on the smallest one
    whose lambda2 in view 0 is positive (bisection over the fp32 bit patterns; lambda2 is non-decreasing in the scale there)."""
    sc, cams, sizes = scene(W, H, mixed)
    mean0 = torch.tensor(sc.pose_3d_init, dtype=torch.float32)[0:1]

    def l2_of(s):
        return float(twin_lambdas(cams[:1], mean0, torch.full((1, 3), float(s)), _ident(1), 1.0)[0, 0, 1])
    lo, hi = np.float32(1.0).view(np.int32), np.float32(100.0).view(np.int32)
    assert l2_of(np.float32(1.0)) < 0 < l2_of(np.float32(100.0))
    while hi - lo > 1:
        mid = np.int32((int(lo) + int(hi)) // 2)
        if l2_of(mid.view(np.float32)) > 0:
            hi = mid
        else:
            lo = mid
    centre = hi.view(np.float32)
    s = _next(centre, np.arange(-ZERO_J // 2, ZERO_J // 2))
    scales = torch.tensor(s)[:, None].repeat(1, 3)
    return _case(W, H, mixed, mean0.repeat(ZERO_J, 1), scales, _ident(ZERO_J), detections(2, ZERO_J, W, H), modifier=1.0, centre=float(centre))


# ------------------------------------------------------------------------------------------------ 3: non-finite and huge inputs
INF = float("inf")
POISONED = 4            # the joint the kinds below poison, one kind per launch (ordinary_case draws its rows with radius 12);
                        # every other joint is ordinary


def _near_plane(cam, mean, depth):
    """`mean` moved along camera 0's viewing axis, in fp64 from the view matrix, until it is `depth` in front of the camera plane."""
    M = cam.world_view_transform.detach().cpu().double().T.numpy()              # camera <- world
    p = mean.detach().cpu().double().numpy()
    tz = M[2, :3] @ p + M[2, 3]
    return torch.tensor(p - M[2, :3] * (tz - depth) / (M[2, :3] @ M[2, :3]), dtype=torch.float32)


def _mean(axis, value):
    return lambda c, j: c.means[j, axis:axis + 1].fill_(value)


KINDS = {
    **{f"mean-{'xyz'[a]}{'+' if s > 0 else '-'}inf": _mean(a, s * INF) for a in range(3) for s in (1, -1)},
    "mean-x+3e38": _mean(0, 3e38), "mean-x-3e38": _mean(0, -3e38), "mean-z+1e30": _mean(2, 1e30),
    "scale-inf": lambda c, j: c.scales[j].fill_(INF), "scale-0": lambda c, j: c.scales[j].fill_(0.0),
    "scale-1e9": lambda c, j: c.scales[j].fill_(1e9), "scale-1e11": lambda c, j: c.scales[j].fill_(1e11),
    "scale-3e38": lambda c, j: c.scales[j].fill_(3e38),
    "quaternion-0": lambda c, j: c.rot[j].fill_(0.0),
    "near-plane-1e-2": lambda c, j: c.means[j].copy_(_near_plane(c.cams[0], c.means[j], 1e-2)),
    "near-plane-1e-3": lambda c, j: c.means[j].copy_(_near_plane(c.cams[0], c.means[j], 1e-3)),
}


@functools.lru_cache(maxsize=None)
def ordinary_case(W, H, mixed):
    """17 joints at ordinary radii (1 .. about 2 n), every plane draws."""
    sc, cams, sizes = scene(W, H, mixed)
    means = torch.tensor(sc.pose_3d_init, dtype=torch.float32)
    J = means.shape[0]
    cycle = [(1, 1), (0, max(H, 4)), (1, W), (0, 4), (0, 12), (0, max(2 * H, 4)), (1, 3), (1, 2 * W), (1, max(W // 2, 1))]
    targets = [cycle[j % len(cycle)] for j in range(J)]
    scales = solve_scales(cams[0], means, [(1.0, 1.0, 1.0)] * J, targets)
    return _case(W, H, mixed, means, scales, _ident(J), detections(2, J, W, H), targets=targets)


def poisoned_case(W, H, mixed, kind, j=POISONED):
    """ordinary_case with joint j poisoned by KINDS[kind] (a fresh copy)."""
    base = ordinary_case(W, H, mixed)
    c = Case()
    c.__dict__.update(base.__dict__)
    c.means, c.scales, c.rot = base.means.clone(), base.scales.clone(), base.rot.clone()
    KINDS[kind](c, j)
    c.lam = twin_lambdas(c.cams, c.means, c.scales, c.rot, c.modifier)
    c.kind = kind
    return c


def margins_ok(c):
    """No 4 sigma + 0.5 of a kept or capped plane within 1e-3 of an integer (twin lambdas; planes with a lambda that is not
    positive or not finite have no radius).  Asked of every radius below 4 R_MAX: from sigma = 2^20 (radius 16 R_MAX) on, the
    spacing of fp32 makes 4 sigma + 0.5 a multiple of 0.5, every other value an integer, and what keeps such a plane's class
    safe is its distance from the cap, a factor of 4 or more, not from an integer."""
    lam = c.lam
    with np.errstate(invalid="ignore"):
        x = 4.0 * np.sqrt(lam).astype(np.float64) + 0.5
        has = (np.isfinite(lam).all(-1) & (lam > 0).all(-1))[..., None] & (x < 4.0 * R_MAX)
    d = np.abs(x - np.round(x))[has]
    return bool((d > 1e-3).all()), (float(d.min()) if d.size else math.inf)


def max_trips(c, lam=None):
    """The largest per-thread exp count over the planes of `c` that draw."""
    lam = c.lam if lam is None else lam
    draw = draws(lam, c.p2d.numpy())
    worst = 0
    for v, (w, h) in enumerate(c.sizes):
        for j in range(c.J):
            if draw[v, j]:
                worst = max(worst, trips(h, radius_of(lam[v, j, 0])), trips(w, radius_of(lam[v, j, 1])))
    return worst
