"""Degenerate footprints (DESIGN.md "Degenerate footprints"), the part that needs no GPU: the constant is one number in the
header, the binding and the twin; the cases of tests/heatmap_degenerate_cases.py reach what tests/test_heatmap_degenerate_gpu.py
relies on (on the twin's fp32 lambdas); and the twin under the new mask is total -- kept planes are the fp64 definition
(tests/tail_ref.impulse_ref), degenerate planes the no-impulse plane, the golden scene untouched."""
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import heatmaps_ref as HR
from tests import heatmap_degenerate_cases as DC, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = DC.R_MAX
shapes = pytest.mark.parametrize("W,H,mixed", DC.SHAPES, ids=DC.SHAPE_IDS)
# the twin's closed form walks (radius + n - 1) / 2n pairs of bounces in Python: 131 072 of them on the one-sample axis of 130x1
# at the cap (14 s) and 2 x 8 192 at 16x16 (6 s), so at the cap the twin is run on the two 40x24 shapes (2 s each; its code has no
# path that depends on the size); the definition itself (impulse_ref) is what all four shapes are held to on the GPU
twin_shapes = pytest.mark.parametrize("W,H,mixed", [s for s in DC.SHAPES if s[1] > 16], ids=[i for s, i in zip(DC.SHAPES, DC.SHAPE_IDS) if s[1] > 16])


def test_the_cap_is_one_number():
    from skelsplat_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "skelsplat_hip.h")).read()
    assert int(re.search(r"#define\s+SKS_HEATMAP_MAX_RADIUS\s+(\d+)", hdr).group(1)) == _lib.SKS_HEATMAP_MAX_RADIUS == HR.HEATMAP_MAX_RADIUS == 1 << 18


def test_the_rule():
    """draws(): (a) non-finite lambda or detection, (b) a lambda that is not positive (-0.016, -0, +0), (c) a radius beyond the cap
    on either axis; R_MAX itself is kept."""
    s_at = lambda r: np.float32((r / 4.0) ** 2)          # 4 sigma + 0.5 = r + 0.5
    assert DC.radius_of(s_at(R)) == R and DC.radius_of(s_at(R + 1)) == R + 1
    ok, inf, nan = [1.0, 1.0], float("inf"), float("nan")
    cases = [([1.0, 0.5], ok, True), ([s_at(R), s_at(R)], ok, True), ([s_at(R - 1), 3e-8], ok, True),
             ([nan, 1.0], ok, False), ([1.0, nan], ok, False), ([inf, 1.0], ok, False), ([1.0, 0.5], [nan, 1.0], False),
             ([1.0, 0.5], [1.0, inf], False), ([0.6, -0.016], ok, False), ([0.6, 0.0], ok, False), ([0.6, -0.0], ok, False),
             ([s_at(R + 1), 1.0], ok, False), ([s_at(R + 1), s_at(R + 1)], ok, False), ([s_at(16 * R), s_at(R)], ok, False),
             ([1e19, 1e19], ok, False)]
    for lam, det, want in cases:
        assert bool(DC.draws(np.float32([[lam]]), np.float32([[det]]))[0, 0]) == want, (lam, det)


def test_the_trip_bound():
    """The bound of k_heatmap_factors' comment at the cap: at most 1024 normalisation trips, 2^19 + 4 (+ 3) exp at n = 1, about
    2^11 at n >= 256."""
    assert DC.trips(1, R) - R // 256 == (1 << 19) + 3 and R // 256 == 1024
    for n in (1, 16, 24, 40, 130, 256, 1000, 4100):
        bound = R // 256 + 4 * ((n + 255) // 256) * (R // (2 * n) + 1) + 3 * ((n + 255) // 256)
        assert DC.trips(n, R) <= bound <= DC.TRIP_CAP, (n, DC.trips(n, R), bound)
    assert DC.trips(256, R) - 1024 < 1.01 * (1 << 11) and DC.trips(4100, R) - 1024 < 2.2 * (1 << 11)


@shapes
def test_the_cap_case_reaches_the_cap(W, H, mixed):
    c = DC.cap_case(W, H, mixed)
    both = np.stack([DC.radius_of(c.lam[..., 0]), DC.radius_of(c.lam[..., 1])], -1)          # (V, J, 2)
    r = both[0]
    draw = DC.draws(c.lam, c.p2d.numpy())
    assert [int(x) for x in r[:4, 0]] == list(DC.CAP_RADII[:4]) and int(both[c.top_view[4], 4, 0]) == 16 * R, (r[:5], both[:, 4])
    assert (both[:, :5, 1] <= DC.R_MAX // 2).all(), "joints 0-4: axis 1 is not far below the cap"
    assert [tuple(int(x) for x in r[j]) for j in (5, 6)] == [(R - 1, R - 1), (R, R)]
    assert all(min(r[j]) >= DC.CAP_RADII[j - 5] for j in (7, 8)) and 16 * R - 8 <= both[c.top_view[9], 9].min() and both[:, [4, 9]].max(-1).min() > 8 * R
    assert both.max() <= 16 * R, "a radius beyond 16 R_MAX: too long a launch for a kernel without the cap"
    assert draw[0].tolist() == [True, True, False, False, False, True, True, False, False, False] + [True] * 7
    # the detections of the planes at the cap: at 0, at n - 1 and in the middle, kept and capped alike
    assert {j % 3 for j in (0, 1, 5, 6)} == {0, 1, 2} == {j % 3 for j in (2, 3, 4, 7, 8, 9)}
    ok, least = DC.margins_ok(c)
    assert ok, f"a truncation radius sits on a rounding step ({least})"
    assert DC.max_trips(c) <= DC.TRIP_CAP


@shapes
def test_the_zero_case_crosses_zero(W, H, mixed):
    """The sweep of 256 consecutive fp32 scales holds a negative lambda2, an exact 0 and a positive one in view 0, lambda2 runs
    through consecutive multiples of 2^-25 there, and every positive one has radius 0."""
    c = DC.zero_case(W, H, mixed)
    s = c.scales[:, 0].numpy()
    assert (np.diff(s.view(np.int32)) == 1).all() and c.J == 256
    l2 = c.lam[0, :, 1]
    assert (l2 < 0).any() and (l2 == 0).any() and (l2 > 0).any()
    steps = l2.astype(np.float64) * 2.0 ** 25
    assert (steps == np.round(steps)).all() and set(np.diff(steps)) <= {0.0, 1.0}
    assert (DC.radius_of(l2[l2 > 0]) == 0).all() and (DC.radius_of(c.lam[0, :, 0]) == 3).all()
    if (W, H) == (40, 24):
        assert abs(c.centre - 4.7732325) < 1e-5, c.centre
    assert DC.margins_ok(c)[0] and DC.max_trips(c) <= DC.TRIP_CAP
    draw = DC.draws(c.lam, c.p2d.numpy())
    assert np.array_equal(draw[0], l2 > 0)


@shapes
def test_the_poisoned_cases(W, H, mixed):
    """Every kind leaves the poisoned joint without an impulse in view 0 (by the rule on the twin's lambdas) and every other
    joint's lambdas untouched; the near-plane joint is capped in view 0 only."""
    base = DC.ordinary_case(W, H, mixed)
    assert DC.draws(base.lam, base.p2d.numpy()).all() and DC.margins_ok(base)[0] and DC.max_trips(base) <= DC.TRIP_CAP
    others = [j for j in range(base.J) if j != DC.POISONED]
    for kind in DC.KINDS:
        c = DC.poisoned_case(W, H, mixed, kind)
        draw = DC.draws(c.lam, c.p2d.numpy())
        assert np.array_equal(c.lam[:, others], base.lam[:, others]) and draw[:, others].all(), kind
        assert not draw[0, DC.POISONED], kind
        assert DC.margins_ok(c)[0] and DC.max_trips(c) <= DC.TRIP_CAP, kind
        r = DC.radius_of(c.lam[:, DC.POISONED])
        if kind.startswith("near-plane"):
            assert r[0].min() > 4 * R and r[1].max() < 100 and draw[1, DC.POISONED], (kind, r)
            depth = float(c.means[DC.POISONED].double() @ c.cams[0].world_view_transform.double()[:3, 2] + c.cams[0].world_view_transform.double()[3, 2])
            assert 0.2 * float(kind[-4:]) < depth < 5 * float(kind[-4:]), (kind, depth)
        elif kind in ("scale-1e9", "scale-1e11"):
            assert not np.isfinite(c.lam[0, DC.POISONED]).all() or r[0].min() > 4 * R, (kind, r)
        else:
            assert not draw[1, DC.POISONED], kind


def _twin(c, v):
    cam = c.cams[v]
    return HR.heatmap_factors(c.means, c.scales, c.rot, c.p2d[v:v + 1], [cam], scaling_modifier=c.modifier)


@twin_shapes
def test_the_twin_is_total_at_the_cap(W, H, mixed):
    """oracle/heatmaps_ref.heatmap_factors on the cap case: no exception, kept planes equal impulse_ref at the GPU test's
    tolerance, planes beyond the cap are the no-impulse plane."""
    c = DC.cap_case(W, H, mixed)
    for v in range(1):          # (view 0, the one the radii are solved in; its 2 x 5 000 pairs of bounces take the twin 2 s)
        row, col, cmin, den = _twin(c, v)
        draw = DC.hold(f"twin {W}x{H}", row, col, cmin, den, c.lam[v:v + 1], c.p2d[v:v + 1].numpy(), c.sizes[v:v + 1], util.assert_close)
        assert draw.any() and not draw.all()


@shapes
def test_the_twin_is_total_across_zero_and_on_poisoned_joints(W, H, mixed):
    c = DC.zero_case(W, H, mixed)
    row, col, cmin, den = _twin(c, 0)
    draw = DC.hold("twin, zero crossing", row, col, cmin, den, c.lam[:1], c.p2d[:1].numpy(), c.sizes[:1], util.assert_close)
    kept = np.nonzero(draw[0])[0]
    assert len(kept) and not draw[0].all()
    for j in kept:        # radius 0: the delta
        p = min(max(int(c.p2d[0, j, 0]), 0), c.sizes[0][0] - 1)
        assert float(col[0, j, p]) == 1.0 and float(col[0, j].sum()) == 1.0
    for kind in DC.KINDS:
        c = DC.poisoned_case(W, H, mixed, kind)
        for v in range(c.V):
            row, col, cmin, den = _twin(c, v)
            DC.hold(f"twin, {kind}", row, col, cmin, den, c.lam[v:v + 1], c.p2d[v:v + 1].numpy(), c.sizes[v:v + 1], util.assert_close)


def test_the_golden_scene_has_no_degenerate_plane():
    """tests/golden/reference_heatmaps.npz (the reference's own output, which tests/test_cpu.py holds the twin to): every plane
    draws under the rule, so the mask changes nothing there."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_heatmaps.npz"))
    W, H = int(g["W"]), int(g["H"])
    cams = [types.SimpleNamespace(image_width=W, image_height=H, world_view_transform=torch.tensor(g["world_view_transform"][v]),
                                  FoVx=float(g["fov"][v, 0]), FoVy=float(g["fov"][v, 1])) for v in range(2)]
    lam = DC.twin_lambdas(cams, torch.tensor(g["xyz"]), torch.exp(torch.tensor(g["scaling_raw"])), torch.tensor(g["rotation_raw"]), 1.0)
    assert DC.draws(lam, g["poses_2d"]).all()
