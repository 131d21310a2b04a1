"""Degenerate footprints on the device (DESIGN.md "Degenerate footprints"): sks_heatmap_factors(_dv) at the truncation-radius
cap, across the sign change of lambda2, and on non-finite and huge inputs; then the public surface and a whole loop.

Every plane's class comes from the KERNEL's own lambdas (sks_view_footprints, the float sequence the factors share) and the rule
of tests/heatmap_degenerate_cases.draws; a plane that draws is held to the fp64 definition (tests/tail_ref.impulse_ref at the
kernel's own fp32 sigma) at the tolerance of test_heatmap_factors_at_any_radius, a plane that does not to the no-impulse bits;
cmin / den are asserted bit for bit as functions of the rows the kernel wrote.  Output buffers start as NaN.
tests/test_heatmap_degenerate_cpu.py shows on the twin that the cases reach what they claim and that no plane that draws takes
more than 2^20 exp per thread."""
import numpy as np
import pytest
import torch

from tests import heatmap_degenerate_cases as DC, util

pytestmark = pytest.mark.gpu

NAN = float("nan")
R = DC.R_MAX
shapes = pytest.mark.parametrize("W,H,mixed", DC.SHAPES, ids=DC.SHAPE_IDS)


def _views(c, device, dv=False, cams=None):
    from skelsplat_amd.rasterizer import ViewBatch
    cams = [cam.to(device) for cam in (c.cams if cams is None else cams)]
    if not dv:
        return ViewBatch.from_cameras(cams, allow_mixed=True), None
    # per-view scalars in a device table (what a frame batch over a rig bank hands the *_dv entry points)
    from skelsplat_amd.rigs import RigBank, RigSelection
    bank = RigBank([cams], device)
    sz = bank.sizes
    vb = ViewBatch(bank.viewmatrix_dev[0].clone(), bank.projmatrix_dev[0].clone(), bank.tan[0, :, 0].tolist(), bank.tan[0, :, 1].tolist(),
                   max(s[0] for s in sz), max(s[1] for s in sz), sz)
    sel = RigSelection(bank, 1, vb.viewmatrix, vb.projmatrix)
    vb.table = sel.table
    sel.select([0])
    return vb, sel


def _factors(c, device, dv=False, means=None, scales=None, rot=None):
    """One sks_heatmap_factors(_dv) launch on the case into NaN buffers, and the kernel's own lambdas of the same inputs:
    (row, col, cmin, den, lam (V,J,2) numpy), all on the host."""
    from skelsplat_amd import _lib
    from skelsplat_amd.heatmaps import heatmap_factors
    from skelsplat_amd.rasterizer import HeatmapFactors
    views, sel = _views(c, device, dv)
    d = lambda t: t.contiguous().to(device)
    m, s, q, p = d(c.means if means is None else means), d(c.scales if scales is None else scales), d(c.rot if rot is None else rot), d(c.p2d)
    fac = HeatmapFactors(c.V, c.J, c.W, c.H, device)
    for t in (fac.row, fac.col, fac.cmin, fac.den):
        t.fill_(NAN)
    heatmap_factors(m, s, q, p, c.cams, scaling_modifier=c.modifier, views=views, out=fac)
    lam = torch.full((c.V, c.J, 2), NAN, device=device)
    host = views.table is None
    _lib.check(_lib.load().sks_view_footprints(c.V, c.J, views.W, views.H, m.data_ptr(), s.data_ptr(), q.data_ptr(), float(c.modifier),
                                               views.viewmatrix.data_ptr(), views.tanfovx if host else None,
                                               views.tanfovy if host else None, views.wh if host else None,
                                               None if host else views.table.data_ptr(), 1, lam.data_ptr(),
                                               torch.cuda.current_stream(device).cuda_stream), "sks_view_footprints")
    torch.cuda.synchronize()
    if sel is not None:
        sel.check()
    return fac.row.cpu(), fac.col.cpu(), fac.cmin.cpu(), fac.den.cpu(), lam.cpu().numpy()


def _same_bits(a, b):
    """Equal bit for bit, the NaN a launch left beyond a smaller view's size included."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _radii(lam):
    return np.stack([DC.radius_of(lam[..., 0]), DC.radius_of(lam[..., 1])], -1)


# ------------------------------------------------------------------------------------------------ 1: at the cap
@shapes
def test_factors_at_the_radius_cap(device, W, H, mixed):
    """Radii R_MAX - 1 and R_MAX are kept and held to the definition, R_MAX + 1, 2 R_MAX and 16 R_MAX give the no-impulse bits in
    row and column alike -- with axis 0 alone beyond the cap (joints 0-4: lambda2's radius is 32 x smaller) and with both axes at
    it (joints 5-9; lambda1 >= lambda2, so axis 1 is never alone beyond it); detections at 0, n - 1 and the middle; the view
    other than the one a radius is solved in (view 0; for 16 R_MAX the view that sees the joint larger, so that no radius of the case is beyond
    16 R_MAX) takes whatever class its own lambdas give.  The kernel's own radii are the ones the case was built for."""
    c = DC.cap_case(W, H, mixed)
    row, col, cmin, den, lam = _factors(c, device)
    r, want = _radii(lam), _radii(c.lam)
    print(f"\nradii of joints 0-9, kernel: {r[:, :10].astype(np.int64).tolist()}\n                    twin:   {want[:, :10].astype(np.int64).tolist()}")
    draw = DC.hold(f"{W}x{H}", row, col, cmin, den, lam, c.p2d.numpy(), c.sizes, util.assert_close)
    assert [int(x) for x in r[0, :4, 0]] == list(DC.CAP_RADII[:4]) and int(r[c.top_view[4], 4, 0]) == 16 * R and (r[:, :5, 1] <= R // 2).all()
    assert [tuple(int(x) for x in r[0, j]) for j in (5, 6)] == [(R - 1, R - 1), (R, R)] and all(r[0, j].min() > R for j in (7, 8, 9))
    assert 16 * R - 8 <= r[c.top_view[9], 9].min() and r.max() <= 16 * R
    assert draw[0].tolist() == [True, True, False, False, False, True, True, False, False, False] + [True] * 7
    assert np.array_equal(draw, DC.draws(c.lam, c.p2d.numpy())), "the kernel's lambdas and the twin's disagree on a plane's class"


# ------------------------------------------------------------------------------------------------ 2: the zero crossing
@shapes
def test_factors_across_the_sign_change_of_lambda2(device, W, H, mixed):
    """256 consecutive fp32 scales centred on the sign change of lambda2: the kernel's own lambda2 takes a negative value, an exact
    0.0 and a positive one; every output is finite; a plane with !(lambda2 > 0) draws nothing; one with lambda2 > 0 has radius 0
    and is the delta col[p] = 1, its row by the definition."""
    c = DC.zero_case(W, H, mixed)
    row, col, cmin, den, lam = _factors(c, device)
    l2 = lam[0, :, 1]
    print(f"\nlambda2 over the sweep: {int((l2 < 0).sum())} negative, {int((l2 == 0).sum())} zero, {int((l2 > 0).sum())} positive")
    assert (l2 < 0).any() and (l2 == 0).any() and (l2 > 0).any()
    draw = DC.hold(f"{W}x{H}", row, col, cmin, den, lam, c.p2d.numpy(), c.sizes, util.assert_close)
    assert np.array_equal(draw[0], l2 > 0)
    w0 = c.sizes[0][0]
    for j in np.nonzero(draw[0])[0]:
        assert DC.radius_of(l2[j]) == 0
        p = min(max(int(c.p2d[0, j, 0]), 0), w0 - 1)
        delta = torch.zeros(w0)
        delta[p] = 1.0
        assert torch.equal(col[0, j, :w0], delta), j


# ------------------------------------------------------------------------------------------------ 3: non-finite and huge inputs
@pytest.mark.parametrize("dv", [False, True], ids=["by-value", "dv"])
@shapes
def test_factors_of_non_finite_and_huge_inputs(device, W, H, mixed, dv):
    """One joint among sixteen ordinary ones, one kind per launch: a mean coordinate +-inf (each axis), +-3e38, 1e30; a scale of
    inf, 0, 1e9, 1e11, 3e38; an all-zero quaternion; a mean 1e-2 and 1e-3 in front of camera 0's plane.  The joint's class in each
    view is the rule's on the kernel's own lambdas, every output is finite, and every other joint keeps the bits of the launch
    with ordinary values in that row.  The near-plane joint is capped in view 0 only."""
    base = DC.ordinary_case(W, H, mixed)
    clean = _factors(base, device, dv)
    assert DC.hold("ordinary", *clean, base.p2d.numpy(), base.sizes, util.assert_close).all()
    others = [j for j in range(base.J) if j != DC.POISONED]
    for kind in DC.KINDS:
        c = DC.poisoned_case(W, H, mixed, kind)
        got = _factors(c, device, dv)
        lam = got[4]
        draw = DC.hold(kind, *got, c.p2d.numpy(), c.sizes, util.assert_close)
        print(f"{kind}: lambdas {lam[:, DC.POISONED].tolist()} draw {draw[:, DC.POISONED].tolist()}")
        assert not draw[0, DC.POISONED], kind
        for name, a, b in zip(("row", "col", "cmin", "den"), got, clean):
            assert _same_bits(a[:, others], b[:, others]), f"{kind}: {name} of another joint changed"
        if kind.startswith("near-plane"):
            assert draw[1, DC.POISONED] and DC.radius_of(lam[0, DC.POISONED]).min() > R and np.isfinite(lam[0, DC.POISONED]).all(), kind


# ------------------------------------------------------------------------------------------------ 4: the public surface
def test_generate_heatmaps_treats_degenerate_planes_as_dropped(device):
    """generate_heatmaps(..., totals=) on the cap case: planes and totals are bit-identical to the same call with drop_mask set at
    the degenerate (view, joint)."""
    from skelsplat_amd.heatmaps import generate_heatmaps
    c = DC.cap_case(40, 24, False)
    lam = _factors(c, device)[4]
    gone = torch.tensor(~DC.draws(lam, c.p2d.numpy()))
    assert bool(gone.any()) and not bool(gone.all())
    d = lambda t: t.contiguous().to(device)
    res = []
    for mask in (None, gone):
        tot = torch.zeros((c.V, 2), dtype=torch.float64, device=device)
        out = torch.full((c.V, c.J, c.H, c.W), NAN, device=device)
        generate_heatmaps(d(c.means), d(c.scales), d(c.rot), d(c.p2d), c.cams, scaling_modifier=c.modifier, out=out, totals=tot, drop_mask=mask)
        torch.cuda.synchronize()
        res.append((out.cpu(), tot.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(torch.isfinite(res[0][0]).all()) and not res[0][0][gone].any() and bool((res[0][1][:, 1] > 0).all())


def test_frames_and_device_table_give_the_per_frame_bits(device):
    """heatmap_factors(frames=2) -- the cap case and a poisoned case stacked -- and the *_dv entry point give, bit for bit, what
    the per-frame by-value calls give."""
    from skelsplat_amd.heatmaps import heatmap_factors
    from skelsplat_amd.rasterizer import HeatmapFactors, ViewBatch
    W, H = 40, 24
    a, b = DC.cap_case(W, H, False), DC.poisoned_case(W, H, False, "near-plane-1e-3")
    one = [_factors(x, device) for x in (a, b)]
    for x, ref in zip((a, b), one):
        for name, got, want in zip(("row", "col", "cmin", "den"), _factors(x, device, dv=True), ref):
            assert _same_bits(got, want), f"dv: {name}"
    cams = [cam.to(device) for cam in a.cams + b.cams]
    views = ViewBatch.from_cameras(cams, allow_mixed=True)
    fac = HeatmapFactors(4, a.J, W, H, device)
    for t in (fac.row, fac.col, fac.cmin, fac.den):
        t.fill_(NAN)
    st = lambda k: torch.stack([getattr(a, k), getattr(b, k)]).contiguous().to(device)
    heatmap_factors(st("means"), st("scales"), st("rot"), torch.cat([a.p2d, b.p2d]).to(device), cams, scaling_modifier=a.modifier,
                    views=views, frames=2, out=fac)
    torch.cuda.synchronize()
    for i, (name, got) in enumerate(zip(("row", "col", "cmin", "den"), (fac.row, fac.col, fac.cmin, fac.den))):
        assert _same_bits(got.cpu(), torch.cat([one[0][i], one[1][i]])), f"frames = 2: {name}"


# ------------------------------------------------------------------------------------------------ 5: a whole loop
LOOP_ITERS, LOOP_JOINT = 8, 13
# 0.05 in front of camera 0's plane: on the twin the radius in view 0 is 1.08e6 = 4.1 R_MAX (12 to 25 in the other views), beyond
# the cap by a factor and short of the 16 R_MAX up to which a kernel without the cap is still a short launch
LOOP_DEPTH = 5e-2


def test_a_capped_plane_is_a_dropped_plane_to_the_loop(device):
    """FrameBatchLoop.new_scenes(points, poses_2d), F = 2, 8 iterations, joint 13 of frame 0 placed 0.05 in front of camera 0's
    plane: its plane in view 0 is capped (the kernel's own lambdas say so), the other views draw.  Frame 0 ends with the bits --
    joints, parameters, moments, counters -- of the run with drop_masks[0, 0, 13] = True: a capped plane and a dropped one are
    +0 in every consumer (the totals skip them, the fused loss forms (0 * col - 0) / den).  Frame 1 ends with the bits it has in
    a batch without the degenerate joint."""
    from skelsplat_amd import _lib
    from skelsplat_amd.loop import FrameBatchLoop
    from skelsplat_amd.rasterizer import ViewBatch
    from tests import nan_joint_cases as NC
    sc, model = NC.loop_scene(device)
    V, J, F = len(sc.cameras), sc.n_joints, 2
    p2d = np.stack([np.asarray(sc.poses_2d, np.float32)] * F)
    pts = torch.tensor(np.stack([np.asarray(sc.pose_3d_init, np.float32)] * F))
    near = pts.clone()
    near[0, LOOP_JOINT] = DC._near_plane(sc.cameras[0], pts[0, LOOP_JOINT], LOOP_DEPTH)
    drop = np.zeros((F, V, J), bool)
    drop[0, 0, LOOP_JOINT] = True
    state = lambda fb, f: [t[f].clone() for t in (fb.xyz, fb.scaling, fb.rotation, fb.opacity, fb.exp_avg, fb.exp_avg_sq, fb.counters)]
    res = {}
    for name, points, masks in (("capped", near, None), ("dropped", near, drop), ("clean", pts, None)):
        fb = FrameBatchLoop(model(device), sc.cameras, F, dataset="h36m")
        fb.new_scenes(points, poses_2d=p2d, drop_masks=masks)
        if name == "capped":        # the class of every plane of frame 0, from the kernel's own lambdas
            lam = torch.full((V, J, 2), NAN, device=device)
            vb = ViewBatch.from_cameras(sc.cameras)
            act = torch.exp(fb.scaling[0]).contiguous()         # (the tensor new_scenes hands sks_heatmap_factors)
            _lib.check(_lib.load().sks_view_footprints(V, J, vb.W, vb.H, fb.xyz[0].contiguous().data_ptr(), act.data_ptr(),
                                                       fb.rotation[0].contiguous().data_ptr(), 1.0, vb.viewmatrix.data_ptr(),
                                                       vb.tanfovx, vb.tanfovy, None, None, 1, lam.data_ptr(),
                                                       torch.cuda.current_stream(device).cuda_stream), "sks_view_footprints")
            torch.cuda.synchronize()
            draw = DC.draws(lam.cpu().numpy(), p2d[0])
            want = np.ones((V, J), bool)
            want[0, LOOP_JOINT] = False
            assert np.array_equal(draw, want), draw
            assert 2 * R < DC.radius_of(lam[0, LOOP_JOINT].cpu().numpy()).min() < 16 * R
            f0 = fb.factors
            assert not f0.row[0, LOOP_JOINT].any() and not f0.col[0, LOOP_JOINT].any() and float(f0.den[0, LOOP_JOINT]) == float(DC.DEN0)
        start = fb.xyz.clone()
        fb.run(LOOP_ITERS, groups_per_graph=4)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(fb.xyz).all()) and not torch.equal(fb.xyz, start)
        res[name] = [state(fb, f) for f in range(F)]
    for k, (x, y) in enumerate(zip(res["capped"][0], res["dropped"][0])):
        assert torch.equal(x, y), f"frame 0, state {k}: a capped plane and a dropped plane differ"
    for k, (x, y) in enumerate(zip(res["capped"][1], res["clean"][1])):
        assert torch.equal(x, y), f"frame 1, state {k}: the other frame noticed the degenerate joint"
