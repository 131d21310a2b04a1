"""Unobserved joints (DESIGN.md "Unobserved joints") on the references alone, no GPU: every case of tests/nan_joint_cases.py
reaches what it claims, and the references the GPU tests compare with say what the contract says."""
import math

import numpy as np
import pytest
import torch

from tests import geometry_cases as G, nan_joint_cases as NC, nan_joint_ref as NR, tail_ref


@pytest.mark.parametrize("name", NC.NAMES)
def test_the_replacement_point_is_culled_in_every_view(name):
    """The finite stand-in of the NaN rows is behind every camera: oracle radius 0 in every view, every other Gaussian as the
    clean scene has it, and the shape takes the launch forms the regime is there for."""
    c, fwd, bwd, _, _ = NR.raster_reference(name)
    G.check_claims(c.cull)
    assert (c.regime == "p17-v9") == (c.V > 8)           # (V > 8: the `wide` slot walk of adam_block_finish)
    rows = list(c.rows)
    for v in range(c.V):
        cam = c.cull.cams[v]
        z = (np.asarray(cam.world_view_transform.cpu().numpy(), np.float64).T @ np.append(c.point.astype(np.float64), 1.0))[2]
        assert z <= -1000.0, (name, v, z)
        assert (fwd[v]["radii"][rows] == 0).all(), (name, v)
        for key in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dmeans2D"):
            assert not np.any(bwd[v][key][rows]), (name, v, key)
            assert np.isfinite(bwd[v][key]).all()
    others = np.setdiff1d(np.arange(c.P), rows)
    if len(others):
        assert max(int((fwd[v]["radii"][others] > 0).sum()) for v in range(c.V)) >= min(len(others), 8), "nothing else is rendered"
        assert max(float(np.abs(bwd[v]["dL_dopacity"][others]).max()) for v in range(c.V)) > 0
    else:
        assert all(not f["color"].any() for f in fwd)
    # the two forms differ in the rows of the placement, and only there
    same = c.nan.means == c.cull.means
    assert same[others].all() and not same[rows][:, list(c.coords)].any()
    assert np.isnan(c.nan.means[rows][:, list(c.coords)]).all()


@pytest.mark.parametrize("pl", NC.PLACEMENTS)
def test_the_pair_a_case_claims_to_drop_is_the_pair_the_masked_model_drops(pl):
    """The masked limb loss of the references (tail_ref.limb_loss / ref_loop.limb_loss_without with `missing=`) and the library's
    tensor-op rule (loop.limb_consistency_observed on the NaN joints themselves) agree on value and gradient: the pairs in
    `dropped` give every one of their four joints a zero gradient, the other pair the gradient it has in the clean skeleton."""
    from skelsplat_amd import loop
    from tests.ref_loop import limb_loss_without
    rows, coords, dropped = NC.placement(pl, NC.J)
    g = torch.Generator().manual_seed(5)
    clean = (torch.randn((NC.J, 3), generator=g) * 300.0).double()
    nan = clean.clone()
    for r in rows:
        nan[r, list(coords)] = float("nan")

    def val_grad(fn, x):
        x = x.clone().requires_grad_(True)
        y = fn(x)
        (gx,) = torch.autograd.grad(y, x, allow_unused=True) if y.requires_grad else (None,)
        return y.detach(), torch.zeros_like(x) if gx is None else gx

    v_clean, g_clean = val_grad(lambda x: loop.limb_3d_consistency_loss(x, "h36m"), clean)
    v_lib, g_lib = val_grad(lambda x: loop.limb_consistency_observed(x, "h36m"), nan)
    v_ref, g_ref = val_grad(lambda x: limb_loss_without(x, "h36m", set(rows)), nan)
    v_tail, g_tail = val_grad(lambda x: tail_ref.limb_loss(x, tail_ref.H36M_LIMB, set(rows)), nan)
    assert torch.isfinite(g_lib).all() and torch.isfinite(v_lib)
    for v_, g_ in ((v_ref, g_ref), (v_tail, g_tail)):
        assert torch.equal(v_, v_lib) and torch.equal(g_, g_lib)
    kept = tail_ref.pairs_kept(tail_ref.H36M_LIMB, rows)
    assert kept == ("arms" not in dropped, "legs" not in dropped)
    for name, idx in (("arms", NC.ARMS), ("legs", NC.LEGS)):
        if name in dropped:
            assert not g_lib[list(idx)].any(), (pl, name)
        else:
            assert torch.equal(g_lib[list(idx)], g_clean[list(idx)]) and bool(g_lib[list(idx)].any()), (pl, name)
    assert not g_lib[list(NC.NO_LIMB)].any()
    # what the rule replaces: the reference's formula through autograd carries the NaN to the partner joints of the pair
    if dropped and pl != "all":
        _, g_old = val_grad(lambda x: loop.limb_3d_consistency_loss(x, "h36m"), nan)
        partners = [i for n_, idx in (("arms", NC.ARMS), ("legs", NC.LEGS)) if n_ in dropped for i in idx if i not in rows]
        assert bool(torch.isnan(g_old[partners]).any()), "the plain formula no longer spreads the NaN: the rule may be moot"


def test_the_tensor_op_rule_is_the_plain_formula_for_finite_joints():
    """loop.limb_consistency_observed == loop.limb_3d_consistency_loss, value and gradient bit for bit, fp32 and fp64, on
    random skeletons of every dataset (and one with a limb of length zero)."""
    from skelsplat_amd import loop
    from skelsplat_amd.scene import DATASETS
    g = torch.Generator().manual_seed(1)
    for ds in DATASETS:
        n = DATASETS[ds]["n_joints"] if "n_joints" in DATASETS[ds] else 1 + max(i for pair in DATASETS[ds]["limbs"] for i in pair)
        for dt in (torch.float32, torch.float64):
            for k in range(4):
                x = (torch.randn((n, 3), generator=g) * 300.0).to(dt)
                if k == 3:
                    a, b = DATASETS[ds]["limbs"][0]
                    x[a] = x[b]
                xs = [x.clone().requires_grad_(True) for _ in range(2)]
                ya, yb = loop.limb_3d_consistency_loss(xs[0], ds), loop.limb_consistency_observed(xs[1], ds)
                ga, gb = torch.autograd.grad(ya * 1e-5, xs[0])[0], torch.autograd.grad(yb * 1e-5, xs[1])[0]
                assert torch.equal(ya, yb) and (torch.equal(ga, gb) or (k == 3 and torch.equal(torch.isnan(ga), torch.isnan(gb))))


def _twin_inputs():
    sc, model = NC.loop_scene("cpu")
    gm = model("cpu")
    means = torch.tensor(np.asarray(sc.pose_3d_init), dtype=torch.float32)
    p2d = torch.tensor(np.asarray(sc.poses_2d), dtype=torch.float32)
    return sc, means, gm.get_scaling.detach(), gm._rotation.detach(), p2d


def test_the_heat_map_twin_gives_zero_planes_and_unchanged_totals():
    """oracle/heatmaps_ref.py with a NaN mean (all three coordinates, y only) and with a non-finite detection (x, y, both) on
    one view: that plane is row = col = cmin = 0, den = 1e-8, all zero; every other plane keeps its bits; the view's totals are
    the clean totals without that plane's share.  Nothing raises."""
    from oracle import heatmaps_ref as HR
    sc, means, scaling, rot, p2d = _twin_inputs()
    V, Jn = p2d.shape[0], p2d.shape[1]
    clean_f = HR.heatmap_factors(means, scaling, rot, p2d, sc.cameras)
    tot_clean = torch.zeros((V, 2), dtype=torch.float64)
    clean = HR.generate_heatmaps(means, scaling, rot, p2d, sc.cameras, totals=tot_clean)
    nan = float("nan")
    j = NC.MISSING
    cases = {"mean": (lambda m, p: m[j].fill_(nan), range(V)), "mean-y": (lambda m, p: m[j, 1:2].fill_(nan), range(V)),
             "det-x": (lambda m, p: p[1, j, 0:1].fill_(nan), (1,)), "det-y": (lambda m, p: p[2, j, 1:2].fill_(nan), (2,)),
             "det-xy": (lambda m, p: p[0, j].fill_(nan), (0,))}
    for name, (poison, views) in cases.items():
        m, p = means.clone(), p2d.clone()
        poison(m, p)
        row, col, cmin, den = HR.heatmap_factors(m, scaling, rot, p, sc.cameras)
        tot = torch.zeros((V, 2), dtype=torch.float64)
        planes = HR.generate_heatmaps(m, scaling, rot, p, sc.cameras, totals=tot)
        assert not torch.isnan(planes).any(), name
        gone = torch.zeros((V, Jn), dtype=torch.bool)
        for v in views:
            gone[v, j] = True
            NR.zero_plane_factors(row, col, cmin, den, v, j)
            assert not planes[v, j].any()
            # the separable form evaluated as the kernels evaluate it
            assert not ((row[v, j][:, None] * col[v, j][None, :] - cmin[v, j]) / den[v, j]).any()
        for a, b in zip((row, col, cmin, den), clean_f):
            assert torch.equal(a[~gone], b[~gone]), name
        assert torch.equal(planes[~gone], clean[~gone]), name
        want = tot_clean.clone()
        for v in views:
            want[v, 0] -= (clean[v, j].double() ** 2).sum()
            want[v, 1] -= (clean[v, j] > 0).double().sum()
        assert torch.equal(tot[:, 1], want[:, 1]) and float((tot[:, 0] - want[:, 0]).abs().max()) <= 1e-9 * float(want[:, 0].max()), name
        assert float(tot_clean[list(views)[0], 1] - tot[list(views)[0], 1]) > 0, "the plane had nothing to lose"


def _loop_inputs(iters_scene_seed=9):
    from oracle import heatmaps_ref as HR
    sc, model = NC.loop_scene("cpu", seed=iters_scene_seed)
    gm = model("cpu")
    pts = torch.tensor(np.asarray(sc.pose_3d_init), dtype=torch.float32)
    p2d = torch.tensor(np.asarray(sc.poses_2d), dtype=torch.float32)
    return sc, model, gm, pts, p2d, HR


def test_the_masked_literal_loop_moves_the_observed_joints():
    """24 iterations of the masked literal loop from the scene's initial joints with joint MISSING unobserved: the sixteen others
    move by more than the 0.05 mm test_loop_matches_reference_loop demands for non-vacuity, differently from the clean loop on
    the partner joints of the arm pair, and the unobserved row stays NaN."""
    sc, model, gm, pts, p2d, HR = _loop_inputs()
    nan_pts = pts.clone()
    nan_pts[NC.MISSING] = float("nan")
    hm = HR.generate_heatmaps(nan_pts, gm.get_scaling.detach(), gm._rotation.detach(), p2d, sc.cameras)
    assert not hm[:, NC.MISSING].any() and not torch.isnan(hm).any()
    out, moved = NR.masked_literal_loop(sc, model, nan_pts, hm, 24, {NC.MISSING})
    assert moved > 0.05, moved
    assert torch.isnan(out[NC.MISSING]).all()
    seen = [p for p in range(NC.J) if p != NC.MISSING]
    assert torch.isfinite(out[seen]).all()
    print(f"\nmasked literal loop, 24 iterations: observed joints moved {moved:.3f} mm on average")


def test_missing_nothing_is_the_loop_as_it_was():
    """run_reference_loop(missing=set()) against the loop body it had before `missing=` existed, restated here: the same bits
    after 8 iterations (two optimiser steps), parameters and moments."""
    from tests.ref_loop import run_reference_loop, render_ref
    from skelsplat_amd.loop import limb_3d_consistency_loss, l2_loss_gaussian
    import copy
    sc, model, gm0, pts, p2d, HR = _loop_inputs()
    hm = HR.generate_heatmaps(pts, gm0.get_scaling.detach(), gm0._rotation.detach(), p2d, sc.cameras)
    cams = [copy.copy(c).to("cpu") for c in sc.cameras]
    W, H, V, iters = sc.W, sc.H, len(cams), 8

    gm = model("cpu")
    got = run_reference_loop(gm, cams, hm, W, H, "h36m", iters, missing=set())

    ref = model("cpu")
    accumulated = torch.zeros((V,) + tuple(ref._xyz.shape))
    for iteration in range(1, iters + 1):
        ref.update_learning_rate(iteration)
        idx = (iteration - 1) % V
        P = ref._xyz.shape[0]
        from oracle import torch_ref
        color, _, _ = torch_ref.rasterize(ref.get_xyz, None, ref.get_features.reshape(P, -1), ref.get_opacity, ref.get_scaling,
                                          ref.get_rotation, None, cams[idx].world_view_transform, cams[idx].full_proj_transform,
                                          W, H, math.tan(cams[idx].FoVx * 0.5), math.tan(cams[idx].FoVy * 0.5))
        l2, _ = l2_loss_gaussian(color.clamp(0, 1), hm[idx])
        loss = l2 + limb_3d_consistency_loss(ref.get_xyz, "h36m") * 1e-5
        params = [ref._xyz, ref._scaling, ref._rotation, ref._opacity]
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        gx, gs, gr, go = [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, params)]
        accumulated[idx] = gx
        ref._scaling.grad, ref._rotation.grad, ref._opacity.grad = gs, gr, go
        if iteration % 4 == 0:
            ref._xyz.grad = accumulated.mean(dim=0)
            with torch.no_grad():
                ref.optimizer.step()
                ref.optimizer.zero_grad(set_to_none=True)
    assert torch.equal(got, ref._xyz.detach())
    for a, b in ((gm._scaling, ref._scaling), (gm._rotation, ref._rotation), (gm._opacity, ref._opacity)):
        assert torch.equal(a.detach(), b.detach())
    assert not torch.equal(got, pts)


def test_the_tail_reference_with_a_missing_joint():
    """tail_ref.adam_step_ref(missing=): the unobserved row keeps its NaN and zero moments, the dropped pair's joints get the
    step they get with lambda 0, the kept pair's joints the step of the clean skeleton; missing=() is the call without it."""
    g = torch.Generator().manual_seed(3)
    V, P = 4, 17
    xyz = torch.randn((P, 3), generator=g) * 300.0
    grads = torch.randn((V, P, 11), generator=g)
    slots = torch.randn((V, P, 3), generator=g)
    rest = (torch.randn((P, 3), generator=g), torch.randn((P, 4), generator=g), torch.randn((P, 1), generator=g))
    m = v = torch.zeros((P, 11))
    sched, lrs, adam = (2.0, 0.02, 0.0, 0.0, 4000.0), (0.005, 0.001, 0.05), (0.9, 0.999, 1e-15)
    call = lambda x, gr, lam, missing: tail_ref.adam_step_ref(gr, slots, 0xF, 3, (x,) + rest, m, v, (0, 0), 4, sched, lrs, adam, lam,
                                                              tail_ref.H36M_LIMB, missing=missing)
    a, b = call(xyz, grads, 1.0, ()), tail_ref.adam_step_ref(grads, slots, 0xF, 3, (xyz,) + rest, m, v, (0, 0), 4, sched, lrs, adam, 1.0,
                                                             tail_ref.H36M_LIMB)
    for k in ("slots", "m", "v", "xyz"):
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1])
    j = 12
    nan_xyz, g0 = xyz.clone(), grads.clone()
    nan_xyz[j] = float("nan")
    g0[:, j] = 0.0
    slots[:, j] = 0.0
    with_lam, no_lam, clean = call(nan_xyz, g0, 1.0, {j}), call(nan_xyz, g0, 0.0, {j}), call(xyz, g0, 1.0, ())
    assert torch.isnan(with_lam["xyz"][0][j]).all() and not with_lam["m"][0][j].any() and not with_lam["v"][0][j].any()
    arms, legs = [i for i in NC.ARMS if i != j], list(NC.LEGS)
    assert torch.equal(with_lam["xyz"][0][arms], no_lam["xyz"][0][arms])
    assert torch.equal(with_lam["xyz"][0][legs], clean["xyz"][0][legs])
    assert not torch.equal(with_lam["xyz"][0][legs], no_lam["xyz"][0][legs])
    assert torch.isfinite(with_lam["xyz"][0][[i for i in range(P) if i != j]]).all()
