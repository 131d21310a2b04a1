"""Unobserved joints on the device (DESIGN.md "Unobserved joints"): a joint whose mean holds a NaN when a loop starts renders
nothing, has zero pseudo-GT planes, takes its limb pair out of the loss, stays NaN -- and nothing else changes in a single bit.

3a  every rasterizer entry point with the NaN rows of tests/nan_joint_cases.py against the same call with those rows at a finite
    point behind every camera (torch.equal, every output) and against the CPU oracle of that culled scene (forward and lists bit
    for bit, gradients within the oracle's computed rounding bound);
3b  the heat-map factor / totals / plane kernels, one call at a time, for a NaN mean and for non-finite detections;
3d  whole loops: the other frames of a batch, a stream, a pipeline end bit-identical to the batch with that frame clean; the
    frame itself follows the masked literal loop (tests/ref_loop.py `missing=`); the MultiViewLoop paths agree with each other;
    early stopping fires where the host criterion fires on the loop's own reported losses.
(3c, the tail one call at a time, is in tests/test_loop_tail_gpu.py.)  tests/test_nan_joint_cpu.py shows on the references alone
that the cases reach what they claim.  Only NaN is fed to any kernel here: no infinity, no huge coordinate."""
import copy

import numpy as np
import pytest
import torch

from tests import fused_loss_cases as FC, fused_loss_ref as FR, geometry_cases as G, nan_joint_cases as NC, nan_joint_ref as NR
from tests import tail_ref, util
from skelsplat_amd import _lib, rasterizer as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
SEEN = {"grad_excess": 0.0, "fused_excess": 0.0}      # largest bound excess over the cases run (printed per test)


def _clean(name, t):
    assert not torch.isnan(t).any(), f"{name} holds a NaN"


def _same(name, a, b):
    assert a.shape == b.shape and torch.equal(a, b), f"{name}: the NaN rows and the culled rows give different bits"


def _positive_zero(name, t):
    assert not t.any() and not torch.signbit(t).any(), f"{name}: the unobserved rows' gradient is not +0.0"


def _runs(name, device):
    """(case, Run of the culled form with the oracle's forward / backward, the same Run with the NaN means on the device)"""
    c, fwd, _, _, _ = NR.raster_reference(name)
    cull = G.Run(c.cull, device, fwd=fwd, bound=True)
    nan = copy.copy(cull)
    nan.args = (torch.tensor(c.nan.means, device=device),) + cull.args[1:]
    assert int(torch.isnan(nan.args[0]).any(dim=1).sum()) == len(c.rows)
    return c, cull, nan


# ------------------------------------------------------------------------------------------------------------ 3a
@pytest.mark.parametrize("name", NC.NAMES)
def test_nan_rows_render_like_culled_rows(device, name):
    """sks_forward + sks_backward, sks_forward_backward and the prefilled forms."""
    c, cull, nan = _runs(name, device)
    rows = list(c.rows)
    binned = cull.regime["path"] == _lib.PATH_BINNED
    # against the oracle of the culled scene: forward, lists, the seven gradients
    G.check_forward_bits(nan)
    stats = {}
    if len(rows) < c.P:
        G.check_gradients(nan, stats=stats)
    else:       # every row unobserved: nothing is rendered and the oracle's gradients are all zero (no "gradient to get wrong")
        _, _, _, st = nan.forward()
        g = nan.backward(st, want_dfeatures=True)
        torch.cuda.synchronize()
        for key, oname in G.GRADS:
            got = g[key].cpu().numpy()
            for v in range(c.V):
                assert not nan.bwd[v][oname].any()
                stats[oname] = max(stats.get(oname, 0.0), util.bound_excess(got[v], nan.bwd[v][oname], nan.bwd[v]["bound"][oname]))
                util.assert_close_bound(f"{name} view {v} {oname}", got[v], nan.bwd[v][oname], nan.bwd[v]["bound"][oname])
    SEEN["grad_excess"] = max([SEEN["grad_excess"]] + list(stats.values()))
    print(f"{name}: largest gradient excess {max(stats.values()):.2f} x 2^-24 x sum|terms| (so far {SEEN['grad_excess']:.2f})")
    # against the culled rows on the device: every output
    outs = {}
    for key, run in (("nan", nan), ("cull", cull)):
        color, inv, radii, st, final_T, n_contrib = run.forward(want_aux=True)
        lists = {}
        if binned:      # (the exported point list is written up to each view's entry count)
            pl, rg, nr = R.export_lists(st)
            lists = dict(ranges=rg.clone(), num_rendered=nr.clone(),
                         **{f"point_list{v}": pl[v, :int(nr[v].item())].clone() for v in range(c.V)})
        g = run.backward(st, want_dfeatures=True)
        torch.cuda.synchronize()
        outs[key] = dict(color=color.clone(), inv=inv.clone(), radii=radii.clone(), final_T=final_T.clone(), n_contrib=n_contrib.clone(),
                         **lists, **{f"d_{k}": x.clone() for k, x in g.items() if x is not None})
    assert len([k for k in outs["nan"] if k.startswith("d_")]) == 7
    for k, a in outs["nan"].items():
        if binned and k == "d_features":
            # the one documented exception: the binned path adds the feature gradient up with float atomics, so it repeats from
            # run to run only to rounding (test_two_backwards_give_the_same_bits holds it to rtol 1e-4, and so does this)
            util.assert_close(f"{name} {k}", a.cpu().numpy(), outs["cull"][k].cpu().numpy(), rtol=1e-4)
        else:
            _same(f"{name} {k}", a, outs["cull"][k])
        if a.is_floating_point():
            _clean(f"{name} {k}", a)
    assert not outs["nan"]["radii"][:, rows].any()
    for k, a in outs["nan"].items():
        if k.startswith("d_"):
            _positive_zero(f"{name} {k}", a[:, rows])
    # forward + backward as one call, three rounds through a workspace (the later ones replay the records)
    one = {}
    for key, run in (("nan", nan), ("cull", cull)):
        ws = R.Workspace()
        for _ in range(3):
            out = R.forward_backward_views(run.views, *run.args, run.dLc, run.dLi, bg=run.bg, force_binned=c.force_binned, workspace=ws)
        torch.cuda.synchronize()
        one[key] = dict(color=out[0].clone(), inv=out[1].clone(), radii=out[2].clone(), **{f"d_{k}": x.clone() for k, x in out[4].items() if x is not None})
    for k, a in one["nan"].items():
        if binned and k == "d_features":
            continue
        _same(f"{name} one call {k}", a, one["cull"][k])
        if k in outs["nan"]:
            _same(f"{name} one call against two calls {k}", a, outs["nan"][k])
    # the prefilled forms (the wave-resident small path only: sks_backward_prefill refuses every other shape): the replayed
    # backward zeroes planes of the next forward's output set
    if not binned and cull.regime["bwd"] == _lib.BWD_WAVE:
        pre = {}
        for key, run in (("nan", nan), ("cull", cull)):
            ws = R.Workspace(prefill=(5, 3))
            for _ in range(3):
                color, inv, radii, st = R.forward_views(run.views, *run.args, workspace=ws)
                g = R.backward_views(st, *run.args, run.dLc, run.dLi, bg=run.bg, workspace=ws)
            assert ws._pf is not None and ws._pf.note is not None, "the backward did not prefill"
            torch.cuda.synchronize()
            pre[key] = dict(color=color.clone(), inv=inv.clone(), radii=radii.clone(), **{f"d_{k}": x.clone() for k, x in g.items() if x is not None})
        for k, a in pre["nan"].items():
            _same(f"{name} prefilled {k}", a, pre["cull"][k])
            _same(f"{name} prefilled against plain {k}", a, outs["nan"][k])


def _records(st):
    """the (view, Gaussian) records of a geometry pass, as raw bytes per segment (padding between segments is never written)"""
    n = st.views.V * st.P * 16
    seg = (n + 255) // 256 * 256
    return [st.geom[k * seg:k * seg + n].clone() for k in range(3)] + [st.radii.clone()]


def _dv_views(cams, device):
    """A ViewBatch whose per-view scalars live in a device table (what a frame batch over a rig bank hands the *_dv entry points)."""
    from skelsplat_amd.rigs import RigBank, RigSelection
    bank = RigBank([cams], device)
    sz = bank.sizes
    vb = R.ViewBatch(bank.viewmatrix_dev[0].clone(), bank.projmatrix_dev[0].clone(), bank.tan[0, :, 0].tolist(), bank.tan[0, :, 1].tolist(),
                     max(s[0] for s in sz), max(s[1] for s in sz), sz)
    sel = RigSelection(bank, 1, vb.viewmatrix, vb.projmatrix)
    vb.table = sel.table
    sel.select([0])
    return vb, sel


@pytest.mark.parametrize("name", NC.NAMES)
def test_nan_rows_in_the_geometry_pass(device, name):
    """sks_geometry, sks_geometry_dv and frame-stacked parameters (vf > 0) with the NaN in one frame only: the records and radii of
    the NaN rows are those of the culled rows, every other record -- the other frame's included -- keeps its bits."""
    c, cull, nan = _runs(name, device)
    rows = list(c.rows)
    cams = [cam.to(device) for cam in c.cull.cams]
    geo = lambda views, means, frames=1, rest=cull.args: R.geometry_views(views, means, c.C, rest[2], rest[3], rest[4], None, frames=frames)
    a, b = _records(geo(cull.views, nan.args[0])), _records(geo(cull.views, cull.args[0]))
    for k, (x, y) in enumerate(zip(a, b)):
        _same(f"{name} sks_geometry segment {k}", x, y)
    assert not a[3][:, rows].any()
    for v in range(c.V):
        assert np.array_equal(a[3][v].cpu().numpy(), cull.fwd[v]["radii"])
    dv, sel = _dv_views(cams, device)
    for k, (x, y) in enumerate(zip(_records(geo(dv, nan.args[0])), a)):
        _same(f"{name} sks_geometry_dv segment {k}", x, y)
    sel.check()
    if c.V * 2 <= _lib.SKS_MAX_VIEWS:
        two = R.ViewBatch.from_cameras(cams + cams)
        stack = lambda t0, t1: torch.stack([t0, t1]).contiguous()
        clean_means = torch.tensor(NC.get(name).cull.means, device=device)       # frame 0: the culled form, finite
        rest = (None, None, stack(cull.args[2], cull.args[2]), stack(cull.args[3], cull.args[3]), stack(cull.args[4], cull.args[4]))
        f_nan = _records(geo(two, stack(clean_means, nan.args[0]), frames=2, rest=rest))
        n = c.V * c.P * 16
        for k in range(3):
            _same(f"{name} frames: segment {k} of the clean frame", f_nan[k][:n], b[k])
            _same(f"{name} frames: segment {k} of the frame with the NaN", f_nan[k][n:], b[k])
        _same(f"{name} frames: radii", f_nan[3], torch.cat([b[3], b[3]]))


def _fused_case(c, form, gt, hm):
    fc = FC.FusedLossCase()
    fc.name, fc.seed, fc.scene = c.name, c.seed, form.scene
    fc.means, fc.feat, fc.opac, fc.scales, fc.quats = form.means, form.feat, form.opac, form.scales, form.quats
    fc.cov, fc.cams, fc.ocams = None, list(form.cams), list(form.ocams)
    fc.bg, fc.aa, fc.smod, fc.bounds, fc.claims, fc.hm, fc.gt = None, False, 1.0, True, {"culled"}, hm, gt
    return fc


FUSED = tuple(n for n in NC.NAMES if NC.regime_of(n) in ("p17", "p17-v9"))       # (the sparse step takes up to 64 Gaussians)


@pytest.mark.parametrize("name", FUSED)
def test_nan_rows_in_the_fused_loss_step(device, name):
    """sks_geometry + sks_backward_fused_loss (P <= 64), heat-maps as planes and as factors: tests/fuzz_cases.run_hard_loss_case
    with the NaN rows on the device against the CPU reference of the culled scene (mask counts exactly, loss sums, gradients within
    the oracle's bound, every workgroup count, the dense device path), then NaN rows against culled rows bit for bit."""
    from tests.fuzz_cases import run_hard_loss_case
    from skelsplat_amd.heatmaps import heatmap_factors
    c, cull, nan = _runs(name, device)
    rows = list(c.rows)
    rng = np.random.default_rng(c.seed + 7000)
    gt = FC._planes(rng, c.C, [(c.W, c.H)] * c.V)
    fc_n, fc_c = _fused_case(c, c.nan, gt, None), _fused_case(c, c.cull, gt, None)
    refs = FR.case_reference(fc_c)
    seen = run_hard_loss_case(c.seed, device, case=fc_n, refs=refs)
    SEEN["fused_excess"] = max(SEEN["fused_excess"], seen["grad_excess"])
    print(f"{name}: fused-loss gradient excess {seen['grad_excess']:.2f} x 2^-24 x sum|terms| (so far {SEEN['fused_excess']:.2f})")
    # planes and factors, NaN rows against culled rows
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=device)
    sc = c.cull.scene
    hm = [t(np.asarray(sc.pose_3d_gt)[:c.C]), t(np.exp(rng.normal(4.0, 0.2, (c.C, 3)))), t(np.tile([1.0, 0, 0, 0], (c.C, 1))),
          t(np.asarray(sc.poses_2d)[:, :c.C])]
    cams = [cam.to(device) for cam in c.cull.cams]
    fac = R.HeatmapFactors(c.V, c.C, c.W, c.H, device)
    heatmap_factors(*hm, cams, views=cull.views, out=fac)
    fst = R.GtStats.of_factors(fac)
    fac.totals(cull.views, fst.totals)
    pst = R.gt_tile_stats(torch.stack([t(g) for g in gt]))
    for what, stats in (("planes", pst), ("factors", fst)):
        res = []
        for run in (nan, cull):
            st = R.geometry_views(run.views, run.args[0], c.C, run.args[2], run.args[3], run.args[4], None)
            packed = torch.full((c.V, c.P, 11), NAN, device=device)
            g, sums = R.backward_fused_loss(st, stats, *run.args, packed_out=packed)
            torch.cuda.synchronize()
            res.append(dict(sums=sums.clone(), packed=packed.clone(), **{k: x.clone() for k, x in g.items() if x is not None}))
        for k, a in res[0].items():
            _same(f"{name} fused loss, {what}: {k}", a, res[1][k])
            _clean(f"{name} fused loss, {what}: {k}", a)
            if k != "sums":
                _positive_zero(f"{name} fused loss, {what}: {k}", a[:, rows])


# ------------------------------------------------------------------------------------------------------------ 3b
def _hm_inputs(device):
    sc, model = NC.loop_scene(device)
    gm = model(device)
    means = torch.tensor(np.asarray(sc.pose_3d_init), dtype=torch.float32, device=device)
    p2d = torch.tensor(np.asarray(sc.poses_2d), dtype=torch.float32, device=device)
    return sc, means, gm.get_scaling.detach().clone(), gm._rotation.detach().clone(), p2d


HM_KINDS = {"mean": (lambda m, p, j: m[j].fill_(NAN), None), "mean-y": (lambda m, p, j: m[j, 1:2].fill_(NAN), None),
            "det-x": (lambda m, p, j: p[1, j, 0:1].fill_(NAN), 1), "det-y": (lambda m, p, j: p[2, j, 1:2].fill_(NAN), 2),
            "det-xy": (lambda m, p, j: p[0, j].fill_(NAN), 0)}


@pytest.mark.parametrize("dv", [False, True], ids=["by-value", "dv"])
@pytest.mark.parametrize("kind", list(HM_KINDS))
def test_heatmap_factors_of_a_plane_without_an_impulse(device, kind, dv):
    """sks_heatmap_factors(_dv), sks_heatmap_totals(_dv), sks_heatmaps, called directly: a NaN mean (all coordinates, y only) zeroes
    the joint's plane in every view, a non-finite detection (x, y, both) the plane of its view -- row, col, cmin exactly 0, den
    exactly 1e-8, the planes all zero; every other plane's factors keep the clean call's bits; a view's totals are those of the
    call without that plane; and the twin (oracle/heatmaps_ref.py) says the same."""
    from skelsplat_amd.heatmaps import heatmap_factors, heatmap_planes
    from oracle import heatmaps_ref as HR
    sc, means, scaling, rot, p2d = _hm_inputs(device)
    V, Jn, W, H = len(sc.cameras), NC.J, sc.W, sc.H
    j = NC.MISSING
    if dv:
        views, sel = _dv_views(list(sc.cameras), device)
    else:
        views = R.ViewBatch.from_cameras(sc.cameras)

    def call(m, p, drop=None):
        fac = R.HeatmapFactors(V, Jn, W, H, device)
        for t_ in (fac.row, fac.col, fac.cmin, fac.den):
            t_.fill_(NAN)
        heatmap_factors(m, scaling, rot, p, sc.cameras, views=views, out=fac, drop_mask=drop)
        tot = fac.totals(views, torch.zeros((V, 2), dtype=torch.float64, device=device))
        planes = heatmap_planes(fac.row, fac.col, fac.cmin, fac.den)
        torch.cuda.synchronize()
        return fac, tot, planes
    clean, tot_clean, planes_clean = call(means, p2d)
    m, p = means.clone(), p2d.clone()
    poison, view = HM_KINDS[kind]
    poison(m, p, j)
    got, tot, planes = call(m, p)
    gone = torch.zeros((V, Jn), dtype=torch.bool, device=device)
    gone[:, j] = True
    if view is not None:
        gone[:] = False
        gone[view, j] = True
    for v in range(V):
        if bool(gone[v, j]):
            NR.zero_plane_factors(got.row, got.col, got.cmin, got.den, v, j)
            assert not planes[v, j].any()
    for name, a, b in (("row", got.row, clean.row), ("col", got.col, clean.col), ("cmin", got.cmin, clean.cmin), ("den", got.den, clean.den)):
        assert torch.equal(a[~gone], b[~gone]), f"{kind}: {name} of another plane changed"
        _clean(name, a)
    assert torch.equal(planes[~gone], planes_clean[~gone]) and not torch.isnan(planes).any()
    # the totals: those of the call without that plane (a dropped plane: row = 0, cmin = 0, den = 1 -- all zero as well)
    _, tot_dropped, _ = call(means, p2d, drop=gone.cpu())
    assert torch.equal(tot, tot_dropped), (tot, tot_dropped)
    hit = [v for v in range(V) if bool(gone[v, j])]
    assert all(float(tot_clean[v, 1] - tot[v, 1]) > 0 for v in hit), "the plane had nothing to lose"
    assert all(torch.equal(tot[v], tot_clean[v]) for v in range(V) if v not in hit)
    # the twin
    t_row, t_col, t_cmin, t_den = HR.heatmap_factors(m.cpu(), scaling.cpu(), rot.cpu(), p.cpu(), [copy.copy(cam).to("cpu") for cam in sc.cameras])
    for v in hit:
        NR.zero_plane_factors(t_row, t_col, t_cmin, t_den, v, j)
    for name, a, b in (("row", got.row, t_row), ("col", got.col, t_col), ("cmin", got.cmin, t_cmin), ("den", got.den, t_den)):
        util.assert_close(f"{kind} {name} against the twin", a.cpu(), b, rtol=2e-5, atol_scale=1e-6)
    if dv:
        sel.check()


# ------------------------------------------------------------------------------------------------------------ 3d
ITERS = 32
ES_ITERS = 40
# window == views: a loss faces the same view's loss one group earlier.  The tolerance is chosen on the masked literal loop's own
# losses (CPU, tests/nan_joint_ref.masked_literal_loop from a numpy DLT of the same detections): the four differences of a window
# fall below 5e-4 between iterations 8 and 20 in every frame, at 14 in the poisoned one -- inside a group, past the first window
ES_WINDOW, ES_TOL = 4, 5e-4


def _state(fb, f):
    V = fb.V
    out = [fb.xyz[f], fb.scaling[f], fb.rotation[f], fb.opacity[f], fb.exp_avg[f], fb.exp_avg_sq[f], fb.accumulated_grads[f],
           fb.counters[f], fb._sums[f * V:(f + 1) * V]]
    if fb._es_state is not None:
        out.append(fb._es_state[f])
    return [t.clone() for t in out]


def _batch(device, poisoned, use_graph=False, factored=True, es=False, rigs=False, explicit=False, **kw):
    """The four frames of nan_joint_cases.loop_frames through one FrameBatchLoop; `poisoned`: frame POISONED has joint MISSING
    dropped in every view but one (or, `explicit`, NaN in explicit points); else the same batch with that frame clean."""
    from skelsplat_amd.loop import FrameBatchLoop, OptEarlyStopping
    from skelsplat_amd.rigs import RigBank
    from skelsplat_amd.triangulation import triangulate_sequence
    sc, model = NC.loop_scene(device)
    p2d, drop, clean = NC.loop_frames(sc)
    F = NC.LOOP_F
    if es:
        kw["early_stopping"] = OptEarlyStopping(window_size=ES_WINDOW, repeat_tolerance=ES_TOL)
    rig_ids = None
    if rigs:        # the poisoned frame on a rig of its own: other cameras, its detections those of that rig's scene
        sc2, _ = NC.loop_scene(device, seed=10)
        p2d = p2d.copy()
        p2d[NC.POISONED] = np.asarray(sc2.poses_2d, np.float32)
        bank = RigBank([sc.cameras, sc2.cameras])
        fb = FrameBatchLoop(model(device), rigs=bank.to(device), frames=F, dataset="h36m", use_graph=use_graph, factored=factored, **kw)
        rig_ids = [1 if f == NC.POISONED else 0 for f in range(F)]
    else:
        fb = FrameBatchLoop(model(device), sc.cameras, F, dataset="h36m", use_graph=use_graph, factored=factored, **kw)
    if explicit:
        pts = triangulate_sequence(fb._proj, torch.tensor(p2d, device=device)).to(torch.float32).clone()
        assert tuple(pts.shape) == (F, NC.J, 3) and bool(torch.isfinite(pts).all())
        if poisoned:
            pts[NC.POISONED, NC.MISSING] = NAN
        fb.new_scenes(pts, poses_2d=p2d)
    else:
        fb.new_scenes(None, poses_2d=p2d, drop_masks=drop if poisoned else clean, rig_ids=rig_ids)
    return sc, model, fb, p2d


def _check_frame(fb, poisoned):
    x = fb.xyz[NC.POISONED]
    others = [p for p in range(NC.J) if p != NC.MISSING]
    assert bool(torch.isfinite(x[others]).all()) and bool(torch.isfinite(fb.xyz[[f for f in range(fb.F) if f != NC.POISONED]]).all())
    assert bool(torch.isnan(x[NC.MISSING]).all()) == poisoned
    if poisoned:      # it stays NaN; its Adam moments stay 0 (all eleven columns: its other parameters never move either)
        assert not fb.exp_avg[NC.POISONED, NC.MISSING].any() and not fb.exp_avg_sq[NC.POISONED, NC.MISSING].any()
        assert torch.equal(fb.scaling[NC.POISONED, NC.MISSING], fb._init[0][0, NC.MISSING])
        assert not fb.accumulated_grads[NC.POISONED, :, NC.MISSING].any()


@pytest.mark.parametrize("es", [False, True], ids=["run-to-end", "early-stopping"])
@pytest.mark.parametrize("factored", [True, False], ids=["factors", "planes"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_the_other_frames_of_a_batch_do_not_change(device, use_graph, factored, es):
    """F = 4 frames, 32 iterations; frame 2 has joint 13 kept in one view only (new_scenes(None, ...) gives it no triangulation).
    Frames 0, 1 and 3 end with the bits they have in the same batch with frame 2 clean: joints, parameters, moments, slots,
    counters, loss sums, criterion state."""
    res = {}
    for poisoned in (True, False):
        sc, model, fb, _ = _batch(device, poisoned, use_graph=use_graph, factored=factored, es=es)
        start = fb.xyz.clone()
        fb.run(ITERS, groups_per_graph=4)
        torch.cuda.synchronize()
        _check_frame(fb, poisoned)
        res[poisoned] = ([_state(fb, f) for f in range(fb.F)], fb.stopped_at, start)
    for f in range(NC.LOOP_F):
        if f != NC.POISONED:
            assert res[True][1][f] == res[False][1][f]
            for k, (a, b) in enumerate(zip(res[True][0][f], res[False][0][f])):
                assert torch.equal(a, b), (f, k)
            assert not torch.equal(res[True][0][f][0], res[True][2][f]), "the frame did not move"
    # the frame itself moved too, and not like the clean frame
    assert not torch.equal(torch.nan_to_num(res[True][0][NC.POISONED][0]), torch.nan_to_num(res[True][2][NC.POISONED]))
    print(f"stopped at: with the unobserved joint {res[True][1]}, clean {res[False][1]}")


def test_the_other_frames_with_explicit_nan_points_and_on_a_rig_of_their_own(device):
    """The same isolation with the NaN in explicit `points`, and with the poisoned frame seen by its own rig of a RigBank (the
    *_dv entry points)."""
    for kw in (dict(explicit=True), dict(rigs=True), dict(rigs=True, es=True, use_graph=True)):
        res = {}
        for poisoned in (True, False):
            sc, model, fb, _ = _batch(device, poisoned, **kw)
            fb.run(ITERS, groups_per_graph=4)
            torch.cuda.synchronize()
            fb.check_rigs()
            _check_frame(fb, poisoned)
            res[poisoned] = [_state(fb, f) for f in range(fb.F)]
        for f in range(NC.LOOP_F):
            if f != NC.POISONED:
                for k, (a, b) in enumerate(zip(res[True][f], res[False][f])):
                    assert torch.equal(a, b), (kw, f, k)


def test_the_other_frames_of_a_pipeline_do_not_change(device):
    """N = 5 frames through FramePipeline, 2 loops of 2 frames on 2 streams, the last batch padded: the four clean frames end
    bit-identical to the sequence with frame 2 clean; frame 2's joint stays NaN, its other joints are finite."""
    from skelsplat_amd.loop import FramePipeline
    from skelsplat_amd.triangulation import triangulate_sequence, device_projection_matrices
    sc, model = NC.loop_scene(device)
    p2d, _, _ = NC.loop_frames(sc, n=5)
    pts = triangulate_sequence(device_projection_matrices(sc.cameras, device), torch.tensor(p2d, device=device)).to(torch.float32).clone()
    outs = {}
    for poisoned in (True, False):
        x = pts.clone()
        if poisoned:
            x[NC.POISONED, NC.MISSING] = NAN
        pipe = FramePipeline(model(device), sc.cameras, frames=2, streams=2, dataset="h36m")
        outs[poisoned] = pipe.optimize_sequence(x, p2d, iterations=ITERS, groups_per_graph=4, interleave=8).clone()
        torch.cuda.synchronize()
    keep = [f for f in range(5) if f != NC.POISONED]
    assert torch.equal(outs[True][keep], outs[False][keep])
    assert bool(torch.isnan(outs[True][NC.POISONED, NC.MISSING]).all())
    assert bool(torch.isfinite(outs[True][NC.POISONED, [p for p in range(NC.J) if p != NC.MISSING]]).all())
    assert not torch.equal(outs[True][keep], pts[keep])


def test_the_frame_follows_the_masked_literal_loop(device):
    """The sixteen observed joints of the poisoned frame against tests/ref_loop.run_reference_loop(missing={13}) from the same
    initial joints and heat-map planes, at the two bars of test_loop_matches_reference_loop: under 0.5 mm and under 0.02 x the
    distance moved.  Measured (MEASUREMENTS.md, "unobserved joints"): see the printed line."""
    sc, model, fb, p2d = _batch(device, True)
    V, f = fb.V, NC.POISONED
    start = fb.xyz[f].clone().cpu()
    hm = torch.stack([fb.factors.planes(f * V + v) for v in range(V)]).cpu()
    assert bool(torch.isnan(start[NC.MISSING]).all()) and not hm[:, NC.MISSING].any()
    fb.run(ITERS)
    torch.cuda.synchronize()
    got = fb.xyz[f].cpu()
    want, moved = NR.masked_literal_loop(sc, model, start, hm, ITERS, {NC.MISSING})
    others = [p for p in range(NC.J) if p != NC.MISSING]
    diff = float((got[others] - want[others]).norm(dim=1).max())
    print(f"\nunobserved joint, {ITERS} iterations: observed joints moved {moved:.3f} mm, HIP loop vs masked literal loop {diff:.3e} mm")
    assert moved > 0.05, moved
    assert diff < 0.5 and diff < 0.02 * max(moved, 1.0), (diff, moved)
    assert bool(torch.isnan(got[NC.MISSING]).all()) and bool(torch.isnan(want[NC.MISSING]).all())


def test_the_multi_view_loop_paths_agree_on_the_poisoned_frame(device):
    """MultiViewLoop.new_scene(points with the NaN, poses_2d) through the sparse fused step, the separate device tail, the dense
    loop and the tensor-op tail (loss_grad=masked_l2_grad_torch): fused == separate bit for bit (as
    test_fused_step_tail_equals_separate_kernels), sparse vs dense and device vs tensor-op tail within 2e-3 of the distance moved
    (as test_sparse_loop_equals_dense_loop / test_device_tail_loop_matches_tensor_op_tail); the frame batch equals the fused step."""
    from skelsplat_amd.loop import MultiViewLoop, masked_l2_grad_torch
    sc, model, fb, p2d = _batch(device, True)
    f = NC.POISONED
    start = fb.xyz[f].clone()
    fb.run(ITERS)
    modes = {"fused": dict(sparse=True, fused_tail=True), "separate": dict(sparse=True, fused_tail=False), "dense": dict(sparse=False),
             "tensor-op": dict(loss_grad=masked_l2_grad_torch)}
    out = {}
    for name, kw in modes.items():
        gm = model(device)
        loop = MultiViewLoop(gm, sc.cameras, torch.zeros((fb.V, NC.J, sc.H, sc.W), device=device), dataset="h36m", **kw)
        assert loop.device_tail == (name != "tensor-op") and loop.sparse == (name in ("fused", "separate"))
        loop.new_scene(start, poses_2d=torch.tensor(p2d[f], device=device))
        loop.run(ITERS)
        torch.cuda.synchronize()
        out[name] = gm._xyz.detach().clone()
        assert bool(torch.isnan(out[name][NC.MISSING]).all())
    others = [p for p in range(NC.J) if p != NC.MISSING]
    for name in out:
        assert bool(torch.isfinite(out[name][others]).all()), name
    moved = float((out["tensor-op"][others] - start[others]).norm(dim=1).mean())
    assert moved > 1.0, moved
    assert torch.equal(out["fused"][others], out["separate"][others])
    for a, b in (("separate", "dense"), ("separate", "tensor-op")):
        d = float((out[a][others] - out[b][others]).norm(dim=1).max())
        print(f"{a} vs {b}: {d:.3e} mm of {moved:.3f} mm moved")
        assert d < 2e-3 * moved, (a, b, d, moved)
    # the frame batch's planes-free path: same joints as the fused step up to the fp64 totals' last bits (tests/test_frames_es_gpu.py)
    d = float((fb.xyz[f][others] - out["fused"][others]).norm(dim=1).max())
    assert d < 2e-3 * moved, d


def test_early_stopping_of_the_poisoned_frame_follows_the_host_criterion(device):
    """The device criterion of the poisoned frame fires at the iteration at which the host OptEarlyStopping fires when fed the
    loop's own reported losses (report.trace_losses) plus the limb term of the masked model, float32(lambda x loss without the
    arm pair) of the joints before each step -- and it does fire: with the arm pair's NaN length in the loss, every loss would
    be NaN and the frame could never stop."""
    sc, model, fb, _ = _batch(device, True, es=True, report_steps=ES_ITERS // 4 + 2)
    f, V = NC.POISONED, fb.V
    crit = tail_ref.EsRef(ES_WINDOW, ES_TOL)
    want = 0
    while fb.iteration < ES_ITERS and not fb._all_stopped():
        torch.cuda.synchronize()
        before, n0 = fb.xyz[f].clone(), int(fb.counters[f, 1])
        fb.step_group(parameters_untouched=True)
        torch.cuda.synchronize()
        if want or int(fb.counters[f, 1]) == n0:
            continue
        cons = NR.masked_cons32(before, fb.lambda_consistency, {NC.MISSING})
        row = fb.trace_losses[f, n0 + 1].cpu().numpy()
        assert np.isfinite(row).all() and np.isfinite(cons)
        for v in range(V):          # (V == accumulation_steps: a group renders views 0 .. V-1 in order)
            want = want or crit.feed(float(np.float32(np.float32(row[v]) + np.float32(cons))))
    stops = fb.stopped_at
    print(f"stopped at {stops}; the host criterion on the poisoned frame's reported losses: {want}")
    assert want > 2 * ES_WINDOW, "the host criterion fires in its first window or never within the run: the case shows nothing"
    assert stops[f] == want, (stops, want)
