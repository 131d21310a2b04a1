"""Per-step pose errors, snapshots and sequence MPJPE on the device (csrc/sks_report.hip, skelsplat_amd/report.py, the report
launch of FrameBatchLoop / FramePipeline): the kernels against float64 references within allowances counted from their order of
operations (tests/report_ref.py), the loop's traces bit for bit against what an eager caller reads group by group, and no side
effect on the optimisation."""
import ctypes

import numpy as np
import pytest
import torch

from tests import report_ref as rr

pytestmark = pytest.mark.gpu

V, J = 4, 17
TOL = 3e-4          # with these frames: stops inside groups and frames that run to the end (tests/test_frames_es_gpu.py)
ITERS = 160
ROWS = ITERS // 4 + 1
NOISE3, NOISE2 = 20.0, 2.0
F = 4


def _scene(dev, seed=9):
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    W, H = 160, 128
    sc = SyntheticScene("h36m", n_views=V, seed=seed, W=W, H=H, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5, device=dev)

    def model(device):
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9,
                                                scaling_modifier=1.0, device=device)
        gm.training_setup()
        return gm
    return sc, model


def _frames(sc, n, rng_seed=11):
    """the first n of five frames around the scene's pose; frame f has noise f x (NOISE3 mm, NOISE2 px)"""
    rng = np.random.default_rng(rng_seed)
    base3, base2 = np.asarray(sc.pose_3d_init, np.float32), np.asarray(sc.poses_2d, np.float32)
    pts = np.stack([base3 + rng.normal(0, NOISE3 * f, base3.shape) for f in range(5)]).astype(np.float32)
    p2d = np.stack([base2 + rng.normal(0, NOISE2 * f, base2.shape) for f in range(5)]).astype(np.float32)
    return pts[:n], p2d[:n]


def _check_preconditions(stops, iters):
    hit = [s for s in stops if s is not None]
    assert len(set(hit)) >= 2, stops                   # frames stop at different iterations
    assert any(s % 4 != 0 for s in hit), stops         # ... one of them inside an accumulation group
    assert any(s is None for s in stops), stops        # ... and one frame runs to the end
    assert all(s <= iters for s in hit), stops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """bit for bit, NaN included"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _state(fb):
    return [fb.xyz, fb.scaling, fb.rotation, fb.opacity, fb.exp_avg, fb.exp_avg_sq, fb.accumulated_grads, fb.counters, fb._sums]


class _World:
    def __init__(self, dev):
        self.dev = dev
        self.sc, self.model = _scene(dev)
        self.pts, self.p2d = _frames(self.sc, 5)
        self.gt = torch.as_tensor(np.asarray(self.sc.pose_3d_gt, np.float32), device=dev)[None].repeat(5, 1, 1).contiguous()

    def loop(self, frames=F, es=True, **kw):
        from skelsplat_amd.loop import FrameBatchLoop, OptEarlyStopping
        if es:
            kw["early_stopping"] = OptEarlyStopping(window_size=4, repeat_tolerance=TOL)
        return FrameBatchLoop(self.model(self.dev), self.sc.cameras, frames, dataset="h36m", **kw)

    def eager(self, es, **kw):
        """An eager loop stepped group by group to ITERS; returns it with the clones of xyz, counters and the loss sums after the
        initialisation ([0]) and after every group."""
        fb = self.loop(es=es, **kw)
        if kw.get("report_steps"):
            fb.set_ground_truth(self.gt[:F])
        fb.new_scenes(self.pts[:F], poses_2d=self.p2d[:F])
        hist = [(fb.xyz.clone(), fb.counters.clone(), None)]
        while fb.iteration < ITERS and not fb._all_stopped():
            fb.step_group(parameters_untouched=True)
            S, N = fb.last_losses
            hist.append((fb.xyz.clone(), fb.counters.clone(), (S.clone(), N.clone())))
        torch.cuda.synchronize()
        return fb, hist


@pytest.fixture(scope="module")
def world(device):
    return _World(device)


@pytest.fixture(scope="module")
def plain_es(world):
    """early stopping, eager, no reporting: the trajectory everything else is compared with"""
    fb, hist = world.eager(True)
    _check_preconditions(fb.stopped_at, ITERS)
    return fb, hist


@pytest.fixture(scope="module")
def reported_es(world):
    """the same with reporting on"""
    return world.eager(True, report_steps=ROWS, save_iterations=(0, 10, ITERS))


# ------------------------------------------------------------------------------------------------------------ 1. pose_errors
def _random_poses(N, P, seed, dev):
    """mm scale (+-3 000), errors from 1e-3 to 1e3 mm (log-uniform per joint)"""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(-3000.0, 3000.0, (N, P, 3)).astype(np.float32)
    mag = 10.0 ** rng.uniform(-3.0, 3.0, (N, P, 1))
    d = rng.normal(size=(N, P, 3))
    pred = (gt + mag * d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    return torch.as_tensor(pred, device=dev), torch.as_tensor(gt, device=dev)


def _assert_pose_errors(pj, mean, pred, gt):
    """allowance per joint: 2^-24 x (4 ||d|| + sum of |operands of the subtractions|); the mean against the float64 mean of the
    kernel's own per-joint values: (P + 2) x 2^-24 x mean (tests/report_ref.py counts both)"""
    p, g = pred.cpu().numpy(), gt.cpu().numpy()
    want, _ = rr.pose_errors_ref(p, g)
    got = pj.cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= rr.per_joint_allowance(p, g)).all(), np.abs(got - want).max()
    assert (np.abs(mean.cpu().numpy().astype(np.float64) - got.mean(axis=1)) <= rr.mean_allowance(got)).all()


@pytest.mark.parametrize("P", [1, 17, 19, 64, 65, 130])
@pytest.mark.parametrize("N", [1, 3, 70])
def test_pose_errors_against_float64(device, N, P):
    from skelsplat_amd.report import pose_errors
    pred, gt = _random_poses(N, P, 1000 * N + P, device)
    pj, mean = pose_errors(pred, gt, per_joint=True)
    assert tuple(pj.shape) == (N, P, 2) and tuple(mean.shape) == (N, 2)
    _assert_pose_errors(pj, mean, pred, gt)
    assert _same(pose_errors(pred, gt), mean)                   # without the per-joint output; and run to run
    assert float(pj[:, 0, 1].abs().max()) == 0.0                # the root joint's relative error
    # pred == gt: exactly 0
    pj0, mean0 = pose_errors(gt, gt.clone(), per_joint=True)
    assert int(_bits(pj0).abs().max()) == 0 and int(_bits(mean0).abs().max()) == 0
    # one NaN joint touches its own frame only
    f, p = N // 2, P - 1
    bad = pred.clone()
    bad[f, p, 1] = float("nan")
    pjn, meann = pose_errors(bad, gt, per_joint=True)
    assert bool(torch.isnan(meann[f]).all()) and bool(torch.isnan(pjn[f, p]).all())
    keep = torch.ones(N, dtype=torch.bool, device=device)
    keep[f] = False
    assert _same(meann[keep], mean[keep]) and _same(pjn[keep], pj[keep])
    if p > 0:
        assert _same(pjn[f, :p], pj[f, :p])
    # a single pose
    pj1, mean1 = pose_errors(pred[0], gt[0], per_joint=True)
    assert _same(pj1, pj[0]) and _same(mean1, mean[0])


# ----------------------------------------------------------------------------------------------------------------- 2. bounds
def test_report_rows_stay_inside_their_buffers(device):
    """Every output of sks_loop_report is a slice between canary rows of a larger buffer; 10 steps into a capacity of 5 rows:
    rows 0-4 are the errors and losses of their steps, nothing else is written."""
    from skelsplat_amd.report import loop_report, pose_errors
    Fr, P, Vv, cap, K = 3, 19, 4, 5, 3
    CAN = 777.0
    rng = np.random.default_rng(3)

    def canaried(*shape):
        big = torch.full((shape[0] + 2,) + shape[1:], CAN, dtype=torch.float32, device=device)
        return big, big[1:-1]
    big_te, te = canaried(Fr, cap, 2)
    big_tl, tl = canaried(Fr, cap, Vv)
    big_fe, fe = canaried(Fr, P, 2)
    big_sn, sn = canaried(Fr, K, P, 3)
    for t in (te, tl, fe, sn):
        t.fill_(float("nan"))
    gt = torch.as_tensor(rng.uniform(-3000, 3000, (Fr, P, 3)).astype(np.float32), device=device)
    counters = torch.zeros((Fr, 2), dtype=torch.int32, device=device)
    want_te, want_tl, want_sn, xs = {}, {}, {}, []
    saves = (0, 9, 36)                  # acc_steps 4: the states after 0, 2 and 9 steps
    for n in range(11):
        xyz = gt + torch.as_tensor(rng.normal(0, 30.0, (Fr, P, 3)).astype(np.float32), device=device)
        sums = torch.as_tensor(np.stack([rng.uniform(0, 50, Fr * Vv), rng.integers(0, 3, Fr * Vv) * 1000.0], 1), device=device)
        counters[:, 0], counters[:, 1] = 4 * n, n
        loop_report(counters, None, 0, xyz, gt, sums, 4, te, tl, fe, saves, sn)
        want_te[n] = pose_errors(xyz, gt)
        want_tl[n] = torch.as_tensor(rr.loss_row_ref(sums[:, 0].cpu().numpy(), sums[:, 1].cpu().numpy()), device=device).view(Fr, Vv)
        xs.append(xyz)
    for n in range(cap):
        assert _same(te[:, n], want_te[n]) and _same(tl[:, n], want_tl[n]), n
    assert _same(fe, pose_errors(xs[-1], gt, per_joint=True)[0])
    assert _same(sn[:, 0], xs[0]) and _same(sn[:, 1], xs[2]) and _same(sn[:, 2], xs[9])
    for big in (big_te, big_tl, big_fe, big_sn):
        assert bool((big[0] == CAN).all()) and bool((big[-1] == CAN).all())
    # no capacity at all, snapshots only: nothing but the slots is touched
    sn.fill_(float("nan"))
    counters[:, 1] = 2
    loop_report(counters, None, 0, xs[5], None, None, 4, None, None, None, saves, sn)
    assert _same(sn[:, 1], xs[5]) and bool(torch.isnan(sn[:, 0]).all()) and bool(torch.isnan(sn[:, 2]).all())
    assert bool((big_sn[0] == CAN).all()) and bool((big_sn[-1] == CAN).all())


def test_pose_errors_and_evaluation_stay_inside_their_buffers(device):
    """The C entry points write (N,P,2), (N,2) and (1 + n_groups, 2) and not a word more: canary rows on both sides."""
    from skelsplat_amd import _lib
    from skelsplat_amd.report import evaluate_sequence, pose_errors
    N, P, G, CAN = 3, 19, 2, 777.0
    pred, gt = _random_poses(N, P, 5, device)
    big_pj = torch.full((N + 2, P, 2), CAN, dtype=torch.float32, device=device)
    big_mean = torch.full((N + 2, 2), CAN, dtype=torch.float32, device=device)
    big_ev = torch.full((1 + G + 2, 2), CAN, dtype=torch.float64, device=device)
    ids = torch.tensor([0, 1, 0], dtype=torch.int32, device=device)
    lib, stream = _lib.load(), torch.cuda.current_stream(device).cuda_stream
    assert lib.sks_pose_errors(N, P, pred.data_ptr(), gt.data_ptr(), big_pj[1:].data_ptr(), big_mean[1:].data_ptr(), stream) == 0
    assert lib.sks_eval_sequence(N, P, pred.data_ptr(), gt.data_ptr(), ids.data_ptr(), G, None, big_ev[1:].data_ptr(), stream) == 0
    pj, mean = pose_errors(pred, gt, per_joint=True)
    ev = evaluate_sequence(pred, gt, groups=ids, n_groups=G)
    assert _same(big_pj[1:-1], pj) and _same(big_mean[1:-1], mean)
    assert torch.equal(big_ev[1:-1, 0], torch.cat([ev["abs"][None], ev["abs_groups"]]))
    assert torch.equal(big_ev[1:-1, 1], torch.cat([ev["rel"][None], ev["rel_groups"]]))
    for big in (big_pj, big_mean, big_ev):
        assert bool((big[0] == CAN).all()) and bool((big[-1] == CAN).all())


# ------------------------------------------------------------------------------------------- 3. + 6. eager trace, early stopping
def test_eager_trace_is_what_a_caller_reads_group_by_group(device, reported_es, plain_es):
    from skelsplat_amd.report import pose_errors
    fb, hist = reported_es
    gt = fb._report.gt
    stops = fb.stopped_at
    assert stops == plain_es[0].stopped_at
    te, tl = fb.trace_errors, fb.trace_losses
    assert tuple(te.shape) == (F, ROWS, 2) and tuple(tl.shape) == (F, ROWS, V) and tuple(fb.final_errors.shape) == (F, J, 2)
    seen = torch.zeros((F, ROWS), dtype=torch.bool)
    for xyz, counters, losses in hist:
        means = pose_errors(xyz, gt)
        for f in range(F):
            n = int(counters[f, 1])
            seen[f, n] = True
            assert _same(te[f, n], means[f]), (f, n)
            if losses is not None:
                S, N = losses
                want = (S[f] / N[f].clamp_min(1.0)).float()
                assert _same(tl[f, n], want), (f, n)
    assert bool(torch.isnan(tl[:, 0]).all())                    # no group leads to the initial row
    # early stopping: the last row is the frame's last step, everything behind it is NaN
    assert torch.equal(fb.steps, fb.counters[:, 1])
    for f in range(F):
        n = int(fb.steps[f])
        assert n == (ITERS // 4 if stops[f] is None else -(-stops[f] // 4))
        assert bool(seen[f, :n + 1].all()) and not bool(seen[f, n + 1:].any())
        assert not bool(torch.isnan(te[f, :n + 1]).any()) and bool(torch.isnan(te[f, n + 1:]).all())
        assert bool(torch.isnan(tl[f, n + 1:]).all())
    pj, _ = pose_errors(fb.xyz, gt, per_joint=True)
    assert _same(fb.final_errors, pj)
    # replays past the stop change nothing
    before = [t.clone() for t in (te, tl, fb.final_errors, fb.snapshots)]
    for _ in range(3):
        fb._report.launch(fb)
    torch.cuda.synchronize()
    for a, b in zip(before, (te, tl, fb.final_errors, fb.snapshots)):
        assert _same(a, b)


# ----------------------------------------------------------------------------------------------------------------- 4. graphs
def test_graphs_report_what_eager_reports(device, world):
    outs = []
    for use_graph in (False, True):
        fb = world.loop(es=False, use_graph=use_graph, report_steps=11, save_iterations=(0, 4, 10, 40))
        fb.set_ground_truth(world.gt[:F]).new_scenes(world.pts[:F], poses_2d=world.p2d[:F])
        fb.run(40, 4)
        torch.cuda.synchronize()
        assert (fb._multi is not None) == use_graph
        outs.append([t.clone() for t in (fb.trace_errors, fb.trace_losses, fb.final_errors, fb.snapshots, fb.steps, fb.xyz)])
    for k, (a, b) in enumerate(zip(*outs)):
        assert _same(a, b), k
    te = outs[1][0]
    assert not bool(torch.isnan(te).any()) and int(outs[1][4].min()) == 10


def test_graphs_report_what_eager_reports_with_early_stopping(device, world, reported_es):
    eager, _ = reported_es
    fb = world.loop(es=True, use_graph=True, report_steps=ROWS, save_iterations=(0, 10, ITERS))
    fb.set_ground_truth(world.gt[:F]).new_scenes(world.pts[:F], poses_2d=world.p2d[:F])
    fb.run(ITERS, 4)            # graphs of 4 groups replay past the stops
    torch.cuda.synchronize()
    assert fb._multi is not None and fb.stopped_at == eager.stopped_at
    for name in ("trace_errors", "trace_losses", "final_errors", "snapshots", "steps", "xyz"):
        assert _same(getattr(fb, name), getattr(eager, name)), name


def test_heat_map_planes_report_what_the_factors_report(device, world):
    """factored=False (heat-maps as planes, the path that also takes ready heat-maps): a reporting loop takes its ground truth,
    and every trace row is pose_errors of the joints an eager caller clones after that group, every loss row the loss of the
    sums it clones; then against the factored loop: bit-identical where the trajectories are, and in any case the same
    snapshots of iteration 0 and the same initial row."""
    from skelsplat_amd.report import pose_errors
    runs = []
    for factored in (False, True):
        fb = world.loop(es=False, factored=factored, report_steps=11, save_iterations=(0, 10, 40))
        assert bool(fb.size_groups) == (not factored)
        fb.set_ground_truth(world.gt[:F]).new_scenes(world.pts[:F], poses_2d=world.p2d[:F])
        assert _same(fb._report.gt, world.gt[:F])
        hist = [(fb.xyz.clone(), None)]
        while fb.iteration < 40:
            fb.step_group(parameters_untouched=True)
            S, N = fb.last_losses
            hist.append((fb.xyz.clone(), (S / N.clamp_min(1.0)).float()))
        torch.cuda.synchronize()
        for n, (xyz, loss) in enumerate(hist):
            assert _same(fb.trace_errors[:, n], pose_errors(xyz, world.gt[:F])), (factored, n)
            if loss is not None:
                assert _same(fb.trace_losses[:, n], loss), (factored, n)
        assert _same(fb.final_errors, pose_errors(fb.xyz, world.gt[:F], per_joint=True)[0])
        assert _same(fb.snapshots[:, 0], hist[0][0]) and _same(fb.snapshots[:, 1], hist[2][0]) and _same(fb.snapshots[:, 2], hist[10][0])
        first = [t.clone() for t in (fb.trace_errors, fb.final_errors, fb.snapshots)]
        # the next batch without a ground truth: NaN errors, losses and snapshots all the same
        fb.new_scenes(world.pts[:F], poses_2d=world.p2d[:F])
        fb.run(8)
        torch.cuda.synchronize()
        assert bool(torch.isnan(fb.trace_errors).all()) and not bool(torch.isnan(fb.trace_losses[:, 1:3]).any())
        assert _same(fb.snapshots[:, 0], hist[0][0])
        runs.append((hist, first))
    (planes, rep_planes), (factors, rep_factors) = runs
    assert _same(planes[0][0], factors[0][0]) and _same(rep_planes[0][:, 0], rep_factors[0][:, 0])
    # planes and factors describe the same heat-maps; where they give the same joints, group for group, the reports are the same bits
    if all(_same(a[0], b[0]) for a, b in zip(planes, factors)):
        for a, b in zip(rep_planes, rep_factors):
            assert _same(a, b)


# --------------------------------------------------------------------------------------------------------- 5. no side effect
@pytest.mark.parametrize("es", [False, True], ids=["no_stopping", "early_stopping"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_reporting_changes_nothing_of_the_optimisation(device, world, es, use_graph):
    iters = ITERS if es else 40
    res = []
    for kw in ({}, dict(report_steps=iters // 4 + 1, save_iterations=(0, 10, iters))):
        fb = world.loop(es=es, use_graph=use_graph, **kw)
        if kw:
            fb.set_ground_truth(world.gt[:F])
        fb.new_scenes(world.pts[:F], poses_2d=world.p2d[:F])
        fb.run(iters, 4)
        torch.cuda.synchronize()
        res.append([t.clone() for t in _state(fb)] + ([fb._es_state.clone()] if es else []))
        assert (fb._report is not None) == bool(kw)
    for k, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), k


# -------------------------------------------------------------------------------------------------------------- 7. snapshots
def test_snapshots_are_the_joints_of_a_fresh_run(device, world, plain_es):
    plain, hist = plain_es
    stops = plain.stopped_at
    inside = next(s for s in stops if s is not None and s % 4 != 0)
    saves = (0, 4, 10, 40, inside, inside + 1, ITERS)
    fb = world.loop(es=True, use_graph=True, save_iterations=saves)         # snapshots only: no ground truth, no traces
    assert fb.trace_errors is None and fb.final_errors is None
    fb.new_scenes(world.pts[:F], poses_2d=world.p2d[:F])
    fb.run(ITERS, 4)
    torch.cuda.synchronize()
    assert fb.stopped_at == stops
    snaps = fb.snapshots
    assert tuple(snaps.shape) == (F, len(saves), J, 3)
    n_nan = 0
    for f in range(F):
        for k, s in enumerate(saves):
            if stops[f] is not None and s > stops[f]:
                assert bool(torch.isnan(snaps[f, k]).all()), (f, s)       # the frame had stopped before iteration s
                n_nan += 1
            elif stops[f] is not None and s == stops[f]:
                assert _same(snaps[f, k], plain.xyz[f]), (f, s)           # the stop saves the final joints
            else:
                assert _same(snaps[f, k], hist[s // 4][0][f]), (f, s)     # (10 -> the state after 2 steps)
    assert n_nan >= 2 and _same(snaps[:, 0], torch.as_tensor(world.pts[:F], device=device))


# ---------------------------------------------------------------------------------------------------------- 8. FramePipeline
@pytest.mark.parametrize("es", [False, True], ids=["no_stopping", "early_stopping"])
def test_frame_pipeline_reports_every_frame_like_its_own_loop(device, world, es):
    from skelsplat_amd.loop import FramePipeline, OptEarlyStopping
    N = 5
    saves = (0, 10, ITERS)
    kw = dict(early_stopping=OptEarlyStopping(window_size=4, repeat_tolerance=TOL)) if es else {}
    pipe = FramePipeline(world.model(device), world.sc.cameras, frames=2, streams=2, dataset="h36m", report_steps=ROWS,
                         save_iterations=saves, **kw)
    pipe.set_ground_truth(world.gt)
    out = pipe.optimize_sequence(world.pts, world.p2d, iterations=ITERS, groups_per_graph=4, interleave=16)
    torch.cuda.synchronize()
    rep = pipe.report
    assert tuple(rep.trace_errors.shape) == (N, ROWS, 2) and tuple(rep.trace_losses.shape) == (N, ROWS, V)
    assert tuple(rep.final_errors.shape) == (N, J, 2) and tuple(rep.snapshots.shape) == (N, 3, J, 3) and tuple(rep.steps.shape) == (N,)
    for f in range(N):
        one = world.loop(frames=1, es=es, use_graph=True, report_steps=ROWS, save_iterations=saves)
        one.set_ground_truth(world.gt[f:f + 1]).new_scenes(world.pts[f:f + 1], poses_2d=world.p2d[f:f + 1])
        one.run(ITERS, 4)
        torch.cuda.synchronize()
        assert _same(out[f], one.xyz[0]), f
        assert _same(rep.trace_errors[f], one.trace_errors[0]) and _same(rep.trace_losses[f], one.trace_losses[0]), f
        assert _same(rep.final_errors[f], one.final_errors[0]) and _same(rep.snapshots[f], one.snapshots[0]), f
        assert int(rep.steps[f]) == int(one.steps[0])
        if es:
            assert int(pipe.stopped_at[f]) == (one.stopped_at[0] or 0)
    if es:
        assert len(set(rep.steps.tolist())) >= 2
    # the ground truth was taken by that sequence: without a new one the same loops report losses and snapshots, the errors are NaN
    out2 = pipe.optimize_sequence(world.pts, world.p2d, iterations=ITERS, groups_per_graph=4, interleave=16)
    torch.cuda.synchronize()
    assert _same(out2, out) and _same(pipe.report.snapshots, rep.snapshots) and _same(pipe.report.trace_losses, rep.trace_losses)
    assert bool(torch.isnan(pipe.report.trace_errors).all()) and bool(torch.isnan(pipe.report.final_errors).all())


# ------------------------------------------------------------------------------------------------------ 9. evaluate_sequence
def test_evaluate_sequence_against_float64(device):
    from skelsplat_amd.report import evaluate_sequence
    N, P, G = 70, 17, 3
    pred, gt = _random_poses(N, P, 77, device)
    rng = np.random.default_rng(78)
    groups = rng.integers(0, 2, N) * 2              # groups 0 and 2; group 1 is empty
    valid = rng.uniform(size=N) > 0.2
    assert (groups == 1).sum() == 0 and 0 < valid.sum() < N
    res = evaluate_sequence(pred, gt, groups=torch.as_tensor(groups, device=device), n_groups=G,
                            abs_valid=torch.as_tensor(valid, device=device))
    again = evaluate_sequence(pred, gt, groups=groups, abs_valid=valid, n_groups=G)     # ids and mask from the host
    got = torch.stack([torch.cat([res["abs"][None], res["abs_groups"]]), torch.cat([res["rel"][None], res["rel_groups"]])], 1)
    assert got.dtype == torch.float64 and tuple(got.shape) == (1 + G, 2)
    for k in res:
        assert torch.equal(res[k].view(torch.int64), again[k].view(torch.int64)), k       # bit-identical, NaN included
    p, g = pred.cpu().numpy(), gt.cpu().numpy()
    want = rr.eval_sequence_ref(p, g, groups, G, valid)
    # allowance: the float norms' (test 1's per-joint allowance, averaged over the row's joints) + N P 2^-53 relative for the sums
    allow_pj = rr.per_joint_allowance(p, g)
    got = got.cpu().numpy()
    for r in range(1 + G):
        sel = np.ones(N, bool) if r == 0 else groups == r - 1
        for c, rows in ((0, sel & valid), (1, sel)):
            if not rows.any():
                assert np.isnan(got[r, c]) and np.isnan(want[r, c])
                continue
            allow = allow_pj[rows, :, c].mean() + N * P * rr.U64 * want[r, c]
            assert abs(got[r, c] - want[r, c]) <= allow, (r, c, got[r, c], want[r, c], allow)
    assert np.isnan(got[2]).all()
    plain = evaluate_sequence(pred, gt)
    assert tuple(plain["abs_groups"].shape) == (0,)
    assert abs(float(plain["rel"]) - want[0, 1]) <= allow_pj[:, :, 1].mean() + N * P * rr.U64 * want[0, 1]


# -------------------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals(device, world):
    from skelsplat_amd import _lib
    from skelsplat_amd.loop import FrameBatchLoop, FramePipeline
    from skelsplat_amd.report import evaluate_sequence, pose_errors
    sc, model = world.sc, world.model
    with pytest.raises(ValueError, match="at most 8"):
        FrameBatchLoop(model(device), sc.cameras, 2, save_iterations=range(9))
    with pytest.raises(ValueError, match="save_iterations"):
        FrameBatchLoop(model(device), sc.cameras, 2, save_iterations=(4, -4))
    with pytest.raises(ValueError, match="report_steps"):
        FrameBatchLoop(model(device), sc.cameras, 2, report_steps=-1)
    fb = FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m", report_steps=5)
    pts, p2d = world.pts[:2], world.p2d[:2]
    gt = world.gt[:2]
    for bad, text in ((gt[:, :5], "frames,P,3"), (gt[0], "frames,P,3"), (gt.double(), "float32"), (gt.cpu(), "on cuda"),
                      (gt.cpu().numpy(), "tensor")):
        with pytest.raises(ValueError, match=text):
            fb.set_ground_truth(bad)
    with pytest.raises(ValueError, match="new_scenes.*must be"):          # one frame's ground truth for a batch of two
        fb.set_ground_truth(gt[:1]).new_scenes(pts, poses_2d=p2d)
    assert fb.set_ground_truth(gt).set_ground_truth(None)._gt_next is None     # withdrawn
    off = FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m")
    assert off._report is None and off.trace_errors is None and off.snapshots is None
    with pytest.raises(ValueError, match="reporting is off"):
        off.set_ground_truth(gt)
    snaps_only = FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m", save_iterations=(4,))
    with pytest.raises(ValueError, match="reporting is off"):
        snaps_only.set_ground_truth(gt)
    pipe = FramePipeline(model(device), sc.cameras, frames=2, streams=1, dataset="h36m", report_steps=5)
    with pytest.raises(ValueError, match="optimize_sequence.*must be"):   # three frames' ground truth for a sequence of two
        pipe.set_ground_truth(world.gt[:3]).optimize_sequence(pts, p2d, iterations=4)
    with pytest.raises(ValueError, match="float32"):
        pipe.set_ground_truth(gt.double())
    with pytest.raises(ValueError, match="float32"):
        pose_errors(gt.double(), gt.double())
    with pytest.raises(ValueError, match="must both be"):
        pose_errors(gt, gt[:1])
    with pytest.raises(ValueError, match="n_groups"):
        evaluate_sequence(gt, gt, groups=torch.zeros(2, dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="at most 64"):
        evaluate_sequence(gt, gt, groups=[0, 1], n_groups=65)
    # the C entry points: rc < 0 and a text, for NULL or mismatched pointers
    lib = _lib.load()
    x = gt.data_ptr()
    R, E, Pe = lib.sks_loop_report, lib.sks_eval_sequence, lib.sks_pose_errors
    for fn, args, text in ((Pe, (2, J, None, x, None, x, None), "pred"),
                           (Pe, (2, J, x, x, None, None, None), "mean"),
                           (R, (2, V, J, None, None, 0, x, None, None, 4, 0, None, None, None, 0, None, None, None), "counters"),
                           (R, (2, V, J, x, None, 0, x, x, None, 4, 5, x, None, None, 0, None, None, None), "final_err"),
                           (R, (2, V, J, x, None, 0, x, None, x, 4, 5, None, None, None, 0, None, None, None), "go together"),
                           (R, (2, V, J, x, None, 0, x, None, None, 4, 0, None, None, None, 9, x, x, None), "SKS_REPORT_MAX_SAVES"),
                           (E, (2, J, x, x, None, 2, None, x, None), "group_ids"),
                           (E, (2, J, x, x, None, 0, None, None, None), "out")):
        assert fn(*args) < 0, text
        assert text in lib.sks_last_error().decode(), text
    # the report entry points were added to ABI version 14 (the header says so): present, and the version has not gone back
    assert all(hasattr(lib, s) for s in ("sks_pose_errors", "sks_loop_report", "sks_eval_sequence")) and lib.sks_version() >= 14
