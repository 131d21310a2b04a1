"""csrc/sks_reproject.hip on the device, against the float64 restatement of tests/reproj_ref.py: sks_reproject within a rounding
allowance counted from the restatement's own magnitudes, sks_eval_reprojection with exact counts, sks_triangulate_refine at the
project's bar for joints with its iteration counts equal; every kernel bit for bit against itself across batch sizes, batch
positions, streams and rig forms; and the two switches of the loops (set_refinement, set_reprojection_report) through
FramePipeline."""
import numpy as np
import pytest
import torch

from skelsplat_amd import reprojection, triangulation
from tests import reproj_cases as RC
from tests import reproj_ref as REF
from tests import tri_cases as TC

pytestmark = pytest.mark.gpu

SEEN = {"uv": 0.0, "err": 0.0, "mean": 0.0}         # the largest fraction of an allowance the device used, printed per test


def _dev(a, device, dtype=None):
    return None if a is None else torch.as_tensor(a if dtype is None else np.asarray(a).astype(dtype), device=device)


def _np(t):
    return t.cpu().numpy()


def _hold(name, got, ref, allow, kind):
    got = _np(got)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), name
    diff = np.abs(np.nan_to_num(got) - np.nan_to_num(ref))
    with np.errstate(all="ignore"):
        frac = float(np.nanmax(np.where(diff > 0, diff / allow, 0.0)))
    SEEN[kind] = max(SEEN[kind], frac)
    assert np.all(diff <= allow), (name, frac)


def _check_reproject(device, P, X, det, valid, ref):
    got = reprojection.reproject(_dev(P, device), _dev(X, device), _dev(det, device), _dev(valid, device))
    allow_uv, allow_err = RC.pixel_allowances(ref)
    _hold("uv", got.uv, ref["uv"], allow_uv, "uv")
    _hold("err", got.err, ref["err"], allow_err, "err")
    assert got.in_front.dtype == torch.bool and np.array_equal(_np(got.in_front), ref["in_front"])
    assert got.n_used.dtype == torch.int32 and np.array_equal(_np(got.n_used), ref["n_used"])
    _hold("per_joint", got.per_joint, ref["per_joint"], RC.mean_allowance(ref["err"], allow_err, 1), "mean")
    _hold("per_view", got.per_view, ref["per_view"], RC.mean_allowance(ref["err"], allow_err, 2), "mean")
    n = ref["err"].shape[0]
    _hold("per_frame", got.per_frame, ref["per_frame"], RC.mean_allowance(ref["err"].reshape(n, -1), allow_err.reshape(n, -1), 1), "mean")
    return got


@pytest.mark.parametrize("J", RC.REPROJECT_JOINTS)
@pytest.mark.parametrize("V", RC.REPROJECT_VIEWS)
def test_reproject_against_the_restatement(device, V, J):
    P, X, det = RC.scene(V, J)
    full = _check_reproject(device, P, X, det, None, REF.reproject(P, X, det))
    # float joints and detections are widened exactly: the restatement of the rounded inputs
    X32, d32 = X.astype(np.float32), det.astype(np.float32)
    _check_reproject(device, P, X32, d32, None, REF.reproject(P, X32, d32))
    _check_reproject(device, P, X32, det, None, REF.reproject(P, X32, det))
    # one rig per frame
    rigs = RC.rigs_per_frame(P)
    _check_reproject(device, rigs, X, d32, None, REF.reproject(rigs, X, d32))
    # the mask that empties a joint, a view and a frame, a NaN detection, a joint behind a camera
    Ph, Xh, dh, valid, behind = RC.hard_reproject_case(V, J)
    ref = REF.reproject(Ph, Xh, dh, valid)
    got = _check_reproject(device, Ph, Xh, dh, valid, ref)
    assert not bool(got.in_front[behind]) and ref["u"][behind][2] < 0
    assert bool(torch.isnan(got.per_joint[0, J - 1])) and bool(torch.isnan(got.per_view[1, V - 1])) and bool(torch.isnan(got.per_frame[2]))
    assert bool(torch.isnan(got.err[0, 0, 0])) and int(got.n_used[2].sum()) == 0
    # project only, and a selection of the outputs
    only = reprojection.reproject(_dev(P, device), _dev(X, device), want=("uv", "in_front", "per_frame", "n_used"))
    assert torch.equal(only.uv, full.uv) and torch.equal(only.in_front, full.in_front) and only.err is None
    assert bool(torch.isnan(only.per_frame).all()) and int(only.n_used.sum()) == 0
    print(f"V = {V}, J = {J}: largest fraction of the allowance used so far:", SEEN)


@pytest.mark.parametrize("N", [1, 257, 600])
def test_eval_reprojection(device, N):
    V, J = 4, 17
    rng = np.random.default_rng(N)
    err = rng.uniform(0.5, 9.0, (N, V, J))
    err[rng.uniform(size=err.shape) < 0.2] = np.nan
    err[:, 2, :] = np.nan                           # a view nobody kept
    err[:, :, 5] = np.nan                           # ... and a joint
    groups = rng.integers(0, 3, N)
    groups[groups == 1] = 7                         # group 1 is empty, id 7 lies outside the range
    ref, cnt = REF.eval_reprojection(err, groups, 3)
    got = _np(reprojection.evaluate_sequence_reprojection(_dev(err, device), _dev(groups, device), n_groups=3))
    assert got.shape == (4, 1 + V + J)
    # the counts, through the placement of the NaNs: a mean is NaN exactly where nothing was counted
    assert np.array_equal(np.isnan(got), cnt == 0) and np.isnan(got[2]).all() and np.isnan(got[:, 3]).all() and np.isnan(got[:, 1 + V + 5]).all()
    assert cnt[0, 0] == (~np.isnan(err)).sum() and cnt[1, 0] + cnt[3, 0] == (~np.isnan(err[groups != 7])).sum()
    # a thread adds at most ceil(N / 256) frames x V x J terms one after the other, then 8 tree levels and the division: that
    # many roundings of the running sum on either side, relative to a mean of positive terms
    terms = -(-N // 256) * V * J + 8 + 1
    assert np.allclose(got, ref, rtol=2 * terms * RC.EPS, atol=0, equal_nan=True), np.nanmax(np.abs(got / ref - 1))
    plain = _np(reprojection.evaluate_sequence_reprojection(_dev(err, device)))
    assert plain.shape == (1, 1 + V + J) and np.array_equal(plain[0], got[0], equal_nan=True)


def _refine(device, P, det, valid, start, huber, **kw):
    return reprojection.refine_triangulation(_dev(P, device), _dev(det, device), _dev(start, device), valid=_dev(valid, device),
                                             huber_px=huber or None, return_cost=True, return_iters=True, **kw)


@pytest.mark.parametrize("kind", ["plain", "huber", "masks"])
@pytest.mark.parametrize("V", RC.REFINE_VIEWS)
def test_refine_against_the_restatement(device, V, kind):
    P, det, valid, start, huber = RC.refine_case(V, kind)
    X, cost, iters, near = REF.refine(P, det, valid, start, huber)
    got, gcost, giters = _refine(device, P, det, valid, start, huber)
    g = _np(got)
    assert got.dtype == torch.float64 and np.array_equal(np.isnan(g), np.isnan(X))
    print(f"V = {V} {kind}: max distance to the restatement {np.nanmax(np.abs(g - X)):.3g}, iterations {np.bincount(iters.ravel())}, "
          f"near ties {int(near.sum())}")
    assert np.allclose(g, X, equal_nan=True, **TC.GOLDEN_TOL)
    differ = _np(giters) != iters
    assert not np.any(differ & ~near) and near.sum() <= RC.NEAR_TIE_SHARE * near.size, (int(differ.sum()), int(near.sum()))
    c = _np(gcost)
    known = ~np.isnan(c[..., 0])
    assert np.all(c[known][:, 1] <= c[known][:, 0]) and int(giters.max()) <= 16
    still = _np(giters) == 0
    assert np.array_equal(g[still], start[still], equal_nan=True)
    # float32 start and detections: in place on the start (xyz aliases xyz0), the restatement of the rounded inputs rounded
    s32, d32 = start.astype(np.float32), det.astype(np.float32)
    X32 = REF.refine(P, d32, valid, s32, huber)[0]
    buf = _dev(s32, device)
    out = reprojection.refine_triangulation(_dev(P, device), _dev(d32, device), buf, valid=_dev(valid, device), huber_px=huber or None, out=buf)
    assert out is buf and buf.dtype == torch.float32
    assert np.allclose(_np(buf), X32.astype(np.float32), equal_nan=True, rtol=1e-6, atol=1e-3)     # (one float32 rounding of mm)
    # max_iters = 1 is one trip
    one, _, i1 = _refine(device, P, det, valid, start, huber, max_iters=1)
    r1 = REF.refine(P, det, valid, start, huber, max_iters=1)
    assert np.array_equal(_np(i1), r1[2]) and np.allclose(_np(one), r1[0], equal_nan=True, **TC.GOLDEN_TOL)


def test_refine_from_the_robust_triangulation(device):
    """A start from sks_triangulate_robust with valid = its inliers: the outlier view stays out of the refinement."""
    P, det, _, _, _ = RC.refine_case(5, "plain", seed=2)
    det[:, 3, ::2, :] += 60.0                                   # every other joint: view 3 is far off
    Pd, dd = _dev(P, device), _dev(det, device)
    start, inl, _ = triangulation.triangulate_sequence(Pd, dd, homogeneous=True, reject_px=15.0, return_inliers=True)
    start = start[..., :3].contiguous()
    assert not bool(inl[:, 3, ::2].any()) and bool(inl[:, 3, 1::2].all())
    got, cost, iters = reprojection.refine_triangulation(Pd, dd, start, valid=inl, return_cost=True, return_iters=True)
    X, rcost, riters, near = REF.refine(P, det, _np(inl), _np(start))
    assert np.allclose(_np(got), X, **TC.GOLDEN_TOL) and np.array_equal(_np(iters), riters) and not near.any()
    assert bool((cost[..., 1] < cost[..., 0]).all())
    blind = reprojection.refine_triangulation(Pd, dd, start)
    assert not torch.equal(blind, got)


@pytest.mark.parametrize("V", [4, 31])
def test_bit_for_bit_against_itself(device, V):
    """A frame alone, inside a batch of 3 and of 130 (more than one workgroup), at another place, on another stream, and with
    the one rig repeated per frame: the same bits from both kernels."""
    P, _, det3 = RC.scene(V, 17, seed=5)
    rng = np.random.default_rng(11)
    det = (det3[np.arange(130) % 3] + rng.normal(0, 1.0, (130,) + det3.shape[1:])).astype(np.float32)
    det[7, 1 % V, 3] = np.nan
    Pd, dd = _dev(P, device), _dev(det, device)
    start = triangulation.triangulate_sequence(Pd, dd)
    side = torch.cuda.Stream(device)

    def both(Pm, x, s):
        r = reprojection.reproject(Pm, s, x)
        f = reprojection.refine_triangulation(Pm, x, s, huber_px=10.0, return_cost=True, return_iters=True)
        return [r.uv, r.err, r.in_front, r.per_joint, r.per_view, r.per_frame, r.n_used, *f]

    def same(a, b):
        return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())
    whole = both(Pd, dd, start)
    for f in (0, 2, 7, 63, 64, 129):
        for lo, hi in ((f, f + 1), (max(0, f - 1), min(130, max(0, f - 1) + 3))):
            part = both(Pd, dd[lo:hi], start[lo:hi])
            for k, (a, b) in enumerate(zip(part, whole)):
                assert same(a[f - lo], b[f]), (f, lo, hi, k)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            other = both(Pd, dd[f:f + 1], start[f:f + 1])
        side.synchronize()
        for k, (a, b) in enumerate(zip(other, whole)):
            assert same(a[0], b[f]), (f, k)
    rigs = Pd[None].repeat(130, 1, 1, 1).contiguous()
    for k, (a, b) in enumerate(zip(both(rigs, dd, start), whole)):
        assert same(a, b), k


# ------------------------------------------------------------------------------------------------ through the pipeline
V, J, F, N, ITERS = 4, 17, 4, 9, 8


def _scene(dev, seed=9):
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    W, H = 160, 128
    sc = SyntheticScene("h36m", n_views=V, seed=seed, W=W, H=H, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5, device=dev)

    def model():
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9,
                                                scaling_modifier=1.0, device=dev)
        gm.training_setup()
        return gm
    return sc, model


def _detections(sc, n, dev, seed=11):
    rng = np.random.default_rng(seed)
    base = np.asarray(sc.poses_2d, np.float32)
    return torch.as_tensor(np.stack([base + rng.normal(0, 1.0 + 0.5 * f, base.shape) for f in range(n)]).astype(np.float32), device=dev)


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


def _check_report(pipe, P, p2d, initial, final):
    rep = pipe.reprojection
    a, b = reprojection.reproject(P, initial, p2d), reprojection.reproject(P, final, p2d)
    assert _same(rep.initial_err, a.err) and _same(rep.final_err, b.err) and _same(rep.final_uv, b.uv)
    assert _same(rep.per_joint, b.per_joint) and _same(rep.per_frame, b.per_frame)
    assert bool(torch.isfinite(rep.final_err).all()) and tuple(rep.initial_err.shape) == (p2d.shape[0], V, J)
    s = rep.summary()
    assert _same(s["final"], reprojection.evaluate_sequence_reprojection(b.err)) and tuple(s["initial"].shape) == (1, 1 + V + J)


@pytest.mark.parametrize("early_stopping", ["no_stopping", "opt_early_stopping"])
def test_pipeline_switches(device, early_stopping):
    """H36M, 4 views, 4 frames per launch on 2 streams, 9 frames (a padded last batch), 8 iterations."""
    from skelsplat_amd.loop import FramePipeline, OptEarlyStopping
    sc, model = _scene(device)
    p2d = _detections(sc, N, device)
    es = lambda: early_stopping if early_stopping == "no_stopping" else OptEarlyStopping(2, 1e-2)
    run = lambda pipe, pts=None: pipe.optimize_sequence(pts, p2d, iterations=ITERS, groups_per_graph=2, interleave=4, return_initial=True)
    never = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m", early_stopping=es())
    want, want_init = (t.clone() for t in run(never))
    assert never.reprojection is None
    P = never.loops[0]._proj
    pipe = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m", early_stopping=es())
    # the report alone: the joints are those of a pipeline that never had it
    assert pipe.set_reprojection_report() is pipe
    got, init = run(pipe)
    assert torch.equal(got, want) and torch.equal(init, want_init)
    _check_report(pipe, P, p2d, init, got)
    # the refinement as well: the initial joints are refine_triangulation(triangulate_sequence(..)), the report follows them
    assert pipe.set_refinement(16, huber_px=10.0) is pipe
    got, init = run(pipe)
    refined = reprojection.refine_triangulation(P, p2d, triangulation.triangulate_sequence(P, p2d), huber_px=10.0)
    assert torch.equal(init, refined) and not torch.equal(init, want_init)
    _check_report(pipe, P, p2d, init, got)
    assert float(pipe.reprojection.initial_err.mean()) < float(reprojection.reproject(P, want_init, p2d).err.mean())
    # ... and equals the run from these points given explicitly, which the refinement refuses while it is on
    with pytest.raises(ValueError, match="set_refinement"):
        run(pipe, refined)
    explicit = pipe.set_refinement(None).optimize_sequence(refined, p2d, iterations=ITERS, groups_per_graph=2, interleave=4)
    assert torch.equal(explicit, got)
    # both switches off again: what a pipeline that never had them computes, and no report
    pipe.set_reprojection_report(False)
    got, init = run(pipe)
    assert torch.equal(got, want) and torch.equal(init, want_init) and pipe.reprojection is None
    with pytest.raises(ValueError, match="max_iters"):
        pipe.set_refinement(17)


def test_pipeline_refines_over_the_inliers(device):
    from skelsplat_amd.loop import FramePipeline
    sc, model = _scene(device)
    p2d = _detections(sc, N, device).clone()
    p2d[:, 2, ::3, 0] += 50.0                                    # every third joint: view 2 is off by 50 px
    pipe = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m")
    pipe.set_outlier_rejection(12.0).set_refinement(8).set_reprojection_report()
    got, init = pipe.optimize_sequence(None, p2d, iterations=ITERS, groups_per_graph=2, interleave=4, return_initial=True)
    P = pipe.loops[0]._proj
    dlt, inl, _ = triangulation.triangulate_sequence(P, p2d, reject_px=12.0, return_inliers=True)
    assert torch.equal(pipe.inliers, inl) and float(inl[:, 2, ::3].float().mean()) < 0.5      # most shifted detections are out
    assert torch.equal(init, reprojection.refine_triangulation(P, p2d, dlt, valid=inl, max_iters=8))
    assert not torch.equal(init, reprojection.refine_triangulation(P, p2d, dlt, max_iters=8))
    _check_report(pipe, P, p2d, init, got)


def test_pipeline_over_a_rig_bank(device):
    from skelsplat_amd.loop import FramePipeline
    from tests.test_rigs_gpu import Setup
    s = Setup(device, "h36m", 3)
    ids = [(f * 2 + f // 5) % 3 for f in range(N)]
    _, p2d = s.frames(ids)
    p2d = torch.tensor(p2d, device=device)
    pipe = FramePipeline(s.model(), rigs=s.bank, frames=F, streams=2, dataset="h36m")
    pipe.set_refinement(16).set_reprojection_report()
    got, init = pipe.optimize_sequence(None, p2d, iterations=ITERS, groups_per_graph=2, interleave=4, return_initial=True,
                                       rig_ids=ids)
    torch.cuda.synchronize()
    pipe.check_rigs()
    P = torch.stack([s.bank.proj_dev[r] for r in ids]).contiguous()
    assert torch.equal(init, reprojection.refine_triangulation(P, p2d, triangulation.triangulate_sequence(P, p2d)))
    _check_report(pipe, P, p2d, init, got)


def test_loop_refusals(device):
    from skelsplat_amd.loop import FrameBatchLoop
    sc, model = _scene(device)
    p2d = _detections(sc, F, device)
    fb = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", factored=False)
    pts = triangulation.triangulate_sequence(sc.cameras, p2d)
    fb.set_refinement(4)
    with pytest.raises(ValueError, match="set_refinement"):
        fb.new_scenes(pts, poses_2d=p2d)
    with pytest.raises(ValueError, match="set_refinement"):
        fb.new_scenes(None, poses_2d=p2d, poses_3d=torch.zeros((F, V, J, 3), device=device))
    fb.new_scenes(None, poses_2d=p2d)
    assert torch.equal(fb.xyz, reprojection.refine_triangulation(sc.cameras, p2d, pts, max_iters=4))
    fb.set_refinement(None).set_reprojection_report()
    with pytest.raises(ValueError, match="set_reprojection_report"):
        fb.new_scenes(pts, heatmaps=torch.zeros((F, V, J, sc.H, sc.W), device=device))
