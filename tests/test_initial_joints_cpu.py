"""_sequence.InitialJoints, the one owner of "where do a scene's initial joints come from", and the loops' switches, on CPU
tensors: every source equals the direct call of the entry point it stands for (equal, NaN equal to NaN), the launches come in
their order and in place, every refusal is raised by check with the caller's name before anything is called, and a switch
reaches all the loops an object drives or none."""
import types

import numpy as np
import pytest
import torch

from skelsplat_amd import initial_guess, loop, reprojection, triangulation
from skelsplat_amd._sequence import InitialJoints, JointSwitches, SequenceSwitches

F, V, J = 2, 4, 5
TAU, REFINE = 10.0, (4.0, 8)         # reject_px; set_refinement's (huber_px, max_iters)
CPU = torch.device("cpu")


def _scene():
    """Four cameras on a ring around five joints, two frames: exact detections plus half a pixel of noise, one of them (frame 0,
    view 1, joint 2) pushed 80 px off; `keep` leaves joint 4 of frame 1 to a single view (no triangulation: NaN) and drops one more
    detection; predictions = the joints plus a few mm per view."""
    rng = np.random.default_rng(4)
    K = np.array([[1100.0, 0.0, 500.0], [0.0, 1100.0, 500.0], [0.0, 0.0, 1.0]])
    P = []
    for a in np.linspace(0.3, 0.3 + 1.5 * np.pi, V):
        C = np.array([4000.0 * np.cos(a), 4000.0 * np.sin(a), 300.0])
        z = -C / np.linalg.norm(C)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        Rw = np.stack([x, np.cross(z, x), z])                       # world -> camera
        P.append(K @ np.hstack([Rw, (-Rw @ C)[:, None]]))
    P = np.stack(P)
    X = rng.uniform(-500.0, 500.0, (F, J, 3))
    u = np.einsum("vrk,fjk->fvjr", P, np.concatenate([X, np.ones((F, J, 1))], -1))
    p2d = u[..., :2] / u[..., 2:] + rng.normal(0.0, 0.5, (F, V, J, 2))
    p2d[0, 1, 2] += 80.0
    keep = np.ones((F, V, J), dtype=bool)
    keep[1, 1:, 4] = False
    keep[0, 3, 0] = False
    p3d = X[:, None] + rng.normal(0.0, 5.0, (F, V, J, 3))
    t = torch.as_tensor
    return t(P), t(p2d.astype(np.float32)), t(keep), t(p3d.astype(np.float32)), t(X.astype(np.float32))


P, P2D, KEEP, P3D, PTS = _scene()


def _same(a, b):
    return a.dtype == b.dtype and np.array_equal(a.numpy(), b.numpy(), equal_nan=True)


def _plan(points=None, p2d=P2D, p3d=None, reject=None, refine=None, shape=(F, V, J), proj=P, who="new_scenes"):
    return InitialJoints.check(who, points, p2d, p3d, shape, reject, refine, proj, CPU)


def _buffers(frames=F):
    return (torch.zeros((frames, V, J), dtype=torch.bool), torch.full((frames, J), -1, dtype=torch.int32))


def _out(frames=F):
    return torch.full((frames, J, 3), -7.0)


def test_every_source_equals_the_direct_call():
    # explicit points: a plain copy
    out = _out()
    plan = _plan(PTS.numpy().astype(np.float64), p2d=None)
    assert not plan.estimated and plan.write(None, out) is out and torch.equal(out, PTS)
    # the plain DLT, without and with `keep`
    for keep in (None, KEEP):
        want = triangulation.triangulate_sequence(P, P2D, valid=keep, out=_out())
        out = _out()
        assert _plan().write(keep, out, _buffers()) is out and _same(out, want)
    assert torch.isnan(want[1, 4]).all() and int(torch.isnan(want).sum()) == 3      # the joint a single view kept
    # rejection: the masks and counts go into the buffers given
    want, inl, n_cons = triangulation.triangulate_sequence(P, P2D, valid=KEEP, reject_px=TAU, return_inliers=True)
    assert not bool(inl[0, 1, 2]) and bool(KEEP[0, 1, 2]) and not _same(want, triangulation.triangulate_sequence(P, P2D, valid=KEEP))
    out, buf = _out(), _buffers()
    _plan(reject=(TAU, 3)).write(KEEP, out, buf)
    assert _same(out, want) and torch.equal(buf[0], inl) and torch.equal(buf[1], n_cons)
    # rejection + refinement: triangulate, then refine over the inliers
    refined = reprojection.refine_triangulation(P, P2D, want, valid=inl, huber_px=REFINE[0], max_iters=REFINE[1])
    assert not _same(refined, want)
    out, buf = _out(), _buffers()
    _plan(reject=(TAU, 3), refine=REFINE).write(KEEP, out, buf)
    assert _same(out, refined) and torch.equal(buf[0], inl)
    # refinement alone: over `keep` (the moved detection pulls its joint: another result than over the inliers)
    start = triangulation.triangulate_sequence(P, P2D, valid=KEEP)
    want = reprojection.refine_triangulation(P, P2D, start, valid=KEEP, huber_px=REFINE[0], max_iters=REFINE[1])
    out, buf = _out(), _buffers()
    _plan(refine=REFINE).write(KEEP, out, buf)
    assert _same(out, want) and not _same(out, refined) and not buf[0].any() and (buf[1] == -1).all()      # buffers untouched
    # fusion
    for keep in (None, KEEP):
        want = initial_guess.fuse_predictions(P, P3D, P2D, valid=keep)
        out = _out()
        _plan(p3d=P3D).write(keep, out)
        assert _same(out, want)


@pytest.mark.parametrize("source", ["points", "dlt", "robust+refine", "fuse"])
def test_one_frame_form_equals_frame_0_of_the_batch(source):
    kw = dict(points=dict(points=PTS, p2d=None), dlt={}, fuse=dict(p3d=P3D))
    kw["robust+refine"] = dict(reject=(TAU, 3), refine=REFINE)
    batch, buf = _out(), _buffers()
    _plan(**kw[source]).write(KEEP, batch, buf)
    first = lambda t: None if t is None else t[0]
    one_kw = {k: first(v) if k in ("points", "p2d", "p3d") else v for k, v in kw[source].items()}
    one_kw.setdefault("p2d", P2D[0])
    one, one_buf = torch.full((J, 3), -7.0), (torch.zeros((V, J), dtype=torch.bool), torch.full((J,), -1, dtype=torch.int32))
    plan = _plan(shape=(None, V, J), who="new_scene", **one_kw)
    got = plan.write(KEEP[0], one, one_buf)
    assert got is one and _same(one, batch[0])
    assert torch.equal(one_buf[0], buf[0][0]) and torch.equal(one_buf[1], buf[1][0])
    assert all(t is None or t.shape[0] == 1 for t in (plan.points, plan.p2d, plan.p3d))


@pytest.fixture
def calls(monkeypatch):
    """The three entry points replaced by recorders of (name, out, keywords)."""
    log = []

    def recorder(name, where):
        def record(proj, *args, **kw):
            log.append((name, kw.get("out"), kw))
            return kw.get("out")
        monkeypatch.setattr(where, name, record)
    recorder("triangulate_sequence", triangulation)
    recorder("refine_triangulation", reprojection)
    recorder("fuse_predictions", initial_guess)
    return log


def test_launch_order_in_place(calls):
    out, buf = _out(), _buffers()
    _plan(reject=(TAU, 3), refine=REFINE).write(KEEP, out, buf)
    assert [c[0] for c in calls] == ["triangulate_sequence", "refine_triangulation"]
    assert all(c[1] is out for c in calls)
    tri, ref = calls[0][2], calls[1][2]
    assert tri["valid"] is KEEP and tri["reject_px"] == TAU and tri["min_inliers"] == 3 and tri["out_inliers"] is buf
    assert ref["valid"] is buf[0] and (ref["huber_px"], ref["max_iters"]) == REFINE
    del calls[:]
    _plan(refine=REFINE).write(KEEP, out, buf)
    assert [c[0] for c in calls] == ["triangulate_sequence", "refine_triangulation"]
    assert calls[0][2]["out_inliers"] is None and calls[0][2]["reject_px"] is None and calls[1][2]["valid"] is KEEP
    del calls[:]
    _plan().write(None, out, buf)
    assert [c[0] for c in calls] == ["triangulate_sequence"] and calls[0][2]["valid"] is None
    del calls[:]
    _plan(p3d=P3D).write(KEEP, out, buf)
    assert [(c[0], c[1] is out, c[2]["valid"] is KEEP) for c in calls] == [("fuse_predictions", True, True)]
    del calls[:]
    _plan(PTS, p2d=None).write(None, out)
    assert calls == [] and torch.equal(out, PTS)


@pytest.mark.parametrize("who", ["new_scene", "new_scenes", "optimize_sequence"])
def test_refusals_carry_the_callers_name_and_come_before_any_call(calls, who):
    one = who == "new_scene"
    shape = (None, V, J) if one else (F, V, J)
    cut = (lambda t: t[0]) if one else (lambda t: t)
    pts, p2d, p3d = cut(PTS), cut(P2D), cut(P3D)
    ax = "" if one else "F,"
    check = lambda points=None, d2=p2d, d3=None, reject=None, refine=None, proj=P: \
        InitialJoints.check(who, points, d2, d3, shape, reject, refine, proj, CPU)
    table = [
        (dict(points=pts, reject=(TAU, 3)), "outlier rejection .* explicit points"),
        (dict(d3=p3d, reject=(TAU, 3)), "outlier rejection .* poses_3d"),
        (dict(points=pts, refine=REFINE), r"the refinement \(set_refinement\) .* explicit points"),
        (dict(d3=p3d, refine=REFINE), r"the refinement \(set_refinement\) .* poses_3d"),
        (dict(points=pts, d3=p3d), "poses_3d are fused into the initial joints when points is None; give one of the two"),
        (dict(d2=None), r"give poses_2d \(ready heatmaps do not carry the detections\)"),
        (dict(proj=None), "the cameras carry no K / R / T"),
        (dict(points=pts[..., :2]), r"points must be \(%sP,3\)" % ax),
        (dict(points=pts[None]), r"points must be \(%sP,3\)" % ax),
        (dict(d2=p2d[..., :1]), r"poses_2d must be \(%sV,J,2\)" % ax),
        (dict(d2=p2d[..., :3, :]), r"poses_2d must be \(%sV,J,2\)" % ax),
        (dict(d3=p3d[..., :2]), r"poses_3d must be \(%sV,J,3\)" % ax),
    ]
    for kw, text in table:
        with pytest.raises(ValueError, match="^" + who + r"[:(].*" + text):
            check(**kw)
    assert calls == []
    assert check(d2=torch.cat([p2d, p2d[..., :1]], -1)).p2d.shape[-1] == 3        # a confidence column is carried along


class _Loop(SequenceSwitches):
    """What the switches read and set of a FrameBatchLoop."""

    def __init__(self, keep_gaussians=False):
        self._reject = self._refine = self._smooth = self._debug_frames = self._gt_next = None
        self._reproject, self.keep_gaussians, self.rigs = False, keep_gaussians, None
        self._report = types.SimpleNamespace(steps=3)
        self.P, self.xyz = J, torch.zeros((F, J, 3))


class _Pipe(SequenceSwitches):
    def __init__(self, n=3, **kw):
        self.loops, self._gt_next = [_Loop(**kw) for _ in range(n)], None

    def _driven(self):
        return self.loops


SETTINGS = ("_reject", "_refine", "_reproject", "_smooth", "_debug_frames")


def test_a_switch_reaches_every_loop_or_none():
    pipe, alone = _Pipe(), _Loop()
    for owner in (pipe, alone):
        loops = owner._driven()
        assert owner.set_outlier_rejection(TAU, 4) is owner and all(lp._reject == (TAU, 4) for lp in loops)
        assert owner.set_refinement(8, 4.0) is owner and all(lp._refine == (4.0, 8) for lp in loops)
        assert owner.set_reprojection_report() is owner and all(lp._reproject is True for lp in loops)
        assert owner.set_debug_images([3, 0]) is owner and all(lp._debug_frames == (3, 0) for lp in loops)
        assert owner.set_smoothing(2, use_covariance=False) is owner
        assert all(lp._smooth["half_window"] == 2 and lp._smooth["use_covariance"] is False for lp in loops)
        before = [{k: getattr(lp, k) for k in SETTINGS} for lp in loops]
        # a bad argument raises before any loop is changed
        for bad in (lambda: owner.set_outlier_rejection(-1.0), lambda: owner.set_outlier_rejection(TAU, 1),
                    lambda: owner.set_refinement(17), lambda: owner.set_refinement(8, -1.0), lambda: owner.set_debug_images([-1]),
                    lambda: owner.set_smoothing(2, use_covariance=True), lambda: owner.set_smoothing(2, degree=5)):
            with pytest.raises(ValueError):
                bad()
            assert [{k: getattr(lp, k) for k in SETTINGS} for lp in loops] == before
        # None (False) switches a setting off again
        owner.set_outlier_rejection(None).set_refinement(None).set_reprojection_report(False).set_debug_images(None).set_smoothing(None)
        assert all(getattr(lp, k) in (None, False) for lp in loops for k in SETTINGS)
        # the ground truth waits on the object that was given it, checked against the loops' shapes
        gt = torch.zeros((7, J, 3))
        assert owner.set_ground_truth(gt) is owner and owner._gt_next is gt
        with pytest.raises(ValueError, match="float32"):
            owner.set_ground_truth(gt.double())
        assert owner._gt_next is gt and owner.set_ground_truth(None)._gt_next is None
    assert all(lp._gt_next is None for lp in pipe.loops)
    assert _Pipe(keep_gaussians=True).set_smoothing(1).loops[2]._smooth["use_covariance"] is True


def test_the_loops_take_their_switches_from_the_mixins():
    assert not [name for name in vars(loop.FramePipeline) if name.startswith("set_")]
    assert not [name for cls in (loop.MultiViewLoop, loop.FrameBatchLoop) for name in vars(cls) if name.startswith("set_")]
    for cls in (loop.MultiViewLoop, loop.FrameBatchLoop, loop.FramePipeline):
        assert issubclass(cls, JointSwitches) and cls.set_outlier_rejection is JointSwitches.set_outlier_rejection
    assert not issubclass(loop.MultiViewLoop, SequenceSwitches)
    for cls in (loop.FrameBatchLoop, loop.FramePipeline):
        for name in ("set_reprojection_report", "set_smoothing", "set_debug_images", "set_ground_truth"):
            assert getattr(cls, name) is getattr(SequenceSwitches, name)
