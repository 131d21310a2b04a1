"""_sequence.SequenceRun, the record of one optimize_sequence call, against a stub loop on the CPU: which rows of the inputs every
batch gets, which rows of the results begin() and take() write, and the constructor's refusals in the order of its checks."""
import types

import pytest
import torch

from skelsplat_amd._sequence import SequenceRun

N, F, V, P = 5, 2, 4, 17
ROWS = {0: 2, 2: 2, 4: 1}       # batch start -> frames that count: full, full, padded
FILL = -7.0                     # what a result row holds before the run writes it


class StubLoop(types.SimpleNamespace):
    """What SequenceRun reads of a FrameBatchLoop.  new_scenes records what it was given and marks row i of batch number c with
    100 c + i + 1, so that every row of every batch, the filler's included, is recognisable."""

    def __init__(self, **kw):
        z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype)
        super().__init__(F=F, V=V, P=P, device=torch.device("cpu"), xyz=z(F, P, 3), scaling=z(F, P, 3), rotation=z(F, P, 4),
                         opacity=z(F, P, 1), inliers=z(F, V, P, dtype=torch.bool), n_consensus=z(F, P, dtype=torch.int32),
                         counters=z(F, 2, dtype=torch.int32), _es_state=z(F, 2, dtype=torch.int32), _gt_next=None, _report=None,
                         _sel=None, _reject=None, _refine=None, _reproject=False, _smooth=None, _debug_frames=None,
                         keep_gaussians=False, calls=[])
        self.__dict__.update(kw)

    def new_scenes(self, points, poses_2d=None, rig_ids=None, poses_3d=None):
        c = len(self.calls)
        self.calls.append(dict(points=points, poses_2d=poses_2d, rig_ids=rig_ids, poses_3d=poses_3d, gt=self._gt_next))
        mark = 100.0 * c + torch.arange(1, F + 1, dtype=torch.float32)
        self.xyz[:] = mark[:, None, None]
        self.n_consensus[:] = mark.to(torch.int32)[:, None]
        self.inliers[:] = (torch.arange(F) % 2 == c % 2)[:, None, None]
        self._es_state[:, 1] = mark.to(torch.int32) + 50

    def optimise(self):
        self.xyz += 0.5         # the joints take() copies are not the initial ones any more


class Recorder:
    """Stands where the run keeps a SequenceGaussians / SequenceImages / SequenceReport: the (name, loop, b, n) of every call."""

    def __init__(self, log, name):
        self.begin = lambda loop, b, n: log.append((name + ".begin", loop, b, n))
        self.take = lambda loop, b, n: log.append((name + ".take", loop, b, n))


def _inputs():
    mk = lambda *s: torch.arange(float(torch.Size(s).numel())).reshape(s)
    return dict(pts=mk(N, P, 3), p2d=mk(N, V, P, 2), p3d=mk(N, V, P, 3), ids=torch.tensor([1, 0, 2, 0, 1]), gt=mk(N, P, 3) + 0.25)


def _drive(run, loop):
    """Every batch through begin / take, with every result row checked against the rows the batch may write."""
    for t in (run.out, run.initial, run.stopped_at, run.inliers, run.n_consensus):
        if t is not None:
            t.fill_(FILL if t.dtype != torch.bool else False)
    assert list(run.starts()) == [0, 2, 4]
    for c, b in enumerate(run.starts()):
        n, mark = ROWS[b], 100.0 * c + torch.arange(1, F + 1, dtype=torch.float32)
        run.begin(loop, b)
        assert len(loop.calls) == c + 1
        if run.initial is not None:
            assert torch.equal(run.initial[b:b + n], mark[:n, None, None].expand(n, P, 3))
            assert (run.initial[b + n:] == FILL).all()
        if run.inliers is not None:
            assert torch.equal(run.inliers[b:b + n], loop.inliers[:n]) and not run.inliers[b + n:].any()
            assert torch.equal(run.n_consensus[b:b + n], loop.n_consensus[:n]) and (run.n_consensus[b + n:] == int(FILL)).all()
        assert (run.out[b:] == FILL).all()                      # begin() leaves the joints alone
        loop.optimise()
        run.take(loop, b)
        assert torch.equal(run.out[b:b + n], (mark[:n, None, None] + 0.5).expand(n, P, 3)) and (run.out[b + n:] == FILL).all()
        if run.stopped_at is not None:
            assert run.stopped_at[b:b + n].tolist() == [int(m) + 50 for m in mark[:n]] and (run.stopped_at[b + n:] == int(FILL)).all()
    # all N rows written, each by its own frame: the filler (row 2 of the third batch, 202 / 202.5 / 252) is nowhere
    assert run.out[:, 0, 0].tolist() == [1.5, 2.5, 101.5, 102.5, 201.5] and run.out.shape[0] == N
    if run.initial is not None:
        assert run.initial[:, 0, 0].tolist() == [1.0, 2.0, 101.0, 102.0, 201.0]
    if run.n_consensus is not None:
        assert run.n_consensus[:, 0].tolist() == [1, 2, 101, 102, 201]
    if run.stopped_at is not None:
        assert run.stopped_at.tolist() == [51, 52, 151, 152, 251]


def test_rows_are_views_of_full_batches_and_one_index_list_for_the_padded_one():
    d = _inputs()
    sel = types.SimpleNamespace(bank=types.SimpleNamespace(R=3), ids=torch.zeros(F, dtype=torch.int32))
    report = types.SimpleNamespace(trace_err=torch.zeros(F, 3, 2), trace_loss=None, final_err=torch.zeros(F, P, 2), snaps=None, saves=())
    loop = StubLoop(_sel=sel, _report=report, keep_gaussians=True)
    run = SequenceRun(loop, d["gt"], None, d["p2d"], d["p3d"], d["ids"], True)
    assert (run.N, run.F, run.pts, run.stopped_at, run.inliers, run.n_consensus, run.images) == (N, F, None, None, None, None, None)
    assert run.gaussians.xyz is run.out and run.report.steps.shape == (N,) and run.ids.dtype == torch.int32
    assert run.rows(0) == slice(0, 2) and run.rows(2) == slice(2, 4) and run.rows(4) == [4, 4]
    log = []
    run.gaussians, run.images, run.report = Recorder(log, "gaussians"), Recorder(log, "images"), Recorder(log, "report")
    run.stopped_at = torch.empty(N, dtype=torch.int64)
    _drive(run, loop)
    for c, b in enumerate((0, 2)):                              # full batches: the inputs' own storage, nothing gathered
        for got, whole in ((loop.calls[c]["poses_2d"], d["p2d"]), (loop.calls[c]["poses_3d"], d["p3d"]),
                           (loop.calls[c]["rig_ids"], run.ids), (loop.calls[c]["gt"], d["gt"])):
            assert got.data_ptr() == whole[b].data_ptr() == whole.data_ptr() + b * whole.stride(0) * whole.element_size()
            assert got.shape[0] == F and torch.equal(got, whole[b:b + F])
        assert loop.calls[c]["points"] is None
    last = loop.calls[2]                                        # the padded batch: frame 4 twice, in every input alike
    for got, whole in ((last["poses_2d"], d["p2d"]), (last["poses_3d"], d["p3d"]), (last["rig_ids"], run.ids), (last["gt"], d["gt"])):
        assert torch.equal(got, whole[[4, 4]])
    # every batch: images.begin behind new_scenes, then gaussians, images, report take, all with the batch's own n
    assert [(what, b, n) for what, _, b, n in log] == [x for b, n in ROWS.items() for x in (
        ("images.begin", b, n), ("gaussians.take", b, n), ("images.take", b, n), ("report.take", b, n))]
    assert all(lp is loop for _, lp, _, _ in log)
    assert run.result()[0] is run.out and run.result()[1] is run.initial


def test_explicit_points_and_rejection_rows():
    d = _inputs()
    loop = StubLoop()
    run = SequenceRun(loop, None, d["pts"].numpy(), d["p2d"].numpy(), None, None, False)       # arrays become CPU tensors
    _drive(run, loop)
    assert loop.calls[1]["points"].data_ptr() == run.pts[2].data_ptr() and torch.equal(loop.calls[1]["points"], d["pts"][2:4])
    assert torch.equal(loop.calls[2]["points"], d["pts"][[4, 4]]) and torch.equal(loop.calls[2]["poses_2d"], d["p2d"][[4, 4]])
    loop = StubLoop(_reject=(20.0, 3))
    run = SequenceRun(loop, None, None, d["p2d"], None, None, True)
    assert run.inliers.shape == (N, V, P) and run.inliers.dtype == torch.bool
    assert run.n_consensus.shape == (N, P) and run.n_consensus.dtype == torch.int32
    _drive(run, loop)


def test_everything_off_touches_new_scenes_and_out_only():
    d = _inputs()
    loop = StubLoop(_gt_next="the loop's own")
    run = SequenceRun(loop, None, None, d["p2d"], None, None, False)
    for name in ("pts", "p3d", "ids", "gt", "initial", "inliers", "n_consensus", "report", "gaussians", "images", "stopped_at"):
        assert getattr(run, name) is None, name
    before = {k: v.clone() for k, v in vars(loop).items() if torch.is_tensor(v)}
    loop.new_scenes = lambda points, poses_2d=None, rig_ids=None, poses_3d=None: loop.calls.append((points, rig_ids, poses_3d))
    for b in run.starts():
        run.begin(loop, b)
        run.take(loop, b)
    assert loop.calls == [(None, None, None)] * 3 and loop._gt_next == "the loop's own"
    assert all(torch.equal(v, getattr(loop, k)) for k, v in before.items())
    assert run.result() is run.out and torch.equal(run.out, torch.zeros(N, P, 3))


def test_refusals_keep_their_messages_and_their_order():
    d = _inputs()
    sel = types.SimpleNamespace(bank=types.SimpleNamespace(R=3), ids=torch.zeros(F, dtype=torch.int32))
    views = types.SimpleNamespace(W=8, H=8, mixed=False)
    rejecting, picturing = StubLoop(_reject=(20.0, 3)), StubLoop(_debug_frames=(0, N), views_all=views)
    one = lambda loop, gt=None, pts=None, p3d=None, ids=None, p2d=d["p2d"]: SequenceRun(loop, gt, pts, p2d, p3d, ids, False)
    with pytest.raises(ValueError, match="4 frames of points, 5 of detections"):
        one(StubLoop(), pts=d["pts"][:4])
    with pytest.raises(ValueError, match="poses_3d are fused into the initial joints when points is None; give one of the two"):
        one(StubLoop(), pts=d["pts"], p3d=d["p3d"])
    with pytest.raises(ValueError, match=r"optimize_sequence: outlier rejection .* explicit points are taken as they are"):
        one(rejecting, pts=d["pts"])
    with pytest.raises(ValueError, match=r"optimize_sequence: outlier rejection .* fusing poses_3d is a different estimator"):
        one(rejecting, p3d=d["p3d"])
    with pytest.raises(ValueError, match="rig_ids needs a rig bank"):
        one(StubLoop(), ids=d["ids"])
    with pytest.raises(ValueError, match=r"optimize_sequence: the ground truth given to set_ground_truth must be \(5, 17, 3\), got \(4, 17, 3\)"):
        one(StubLoop(), gt=d["gt"][:4])
    with pytest.raises(ValueError, match=r"set_debug_images: frames \[0, 5\] must be indices into the sequence's 5 frames"):
        one(picturing)
    assert one(StubLoop(_debug_frames=(0, N - 1), views_all=views)).images.frames == [0, N - 1]
    # two at once: the earlier check of the preamble wins
    with pytest.raises(ValueError, match="frames of points"):
        one(StubLoop(), pts=d["pts"][:4], p3d=d["p3d"])                         # frame count before poses_3d beside points
    with pytest.raises(ValueError, match="poses_3d are fused"):
        one(rejecting, pts=d["pts"], p3d=d["p3d"])                              # poses_3d beside points before the rejection
    with pytest.raises(ValueError, match="outlier rejection"):
        one(rejecting, p3d=d["p3d"], ids=d["ids"])                              # the rejection before rig_ids without a bank
    with pytest.raises(ValueError, match="rig_ids needs a rig bank"):
        one(StubLoop(), ids=d["ids"], gt=d["gt"][:4])                           # rig_ids before the ground truth
    with pytest.raises(ValueError, match="ground truth given to set_ground_truth"):
        one(picturing, gt=d["gt"][:4])                                          # the ground truth before the debug frames
    assert one(StubLoop(_sel=sel), ids=[0, 2, 1, 0, 2]).ids.tolist() == [0, 2, 1, 0, 2]
