"""Every per-sequence feature of optimize_sequence switched on at once: rejection, ground truth and reports, kept Gaussians, debug
pictures and the initial joints, through a FramePipeline whose last batch is padded.  The other suites switch them on one at a
time; here each result has to be, bit for bit, what a pipeline with that one feature alone gives."""
import pytest
import torch

from tests.robust_tri_cases import TAU
from tests.test_frames_es_gpu import _frames, _scene
from tests.test_preview_gpu import ES_ITERS, ES_TOL, ITERS
from tests.test_report_gpu import ROWS, _same

pytestmark = pytest.mark.gpu

SAVES = (10,)
CHOSEN = [0, 4]         # frame 4 sits alone in the padded last batch of frames=2


@pytest.mark.parametrize("es", [False, True], ids=["no_stopping", "early_stopping"])
def test_all_sequence_features_at_once_equal_each_alone(device, es):
    from skelsplat_amd.loop import FrameBatchLoop, FramePipeline, OptEarlyStopping
    sc, model = _scene(device)
    p2d = torch.as_tensor(_frames(sc, 5)[1], device=device)
    gt = torch.as_tensor(sc.pose_3d_gt, dtype=torch.float32, device=device)[None].repeat(5, 1, 1).contiguous()
    iters = ES_ITERS if es else ITERS

    def pipeline(**kw):
        if es:
            kw["early_stopping"] = OptEarlyStopping(window_size=4, repeat_tolerance=ES_TOL)
        return FramePipeline(model(device), sc.cameras, frames=2, streams=2, dataset="h36m", **kw)

    def run(p, points, **kw):
        res = p.optimize_sequence(points, p2d, iterations=iters, groups_per_graph=2, interleave=8, **kw)
        torch.cuda.synchronize()
        return res

    both = pipeline(report_steps=ROWS, save_iterations=SAVES, keep_gaussians=True)
    both.set_debug_images(CHOSEN).set_outlier_rejection(TAU).set_ground_truth(gt)
    joints, initial = run(both, None, return_initial=True)

    rejecting = pipeline().set_outlier_rejection(TAU)
    want, want_initial = run(rejecting, None, return_initial=True)
    assert torch.equal(joints, want) and torch.equal(initial, want_initial) and not torch.equal(joints, initial)
    assert torch.equal(both.inliers, rejecting.inliers) and torch.equal(both.n_consensus, rejecting.n_consensus)
    assert tuple(both.inliers.shape) == (5, 4, 17) and tuple(both.n_consensus.shape) == (5, 17)
    if es:
        assert torch.equal(both.stopped_at, rejecting.stopped_at) and bool(both.stopped_at.any())      # frames did stop
    # the other features act behind the initial joints: their pipelines are given the ones the rejection left
    reporting = pipeline(report_steps=ROWS, save_iterations=SAVES).set_ground_truth(gt)
    assert torch.equal(run(reporting, want_initial), want)
    for name in ("trace_errors", "trace_losses", "final_errors", "snapshots"):
        assert _same(getattr(both.report, name), getattr(reporting.report, name)), name
    assert torch.equal(both.report.steps, reporting.report.steps) and both.report.save_iterations == reporting.report.save_iterations
    assert bool(torch.isfinite(both.report.final_errors).all())             # the ground truth arrived
    keeping = pipeline(keep_gaussians=True)
    assert torch.equal(run(keeping, want_initial), want)
    assert both.gaussians.xyz is joints
    for name in ("xyz", "scaling", "rotation", "opacity"):
        assert torch.equal(getattr(both.gaussians, name), getattr(keeping.gaussians, name)), name
    picturing = pipeline().set_debug_images(CHOSEN)
    assert torch.equal(run(picturing, want_initial), want)
    assert both.images.frames == picturing.images.frames == CHOSEN
    for name in ("heatmaps", "render_first", "render_last"):
        assert torch.equal(getattr(both.images, name), getattr(picturing.images, name)), name
        assert bool(getattr(both.images, name).amax(dim=(1, 2, 3)).eq(255).all()), name     # both frames were pictured
    assert _same(both.images.minmax, picturing.images.minmax)
    for p in (rejecting, reporting, keeping, picturing):
        assert sum(x is not None for x in (p.inliers, p.report, p.gaussians, p.images)) == 1

    kw = dict(early_stopping=OptEarlyStopping(window_size=4, repeat_tolerance=ES_TOL)) if es else {}
    fb = FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m", use_graph=True, report_steps=ROWS, save_iterations=SAVES,
                        keep_gaussians=True, **kw)
    fb.set_debug_images(CHOSEN).set_outlier_rejection(TAU).set_ground_truth(gt)
    one, one_initial = fb.optimize_sequence(None, p2d, iterations=iters, groups_per_graph=2, return_initial=True)
    torch.cuda.synchronize()
    assert torch.equal(one, joints) and torch.equal(one_initial, initial)
    assert torch.equal(fb.seq_inliers, both.inliers) and torch.equal(fb.seq_n_consensus, both.n_consensus)
