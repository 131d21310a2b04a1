"""The one path the loops' other GPU tests leave out: a MultiViewLoop with outlier rejection AND refinement on AND a dropout
mask.  Its initial joints, inliers and consensus counts equal, bit for bit, the direct triangulate_sequence ->
refine_triangulation calls, and frame 0 of a FrameBatchLoop given the same detections and mask (H36M's four cameras, 17 joints,
160 x 128 images)."""
import pytest
import torch

from skelsplat_amd import reprojection, triangulation
from skelsplat_amd.heatmaps import draw_dropout
from tests.test_robust_triangulate_gpu import J, V, _corrupted_detections, _same, _scene

pytestmark = pytest.mark.gpu

TAU, ITERS, HUBER, SEED = 12.0, 8, 10.0, 1      # (this draw drops 9 planes: one joint is left to a single view)


def test_multi_view_loop_rejects_refines_and_drops_like_the_direct_calls_and_like_a_batch(device):
    from skelsplat_amd.loop import FrameBatchLoop, MultiViewLoop
    sc, model = _scene(device)
    p2d, bad = _corrupted_detections(sc, 2, device)
    torch.manual_seed(SEED)
    drop = draw_dropout(V, J)                       # what new_scene(dropout=True) draws from the same generator state
    assert drop.any() and not drop.all()
    keep = ~drop
    # the direct calls
    dlt, inl, n_cons = triangulation.triangulate_sequence(sc.cameras, p2d[0], valid=keep, reject_px=TAU, return_inliers=True)
    want = reprojection.refine_triangulation(sc.cameras, p2d[0], dlt, valid=inl, huber_px=HUBER, max_iters=ITERS)
    assert not inl.cpu()[torch.as_tensor(bad[0]) & keep].any() and not _same(want, dlt)
    assert not _same(want, reprojection.refine_triangulation(sc.cameras, p2d[0], dlt, valid=keep, huber_px=HUBER, max_iters=ITERS))
    # one frame in a MultiViewLoop
    gm = model()
    loop = MultiViewLoop(gm, sc.cameras, torch.zeros((V, J, sc.H, sc.W), device=device), dataset="h36m")
    loop.set_outlier_rejection(TAU).set_refinement(ITERS, huber_px=HUBER)
    torch.manual_seed(SEED)
    loop.new_scene(None, poses_2d=p2d[0], dropout=True)
    assert _same(gm._xyz.detach(), want) and _same(loop.inliers, inl) and _same(loop.n_consensus, n_cons)
    assert tuple(loop.inliers.shape) == (V, J) and tuple(loop.n_consensus.shape) == (J,)
    # the same frame as frame 0 of a batch of two
    fb = FrameBatchLoop(model(), sc.cameras, 2, dataset="h36m")
    fb.set_outlier_rejection(TAU).set_refinement(ITERS, huber_px=HUBER)
    fb.new_scenes(None, poses_2d=p2d, drop_masks=torch.stack([drop, torch.zeros_like(drop)]))
    assert _same(fb.xyz[0], gm._xyz.detach()) and _same(fb.inliers[0], loop.inliers) and _same(fb.n_consensus[0], loop.n_consensus)
    assert not _same(fb.xyz[1], fb.xyz[0])
