"""The batched DLT on the device (sks_triangulate through triangulation.triangulate_sequence) and `points=None` through
FrameBatchLoop, FramePipeline and MultiViewLoop: against the reference's golden triangulations, against the host path,
bit for bit against itself across batch sizes, batch positions and streams, and bit for bit against the same loops given
the triangulated points explicitly."""
import ctypes

import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, triangulation
from tests import tri_cases as TC

pytestmark = pytest.mark.gpu

V, J = 4, 17
SPIN_US = 20000.0       # as tests/test_streams_gpu.py: an order of magnitude over the host and GPU time of a warmed call
ES_TOL = 3e-4          # with _detections' frames: stops spread over iterations 18 .. 136 (tools/bench_frames_es.py's tolerance)


def _tri(P, x, dev, **kw):
    return triangulation.triangulate_sequence(torch.as_tensor(P, device=dev), torch.as_tensor(x, device=dev), **kw)


def test_golden_cases_in_float64_and_float32_is_its_rounding(device):
    for tag in TC.GOLDEN_TAGS:
        P, x2d, X = TC.golden(tag)
        got = _tri(P, x2d[None], device, homogeneous=True)
        assert got.dtype == torch.float64 and tuple(got.shape) == (1,) + X.shape and got.device.type == "cuda"
        g = got[0].cpu().numpy()
        print(tag, "max abs error against the golden X:", np.abs(g - X).max())
        assert np.all(g[:, 3] == 1.0)
        assert np.allclose(g, X, **TC.GOLDEN_TOL), (tag, np.abs(g - X).max())
        xyz = _tri(P, x2d[None], device)
        assert xyz.dtype == torch.float32 and torch.equal(xyz, got[..., :3].to(torch.float32))
        assert torch.equal(_tri(P, x2d, device, homogeneous=True), got[0])        # (V,J,2): no frame axis


def _many(ds, n_views, N, seed=3):
    """N frames from eight distinct ones plus a pixel of noise each (float32 detections)"""
    sc, P, gt, base = TC.sequence(ds, n_views, frames=8, seed=seed)
    rng = np.random.default_rng(seed + 7)
    p2d = (base[np.arange(N) % 8] + rng.normal(0, 1.0, (N,) + base.shape[1:])).astype(np.float32)
    return sc, P, p2d


@pytest.mark.parametrize("ds,n_views", [("h36m", 2), ("h36m", 4), ("panoptic", 31), ("panoptic", 64)])
def test_batches_equal_the_host_path_and_do_not_depend_on_batch_or_stream(device, ds, n_views):
    sc, P, p2d_all = _many(ds, n_views, 1000)
    Pd, xd = torch.as_tensor(P, device=device), torch.as_tensor(p2d_all, device=device)
    side = torch.cuda.Stream(device)
    whole = None
    for N in (1, 16, 1000):
        got = triangulation.triangulate_sequence(Pd, xd[:N], homogeneous=True)
        assert tuple(got.shape) == (N, sc.n_points, 4)
        ref = triangulation.triangulate_sequence(P, p2d_all[:N], homogeneous=True)
        g = got.cpu().numpy()
        print(ds, n_views, N, "max abs difference to the host path:", np.abs(g - ref).max())
        assert np.allclose(g, ref, **TC.GOLDEN_TOL), (N, np.abs(g - ref).max())
        whole = got
    xyz = triangulation.triangulate_sequence(Pd, xd)
    assert torch.equal(xyz, whole[..., :3].to(torch.float32))
    for f in (0, 7, 15, 16, 501, 999):
        alone = triangulation.triangulate_sequence(Pd, xd[f:f + 1], homogeneous=True)[0]
        assert torch.equal(alone, whole[f]), f
        lo = max(0, f - 3)
        part = triangulation.triangulate_sequence(Pd, xd[lo:f + 6], homogeneous=True)     # another batch, another place in it
        assert torch.equal(part[f - lo], whole[f]), f
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            other = triangulation.triangulate_sequence(Pd, xd[f:f + 1], homogeneous=True)[0]
        side.synchronize()
        assert torch.equal(other, whole[f]), f
    # one rig per frame
    rigs = Pd[None].repeat(16, 1, 1, 1).contiguous()
    assert torch.equal(triangulation.triangulate_sequence(rigs, xd[:16], homogeneous=True), whole[:16])


def test_more_views_than_a_wavefront_are_refused(device):
    x = torch.zeros((1, 65, J, 2), device=device)
    with pytest.raises(ValueError, match="65 views"):
        triangulation.triangulate_sequence(torch.zeros((65, 3, 4), dtype=torch.float64, device=device), x)
    out = torch.zeros((1, J, 3), device=device)
    P = torch.zeros((65, 3, 4), dtype=torch.float64, device=device)
    rc = _lib.load().sks_triangulate(1, 65, J, P.data_ptr(), 0, x.data_ptr(), None, None, out.data_ptr(), None, None, None)
    assert rc < 0 and "65 views" in _lib.load().sks_last_error().decode()


def test_masks_on_the_device(device):
    sc, P, gt, p2d = TC.sequence("h36m", 4, frames=3, seed=5, dtype=np.float64)
    rng = np.random.default_rng(7)
    valid = np.ones((3, 4, J), dtype=bool)
    for f in range(3):
        for j in range(J):
            valid[f, rng.choice(4, size=rng.integers(0, 3), replace=False), j] = False      # 2 .. 4 views kept
    valid[0, :, 9] = True           # an intact joint beside ...
    valid[1, 1:, 3] = False         # ... one kept in a single view
    valid[2, :, 5] = False          # ... and a fully masked one
    x = p2d.copy()
    x[~valid] = np.nan              # a left-out detection is never read
    got, n_used = _tri(P, x, device, valid=torch.as_tensor(valid, device=device), homogeneous=True, return_n_used=True)
    assert n_used.dtype == torch.int32 and np.array_equal(n_used.cpu().numpy(), valid.sum(1))
    assert int(n_used[1, 3]) == 1 and int(n_used[2, 5]) == 0 and int(n_used[0, 9]) == 4
    g = got.cpu().numpy()
    for f in range(3):
        ref = TC.kept_views_reference(P, p2d[f], valid[f])
        assert np.array_equal(np.isnan(g[f]), np.isnan(ref))
        assert np.allclose(g[f], ref, equal_nan=True, **TC.GOLDEN_TOL), np.nanmax(np.abs(g[f] - ref))
    assert np.isnan(g[1, 3]).all() and np.isnan(g[2, 5]).all() and np.isnan(g).sum() == 8
    host = triangulation.triangulate_sequence(P, x, valid=valid, homogeneous=True)
    assert np.allclose(g, host, equal_nan=True, **TC.GOLDEN_TOL)
    xyz = _tri(P, x.astype(np.float32), device, valid=valid)                              # a host mask is uploaded
    assert np.isnan(xyz.cpu().numpy()).sum() == 6
    # an all-true mask is no mask, bit for bit
    assert torch.equal(_tri(P, p2d, device, valid=np.ones_like(valid), homogeneous=True), _tri(P, p2d, device, homogeneous=True))


# ------------------------------------------------------------------------------------------------ through the loops
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
    """frame f: the scene's detections with f x 2 px of noise on top, float32 on the device"""
    rng = np.random.default_rng(seed)
    base = np.asarray(sc.poses_2d, np.float32)
    return torch.as_tensor(np.stack([base + rng.normal(0, 2.0 * f, base.shape) for f in range(n)]).astype(np.float32), device=dev)


def _state(fb, f):
    return [fb.xyz[f], fb.scaling[f], fb.rotation[f], fb.opacity[f], fb.exp_avg[f], fb.exp_avg_sq[f], fb.accumulated_grads[f],
            fb.counters[f]]


@pytest.mark.parametrize("factored", [True, False], ids=["factored", "planes"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_frame_batch_triangulates_into_xyz_and_then_runs_as_with_explicit_points(device, use_graph, factored):
    from skelsplat_amd.loop import FrameBatchLoop
    sc, model = _scene(device)
    F = 4
    p2d = _detections(sc, F, device)
    drop = torch.zeros((F, V, J), dtype=torch.bool)
    drop[0, 1, [2, 5]] = True
    drop[2, 0, 7] = True
    drop[2, 3, 7] = True
    for masks in (None, drop):
        valid = None if masks is None else ~masks
        init = triangulation.triangulate_sequence(sc.cameras, p2d, valid=valid)
        assert init.device.type == "cuda" and bool(torch.isfinite(init).all())
        a = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", use_graph=use_graph, factored=factored)
        b = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", use_graph=use_graph, factored=factored)
        a.new_scenes(None, poses_2d=p2d, drop_masks=masks)
        assert torch.equal(a.xyz, init)                                     # before the first step
        b.new_scenes(init, poses_2d=p2d, drop_masks=masks)
        a.run(40, groups_per_graph=4)
        b.run(40, groups_per_graph=4)
        for f in range(F):
            for k, (s, t) in enumerate(zip(_state(a, f), _state(b, f))):
                assert torch.equal(s, t), (f, k)
        assert not torch.equal(a.xyz, init)
        # the next batch through the same loop (captured graphs replayed), detections as a host array this time
        a.new_scenes(None, poses_2d=p2d.cpu().numpy(), drop_masks=None if masks is None else masks.numpy())
        assert torch.equal(a.xyz, init)
        a.run(40, groups_per_graph=4)
        assert torch.equal(a.xyz, b.xyz)
    with pytest.raises(ValueError, match="poses_2d"):
        a.new_scenes(None)
    if not factored:
        with pytest.raises(ValueError, match="poses_2d"):
            a.new_scenes(None, heatmaps=torch.zeros((F, V, J, sc.H, sc.W), device=device))
    with pytest.raises(ValueError, match=r"\(F,V,J,2\)"):
        a.new_scenes(None, poses_2d=p2d[:2])


@pytest.mark.parametrize("early_stopping", ["no_stopping", "opt_early_stopping"])
def test_sequences_from_detections_alone(device, early_stopping):
    """N = 7 frames through 3 frames per launch on 2 streams (a padded last batch): optimize_sequence(None, detections on the
    device) == optimize_sequence(triangulate_sequence(...), detections), stopping iterations included."""
    from skelsplat_amd.loop import FramePipeline, FrameBatchLoop, OptEarlyStopping
    sc, model = _scene(device)
    N, iters = 7, 120
    p2d = _detections(sc, N, device)
    init = triangulation.triangulate_sequence(sc.cameras, p2d)
    es = lambda: early_stopping if early_stopping == "no_stopping" else OptEarlyStopping(4, ES_TOL)
    pipe = FramePipeline(model(), sc.cameras, frames=3, streams=2, dataset="h36m", early_stopping=es())
    want = pipe.optimize_sequence(init, p2d, iterations=iters, groups_per_graph=4, interleave=40).clone()
    want_stops = None if pipe.stopped_at is None else pipe.stopped_at.clone()
    got, initial = pipe.optimize_sequence(None, p2d, iterations=iters, groups_per_graph=4, interleave=40, return_initial=True)
    assert torch.equal(initial, init)
    assert torch.equal(got, want) and not torch.equal(got, init)
    if early_stopping == "opt_early_stopping":
        stops = pipe.stopped_at.cpu().tolist()
        print("stopping iterations:", stops)
        assert torch.equal(pipe.stopped_at, want_stops)
        assert any(0 < s < iters and s % 4 for s in stops), stops    # the criterion ended frames early, inside a group
        assert len(set(stops)) >= 3 and any(s == 0 for s in stops), stops    # ... at different iterations, and not all of them
    else:
        assert pipe.stopped_at is None
    # points given: return_initial hands them back (as float32 on the device)
    again, initial = pipe.optimize_sequence(init.cpu().numpy(), p2d.cpu().numpy(), iterations=iters, groups_per_graph=4,
                                            interleave=40, return_initial=True)
    assert torch.equal(again, want) and torch.equal(initial, init)
    # one loop, one stream
    fb = FrameBatchLoop(model(), sc.cameras, 3, dataset="h36m", use_graph=True, early_stopping=es())
    one, initial = fb.optimize_sequence(None, p2d, iterations=iters, groups_per_graph=4, return_initial=True)
    assert torch.equal(one, want) and torch.equal(initial, init)
    with pytest.raises(ValueError, match="frames of points"):
        pipe.optimize_sequence(init[:3], p2d)


def test_multi_view_loop_triangulates_its_frame(device):
    from skelsplat_amd.loop import MultiViewLoop
    sc, model = _scene(device)
    p2d = _detections(sc, 3, device)[2]
    init = triangulation.triangulate_sequence(sc.cameras, p2d)
    assert tuple(init.shape) == (J, 3)
    res = []
    for pts in (None, init):
        gm = model()
        loop = MultiViewLoop(gm, sc.cameras, torch.zeros((V, J, sc.H, sc.W), device=device), dataset="h36m")
        loop.new_scene(pts, poses_2d=p2d)
        assert torch.equal(gm._xyz.detach(), init)
        loop.run(24)
        res.append([gm._xyz.detach().clone(), gm._scaling.detach().clone(), loop.exp_avg.clone()])
    for s, t in zip(*res):
        assert torch.equal(s, t)
    assert not torch.equal(res[0][0], init)
    with pytest.raises(ValueError, match="poses_2d"):
        loop.new_scene(None, heatmaps=torch.zeros((V, J, sc.H, sc.W), device=device))
    loop.world = 2                                       # what a view-sharded rank sees
    with pytest.raises(ValueError, match="view-sharded"):
        loop.new_scene(None, poses_2d=p2d)
    loop.world = 1


@pytest.mark.parametrize("early_stopping", ["no_stopping", "opt_early_stopping"])
def test_detections_produced_late_on_the_callers_stream(device, early_stopping):
    """The caller's stream is made late with the bounded sks_prof_spin, the detections are produced on it behind the spin
    (the buffer holds NaN until then), and the sequence is optimised from that stream at once: every batch's DLT, on its own
    stream, must be ordered behind the detections -- or it triangulates NaN."""
    from skelsplat_amd.loop import FramePipeline, OptEarlyStopping
    sc, model = _scene(device)
    N, iters = 7, 80
    p2d = _detections(sc, N, device)
    es = early_stopping if early_stopping == "no_stopping" else OptEarlyStopping(4, ES_TOL)
    pipe = FramePipeline(model(), sc.cameras, frames=3, streams=2, dataset="h36m", early_stopping=es)
    want, want_init = pipe.optimize_sequence(None, p2d, iterations=iters, groups_per_graph=4, interleave=40, return_initial=True)
    want, want_init = want.clone(), want_init.clone()          # (this call also captured the graphs: the next is short)
    assert bool(torch.isfinite(want).all())
    late = torch.full_like(p2d, float("nan"))
    caller = torch.cuda.Stream(device)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(caller):
        _lib.check(_lib.load().sks_prof_spin(SPIN_US, ctypes.c_void_p(caller.cuda_stream)), "sks_prof_spin")
        late.copy_(p2d)
        got, got_init = pipe.optimize_sequence(None, late, iterations=iters, groups_per_graph=4, interleave=40,
                                               return_initial=True)
        got, got_init = got.clone(), got_init.clone()           # read at once, on the caller's stream
    caller.synchronize()
    assert torch.equal(got_init, want_init)
    assert torch.equal(got, want)
