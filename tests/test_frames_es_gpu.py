"""Per-frame early stopping on the frame-batched path (sks_loop_fused_step_es through FrameBatchLoop / FramePipeline): every
frame stops at its own iteration and ends bit for bit where a MultiViewLoop running it alone with the same criterion ends."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, J = 4, 17
TOL = 3e-4          # with these frames: stops at 94, 122, 138 (inside groups) and two frames that run to the end
ITERS = 160
NOISE3, NOISE2 = 20.0, 2.0


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


def _reference(dev, sc, model, pt, p2d_f, tol, iters):
    """MultiViewLoop on one frame with the same criterion, on the heat-map planes the batched generator describes.  Its loss
    constants (sum gt^2, count) are the ones a frame batch takes from the heat-map factors (a one-frame batch's), so that both
    feed the criterion the same numbers: planes and factors give the same gradients, but their fp64 totals may differ in the
    last bits."""
    from skelsplat_amd.loop import MultiViewLoop, FrameBatchLoop, OptEarlyStopping
    from skelsplat_amd.heatmaps import generate_heatmaps
    one = FrameBatchLoop(model(dev), sc.cameras, 1, dataset="h36m")
    one.new_scenes(pt[None], poses_2d=p2d_f[None])
    gm = model(dev)
    hm0 = torch.zeros((V, J, sc.H, sc.W), device=dev)
    loop = MultiViewLoop(gm, sc.cameras, hm0, dataset="h36m", sparse=True,
                         early_stopping=OptEarlyStopping(window_size=4, repeat_tolerance=tol))
    assert loop._es_device and len(loop.size_groups) == 1
    gm.reset_from_points(pt)
    for slots, vb, gt, stats, idx in loop.size_groups:
        generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                          torch.tensor(p2d_f[slots], device=dev), [sc.cameras[k] for k in slots], out=gt, views=vb,
                          totals=stats.totals)
    loop.stats_all.totals.copy_(one.stats_all.totals)
    loop.run(iters)
    return loop, gm


def _state(fb, f):
    return [fb.xyz[f], fb.scaling[f], fb.rotation[f], fb.opacity[f], fb.exp_avg[f], fb.exp_avg_sq[f], fb.accumulated_grads[f],
            fb.counters[f]]


def _check_preconditions(stops, iters):
    hit = [s for s in stops if s is not None]
    assert len(set(hit)) >= 2, stops                   # frames stop at different iterations
    assert any(s % 4 != 0 for s in hit), stops         # ... one of them inside an accumulation group
    assert any(s is None for s in stops), stops        # ... and one frame runs to the end
    assert all(s <= iters for s in hit), stops


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_frame_batch_stops_every_frame_like_its_own_loop(device, use_graph):
    """F = 4 frames, OptEarlyStopping(4, TOL): each frame's parameters, moments, slots and counters equal a MultiViewLoop that
    runs it alone with the criterion; hipGraphs of 4 groups replay past the stops.  A second batch through the same loop
    (new_scenes) starts the criterion over and reproduces the first."""
    from skelsplat_amd.loop import FrameBatchLoop, OptEarlyStopping
    sc, model = _scene(device)
    F = 4
    pts, p2d = _frames(sc, F)
    fb = FrameBatchLoop(model(device), sc.cameras, F, dataset="h36m", use_graph=use_graph,
                        early_stopping=OptEarlyStopping(window_size=4, repeat_tolerance=TOL))
    fb.new_scenes(pts, poses_2d=p2d)
    fb.run(ITERS, groups_per_graph=4)
    got = [[t.clone() for t in _state(fb, f)] for f in range(F)]
    stops = fb.stopped_at
    refs = [_reference(device, sc, model, pts[f], p2d[f], TOL, ITERS) for f in range(F)]
    ref_stops = [loop.stopped_at for loop, _ in refs]
    _check_preconditions(ref_stops, ITERS)
    assert stops == ref_stops, (stops, ref_stops)
    for f, (loop, gm) in enumerate(refs):
        want = [gm._xyz.detach(), gm._scaling.detach(), gm._rotation.detach(), gm._opacity.detach(), loop.exp_avg,
                loop.exp_avg_sq, loop.accumulated_grads, loop.counters]
        for k, (a, b) in enumerate(zip(got[f], want)):
            assert torch.equal(a, b), (f, k)
        assert int(fb.counters[f, 0]) == (stops[f] or ITERS)      # the frame's own iteration
    assert fb.iteration <= ITERS
    # the next batch through the same loop: flags and criterion state start over
    fb.new_scenes(pts, poses_2d=p2d)
    assert fb.stopped_at == [None] * F and int(fb._es_state.abs().sum()) == 0
    fb.run(ITERS, groups_per_graph=4)
    assert fb.stopped_at == stops
    for f in range(F):
        for k, (a, b) in enumerate(zip(_state(fb, f), got[f])):
            assert torch.equal(a, b), (f, k)


def test_a_stopped_frame_is_frozen(device):
    """After its stopping launch nothing of a stopped frame changes -- parameters, moments, slots, counters, geometry radii,
    loss sums, criterion state -- while the frames still running move on."""
    from skelsplat_amd.loop import FrameBatchLoop, OptEarlyStopping
    sc, model = _scene(device)
    F = 4
    pts, p2d = _frames(sc, F)
    fb = FrameBatchLoop(model(device), sc.cameras, F, dataset="h36m",
                        early_stopping=OptEarlyStopping(window_size=4, repeat_tolerance=TOL))
    fb.new_scenes(pts, poses_2d=p2d)

    def snap(f):
        return [t.clone() for t in _state(fb, f)] + [fb._sums[f * V:(f + 1) * V].clone(),
                                                      fb._fstate.radii[f * V:(f + 1) * V].clone(), fb._es_state[f].clone()]
    frozen, moving = None, None
    while fb.iteration < ITERS:
        fb.step_group(parameters_untouched=True)
        torch.cuda.synchronize()
        st = fb.stopped_at
        if frozen is None and any(s is not None for s in st):
            f = next(i for i, s in enumerate(st) if s is not None)
            frozen = (f, st[f], snap(f))
            live = [i for i, s in enumerate(st) if s is None]
            assert live
            moving = (live[-1], fb.xyz[live[-1]].clone())
    assert frozen is not None and moving is not None
    f, it, before = frozen
    assert fb.stopped_at[f] == it and int(fb.counters[f, 0]) == it
    for k, (a, b) in enumerate(zip(snap(f), before)):
        assert torch.equal(a, b), k
    assert not torch.equal(fb.xyz[moving[0]], moving[1])


def test_no_stopping_is_the_loop_without_the_argument(device):
    from skelsplat_amd.loop import FrameBatchLoop
    sc, model = _scene(device)
    pts, p2d = _frames(sc, 3)
    res = []
    for kw in ({}, {"early_stopping": "no_stopping"}):
        fb = FrameBatchLoop(model(device), sc.cameras, 3, dataset="h36m", use_graph=True, **kw)
        assert fb._es is None and fb._es_state is None
        fb.new_scenes(pts, poses_2d=p2d)
        fb.run(40, groups_per_graph=4)
        assert fb.stopped_at == [None] * 3
        res.append([t.clone() for f in range(3) for t in _state(fb, f)])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_frame_pipeline_with_early_stopping(device):
    """N = 5 frames through 2 loops of 2 frames on 2 streams (the last batch padded), each stream taking its next batch as
    soon as its own is done: joints and stopping iterations equal the per-frame MultiViewLoop runs."""
    from skelsplat_amd.loop import FramePipeline, OptEarlyStopping
    sc, model = _scene(device)
    N = 5
    pts, p2d = _frames(sc, N)
    pipe = FramePipeline(model(device), sc.cameras, frames=2, streams=2, dataset="h36m",
                         early_stopping=OptEarlyStopping(window_size=4, repeat_tolerance=TOL))
    out = pipe.optimize_sequence(pts, p2d, iterations=ITERS, groups_per_graph=4, interleave=16)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (N, J, 3) and pipe.stopped_at.dtype == torch.int64 and tuple(pipe.stopped_at.shape) == (N,)
    refs = [_reference(device, sc, model, pts[f], p2d[f], TOL, ITERS) for f in range(N)]
    want_stops = torch.tensor([loop.stopped_at or 0 for loop, _ in refs], dtype=torch.int64)
    assert torch.equal(pipe.stopped_at.cpu(), want_stops), (pipe.stopped_at, want_stops)
    assert int((want_stops == 0).sum()) >= 1 and len(set(want_stops.tolist()) - {0}) >= 2
    for f, (loop, gm) in enumerate(refs):
        assert torch.equal(out[f], gm._xyz.detach()), f


def test_refusals(device):
    from skelsplat_amd import _lib
    from skelsplat_amd.loop import FrameBatchLoop, OptEarlyStopping
    sc, model = _scene(device)
    with pytest.raises(ValueError, match="MultiViewLoop"):
        FrameBatchLoop(model(device), sc.cameras, 2, early_stopping=lambda loss: False)
    for w in (0, 17):
        with pytest.raises(ValueError, match="window"):
            FrameBatchLoop(model(device), sc.cameras, 2, early_stopping=OptEarlyStopping(window_size=w))
    used = OptEarlyStopping(window_size=4)
    used(0.5)
    with pytest.raises(ValueError, match="history"):
        FrameBatchLoop(model(device), sc.cameras, 2, early_stopping=used)
    # the C entry point: no criterion state, a window out of range
    lib = _lib.load()
    fb = FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m", early_stopping="opt_early_stopping")
    fb.new_scenes(*_frames(sc, 2))
    st, stats = fb._fstate, fb.stats_all
    feats = fb.features
    accum = torch.zeros(1 << 20, dtype=torch.uint8, device=device)

    def call(es_state, window):
        return lib.sks_loop_fused_step_es(
            st.views.V, fb.P, fb.C, st.views.W, st.views.H, st.views.viewmatrix.data_ptr(), st.views.projmatrix.data_ptr(),
            st.views.tanfovx, st.views.tanfovy, feats.data_ptr(), st.scale_modifier, st.flags, st.radii.data_ptr(),
            st.geom.data_ptr(), None, stats.totals.data_ptr(), accum.data_ptr(), fb._sums.data_ptr(), fb._packed.data_ptr(),
            fb.accumulated_grads.data_ptr(), 0xF, 3, fb.xyz.data_ptr(), fb.scaling.data_ptr(), fb.rotation.data_ptr(),
            fb.opacity.data_ptr(), fb.exp_avg.data_ptr(), fb.exp_avg_sq.data_ptr(), fb.counters.data_ptr(), 4, fb._sched,
            fb._lrs, fb._adam, 1e-5, fb._limb, st.views.wh, None, st.frames, stats.factors.ptrs, es_state, window,
            ctypes.c_float(1e-3), None, torch.cuda.current_stream(device).cuda_stream)
    for es_state, window, text in ((None, 4, "es_state"), (fb._es_state.data_ptr(), 0, "window"),
                                   (fb._es_state.data_ptr(), 17, "window")):
        rc = call(es_state, window)
        assert rc < 0
        assert text in lib.sks_last_error().decode()
    assert lib.sks_version() >= 12
