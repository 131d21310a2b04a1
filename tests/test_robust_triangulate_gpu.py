"""Outlier rejection by two-view consensus on the device (sks_triangulate_robust through
triangulation.triangulate_sequence(reject_px=..)) and through the loops: against the numpy oracle of
tests/robust_tri_cases.py where it is decisive, bit for bit against the plain kernel given the returned mask, and bit for
bit against itself across batch sizes, positions, streams and rigs."""
import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, triangulation
from tests import robust_tri_cases as RC
from tests import tri_cases as TC
from tests.test_triangulate_gpu import _detections, _scene, _state

pytestmark = pytest.mark.gpu

V, J = 4, 17


def _robust(P, x, dev, valid=None, **kw):
    kw.setdefault("reject_px", RC.TAU)
    return triangulation.triangulate_sequence(torch.as_tensor(P, device=dev), torch.as_tensor(x, device=dev),
                                              valid=None if valid is None else torch.as_tensor(valid, device=dev),
                                              homogeneous=True, return_n_used=True, return_inliers=True, **kw)


def _compare(got, ref, what):
    xyzw, n_used, inl, n_cons = (t.cpu().numpy() for t in got)
    ok = ref["decisive"]
    print(what, "joints:", ok.size, "not decisive:", int((~ok).sum()), "decided by the sum:", int(ref["tie"].sum()))
    assert inl.dtype == np.bool_ and n_cons.dtype == np.int32 and n_used.dtype == np.int32
    assert np.array_equal(inl.transpose(0, 2, 1)[ok], ref["inliers"].transpose(0, 2, 1)[ok])
    assert np.array_equal(n_cons[ok], ref["n_consensus"][ok]) and np.array_equal(n_used[ok], ref["n_used"][ok])
    assert np.array_equal(np.isnan(xyzw[ok]), np.isnan(ref["xyzw"][ok]))
    err = np.nanmax(np.abs(xyzw[ok] - ref["xyzw"][ok]), initial=0.0)
    print(what, "max abs difference of the joints to the oracle:", err)
    assert np.allclose(xyzw[ok], ref["xyzw"][ok], equal_nan=True, **TC.GOLDEN_TOL), err


def _same(a, b):
    """bit for bit, NaN included"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------- 1. 2. 3. 6. oracle, refit, large threshold
@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_device_equals_the_oracle_and_refits_with_the_plain_kernel(device, shape):
    P, x, bad = RC.generated(*shape)
    got = _robust(P, x, device)
    _compare(got, RC.generated_oracle(*shape), f"{shape[0]} V={shape[1]}")
    xyzw, n_used, inl, n_cons = got
    assert np.array_equal(inl.cpu().numpy(), ~bad)
    # the refit IS the plain kernel with valid = inliers
    Pd, xd = torch.as_tensor(P, device=device), torch.as_tensor(x, device=device)
    plain, n_plain = triangulation.triangulate_sequence(Pd, xd, valid=inl, homogeneous=True, return_n_used=True)
    assert _same(xyzw, plain) and _same(n_used, n_plain)
    assert _same(triangulation.triangulate_sequence(Pd, xd, reject_px=RC.TAU), triangulation.triangulate_sequence(Pd, xd, valid=inl))
    # float32 detections: their own decisions (the oracle on the rounded detections), the same refit
    x32 = x.astype(np.float32)
    got32 = _robust(P, x32, device)
    if shape[1] <= 12:      # (the larger oracles take seconds: there the corrupted views, 60 px and more past the threshold)
        _compare(got32, RC.oracle(P, x32.astype(np.float64)), "float32")
    assert np.array_equal(got32[2].cpu().numpy(), ~bad)
    assert _same(got32[0], triangulation.triangulate_sequence(Pd, torch.as_tensor(x32, device=device), valid=got32[2],
                                                              homogeneous=True))
    # a threshold nothing exceeds: every kept view, the plain kernel's bits
    rng = np.random.default_rng(3)
    valid = torch.as_tensor(rng.random(x.shape[:3]) > 0.15, device=device)
    for v in (None, valid):
        plain, n_plain = triangulation.triangulate_sequence(Pd, xd, valid=v, homogeneous=True, return_n_used=True)
        big = _robust(P, x, device, valid=v, reject_px=1e9)
        assert _same(big[0], plain) and _same(big[1], n_plain)
        assert torch.equal(big[2], torch.ones_like(inl) if v is None else v)
        assert torch.equal(big[3], n_plain)


@pytest.mark.parametrize("m", [3, 2])
def test_hand_cases(device, m):
    P, x, valid = RC.hand()
    ref = RC.hand_oracle(m)
    got = _robust(P, x, device, valid=valid, min_inliers=m)
    _compare(got, ref, f"hand m={m}")
    xyzw, n_used, inl, n_cons = (t.cpu().numpy() for t in got)
    for name, (f, j) in RC.HAND.items():
        assert ref["decisive"][f, j], name
        assert np.array_equal(inl[f, :, j], ref["inliers"][f, :, j]) and n_cons[f, j] == ref["n_consensus"][f, j], name
    f, j = RC.HAND["split"]
    assert n_cons[f, j] == 2 and (inl[f, :, j].all() if m == 3 else inl[f, :, j].sum() == 2)
    f, j = RC.HAND["behind"]
    assert inl[f, :, j].tolist() == ([True] * 4 if m == 3 else [False, False, True, True])
    host = triangulation.triangulate_sequence(P, x, valid=valid, homogeneous=True, reject_px=RC.TAU, min_inliers=m,
                                              return_inliers=True)
    assert np.array_equal(host[1], inl) and np.array_equal(host[2], n_cons)
    assert np.allclose(host[0], xyzw, equal_nan=True, **TC.GOLDEN_TOL)


# ------------------------------------------------------------------------------------- 4. 5. batch, position, stream, rig
@pytest.mark.parametrize("shape", [RC.SHAPES[2], RC.SHAPES[3], RC.SHAPES[4]], ids=[RC.SHAPE_IDS[k] for k in (2, 3, 4)])
def test_a_frame_does_not_depend_on_batch_position_stream_or_rig(device, shape):
    P, x, bad = RC.generated(*shape)
    n = x.shape[0]
    Pd = torch.as_tensor(P, device=device)
    many = torch.as_tensor(x[np.arange(37) % n], device=device)          # frame f of 37 = frame f % n
    whole = _robust(Pd, many, device)
    side = torch.cuda.Stream(device)
    for f in (0, 1, n - 1):
        alone = _robust(Pd, many[f:f + 1], device)
        five = _robust(Pd, many[f:f + 5], device)
        moved = _robust(Pd, many[f + n - 3:f + n + 2], device)            # the same frame at position 3 of another batch
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            other = _robust(Pd, many[f:f + 1], device)
        side.synchronize()
        for k in range(4):
            assert _same(alone[k][0], whole[k][f]) and _same(five[k][0], whole[k][f]) and _same(moved[k][3], whole[k][f]), (f, k)
            assert _same(other[k][0], whole[k][f]), (f, k)
    rigs = Pd[None].repeat(37, 1, 1, 1).contiguous()
    per = _robust(rigs, many, device)
    assert all(_same(a, b) for a, b in zip(per, whole))


# ------------------------------------------------------------------------------------------------------- 7. buffers
@pytest.mark.parametrize("shape", [RC.SHAPES[1], RC.SHAPES[2], RC.SHAPES[4]], ids=[RC.SHAPE_IDS[k] for k in (1, 2, 4)])
def test_the_entry_point_stays_inside_its_buffers(device, shape):
    """guard rows on both sides of inliers, n_consensus, xyz, xyzw and n_used keep their canaries"""
    P, x, bad = RC.generated(*shape)
    N, Vn, Jn = bad.shape
    Pd, xd = torch.as_tensor(P, device=device), torch.as_tensor(x, device=device)
    inl = torch.full((N + 2, Vn, Jn), 77, dtype=torch.uint8, device=device)
    cons = torch.full((N + 2, Jn), -777, dtype=torch.int32, device=device)
    used = torch.full((N + 2, Jn), -777, dtype=torch.int32, device=device)
    xyz = torch.full((N + 2, Jn, 3), 777.0, dtype=torch.float32, device=device)
    xyzw = torch.full((N + 2, Jn, 4), 777.0, dtype=torch.float64, device=device)
    rc = _lib.load().sks_triangulate_robust(N, Vn, Jn, Pd.data_ptr(), 0, None, xd.data_ptr(), None, RC.TAU, 3, inl[1:].data_ptr(),
                                            cons[1:].data_ptr(), xyz[1:].data_ptr(), xyzw[1:].data_ptr(), used[1:].data_ptr(),
                                            torch.cuda.current_stream(device).cuda_stream)
    assert rc == 0
    want = _robust(P, x, device)
    assert _same(xyzw[1:-1], want[0]) and _same(used[1:-1], want[1]) and _same(cons[1:-1], want[3])
    assert torch.equal(inl[1:-1], want[2].to(torch.uint8)) and _same(xyz[1:-1], want[0][..., :3].to(torch.float32))
    for big, canary in ((inl, 77), (cons, -777), (used, -777), (xyz, 777.0), (xyzw, 777.0)):
        assert bool((big[0] == canary).all()) and bool((big[-1] == canary).all())


# ------------------------------------------------------------------------------------------------------- 9. refusals
def test_the_c_abi_refuses_with_its_own_texts(device):
    lib = _lib.load()
    P = torch.zeros((V, 3, 4), dtype=torch.float64, device=device)
    x = torch.zeros((1, V, J, 2), device=device)
    inl = torch.zeros((1, V, J), dtype=torch.uint8, device=device)
    out = torch.zeros((1, J, 3), device=device)

    def call(tau=20.0, m=3, inliers=inl.data_ptr(), views=V, xyz=out.data_ptr()):
        return lib.sks_triangulate_robust(1, views, J, P.data_ptr(), 0, x.data_ptr(), None, None, tau, m, inliers, None, xyz,
                                          None, None, None)
    for kw, text in ((dict(tau=0.0), "reject_px"), (dict(tau=-3.0), "reject_px"), (dict(tau=float("nan")), "reject_px"),
                     (dict(tau=float("inf")), "reject_px"), (dict(m=1), "min_inliers"), (dict(m=65), "min_inliers"),
                     (dict(inliers=None), "missing inliers"), (dict(views=65), "65 views"), (dict(xyz=None), "xyz / xyzw")):
        assert call(**kw) < 0, kw
        err = lib.sks_last_error().decode()
        assert text in err and "triangulate_robust" in err, (kw, err)
    assert bool((inl == 0).all()) and bool((out == 0).all())
    with pytest.raises(ValueError, match="reject_px"):
        triangulation.triangulate_sequence(P, x, reject_px=0.0)


# ------------------------------------------------------------------------------------------------ 8. through the loops
def _corrupted_detections(sc, n, dev, seed=23):
    """_detections with two (view, joint) detections per frame moved 50 px towards the image centre (they stay inside)"""
    p2d = _detections(sc, n, dev).cpu().numpy()
    rng = np.random.default_rng(seed)
    bad = np.zeros((n, V, J), dtype=bool)
    centre = np.array([sc.W / 2.0, sc.H / 2.0], dtype=np.float32)
    for f in range(n):
        for j in rng.choice(J, size=2, replace=False):
            v = int(rng.integers(0, V))
            d = centre - p2d[f, v, j]
            p2d[f, v, j] += 50.0 * d / max(float(np.linalg.norm(d)), 1e-3)
            bad[f, v, j] = True
    return torch.as_tensor(p2d, device=dev), bad


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_frame_batch_rejects_and_then_runs_as_with_explicit_points(device, use_graph):
    from skelsplat_amd.loop import FrameBatchLoop
    sc, model = _scene(device)
    F = 4
    p2d, bad = _corrupted_detections(sc, F, device)
    drop = torch.zeros((F, V, J), dtype=torch.bool)
    drop[1, 2, 6] = True
    for masks in (None, drop):
        valid = None if masks is None else ~masks
        init, inl, n_cons = triangulation.triangulate_sequence(sc.cameras, p2d, valid=valid, reject_px=RC.TAU, return_inliers=True)
        plain = triangulation.triangulate_sequence(sc.cameras, p2d, valid=valid)
        assert bool(torch.isfinite(init).all()) and not torch.equal(init, plain)
        assert not bool(inl.cpu()[torch.as_tensor(bad)].any())           # (every moved detection is rejected)
        a = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", use_graph=use_graph)
        b = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", use_graph=use_graph)
        assert a.set_outlier_rejection(RC.TAU) is a
        a.new_scenes(None, poses_2d=p2d, drop_masks=masks)
        assert torch.equal(a.xyz, init) and torch.equal(a.inliers, inl) and torch.equal(a.n_consensus, n_cons)
        assert a.inliers.dtype == torch.bool and tuple(a.inliers.shape) == (F, V, J)
        b.new_scenes(init, poses_2d=p2d, drop_masks=masks)
        a.run(40, groups_per_graph=4)
        b.run(40, groups_per_graph=4)
        for f in range(F):
            for k, (s, t) in enumerate(zip(_state(a, f), _state(b, f))):
                assert torch.equal(s, t), (f, k)
        assert not torch.equal(a.xyz, init)
        held = a.inliers
        a.new_scenes(None, poses_2d=p2d.cpu().numpy(), drop_masks=masks)      # the next batch, the same buffer
        assert a.inliers is held and torch.equal(a.xyz, init) and torch.equal(a.inliers, inl)
    with pytest.raises(ValueError, match="explicit points"):
        a.new_scenes(init, poses_2d=p2d)
    with pytest.raises(ValueError, match="poses_3d"):
        a.new_scenes(None, poses_2d=p2d, poses_3d=torch.zeros((F, V, J, 3), device=device))
    with pytest.raises(ValueError, match="min_inliers"):
        a.set_outlier_rejection(RC.TAU, min_inliers=1)
    a.set_outlier_rejection(None)           # off again: explicit points as ever, the plain triangulation
    a.new_scenes(init, poses_2d=p2d)
    a.new_scenes(None, poses_2d=p2d, drop_masks=masks)
    assert torch.equal(a.xyz, plain)


def test_sequences_reject_per_batch_and_keep_the_masks(device):
    """N = 7 frames through 3 frames per launch on 2 streams (a padded last batch) == one loop on one stream == the same
    pipeline given the robust initial joints; masks and counts of all N frames stay on the device."""
    from skelsplat_amd.loop import FrameBatchLoop, FramePipeline
    sc, model = _scene(device)
    N, iters = 7, 40
    p2d, bad = _corrupted_detections(sc, N, device)
    init, inl, n_cons = triangulation.triangulate_sequence(sc.cameras, p2d, reject_px=RC.TAU, return_inliers=True)
    assert {int(c) for c in n_cons.flatten().cpu()} == {2, 3, 4}        # with a consensus, and without (a fallback)
    pipe = FramePipeline(model(), sc.cameras, frames=3, streams=2, dataset="h36m")
    want = pipe.optimize_sequence(init, p2d, iterations=iters, groups_per_graph=4, interleave=20).clone()
    assert pipe.inliers is None and pipe.n_consensus is None
    pipe.set_outlier_rejection(RC.TAU)
    got, initial = pipe.optimize_sequence(None, p2d, iterations=iters, groups_per_graph=4, interleave=20, return_initial=True)
    assert torch.equal(initial, init) and torch.equal(got, want) and not torch.equal(got, init)
    assert torch.equal(pipe.inliers, inl) and torch.equal(pipe.n_consensus, n_cons)
    fb = FrameBatchLoop(model(), sc.cameras, 3, dataset="h36m", use_graph=True)
    fb.set_outlier_rejection(RC.TAU)
    one, initial = fb.optimize_sequence(None, p2d, iterations=iters, groups_per_graph=4, return_initial=True)
    assert torch.equal(one, want) and torch.equal(initial, init)
    assert torch.equal(fb.seq_inliers, inl) and torch.equal(fb.seq_n_consensus, n_cons)
    with pytest.raises(ValueError, match="explicit points"):
        pipe.optimize_sequence(init, p2d)
    with pytest.raises(ValueError, match="poses_3d"):
        fb.optimize_sequence(None, p2d, poses_3d=torch.zeros((N, V, J, 3), device=device))
    again = pipe.set_outlier_rejection(None).optimize_sequence(init, p2d, iterations=iters, groups_per_graph=4, interleave=20)
    assert torch.equal(again, want) and pipe.inliers is None


def test_multi_view_loop_rejects_in_its_frame(device):
    from skelsplat_amd.loop import MultiViewLoop
    sc, model = _scene(device)
    p2d, bad = _corrupted_detections(sc, 3, device)
    p2d, bad = p2d[2], bad[2]
    init, inl, n_cons = triangulation.triangulate_sequence(sc.cameras, p2d, reject_px=RC.TAU, return_inliers=True)
    assert tuple(init.shape) == (J, 3) and not inl.cpu().numpy()[bad].any()
    res = []
    for pts in (None, init):
        gm = model()
        loop = MultiViewLoop(gm, sc.cameras, torch.zeros((V, J, sc.H, sc.W), device=device), dataset="h36m")
        if pts is None:
            loop.set_outlier_rejection(RC.TAU).new_scene(None, poses_2d=p2d)
            assert torch.equal(loop.inliers, inl) and torch.equal(loop.n_consensus, n_cons)
        else:
            loop.new_scene(pts, poses_2d=p2d)
            assert loop.inliers is None
        assert torch.equal(gm._xyz.detach(), init)
        loop.run(24)
        res.append([gm._xyz.detach().clone(), gm._scaling.detach().clone(), loop.exp_avg.clone()])
    for s, t in zip(*res):
        assert torch.equal(s, t)
    with pytest.raises(ValueError, match="explicit points"):
        loop.set_outlier_rejection(RC.TAU).new_scene(init, poses_2d=p2d)
