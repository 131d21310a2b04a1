"""The fused initial guess on the device (sks_fuse_predictions, directly and through initial_guess.fuse_predictions) and
`poses_3d=` through FrameBatchLoop, FramePipeline and MultiViewLoop: against the reference's golden results by the counted
tolerances of tests/fuse_cases.py, against the restatement and the host path under `valid` masks and per-frame rigs, bit for
bit against itself across batch sizes, batch positions and streams, and bit for bit against the same loops given the fused
points explicitly."""
import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, triangulation
from skelsplat_amd.initial_guess import fuse_predictions
from tests import fuse_cases as fc

pytestmark = pytest.mark.gpu

NORM = {"64": torch.float64, "32": torch.float32}
NP_NORM = {"64": np.float64, "32": np.float32}
V, J = 4, 17


def _dev(a, device):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=device)


def _direct(device, P, p3d, p2d, valid, variant, stream=None):
    """One sks_fuse_predictions call with every output: (xyz f32, xyz f64, ebar, n_used) as arrays.  The inputs go in as the
    dtype they have (float32 -> the float pointer, float64 -> the double pointer)."""
    N, Vn, Jn = p3d.shape[:3]
    Pd, Xd, xd = _dev(np.asarray(P, np.float64), device), _dev(p3d, device), _dev(p2d, device)
    vd = None if valid is None else _dev(valid.astype(np.uint8), device)
    xyz = torch.full((N, Jn, 3), 7.0, dtype=torch.float32, device=device)
    xyz64 = torch.full((N, Jn, 3), 7.0, dtype=torch.float64, device=device)
    err = torch.full((N, Vn, Jn), 7.0, dtype=torch.float64, device=device)
    n_used = torch.full((N, Jn), -1, dtype=torch.int32, device=device)
    X64, x64 = Xd.dtype == torch.float64, xd.dtype == torch.float64
    rc = _lib.load().sks_fuse_predictions(N, Vn, Jn, Pd.data_ptr(), Vn * 12 if Pd.dim() == 4 else 0,
                                          None if X64 else Xd.data_ptr(), Xd.data_ptr() if X64 else None,
                                          None if x64 else xd.data_ptr(), xd.data_ptr() if x64 else None,
                                          None if vd is None else vd.data_ptr(), int(variant == "32"), xyz.data_ptr(),
                                          xyz64.data_ptr(), err.data_ptr(), n_used.data_ptr(),
                                          (stream or torch.cuda.current_stream(device)).cuda_stream)
    _lib.check(rc, "sks_fuse_predictions")
    torch.cuda.synchronize(device)
    return xyz.cpu().numpy(), xyz64.cpu().numpy(), err.cpu().numpy(), n_used.cpu().numpy()


@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("name", fc.NAMES)
def test_golden_cases(device, name, variant):
    """Every golden case, both variants, through the entry itself and through fuse_predictions: the same bits, held to the
    reference by the counted bounds (the measured need is printed).  A case stored as float32 goes through all four
    float / double pointer combinations: widening is exact, so all four give the same bits."""
    c = fc.case(name)
    N, Vn, Jn = c["p3d"].shape[:3]
    xyz, xyz64, err, n_used = _direct(device, c["proj"], c["p3d"], c["p2d"], None, variant)
    fc.check_case(name, variant, xyz64, err, tag="device")
    assert (n_used == Vn).all() and np.array_equal(xyz, xyz64.astype(np.float32))
    if c["p3d"].dtype == np.float32:
        for t3, t2 in ((np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)):
            other = _direct(device, c["proj"], c["p3d"].astype(t3), c["p2d"].astype(t2), None, variant)
            for a, b in zip(other, (xyz, xyz64, err, n_used)):
                assert np.array_equal(a, b), (t3, t2)
    # the public interface: the same launch
    P, X, x = _dev(c["proj"], device), _dev(c["p3d"], device), _dev(c["p2d"], device)
    out = torch.empty((N, Jn, 3), dtype=torch.float64, device=device)
    ret, e, n = fuse_predictions(P, X, x, norm_dtype=NORM[variant], out=out, return_errors=True, return_n_used=True)
    assert ret is out and e.device.type == "cuda" and n.dtype == torch.int32
    assert np.array_equal(out.cpu().numpy(), xyz64) and np.array_equal(e.cpu().numpy(), err) and np.array_equal(n.cpu().numpy(), n_used)
    f32 = fuse_predictions(c["proj"], X, c["p2d"], norm_dtype=NORM[variant])          # host matrices and detections are uploaded
    assert f32.dtype == torch.float32 and f32.device.type == "cuda" and np.array_equal(f32.cpu().numpy(), xyz)
    if Vn == 1:
        assert np.array_equal(xyz64, c["p3d"][:, 0].astype(np.float64))


def test_only_the_outputs_asked_for_are_written(device):
    c = fc.case("v4j17n3")
    P, X, x = _dev(c["proj"], device), _dev(c["p3d"], device), _dev(c["p2d"], device)
    both = _direct(device, c["proj"], c["p3d"], c["p2d"], None, "64")
    lib = _lib.load()
    st = torch.cuda.current_stream(device).cuda_stream
    only32 = torch.empty((3, J, 3), dtype=torch.float32, device=device)
    _lib.check(lib.sks_fuse_predictions(3, V, J, P.data_ptr(), 0, None, X.data_ptr(), None, x.data_ptr(), None, 0, only32.data_ptr(),
                                        None, None, None, st), "sks_fuse_predictions")
    only64 = torch.empty((3, J, 3), dtype=torch.float64, device=device)
    _lib.check(lib.sks_fuse_predictions(3, V, J, P.data_ptr(), 0, None, X.data_ptr(), None, x.data_ptr(), None, 0, None,
                                        only64.data_ptr(), None, None, st), "sks_fuse_predictions")
    assert np.array_equal(only32.cpu().numpy(), both[0]) and np.array_equal(only64.cpu().numpy(), both[1])
    with pytest.raises(ValueError, match="65 views"):
        fuse_predictions(torch.zeros((65, 3, 4), dtype=torch.float64, device=device), torch.zeros((1, 65, 2, 3), device=device),
                         torch.zeros((1, 65, 2, 2), device=device))


@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("name", ("v4j17n3", "v5j19n2", "v31j19n2", "v33j2n1"))
def test_masks_on_the_device(device, name, variant):
    """Joints with 0, 1 and 2 kept views beside partly masked ones: a left-out view is out in both roles and is NEVER READ (its
    candidate and detection are NaN here)."""
    c = fc.case(name)
    N, Vn, Jn = c["p3d"].shape[:3]
    valid = fc.masks(N, Vn, Jn, seed=5)
    want, want_e, want_n = fc.restate(c["proj"], c["p3d"], c["p2d"], valid, NP_NORM[variant])
    p3d, p2d = c["p3d"].copy(), c["p2d"].copy()
    p3d[~valid], p2d[~valid] = np.nan, np.nan
    xyz, xyz64, err, n_used = _direct(device, c["proj"], p3d, p2d, valid, variant)
    assert np.array_equal(n_used, want_n) and (n_used[:, 0] == 0).all() and (n_used[:, 1] == 1).all()
    if Jn > 2 and Vn >= 2:
        assert (n_used[:, 2] == 2).all()
    assert np.array_equal(np.isnan(xyz64), np.isnan(want)) and np.isnan(xyz64[:, 0]).all() and np.isnan(xyz[:, 0]).all()
    assert np.array_equal(np.isnan(err), ~valid)
    al = fc.allowance(c, variant, result=want)
    ok = want_n > 0
    diff = np.abs(xyz64 - want)
    print(name, variant, "masked: max |device - restatement| =", diff[ok].max(), "allowance", al["fused"].max())
    assert (diff[ok] <= np.broadcast_to(al["fused"], diff.shape)[ok]).all()
    assert (np.abs(err - want_e)[valid] / want_e[valid] <= al["err"][valid]).all()
    one = want_n == 1
    cand = np.einsum("nvj,nvjk->njk", (valid & one[:, None]).astype(np.float64), c["p3d"].astype(np.float64))
    assert np.array_equal(xyz64[one], cand[one])                      # one kept view: that candidate, exactly
    # the host path is a second witness; a host mask is uploaded by the public interface
    host = fuse_predictions(c["proj"], c["p3d"], c["p2d"], valid=valid, norm_dtype=NORM[variant], out=torch.empty((N, Jn, 3), dtype=torch.float64))
    assert (np.abs(xyz64 - host.numpy())[ok] <= np.broadcast_to(al["fused"], diff.shape)[ok]).all()
    got = fuse_predictions(c["proj"], _dev(p3d, device), _dev(p2d, device), valid=valid, norm_dtype=NORM[variant])
    assert np.array_equal(got.cpu().numpy(), xyz, equal_nan=True)
    # an all-true mask is no mask, bit for bit
    full = _direct(device, c["proj"], c["p3d"], c["p2d"], np.ones_like(valid), variant)
    none = _direct(device, c["proj"], c["p3d"], c["p2d"], None, variant)
    for a, b in zip(full, none):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("variant", fc.VARIANTS)
def test_one_rig_per_frame(device, variant):
    """(N,V,3,4) matrices, N = 3 with different cameras in every frame's slots: each frame equals, bit for bit, the same frame
    run alone with its own (V,3,4) rig, and sits within the counted bounds of the restatement."""
    c = fc.case("v4j17n3")
    rigs = np.stack([c["proj"][[0, 1, 2, 3]], c["proj"][[2, 0, 3, 1]], c["proj"][[3, 2, 1, 0]]])
    valid = fc.masks(3, V, J, seed=9)
    for mask in (None, valid):
        whole = _direct(device, rigs, c["p3d"], c["p2d"], mask, variant)
        want = fc.restate(rigs, c["p3d"], c["p2d"], mask, NP_NORM[variant])[0]
        for n in range(3):
            alone = _direct(device, rigs[n], c["p3d"][n:n + 1], c["p2d"][n:n + 1], None if mask is None else mask[n:n + 1], variant)
            for a, b in zip(alone, whole):
                assert np.array_equal(a[0], b[n], equal_nan=True), n
            cn = dict(proj=rigs[n], p3d=c["p3d"][n:n + 1], p2d=c["p2d"][n:n + 1])
            al = fc.allowance(cn, variant, result=want[n:n + 1])
            assert float(al["fused64"].max()) < 1e-6
            assert np.all((np.abs(whole[1][n] - want[n]) <= al["fused"][0]) | np.isnan(want[n]))
        assert not np.array_equal(whole[1][1], _direct(device, rigs[0], c["p3d"], c["p2d"], mask, variant)[1][1], equal_nan=True)
    got = fuse_predictions(_dev(rigs, device), _dev(c["p3d"], device), _dev(c["p2d"], device), norm_dtype=NORM[variant])
    assert np.array_equal(got.cpu().numpy(), _direct(device, rigs, c["p3d"], c["p2d"], None, variant)[0])


@pytest.mark.parametrize("variant", fc.VARIANTS)
def test_a_frame_does_not_depend_on_its_batch_its_place_or_its_stream(device, variant):
    """Frame 0 of the H36M case alone == the same frame first, in the middle and last of an N = 37 batch (37 x 17 problems:
    several workgroups and a partial last one) == the same frame on a side stream: every output, bit for bit."""
    c = fc.case("v4j17n3")
    rng = np.random.default_rng(21)
    alone = _direct(device, c["proj"], c["p3d"][:1], c["p2d"][:1], None, variant)
    for at in (0, 18, 36):
        idx = 1 + np.arange(37) % 2
        p3d = c["p3d"][idx] + rng.normal(0, 5.0, (37, V, J, 3))
        p2d = c["p2d"][idx] + rng.normal(0, 1.0, (37, V, J, 2))
        p3d[at], p2d[at] = c["p3d"][0], c["p2d"][0]
        batch = _direct(device, c["proj"], p3d, p2d, None, variant)
        for a, b in zip(alone, batch):
            assert np.array_equal(a[0], b[at]), at
        assert np.isfinite(batch[1]).all() and not np.array_equal(batch[1][(at + 1) % 37], alone[1][0])
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    other = _direct(device, c["proj"], c["p3d"][:1], c["p2d"][:1], None, variant, stream=side)
    for a, b in zip(alone, other):
        assert np.array_equal(a, b)
    # all Panoptic views: two problems per wavefront
    c = fc.case("v31j19n2")
    whole = _direct(device, c["proj"], c["p3d"], c["p2d"], None, variant)
    last = _direct(device, c["proj"], c["p3d"][1:], c["p2d"][1:], None, variant)
    for a, b in zip(last, whole):
        assert np.array_equal(a[0], b[1])


# ------------------------------------------------------------------------------------------------ through the loops
def _scene(dev, seed=9):
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    W, H = 64, 64
    sc = SyntheticScene("h36m", n_views=V, seed=seed, W=W, H=H, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5, device=dev)

    def model():
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9,
                                                scaling_modifier=1.0, device=dev)
        gm.training_setup()
        return gm
    return sc, model


def _inputs(sc, n, dev, seed=11):
    """frame f: the scene's detections with a pixel of noise, and per-view predictions = ground truth + 20-50 mm of noise per
    view; float32 on the device"""
    rng = np.random.default_rng(seed)
    base = np.asarray(sc.poses_2d, np.float32)
    p2d = np.stack([base + rng.normal(0, 1.0, base.shape) for f in range(n)]).astype(np.float32)
    gt = np.asarray(sc.pose_3d_gt, np.float64)
    p3d = np.stack([gt[None] + rng.normal(0, 1.0, (V,) + gt.shape) * np.linspace(20.0, 50.0, V)[:, None, None]
                    for f in range(n)]).astype(np.float32)
    return torch.as_tensor(p2d, device=dev), torch.as_tensor(p3d, device=dev)


def test_frame_batch_fuses_into_xyz(device):
    from skelsplat_amd.loop import FrameBatchLoop
    sc, model = _scene(device)
    F = 4
    p2d, p3d = _inputs(sc, F, device)
    drop = torch.zeros((F, V, J), dtype=torch.bool)
    drop[0, 1, [2, 5]] = True
    drop[2, 0, 7] = True
    drop[2, 3, 7] = True
    a = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", use_graph=True)
    b = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", use_graph=True)
    for masks in (None, drop):
        valid = None if masks is None else ~masks
        init = fuse_predictions(sc.cameras, p3d, p2d, valid=valid, out=torch.empty((F, J, 3), dtype=torch.float32, device=device))
        assert bool(torch.isfinite(init).all())
        assert not torch.equal(init, triangulation.triangulate_sequence(sc.cameras, p2d, valid=valid))
        a.new_scenes(None, poses_2d=p2d, drop_masks=masks, poses_3d=p3d)
        assert torch.equal(a.xyz, init)                                     # before the first step
        b.new_scenes(init, poses_2d=p2d, drop_masks=masks)
        a.run(8, groups_per_graph=4)
        b.run(8, groups_per_graph=4)
        assert torch.equal(a.xyz, b.xyz) and torch.equal(a.exp_avg, b.exp_avg) and not torch.equal(a.xyz, init)
    # the dropped views stay out: their predictions and detections may hold anything (the heat-maps drop those planes too)
    poisoned = p3d.clone()
    poisoned[drop] = float("nan")
    a.new_scenes(None, poses_2d=p2d, drop_masks=drop, poses_3d=poisoned)
    assert torch.equal(a.xyz, init)
    a.new_scenes(None, poses_2d=p2d.cpu().numpy(), drop_masks=drop.numpy(), poses_3d=p3d.cpu().numpy())     # host arrays
    assert torch.equal(a.xyz, init)
    with pytest.raises(ValueError, match="poses_3d"):
        a.new_scenes(init, poses_2d=p2d, poses_3d=p3d)
    with pytest.raises(ValueError, match=r"\(F,V,J,3\)"):
        a.new_scenes(None, poses_2d=p2d, poses_3d=p3d[:2])
    with pytest.raises(ValueError, match="poses_2d"):
        a.new_scenes(None, poses_3d=p3d)


@pytest.mark.parametrize("early_stopping", ["no_stopping", "opt_early_stopping"])
def test_sequences_from_predictions(device, early_stopping):
    """N = 6 frames through 4 frames per launch on 2 streams (a padded last batch), both branches of the pipeline:
    optimize_sequence(None, p2d, poses_3d=p3d) starts from fuse_predictions' bits and ends where
    optimize_sequence(points=that guess, p2d) ends."""
    from skelsplat_amd.loop import FramePipeline, FrameBatchLoop, OptEarlyStopping
    sc, model = _scene(device)
    N, iters = 6, 12
    p2d, p3d = _inputs(sc, N, device)
    init = fuse_predictions(sc.cameras, p3d, p2d, out=torch.empty((N, J, 3), dtype=torch.float32, device=device))
    es = lambda: early_stopping if early_stopping == "no_stopping" else OptEarlyStopping(4, 3e-4)
    pipe = FramePipeline(model(), sc.cameras, frames=4, streams=2, dataset="h36m", early_stopping=es())
    got, initial = pipe.optimize_sequence(None, p2d, iterations=iters, groups_per_graph=4, interleave=8, return_initial=True,
                                          poses_3d=p3d)
    got, initial = got.clone(), initial.clone()
    assert torch.equal(initial, init)
    want = pipe.optimize_sequence(init, p2d, iterations=iters, groups_per_graph=4, interleave=8)
    assert torch.equal(got, want) and not torch.equal(got, init)
    # predictions as a host array; one loop, one stream
    fb = FrameBatchLoop(model(), sc.cameras, 4, dataset="h36m", use_graph=True, early_stopping=es())
    one, initial = fb.optimize_sequence(None, p2d, iterations=iters, groups_per_graph=4, return_initial=True,
                                        poses_3d=p3d.cpu().numpy())
    assert torch.equal(one, want) and torch.equal(initial, init)
    with pytest.raises(ValueError, match="poses_3d"):
        pipe.optimize_sequence(init, p2d, poses_3d=p3d)
    with pytest.raises(ValueError, match="poses_3d"):
        pipe.optimize_sequence(None, p2d, poses_3d=p3d[:3])


def test_multi_view_loop_fuses_its_frame(device):
    from skelsplat_amd.loop import MultiViewLoop
    sc, model = _scene(device)
    p2d, p3d = (t[1] for t in _inputs(sc, 2, device))
    init = fuse_predictions(sc.cameras, p3d, p2d)
    assert tuple(init.shape) == (J, 3) and init.dtype == torch.float32
    res = []
    for pts in (None, init):
        gm = model()
        loop = MultiViewLoop(gm, sc.cameras, torch.zeros((V, J, sc.H, sc.W), device=device), dataset="h36m")
        loop.new_scene(pts, poses_2d=p2d, poses_3d=p3d if pts is None else None)
        assert torch.equal(gm._xyz.detach(), init)
        loop.run(8)
        res.append(gm._xyz.detach().clone())
    assert torch.equal(res[0], res[1]) and not torch.equal(res[0], init)
    with pytest.raises(ValueError, match="poses_3d"):
        loop.new_scene(init, poses_2d=p2d, poses_3d=p3d)
    loop.world = 2                                       # what a view-sharded rank sees
    with pytest.raises(ValueError, match="view-sharded"):
        loop.new_scene(None, poses_2d=p2d, poses_3d=p3d)
    loop.world = 1
