"""csrc/sks_bones.hip on the device: sks_bone_measure, sks_bone_lengths and sks_bone_project against the op-by-op restatement of
tests/bones_ref.py on every case of tests/bones_cases.py, bit for bit in every output -- each definition is a fixed sequence of
+ - x / sqrt in float64 compiled without contraction, and the medians are selected by integer counts; the same bits on a second
stream and inside a captured graph replayed twice; sks_bones_launch's claims; and the loops' switch (set_bone_constraint) through
FramePipeline and FrameBatchLoop."""
import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, skeleton
from tests import bones_cases as BC

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return None if a is None else torch.as_tensor(a, device=device)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(got, want):
    g, w = _bits(got), _bits(want)
    return g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w)


def _same(got, want):
    """Equal values with NaN where the other has NaN (a freshly made NaN carries no promise about its payload)."""
    g = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return g.shape == want.shape and g.dtype == want.dtype and np.array_equal(g, want, equal_nan=True)


def _lengths(c, device):
    return skeleton.bone_lengths(_dev(c["xyz"], device), c["bones"], _dev(c["cov6"], device), _dev(c["valid"], device),
                                 _dev(c["groups"], device), c["max_sigma"], n_groups=c["G"])


def _project(c, target, device):
    return skeleton.project_to_lengths(_dev(c["xyz"], device), c["bones"], _dev(target, device), _dev(c["cov6"], device),
                                       _dev(c["valid"], device), _dev(c["groups"], device), c["floor"], c["iters"], c["tol"])


@pytest.mark.parametrize("name", BC.NAMES)
def test_the_three_kernels_equal_the_restatement(device, name):
    c, ref = BC.cases()[name], BC.reference(name)
    got = _lengths(c, device)
    assert got.measured.dtype == torch.float32 and got.n_used.dtype == torch.int32
    for key in ("measured", "length", "mad", "n_used"):
        assert _same(getattr(got, key), ref[key]), key
    proj = _project(c, ref["target"], device)
    assert _same(proj.residual, ref["residual"]) and _same(proj.n_trips, ref["n_trips"]) and _same(proj.n_active, ref["n_active"])
    # the joints in every bit: a joint that was not moved carries its input's NaN payload and sign
    assert _same_bits(proj.joints, ref["joints"])
    # projecting onto the device's own lengths is the same call (the lengths are the same bits)
    if c["target"] is None:
        assert _same_bits(_project(c, got.length.cpu().numpy(), device).joints, ref["joints"])


def test_second_stream_and_captured_graph(device):
    """One case with covariances, masks and a gate: the three launches on a non-default stream, and captured into a graph that is
    replayed twice, give the bits of the default stream."""
    c, ref = BC.cases()["degenerate_rows"], BC.reference("degenerate_rows")
    x, cov6, valid, target = [_dev(c[k], device) for k in ("xyz", "cov6", "valid")] + [_dev(ref["target"], device)]

    def run():
        lengths = skeleton.bone_lengths(x, c["bones"], cov6, valid, max_sigma_mm=50.0)
        return lengths, skeleton.project_to_lengths(x, c["bones"], target, cov6, valid, cov_floor=c["floor"])
    want_l, want_p = run()
    torch.cuda.synchronize()
    assert _same_bits(want_p.joints, ref["joints"])
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        got_l, got_p = run()
    side.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(got_l + got_p, want_l + want_p))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        run()                                   # (warm: the allocator's blocks exist before the capture)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            cap_l, cap_p = run()
    for _ in range(2):
        for t in cap_l + cap_p:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(cap_l + cap_p, want_l + want_p))


@pytest.mark.parametrize("N,J,B,G", [(1, 2, 1, 1), (5, 17, 16, 1), (1025, 19, 18, 3), (300, 32, 31, 256)])
def test_launch_claims(N, J, B, G):
    """sks_bones_launch (host only) against the layout the header states: one lane per (frame, bone) in workgroups of 256; one
    workgroup of 256 threads per (group, bone) with a 256-bin histogram and three words; one wavefront per frame whose LDS holds
    x, Sigma, u, the right-hand side, a column, S, 64 residuals (doubles) and the bones' and joints' flags (ints)."""
    got = _lib.bones_launch(N, J, B, G)
    assert got == dict(measure_groups=-(-N * B // 256), measure_threads=256, lengths_groups=G * B, lengths_threads=256,
                       lengths_lds_bytes=(256 + 3) * 4, project_groups=N, project_threads=64,
                       project_lds_bytes=8 * (3 * J + 6 * J + 3 * B + B + B + B * B + 64) + 4 * (B + J))
    assert got["project_lds_bytes"] <= 16 * 1024 and got["project_threads"] == 64
    with pytest.raises(RuntimeError, match="bones_launch"):
        _lib.bones_launch(N, 33, B, G)


def test_refusals_of_the_library(device):
    x = torch.zeros((2, 3, 3), device=device)
    L = torch.ones((1, 3), device=device)
    with pytest.raises(ValueError, match="forest"):
        skeleton.bone_lengths(x, ((0, 1), (1, 2), (2, 0)))
    bn = np.array([[0, 1], [1, 2], [2, 0]], dtype=np.int32)
    lib = _lib.load()
    out = torch.empty((2, 3), device=device)
    rc = lib.sks_bone_measure(2, 3, 3, bn.ctypes.data, x.data_ptr(), None, None, 0.0, out.data_ptr(), None)
    assert rc != 0 and b"forest" in lib.sks_last_error()
    o = torch.empty_like(x)
    r, t, a = torch.empty(2, device=device), torch.empty(2, dtype=torch.int32, device=device), torch.empty(2, dtype=torch.int32, device=device)
    rc = lib.sks_bone_project(2, 3, 3, bn.ctypes.data, x.data_ptr(), None, None, None, 1, L.data_ptr(), 0.0, 16, 1e-3, o.data_ptr(),
                              r.data_ptr(), t.data_ptr(), a.data_ptr(), None)
    assert rc != 0 and b"forest" in lib.sks_last_error()
    ok = np.array([[0, 1], [1, 2]], dtype=np.int32)
    rc = lib.sks_bone_project(2, 3, 2, ok.ctypes.data, x.data_ptr(), None, None, None, 1, L.data_ptr(), 0.0, 17, 1e-3, o.data_ptr(),
                              r.data_ptr(), t.data_ptr(), a.data_ptr(), None)
    assert rc != 0 and b"max_iters" in lib.sks_last_error()
    rc = lib.sks_bone_project(2, 3, 2, ok.ctypes.data, x.data_ptr(), None, None, None, 1, L.data_ptr(), 0.0, 16, 1e-3, x.data_ptr(),
                              r.data_ptr(), t.data_ptr(), a.data_ptr(), None)
    assert rc != 0 and b"overlaps" in lib.sks_last_error()
    rc = lib.sks_bone_lengths(2, 3, out.data_ptr(), None, 2, out.data_ptr(), out.data_ptr(), t.data_ptr(), None)
    assert rc != 0 and b"n_groups" in lib.sks_last_error()
    with pytest.raises(ValueError, match="float32"):
        skeleton.project_to_lengths(x.double(), ok, L[:, :2])
    with pytest.raises(ValueError, match="lengths"):
        skeleton.project_to_lengths(x, ok, L)
    with pytest.raises(ValueError, match="cov6"):
        skeleton.project_to_lengths(x, ok, L[:, :2], cov6=torch.zeros((2, 3, 5), device=device))


V, J, F, N, ITERS = 4, 17, 8, 32, 16


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


def test_pipeline_switch(device):
    """H36M, 4 views, 32 frames at 8 per launch on 2 streams, 16 iterations, keep_gaussians=True; joint 13 of frame 3 has NaN
    detections: unobserved, NaN in the joints returned and -- a joint only inactive bones touch -- in the constrained ones."""
    from skelsplat_amd.loop import FrameBatchLoop, FramePipeline
    from skelsplat_amd.scene import DATASETS
    sc, model = _scene(device)
    rng = np.random.default_rng(11)
    base = np.asarray(sc.poses_2d, np.float32)
    p2d = np.stack([base + rng.normal(0, 1.0 + 0.05 * f, base.shape) for f in range(N)]).astype(np.float32)
    p2d[3, :, 13] = np.nan
    p2d = torch.as_tensor(p2d, device=device)
    bones = DATASETS["h36m"]["bones"]
    run = lambda pipe: pipe.optimize_sequence(None, p2d, iterations=ITERS, groups_per_graph=4, interleave=8)
    kept = lambda pipe: [t.clone() for t in (pipe.gaussians.uncertainty().cov6,)]

    never = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m", keep_gaussians=True)
    never.set_smoothing(2, degree=1, cov_floor=1.0)
    want = run(never).clone()
    want_smoothed, want_kept = [t.clone() for t in never.smoothed], kept(never)
    assert never.constrained is None and never.bone_lengths is None

    # with smoothing on: the smoothed joints under the fit's covariance; everything else keeps its bits
    pipe = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m", keep_gaussians=True)
    pipe.set_smoothing(2, degree=1, cov_floor=1.0)
    assert pipe.set_bone_constraint("dataset", cov_floor=1.0) is pipe
    got = run(pipe)
    assert _same_bits(got, want) and all(_same_bits(a, b) for a, b in zip(pipe.smoothed, want_smoothed))
    assert all(_same_bits(a, b) for a, b in zip(kept(pipe), want_kept))
    sm = pipe.smoothed
    lengths = skeleton.bone_lengths(sm.joints, bones, sm.cov6)
    again = skeleton.project_to_lengths(sm.joints, bones, lengths.length, sm.cov6, cov_floor=1.0)
    assert all(_same_bits(a, b) for a, b in zip(pipe.bone_lengths, lengths))
    assert all(_same_bits(a, b) for a, b in zip(pipe.constrained, again))
    assert tuple(pipe.constrained.joints.shape) == (N, J, 3) and int(pipe.constrained.n_active.min()) == 16
    assert int(pipe.constrained.n_trips.max()) >= 1 and not _same_bits(pipe.constrained.joints, sm.joints)

    # without smoothing: the joints returned under the kept Gaussians' covariance; the unobserved joint stays NaN, its bones idle
    pipe.set_smoothing(None)
    pipe.set_bone_constraint(bones, symmetric=True, max_sigma_mm=1e4)
    got = run(pipe)
    assert _same_bits(got, want) and pipe.smoothed is None
    cov6 = pipe.gaussians.uncertainty().cov6
    lengths = skeleton.bone_lengths(got, bones, cov6, max_sigma_mm=1e4)
    pairs = [skeleton.bone_index(bones, DATASETS["h36m"]["limbs"])[i:i + 2] for i in (0, 2)]
    sym = skeleton.symmetrize(lengths.length, pairs)
    assert float(sym[0, pairs[0][0]]) == float(sym[0, pairs[0][1]]) and _same_bits(pipe.bone_lengths.length, sym)
    again = skeleton.project_to_lengths(got, bones, sym, cov6)
    assert all(_same_bits(a, b) for a, b in zip(pipe.constrained, again))
    # (joint 13, the left wrist, ends one bone: at most 15 of the 16 are active in its frame and N - 1 frames enter its median)
    assert bool(torch.isnan(pipe.constrained.joints[3, 13]).all()) and int(pipe.constrained.n_active[3]) <= 15
    assert int(pipe.bone_lengths.n_used[0, skeleton.bone_index(bones, [(12, 13)])[0]]) <= N - 1

    # groups, unit covariance; the wrong length is refused when the sequence is known; off again leaves nothing behind
    groups = torch.tensor([0] * 20 + [1] * 12)
    pipe.set_bone_constraint(bones, use_covariance=False, groups=groups)
    got = run(pipe)
    lengths = skeleton.bone_lengths(got, bones, groups=groups.to(device), n_groups=2)
    assert tuple(pipe.bone_lengths.length.shape) == (2, 16) and all(_same_bits(a, b) for a, b in zip(pipe.bone_lengths, lengths))
    again = skeleton.project_to_lengths(got, bones, lengths.length, groups=groups.to(device))
    assert all(_same_bits(a, b) for a, b in zip(pipe.constrained, again))
    pipe.set_bone_constraint(bones, groups=[0, 1, 2])
    with pytest.raises(ValueError, match="set_bone_constraint"):
        run(pipe)
    pipe.set_bone_constraint(None)
    assert _same_bits(run(pipe), want) and pipe.constrained is None and pipe.bone_lengths is None

    # the covariances need the kept Gaussians; the arguments are checked when the switch is set; one loop alone carries it too
    bare = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m")
    with pytest.raises(ValueError, match="keep_gaussians=True"):
        bare.set_bone_constraint("dataset")
    with pytest.raises(ValueError, match="forest"):
        bare.set_bone_constraint(((0, 1), (1, 0)), use_covariance=False)
    with pytest.raises(ValueError, match="max_iters"):
        bare.set_bone_constraint("dataset", use_covariance=False, max_iters=17)
    assert all(l._bones is None for l in bare.loops)
    loop = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", keep_gaussians=True).set_bone_constraint("dataset")
    one = loop.optimize_sequence(None, p2d, iterations=ITERS, groups_per_graph=4)
    cov6 = loop.gaussians.uncertainty().cov6
    lengths = skeleton.bone_lengths(one, bones, cov6)
    again = skeleton.project_to_lengths(one, bones, lengths.length, cov6)
    assert all(_same_bits(a, b) for a, b in zip(loop.constrained, again)) and bool(torch.isnan(one[3, 13]).all())
