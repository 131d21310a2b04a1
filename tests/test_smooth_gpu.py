"""csrc/sks_smooth.hip on the device: sks_smooth_sequence against reference (a) of tests/smooth_ref.py (np.linalg.lstsq on the
whitened design) on every case of tests/smooth_cases.py, at one float32 ulp for positions and one ulp plus 16 x E64 for velocity and
covariance -- and, since the fit is a fixed sequence of + - x / in float64, against restatement (b) bit for bit; the same frames
bit for bit wherever they stand in a sequence, on either stream, with or without the optional outputs; sks_eval_accel against its
reference with the entries counted equal; and the loops' switch (set_smoothing) through FramePipeline."""
import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, smoothing
from tests import smooth_cases as SC
from tests import smooth_ref as REF

pytestmark = pytest.mark.gpu

SEEN = {"joints": 0.0, "velocity": 0.0, "cov6": 0.0}      # the largest fraction of an allowance the device used, printed per test


def _dev(a, device):
    return None if a is None else torch.as_tensor(a, device=device)


def _run(c, device, **kw):
    return smoothing.smooth_sequence(_dev(c["xyz"], device), _dev(c["cov6"], device), _dev(c["weights"], device), _dev(c["valid"], device),
                                     _dev(c["groups"], device), c["h"], c["d"], c["taper"], c["floor"], **kw)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | ((a != a) & (b != b))).all())


@pytest.mark.parametrize("name", SC.NAMES)
def test_against_the_references(device, name):
    """Every case against (a): NaN pattern and n_used exactly; positions within one float32 ulp of |ref| (float64 leaves E64, far
    below half an ulp, so the last rounding moves the result by one ulp at most); velocity and covariance within one float32 ulp
    plus 16 x E64's absolute figures.  And against (b), the header's sequence on Python floats, rounded to float32: bit for bit
    -- the kernel IS that sequence, compiled without contraction; the allowance above is the binding bar either way."""
    c, a, b = SC.cases()[name], SC.reference(name, "a"), SC.reference(name, "b")
    got = _run(c, device)
    e = SC.e64()
    assert got.n_used.dtype == torch.int32 and np.array_equal(got.n_used.cpu().numpy(), a["n_used"])
    for key, extra in (("joints", 0.0), ("velocity", 16 * e["velocity"]), ("cov6", 16 * e["cov6"])):
        g = getattr(got, key).cpu().numpy()
        assert g.dtype == np.float32 and np.array_equal(np.isnan(g), np.isnan(a[key])), key
        allow = np.nan_to_num(SC.ulp32(a[key])) + extra
        diff = np.nan_to_num(np.abs(g.astype(np.float64) - a[key]))
        frac = float(np.where(diff > 0, diff / np.where(allow > 0, allow, 1.0), 0.0).max())      # (a NaN entry: 0 of an allowance of 0)
        SEEN[key] = max(SEEN[key], frac)
        assert np.all(diff <= allow), (key, frac)
    print(f"{name}: largest fraction of the allowance used so far:", SEEN)
    for key in ("joints", "velocity", "cov6"):
        assert np.array_equal(getattr(got, key).cpu().numpy(), b[key].astype(np.float32), equal_nan=True), key


def test_a_frame_does_not_depend_on_where_it_stands(device):
    """A group of frames smoothed alone equals, bit for bit, the same frames at offsets 0, 1, T - 1, T and T + 1 of a longer sequence
    with other groups around it; the same call gives equal bits on a second stream and with the optional outputs left out."""
    J, h = 17, 2
    T = SC.tile(J, h)
    rng = np.random.default_rng(7)
    L = T + 5                                             # longer than a tile: the group always crosses a seam
    cov6, C = SC.covariances(rng, L, J)
    xyz = SC.trajectory(rng, L, J, C)
    xyz[3, 2] = np.nan
    w = rng.uniform(0.5, 2.0, (L, J)).astype(np.float32)
    args = dict(half_window=h, degree=2, taper="tricube", cov_floor=0.25)
    alone = smoothing.smooth_sequence(_dev(xyz, device), _dev(cov6, device), _dev(w, device), **args)
    assert bool(torch.isfinite(alone.joints).all()) and int(alone.n_used.min()) >= 2
    for off in (0, 1, T - 1, T, T + 1):
        N = off + L + 7
        cov_n, Cn = SC.covariances(rng, N, J)
        xyz_n, w_n = SC.trajectory(rng, N, J, Cn), rng.uniform(0.5, 2.0, (N, J)).astype(np.float32)
        xyz_n[off:off + L], cov_n[off:off + L], w_n[off:off + L] = xyz, cov6, w
        groups = np.full(N, 5, dtype=np.int32)
        groups[:off], groups[off + L:] = 3, 9
        long = smoothing.smooth_sequence(_dev(xyz_n, device), _dev(cov_n, device), _dev(w_n, device), groups=_dev(groups, device), **args)
        for x, y in zip(alone, long):
            assert _same(x, y[off:off + L]), off
        assert bool(torch.isfinite(long.joints).all())
    # a second stream; the optional outputs requested or not
    x, c, wt = _dev(xyz, device), _dev(cov6, device), _dev(w, device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        other = smoothing.smooth_sequence(x, c, wt, **args)
        only = smoothing.smooth_sequence(x, c, wt, want=("joints",), **args)
        some = smoothing.smooth_sequence(x, c, wt, want=("joints", "n_used"), **args)
    side.synchronize()
    assert all(_same(p, q) for p, q in zip(alone, other))
    assert only.velocity is None and only.cov6 is None and only.n_used is None and _same(only.joints, alone.joints)
    assert some.cov6 is None and _same(some.joints, alone.joints) and _same(some.n_used, alone.n_used)


@pytest.mark.parametrize("N", [1, 2, 3, 257, 600])
def test_eval_accel(device, N):
    xyz, gt, groups = SC.accel_case(N)
    J = xyz.shape[1]
    ref, cnt = REF.accel_ref(xyz, gt, groups, 3)
    res = smoothing.sequence_accel(_dev(xyz, device), _dev(gt, device), _dev(groups, device), n_groups=3)
    got = res["table"].cpu().numpy()
    assert got.shape == (4, 2, 1 + J) and got.dtype == np.float64
    # the entries counted, through the placement of the NaNs: a mean is NaN exactly where nothing entered
    assert np.array_equal(np.isnan(got), cnt == 0)
    if N > 4:
        assert cnt[0, 0, 0] > cnt[0, 1, 0] > 0 and cnt[2].sum() == 0 and np.isnan(got[:, :, 1 + 5]).all()
    # a thread adds at most ceil(N / 256) frames x J terms one after the other, then 8 tree levels and the division: that many
    # roundings of the running sum on either side, relative to a mean of positive terms (the terms themselves are the same bits)
    terms = -(-N // 256) * J + 8 + 1
    assert np.allclose(got, ref, rtol=2 * terms * np.finfo(np.float64).eps, atol=0, equal_nan=True), np.nanmax(np.abs(got / ref - 1))
    assert _same(res["accel_joints"], res["table"][0, 0, 1:]) and _same(res["accel_error_groups"], res["table"][1:, 1, 0])
    # without ground truth and groups; the host path agrees
    plain = smoothing.sequence_accel(_dev(xyz, device))["table"].cpu().numpy()
    ref0, cnt0 = REF.accel_ref(xyz)
    assert plain.shape == (1, 2, 1 + J) and np.isnan(plain[0, 1]).all() and np.array_equal(np.isnan(plain), cnt0 == 0)
    assert np.allclose(plain, ref0, rtol=2 * terms * np.finfo(np.float64).eps, atol=0, equal_nan=True)
    again = smoothing.sequence_accel(_dev(xyz, device), _dev(gt, device), _dev(groups, device), n_groups=3)["table"]
    assert _same(again, res["table"])


V, J, F, N, ITERS = 4, 17, 4, 10, 24


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
    """H36M, 4 views, 4 frames per launch on 2 streams, 10 frames (a padded last batch), 24 iterations, keep_gaussians=True; joint
    13 of frame 3 has NaN detections: unobserved, NaN in the joints returned, filled in the smoothed ones."""
    from skelsplat_amd.loop import FrameBatchLoop, FramePipeline
    sc, model = _scene(device)
    rng = np.random.default_rng(11)
    base = np.asarray(sc.poses_2d, np.float32)
    p2d = np.stack([base + rng.normal(0, 1.0 + 0.3 * f, base.shape) for f in range(N)]).astype(np.float32)
    p2d[3, :, 13] = np.nan
    p2d = torch.as_tensor(p2d, device=device)
    run = lambda pipe: pipe.optimize_sequence(None, p2d, iterations=ITERS, groups_per_graph=4, interleave=8)
    never = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m", keep_gaussians=True)
    want = run(never).clone()
    assert never.smoothed is None
    pipe = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m", keep_gaussians=True)
    assert pipe.set_smoothing(2, degree=1, cov_floor=1.0) is pipe
    got = run(pipe)
    sm = pipe.smoothed
    # the joints returned are those of a pipeline that never had the switch; the unobserved joint stays NaN in them
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want)) and _same(got, want)
    assert bool(torch.isnan(got[3, 13]).all()) and int(torch.isnan(got).sum()) == 3
    # ... and the smoothed ones are smooth_sequence of them and of the kept Gaussians' covariances, with the gap filled
    cov6 = pipe.gaussians.uncertainty().cov6
    again = smoothing.smooth_sequence(got, cov6, half_window=2, degree=1, cov_floor=1.0)
    assert all(_same(x, y) for x, y in zip(sm, again))
    assert bool(torch.isfinite(sm.joints).all()) and int(sm.n_used[3, 13]) == 4 and int(sm.n_used[3, 12]) == 5
    assert tuple(sm.joints.shape) == (N, J, 3) and tuple(sm.cov6.shape) == (N, J, 6) and not _same(sm.joints, got)
    # groups, unit weights; the wrong length is refused when the sequence is known
    groups = torch.tensor([0] * 5 + [1] * 5)
    pipe.set_smoothing(2, degree=1, use_covariance=False, groups=groups)
    got2 = run(pipe)
    assert _same(got2, want)
    again = smoothing.smooth_sequence(got2, groups=groups.to(device), half_window=2, degree=1)
    assert all(_same(x, y) for x, y in zip(pipe.smoothed, again)) and int(pipe.smoothed.n_used[4, 0]) == 3
    pipe.set_smoothing(2, groups=[0, 1, 2])
    with pytest.raises(ValueError, match="set_smoothing"):
        run(pipe)
    # off again: nothing is left behind
    pipe.set_smoothing(None)
    assert _same(run(pipe), want) and pipe.smoothed is None
    # the covariances need the kept Gaussians; one loop alone carries the switch too
    bare = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m")
    with pytest.raises(ValueError, match="keep_gaussians=True"):
        bare.set_smoothing(2)
    with pytest.raises(ValueError, match="half_window"):
        bare.set_smoothing(40, use_covariance=False)
    loop = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", keep_gaussians=True).set_smoothing(2, degree=1, cov_floor=1.0)
    one = loop.optimize_sequence(None, p2d, iterations=ITERS, groups_per_graph=4)
    again = smoothing.smooth_sequence(one, loop.gaussians.uncertainty().cov6, half_window=2, degree=1, cov_floor=1.0)
    assert all(_same(x, y) for x, y in zip(loop.smoothed, again)) and bool(torch.isfinite(loop.smoothed.joints).all())
    assert bool(torch.isnan(one[3, 13]).all())
