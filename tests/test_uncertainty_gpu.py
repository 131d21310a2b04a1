"""csrc/sks_uncertainty.hip on the device, one launch at a time against the float64 references of tests/uncertainty_ref.py (rounding
allowances counted there, never chosen), and the loops that keep every frame's Gaussians (FrameBatchLoop / FramePipeline with
keep_gaussians=True).  Every allowance test prints its largest observed / allowed ratio (MEASUREMENTS.md, "uncertainty")."""
import math

import numpy as np
import pytest
import torch

from tests import uncertainty_cases as uc
from tests import uncertainty_ref as ur
from tests import util

pytestmark = pytest.mark.gpu


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _raw_joint_uncertainty(device, c, mod, with_gt=True):
    """One sks_joint_uncertainty launch on a case's ACTIVATED scales; buffers start as NaN.  -> host arrays cov6, spectrum, d2."""
    from skelsplat_amd import _lib
    N, P = c["xyz"].shape[:2]
    d = {k: torch.from_numpy(v).to(device) for k, v in c.items()}
    cov6 = torch.full((N, P, 6), float("nan"), device=device)
    spec = torch.full((N, P, 6), float("nan"), device=device)
    d2 = torch.full((N, P), float("nan"), device=device) if with_gt else None
    rc = _lib.load().sks_joint_uncertainty(N, P, d["xyz"].data_ptr(), d["scales"].data_ptr(), d["rot"].data_ptr(), float(mod),
                                           d["gt"].data_ptr() if with_gt else None, cov6.data_ptr(), spec.data_ptr(),
                                           d2.data_ptr() if with_gt else None, _stream(device))
    _lib.check(rc, "sks_joint_uncertainty")
    torch.cuda.synchronize()
    return cov6.cpu().numpy(), spec.cpu().numpy(), None if d2 is None else d2.cpu().numpy()


def _held(name, got, want, allow, seen):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), name
    ratio = float((np.abs(got - want) / allow).max())
    seen[name] = max(seen.get(name, 0.0), ratio)
    assert ratio <= 1.0, f"{name}: error is {ratio:.2f} x the counted rounding allowance"


# ------------------------------------------------------------------------------------------------ sks_joint_uncertainty
@pytest.mark.parametrize("mod", uc.MODIFIERS)
@pytest.mark.parametrize("N,P", uc.JOINT_SHAPES)
def test_joint_uncertainty_against_fp64(device, N, P, mod):
    c = uc.joint_case(N, P)
    s, q = c["scales"], c["rot"]
    cov6, spec, d2 = _raw_joint_uncertainty(device, c, mod)
    assert cov6.dtype == np.float32 and d2.shape == (N, P)
    # eigenvalues: bit for bit the sorted float32 (modifier x s)^2
    assert np.array_equal(spec[..., :3].view(np.uint32), np.ascontiguousarray(ur.eigenvalues_f32(s, mod)).view(np.uint32))
    seen = {}
    _held(f"cov6 (K_R {ur.K_R:g}, K_TERM {ur.K_TERM:g})", cov6, ur.cov6_of(ur.covariance_ref(s, q, mod)), ur.cov6_allowance(s, q, mod), seen)
    _held("trace", spec[..., 3], ur.trace_ref(s, mod), ur.trace_allowance(s, q, mod), seen)
    _held(f"det (K {ur.K_DET:g})", spec[..., 4], ur.det_ref(s, mod), ur.K_DET * ur.U32 * ur.det_ref(s, mod), seen)
    lam = ur.eigenvalues_ref(s, mod)
    _held(f"anisotropy (K {ur.K_ANISO:g})", spec[..., 5], lam[..., 0] / lam[..., 2], ur.K_ANISO * ur.U32 * lam[..., 0] / lam[..., 2], seen)
    want = ur.d2_ref(c["xyz"], c["gt"], s, q, mod)
    _held(f"d2 (K {ur.K_D2:g})", d2, want, ur.d2_allowance(c["xyz"], c["gt"], s, mod), seen)
    tight = float((np.abs(d2.astype(np.float64) - want) / (ur.U32 * ur.d2_basis_tight(c["xyz"], c["gt"], s, q, mod))).max())
    print(f"\n[joint_uncertainty N={N} P={P} modifier {mod}] observed / allowed: " + ", ".join(f"{k} {v:.3f}" for k, v in seen.items())
          + f"; d2 needs {tight:.2f} units of 2^-24 sum_k ((|R|^T |delta|)_k / sigma_k)^2")
    # without gt: the same cov6 / spectrum bits, d2 not asked for
    cov6_b, spec_b, none = _raw_joint_uncertainty(device, c, mod, with_gt=False)
    assert none is None and np.array_equal(cov6_b.view(np.uint32), cov6.view(np.uint32))
    assert np.array_equal(spec_b.view(np.uint32), spec.view(np.uint32))


def test_a_nan_joint_poisons_only_itself(device):
    """A NaN scale: that joint's covariance, trace, det and d2 are NaN; a NaN position: its d2 alone (the covariance does not read
    it); an inf scale: inf / NaN in its own outputs.  Every other joint keeps its bits."""
    N, P = 3, 17
    c = uc.joint_case(N, P)
    clean = _raw_joint_uncertainty(device, c, 1.3)
    bad = {k: v.copy() for k, v in c.items()}
    bad["scales"][1, 4, 1] = np.nan
    bad["xyz"][2, 0, 2] = np.nan
    bad["scales"][0, 16, 0] = np.inf
    bad["rot"][1, 9, 3] = np.nan
    cov6, spec, d2 = _raw_joint_uncertainty(device, bad, 1.3)
    hit = np.zeros((N, P), bool)
    for f, j in ((1, 4), (2, 0), (0, 16), (1, 9)):
        hit[f, j] = True
    for got, ref in zip((cov6, spec, d2), clean):
        assert np.array_equal(got[~hit].view(np.uint32), ref[~hit].view(np.uint32))
    assert np.isnan(cov6[1, 4]).all() and np.isnan(spec[1, 4, 3:5]).all() and np.isnan(d2[1, 4]) and np.isnan(spec[1, 4, :3]).sum() == 1
    assert np.isnan(cov6[1, 9]).all() and np.isnan(d2[1, 9]) and np.array_equal(spec[1, 9, :3], clean[1][1, 9, :3])
    assert np.isnan(d2[2, 0]) and np.array_equal(cov6[2, 0], clean[0][2, 0]) and np.array_equal(spec[2, 0], clean[1][2, 0])
    # (an infinite standard deviation: the joint's covariance is inf / NaN, and along that axis the ground truth is 0 sigma away)
    assert spec[0, 16, 0] == np.inf and not np.isfinite(cov6[0, 16]).all() and np.isfinite(d2[0, 16]) and d2[0, 16] >= 0


def test_a_frame_alone_and_inside_a_batch_of_300(device):
    """Frame 123 of 300 frames of 17 joints: its rows are the bits a launch with N = 1 gives it."""
    c = uc.joint_case(300, 17, seed=1)
    batch = _raw_joint_uncertainty(device, c, 1.3)
    for f in (0, 123, 299):
        alone = _raw_joint_uncertainty(device, {k: np.ascontiguousarray(v[f:f + 1]) for k, v in c.items()}, 1.3)
        for a, b in zip(alone, batch):
            assert np.array_equal(a[0].view(np.uint32), b[f].view(np.uint32)), f


def test_python_surface(device):
    """joint_uncertainty takes the RAW scaling (torch.exp, as the loops activate it), names its results, and drops the frame axis
    of a single pose; covariance_matrices is unpack_covariance."""
    from skelsplat_amd import uncertainty as un
    fx = uc.fixture()
    t = lambda k: torch.from_numpy(fx[k]).to(device)
    res = un.joint_uncertainty(t("xyz"), t("scaling_raw"), t("rotation_raw"), 1.3, gt=t("gt"))
    act = torch.exp(t("scaling_raw")).cpu().numpy()
    c = dict(xyz=fx["xyz"], scales=act, rot=fx["rotation_raw"], gt=fx["gt"])
    cov6, spec, d2 = _raw_joint_uncertainty(device, c, 1.3)
    for got, want in ((res.cov6, cov6), (res.eigenvalues, spec[..., :3]), (res.trace, spec[..., 3]), (res.det, spec[..., 4]),
                      (res.anisotropy, spec[..., 5]), (res.d2, d2)):
        assert np.array_equal(got.cpu().numpy(), want)
    # against the reference's own float32 covariance: both sit within the float32 allowance of the float64 value
    M = un.covariance_matrices(res.cov6).cpu().numpy()
    assert M.shape == (37, 17, 3, 3) and np.array_equal(M, np.swapaxes(M, -1, -2))
    scale = np.abs(fx["cov_m1"]).max(axis=(-1, -2), keepdims=True)
    assert float((np.abs(M - fx["cov_m1"]) / scale).max()) < 4e-6
    one = un.joint_uncertainty(t("xyz")[5], t("scaling_raw")[5], t("rotation_raw")[5], 1.3)
    assert one.d2 is None and tuple(one.cov6.shape) == (17, 6) and tuple(one.trace.shape) == (17,)
    assert torch.equal(one.cov6, res.cov6[5]) and torch.equal(one.eigenvalues, res.eigenvalues[5])
    with pytest.raises(ValueError, match="float32"):
        un.joint_uncertainty(t("xyz").double(), t("scaling_raw"), t("rotation_raw"))
    with pytest.raises(ValueError, match="rotation_raw"):
        un.joint_uncertainty(t("xyz"), t("scaling_raw"), t("rotation_raw")[:3])
    with pytest.raises(ValueError, match="sigma levels"):
        un.calibration(res.d2, ks=range(1, 10))
    with pytest.raises(ValueError, match="finite and > 0"):
        un.calibration(res.d2, ks=(1, 0))
    with pytest.raises(ValueError, match="valid must be"):
        un.calibration(res.d2, valid=[True] * 5)


# ------------------------------------------------------------------------------------------------ sks_calibration
@pytest.mark.parametrize("P", uc.CAL_P)
@pytest.mark.parametrize("N", uc.CAL_N)
def test_calibration_counts_are_exact(device, N, P):
    from skelsplat_amd import uncertainty as un
    d2, valid = uc.calibration_case(N, P)
    d = torch.from_numpy(d2).to(device)
    for K in uc.CAL_K:
        ks = uc.CAL_LEVELS[:K]
        for mask in (None, valid):
            res = un.calibration(d, ks=ks, valid=None if mask is None else torch.from_numpy(mask))
            want = ur.calibration_counts_ref(d2, ks, mask)
            counts = res["counts"].cpu().numpy()
            assert counts.dtype == np.int32 and counts.shape == (1 + P, K + 1)
            assert np.array_equal(counts, want), (N, P, K, mask is not None)
            overall, per_joint = ur.fractions_of(want)
            assert res["overall"].dtype == torch.float64 and tuple(res["per_joint"].shape) == (P, K)
            assert np.array_equal(res["overall"].cpu().numpy(), overall, equal_nan=True)
            assert np.array_equal(res["per_joint"].cpu().numpy(), per_joint, equal_nan=True)
    empty = un.calibration(d, ks=(1, 2, 3), valid=np.zeros(N, bool))           # a row without entries: NaN
    assert int(empty["counts"].abs().sum()) == 0 and bool(torch.isnan(empty["overall"]).all())


@pytest.mark.parametrize("i", [0, 1], ids=["modifier-1", "modifier-1.3"])
def test_fixture_fractions_are_the_references(device, i):
    """The whole chain on the fixture -- torch.exp, sks_joint_uncertainty, sks_calibration -- gives the fractions the reference's
    percent_inside_sigmas / percent_inside_sigmas_per_joint returned for the covariances the reference's model computed."""
    from skelsplat_amd import uncertainty as un
    fx = uc.fixture()
    t = lambda k: torch.from_numpy(fx[k]).to(device)
    res = un.joint_uncertainty(t("xyz"), t("scaling_raw"), t("rotation_raw"), float(fx["modifiers"][i]), gt=t("gt"))
    cal = un.calibration(res.d2, ks=[int(k) for k in fx["ks"]])
    assert np.array_equal(cal["overall"].cpu().numpy(), fx[f"overall_m{i}"])
    assert np.array_equal(cal["per_joint"].cpu().numpy(), fx[f"per_joint_m{i}"])
    assert int(cal["counts"][0, -1]) == 629


# ------------------------------------------------------------------------------------------------ sks_view_footprints
def _footprint_params(J, frames, seed):
    rng = np.random.default_rng(seed)
    shape = (frames, J) if frames > 1 else (J,)
    scaling_raw = np.log(rng.uniform(8.0, 90.0, shape + (3,))).astype(np.float32)
    q = rng.normal(0.0, 1.0, shape + (4,))
    rot = (q / np.linalg.norm(q, axis=-1, keepdims=True) * rng.uniform(0.5, 2.0, shape + (1,))).astype(np.float32)
    return torch.from_numpy(scaling_raw), torch.from_numpy(rot)


def _oracle_lambdas(means, scaling_raw, rot, cams, modifier):
    """ewa_lambdas_views per view at the view's own size -> (V,J,2) on the host."""
    from oracle import heatmaps_ref
    cov = heatmaps_ref.covariance_from_scaling_rotation(torch.exp(scaling_raw), rot, modifier)
    out = []
    for cam in cams:
        l1, l2 = heatmaps_ref.ewa_lambdas_views(means, cov, [cam], int(cam.image_width), int(cam.image_height))
        out.append(torch.stack([l1[0], l2[0]], -1))
    return torch.stack(out)


def _support(n, p, lam):
    """Samples of an axis of n the factor of variance `lam` is non-zero on: those within floor(4 sigma + 0.5) of the impulse at p,
    sigma the float32 root widened (sks_heatmap_factors' radius)."""
    r = math.floor(4.0 * float(np.sqrt(np.float32(lam))) + 0.5)
    return min(n - 1, p + r) - max(0, p - r) + 1


@pytest.mark.parametrize("W,H,mixed,frames", [(16, 16, False, 1), (40, 24, True, 1), (40, 24, False, 2)],
                         ids=["16x16", "40x24+36x20", "frames=2"])
def test_view_footprints_against_the_oracle_and_the_factors(device, W, H, mixed, frames):
    from skelsplat_amd import uncertainty as un
    from skelsplat_amd.heatmaps import heatmap_factors
    from skelsplat_amd.rasterizer import ViewBatch, HeatmapFactors
    from skelsplat_amd.scene import SyntheticScene
    modifier, Vf = 1.3, 2
    fx = 1145.0 * (W / 1000) * 1.5
    sc = SyntheticScene("h36m", n_views=Vf * frames, seed=4, W=W, H=H, ring=2500.0, fx=fx)
    cams = list(sc.cameras)
    if mixed:
        cams[1] = SyntheticScene("h36m", n_views=Vf, seed=4, W=W - 4, H=H - 4, ring=2500.0, fx=fx).cameras[1]
    V, J = len(cams), sc.n_joints
    means = torch.tensor(sc.pose_3d_init, dtype=torch.float32)
    if frames > 1:
        means = torch.stack([means + 15.0 * f for f in range(frames)])
    scaling_raw, rot = _footprint_params(J, frames, seed=W + frames)
    dev = lambda t: t.contiguous().to(device)
    views = ViewBatch.from_cameras([c.to(device) for c in cams], allow_mixed=True)
    lam, aniso = un.view_footprints(dev(means), dev(scaling_raw), dev(rot), views=views, scaling_modifier=modifier, frames=frames)
    torch.cuda.synchronize()
    assert tuple(lam.shape) == (V, J, 2) and tuple(aniso.shape) == (V, J)
    assert torch.equal(aniso, lam[..., 0] / lam[..., 1]) and bool((lam[..., 0] >= lam[..., 1]).all()) and bool((lam[..., 1] > 0).all())
    if frames > 1:
        want = torch.cat([_oracle_lambdas(means[f], scaling_raw[f], rot[f], cams[f * Vf:(f + 1) * Vf], modifier) for f in range(frames)])
    else:
        want = _oracle_lambdas(means, scaling_raw, rot, cams, modifier)
    for k, name in enumerate(("lambda1", "lambda2")):
        util.assert_close(name, lam[..., k].cpu(), want[..., k], rtol=2e-5, atol_scale=1e-6)
    # the same through cameras=: the same bits
    if frames == 1:
        lam_c, _ = un.view_footprints(dev(means), dev(scaling_raw), dev(rot), cameras=cams, scaling_modifier=modifier)
        assert torch.equal(lam_c, lam)
    # sks_heatmap_factors on the same inputs: sqrt(l1), sqrt(l2) give the truncation radii of the factors it writes
    p2d = torch.zeros((V, J, 2))
    for v, cam in enumerate(cams):
        p2d[v, :, 0], p2d[v, :, 1] = int(cam.image_width) // 2 + 0.4, int(cam.image_height) // 3 + 0.6
    out = HeatmapFactors(V, J, views.W, views.H, device)
    for t_ in (out.row, out.col):
        t_.zero_()
    heatmap_factors(dev(means), torch.exp(dev(scaling_raw)), dev(rot), dev(p2d), [c.to(device) for c in cams], modifier, views=views,
                    frames=frames, out=out)
    torch.cuda.synchronize()
    row, col, lam_h = out.row.cpu(), out.col.cpu(), lam.cpu().numpy()
    narrow = 0
    for v, cam in enumerate(cams):
        w_v, h_v = int(cam.image_width), int(cam.image_height)
        for j in range(J):
            assert int((row[v, j, :h_v] != 0).sum()) == _support(h_v, h_v // 3, lam_h[v, j, 0]), (v, j)
            assert int((col[v, j, :w_v] != 0).sum()) == _support(w_v, w_v // 2, lam_h[v, j, 1]), (v, j)
            narrow += _support(w_v, w_v // 2, lam_h[v, j, 1]) < w_v
    assert narrow > 0           # (some supports end inside the image: the count is a test of the radius)


def test_view_footprints_from_the_device_table(device):
    """A batch of two frames seen by the two rigs of a bank, swapped: the per-view scalars read from the table sks_rig_select
    filled (views_dev) give the bits the host form gives for the same cameras."""
    from skelsplat_amd import uncertainty as un
    from skelsplat_amd.rasterizer import ViewBatch
    from skelsplat_amd.rigs import RigBank, RigSelection
    from skelsplat_amd.scene import SyntheticScene
    W, H, Vf, F = 40, 24, 2, 2
    scenes = [SyntheticScene("h36m", n_views=Vf, seed=30 + r, W=W, H=H, ring=2500.0 + 400.0 * r, fx=1145.0 * (W / 1000) * (1.5 + 0.2 * r))
              for r in range(2)]
    bank = RigBank([list(s.cameras) for s in scenes], device)
    ids = [1, 0]
    cams = [c for r in ids for c in scenes[r].cameras]
    host = ViewBatch.from_cameras([c.to(device) for c in cams])
    table = ViewBatch(torch.zeros((F * Vf, 16), device=device), torch.zeros((F * Vf, 16), device=device), [1.0] * (F * Vf),
                      [1.0] * (F * Vf), W, H)
    sel = RigSelection(bank, F, table.viewmatrix, table.projmatrix)
    sel.select(ids)
    table.table = sel.table
    J = scenes[0].n_joints
    means = torch.stack([torch.tensor(scenes[0].pose_3d_init, dtype=torch.float32) + 10.0 * f for f in range(F)]).to(device)
    scaling_raw, rot = _footprint_params(J, F, seed=5)
    a, _ = un.view_footprints(means, scaling_raw.to(device), rot.to(device), views=host, scaling_modifier=1.3, frames=F)
    b, _ = un.view_footprints(means, scaling_raw.to(device), rot.to(device), views=table, scaling_modifier=1.3, frames=F)
    torch.cuda.synchronize()
    sel.check()
    assert torch.equal(table.viewmatrix, host.viewmatrix)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert not torch.equal(a[:Vf], a[Vf:])          # (the two rigs do see the joints differently)


# ------------------------------------------------------------------------------------------------ the loops keep the Gaussians
ITERS = 24                  # without early stopping: 6 groups
ES_ITERS, ES_TOL = 160, 3e-4        # with it: tests/test_frames_es_gpu.py's run, whose frames stop at 94, 122, 138 or never


@pytest.fixture(scope="module")
def alone(device):
    """Every frame of the sequence through FrameBatchLoop(frames=1) on its own, without and with early stopping: (xyz, scaling,
    rotation, opacity) per frame, computed once."""
    from skelsplat_amd.loop import FrameBatchLoop, OptEarlyStopping
    from tests.test_frames_es_gpu import _scene, _frames
    sc, model = _scene(device)
    pts, p2d = _frames(sc, 5)
    res = {}
    for es in (False, True):
        stop = OptEarlyStopping(window_size=4, repeat_tolerance=ES_TOL) if es else "no_stopping"
        fb = FrameBatchLoop(model(device), sc.cameras, 1, dataset="h36m", early_stopping=stop)
        rows, stops = [], []
        for f in range(5):
            fb.new_scenes(pts[f:f + 1], poses_2d=p2d[f:f + 1])
            fb.run(ES_ITERS if es else ITERS)
            torch.cuda.synchronize()
            rows.append([t[0].clone() for t in (fb.xyz, fb.scaling, fb.rotation, fb.opacity)])
            stops.append(fb.stopped_at[0])
        res[es] = (rows, stops)
    return sc, model, pts, p2d, res


def _assert_kept(g, out, rows):
    assert out is g.xyz
    for f, want in enumerate(rows):
        for name, got, w in zip(("xyz", "scaling", "rotation", "opacity"), (g.xyz[f], g.scaling[f], g.rotation[f], g.opacity[f]), want):
            assert torch.equal(got, w), (f, name)
    assert g.scaling.dtype == g.rotation.dtype == g.opacity.dtype == torch.float32
    assert tuple(g.scaling.shape) == (5, 17, 3) and tuple(g.rotation.shape) == (5, 17, 4) and tuple(g.opacity.shape) == (5, 17, 1)


@pytest.mark.parametrize("es", [False, True], ids=["no-stopping", "early-stopping"])
@pytest.mark.parametrize("kind", ["batch", "pipeline"])
def test_the_loops_keep_every_frames_gaussians(device, alone, kind, es):
    """N = 5 frames, frames=2 (a padded last batch), 24 iterations (160 with early stopping, so that frames do stop): every frame's kept scaling / rotation / opacity / xyz are bit for bit those of
    FrameBatchLoop(frames=1) running that frame alone; xyz is the tensor returned; uncertainty() is joint_uncertainty of the rows.
    With keep_gaussians=False the joints are the same and `gaussians` is None."""
    from skelsplat_amd import uncertainty as un
    from skelsplat_amd.loop import FrameBatchLoop, FramePipeline, OptEarlyStopping
    sc, model, pts, p2d, res = alone
    rows, stops = res[es]
    if es:
        assert any(s is not None and s % 4 for s in stops) and any(s is None for s in stops), stops      # (a stop inside a group)
    outs, iters = {}, ES_ITERS if es else ITERS
    for keep in (True, False):
        stop = OptEarlyStopping(window_size=4, repeat_tolerance=ES_TOL) if es else "no_stopping"
        if kind == "batch":
            loop = FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m", early_stopping=stop, keep_gaussians=keep)
            out = loop.optimize_sequence(pts, p2d, iterations=iters, groups_per_graph=2)
        else:
            loop = FramePipeline(model(device), sc.cameras, frames=2, streams=2, dataset="h36m", early_stopping=stop,
                                 keep_gaussians=keep)
            out = loop.optimize_sequence(pts, p2d, iterations=iters, groups_per_graph=2, interleave=8)
        torch.cuda.synchronize()
        outs[keep] = out
        if keep:
            g = loop.gaussians
            assert isinstance(g, un.SequenceGaussians)
            _assert_kept(g, out, rows)
            gt = torch.from_numpy(pts).to(device)
            a, b = g.uncertainty(gt, scaling_modifier=1.3), un.joint_uncertainty(g.xyz, g.scaling, g.rotation, 1.3, gt)
            for x, y in zip(a, b):
                assert torch.equal(x, y)
            lam, _ = g.footprints(sc.cameras, frame=4)
            want, _ = un.view_footprints(g.xyz[4], g.scaling[4], g.rotation[4], cameras=sc.cameras)
            assert torch.equal(lam, want) and tuple(lam.shape) == (4, 17, 2)
        else:
            assert loop.gaussians is None
            if kind == "pipeline":
                assert all(fb.gaussians is None and not fb.keep_gaussians for fb in loop.loops)
    assert torch.equal(outs[True], outs[False])
    # a sequence run with it off after one with it on leaves None behind
    if kind == "batch" and not es:
        loop = FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m", keep_gaussians=True)
        loop.optimize_sequence(pts[:2], p2d[:2], iterations=4, groups_per_graph=1)
        assert loop.gaussians is not None
        loop.keep_gaussians = False
        loop.optimize_sequence(pts[:2], p2d[:2], iterations=4, groups_per_graph=1)
        assert loop.gaussians is None


def test_kept_gaussians_write_the_references_ply(device, tmp_path):
    """A kept frame through io.save_ply_arrays is save_ply of a model that holds that frame."""
    from skelsplat_amd import io
    from skelsplat_amd.loop import FrameBatchLoop
    from tests.test_frames_es_gpu import _scene, _frames
    sc, model = _scene(device)
    pts, p2d = _frames(sc, 2)
    gm = model(device)
    loop = FrameBatchLoop(gm, sc.cameras, 2, dataset="h36m", keep_gaussians=True)
    loop.optimize_sequence(pts, p2d, iterations=8, groups_per_graph=1)
    g = loop.gaussians
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    io.save_ply_arrays(a, gm, g.xyz[1], g.scaling[1], g.rotation[1], g.opacity[1])
    held = model(device)
    with torch.no_grad():
        for t, v in zip((held._xyz, held._scaling, held._rotation, held._opacity), (g.xyz[1], g.scaling[1], g.rotation[1], g.opacity[1])):
            t.copy_(v.reshape(t.shape))
    io.save_ply(b, held)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert not torch.equal(g.scaling[1], gm._scaling.detach().reshape(g.scaling[1].shape))      # (the frame did move)
