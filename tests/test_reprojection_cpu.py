"""The reprojection error measured and minimised, on the host (skelsplat_amd/reprojection.py's numpy path) and in the restatement
the GPU tests use (tests/reproj_ref.py): against what the reference's own compute_reprojection_error returned, the claims of every
hard case shown on the restatement first, the refinement against scipy's Levenberg-Marquardt, its exact properties, and what the
library refuses on the host before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, reprojection
from tests import reproj_cases as RC
from tests import reproj_ref as REF
from tests import tri_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSE = os.path.join(ROOT, "tests", "golden", "reference_fuse.npz")
# Largest distance, in mm, between the restatement's result and scipy's least_squares(method="lm") run to its limits, per V, as
# measured by test_refinement_against_scipy's own cases (plain squares, tri_cases.sequence scenes, 3 frames of 17 or 19 joints):
# V = 2: 1.15e-2, V = 3: 2.49e-4, V = 4: 6.54e-5, V = 8: 7.13e-5, V = 31: 3.68e-5.  The bar is ten times the largest, because
# LM's own stopping is a threshold and not a limit.
SCIPY_MEASURED_MM = {2: 1.15e-2, 3: 2.49e-4, 4: 6.54e-5, 8: 7.13e-5, 31: 3.68e-5}
SCIPY_BAR_MM = 10 * max(SCIPY_MEASURED_MM.values())


def test_per_joint_is_the_references_mean_l2():
    """reference_fuse.npz keeps what compute_reprojection_error returned for the V candidate poses of every frame (err64[n, i, j]:
    candidate i's mean over the cameras): reproject(xyz = candidate i).per_joint is that row, for every i."""
    G = np.load(FUSE)
    for name in G["names"]:
        P, p3d, p2d, err = (G[f"{name}_{k}"] for k in ("proj", "p3d", "p2d", "err64"))
        for i in range(p3d.shape[1]):
            got = reprojection.reproject(P, p3d[:, i], p2d)
            assert got.per_joint.dtype == np.float64 and np.array_equal(got.n_used, np.full(err[:, i].shape, P.shape[0]))
            assert np.allclose(got.per_joint, err[:, i], **TC.GOLDEN_TOL), (name, i, np.abs(got.per_joint - err[:, i]).max())
            ref = REF.reproject(P, p3d[:, i], p2d)
            assert np.allclose(ref["per_joint"], err[:, i], **TC.GOLDEN_TOL), (name, i)


@pytest.mark.parametrize("V,J", [(1, 1), (4, 17), (5, 19), (31, 19)])
def test_host_path_is_the_restatement_and_the_hard_cases_are_hard(V, J):
    P, X, det, valid, behind = RC.hard_reproject_case(V, J)
    ref = REF.reproject(P, X, det, valid)
    # the claims, on the restatement: the masked pairs are left out, and the mirrored joint lies behind its camera
    assert np.isnan(ref["err"][~valid]).all() and np.isnan(ref["err"][0, 0, 0])
    kept = valid.copy()
    kept[0, 0, 0] = False
    assert np.isfinite(ref["err"][kept]).all() and np.array_equal(ref["n_used"], kept.sum(axis=1))
    assert np.isnan(ref["per_joint"][0, J - 1]) and np.isnan(ref["per_view"][1, V - 1]) and np.isnan(ref["per_frame"][2])
    assert np.isnan(ref["per_joint"][2]).all() and np.isnan(ref["per_view"][2]).all()
    assert ref["u"][behind][2] < 0 and not ref["in_front"][behind] and np.array_equal(ref["in_front"], ref["u"][..., 2] > 0)
    if V > 1:
        assert np.isfinite(ref["per_frame"][:2]).all() and np.isfinite(ref["per_joint"][1]).all()
    got = reprojection.reproject(P, X, det, valid)
    allow_uv, allow_err = RC.pixel_allowances(ref)
    assert np.all(np.abs(got.uv - ref["uv"]) <= allow_uv)
    assert np.array_equal(np.isnan(got.err), np.isnan(ref["err"]))
    assert np.all(np.abs(np.nan_to_num(got.err) - np.nan_to_num(ref["err"])) <= allow_err)
    assert np.array_equal(got.in_front, ref["in_front"]) and np.array_equal(got.n_used, ref["n_used"])
    for name, axis in (("per_joint", 1), ("per_view", 2)):
        tol = RC.mean_allowance(ref["err"], allow_err, axis)
        assert np.array_equal(np.isnan(getattr(got, name)), np.isnan(ref[name])), name
        assert np.all(np.abs(np.nan_to_num(getattr(got, name)) - np.nan_to_num(ref[name])) <= tol), name
    tol = RC.mean_allowance(ref["err"].reshape(RC.N, -1), allow_err.reshape(RC.N, -1), 1)
    assert np.all(np.abs(np.nan_to_num(got.per_frame) - np.nan_to_num(ref["per_frame"])) <= tol)
    # one frame has no frame axis; tensors in, tensors out; project only; a selection
    one = reprojection.reproject(P, X[1], det[1], valid[1])
    assert one.err.shape == (V, J) and np.array_equal(one.err, got.err[1], equal_nan=True)
    t = reprojection.reproject(torch.as_tensor(P), torch.as_tensor(X), torch.as_tensor(det), torch.as_tensor(valid))
    assert torch.is_tensor(t.err) and np.array_equal(t.err.numpy(), got.err, equal_nan=True) and t.in_front.dtype == torch.bool
    only = reprojection.reproject(P, X, want=("uv", "err", "per_frame", "n_used"))
    assert np.array_equal(only.uv, got.uv) and np.isnan(only.err).all() and np.isnan(only.per_frame).all()
    assert not only.n_used.any() and only.in_front is None and only.per_joint is None
    # one rig per frame
    rigs = RC.rigs_per_frame(P)
    per = reprojection.reproject(rigs, X, det, valid)
    for n in range(RC.N):
        alone = reprojection.reproject(rigs[n], X[n], det[n], valid[n])
        assert np.array_equal(per.err[n], alone.err, equal_nan=True) and np.array_equal(per.uv[n], alone.uv)


def test_float_inputs_are_widened_exactly():
    P, X, det = RC.scene(4, 17)
    X32, d32 = X.astype(np.float32), det.astype(np.float32)
    a = reprojection.reproject(P, X32, d32)
    b = reprojection.reproject(P, X32.astype(np.float64), d32.astype(np.float64))
    assert np.array_equal(a.err, b.err) and np.array_equal(a.uv, b.uv) and np.array_equal(a.per_frame, b.per_frame)


def test_sequence_means_on_the_host():
    rng = np.random.default_rng(3)
    err = rng.uniform(0.5, 9.0, (40, 4, 17))
    err[rng.uniform(size=err.shape) < 0.2] = np.nan
    err[:, 2, :] = np.nan                       # a view nobody kept
    groups = rng.integers(0, 3, 40)
    groups[groups == 1] = 7                     # group 1 is empty, 7 lies outside the range
    got = reprojection.evaluate_sequence_reprojection(err, groups, n_groups=3)
    ref, cnt = REF.eval_reprojection(err, groups, 3)
    assert got.shape == (4, 1 + 4 + 17) and np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isnan(ref), cnt == 0)
    assert np.isnan(got[2]).all() and np.isnan(got[:, 3]).all() and cnt[0, 0] == (~np.isnan(err)).sum()
    assert cnt[1, 0] == (~np.isnan(err[groups == 0])).sum() and cnt[3, 0] == (~np.isnan(err[groups == 2])).sum()
    assert np.allclose(got, ref, rtol=64 * RC.EPS, atol=0, equal_nan=True)
    assert np.array_equal(reprojection.evaluate_sequence_reprojection(err)[0], got[0], equal_nan=True)


@pytest.mark.parametrize("ds,V", [("h36m", 2), ("h36m", 3), ("h36m", 4), ("panoptic", 8), ("panoptic", 31)])
def test_refinement_against_scipy(ds, V):
    """The restatement's minimum is scipy's: least_squares(method="lm") on the same residuals, tolerances at the float64 floor,
    restarted from its own result."""
    sc, P, gt, det = TC.sequence(ds, n_views=V, frames=3, seed=0, dtype=np.float64)
    from skelsplat_amd import triangulation
    start = triangulation.triangulate_sequence(P, det, homogeneous=True)[..., :3]
    X, cost, iters, near = REF.refine(P, det, None, start)
    worst = 0.0
    for n in range(3):
        lm = REF.scipy_lm(P, det[n], None, start[n])
        worst = max(worst, float(np.linalg.norm(lm - X[n], axis=-1).max()))
    print(f"V = {V}: largest distance to scipy {worst:.3g} mm (bar {SCIPY_BAR_MM:.3g}), iterations {np.bincount(iters.ravel())}")
    assert worst <= SCIPY_BAR_MM
    host = reprojection.refine_triangulation(P, det, start)
    assert np.allclose(host, X, **TC.GOLDEN_TOL)


@pytest.mark.parametrize("V", RC.REFINE_VIEWS)
@pytest.mark.parametrize("kind", ["plain", "huber", "masks"])
def test_refinement_exact_properties_and_claims(V, kind):
    P, det, valid, start, huber = RC.refine_case(V, kind)
    X, cost, iters, near = REF.refine(P, det, valid, start, huber)
    host, hcost, hiters = reprojection.refine_triangulation(P, det, start, valid=valid, huber_px=huber or None, return_cost=True,
                                                            return_iters=True)
    for x, c, it in ((X, cost, iters), (host, hcost, hiters)):
        moved = it > 0
        known = ~np.isnan(c[..., 0])                   # (a NaN start has a NaN cost)
        assert np.all(c[known][:, 1] <= c[known][:, 0]) and np.array_equal(c[~moved][:, 1], c[~moved][:, 0], equal_nan=True)
        assert it.max() <= 16 and it.min() >= 0
        assert np.array_equal(x[~moved], start[~moved], equal_nan=True)              # pass-through joints: bit-unchanged
    assert np.allclose(host, X, equal_nan=True, **TC.GOLDEN_TOL) and np.array_equal(hiters, iters)
    # the seeds keep the restatement away from ties of its accept / stop comparisons (what the GPU test's iters equality needs)
    assert near.sum() <= RC.NEAR_TIE_SHARE * near.size, (int(near.sum()), near.size)
    # max_iters = 1 is one trip of the restatement
    one, c1, i1 = reprojection.refine_triangulation(P, det, start, valid=valid, huber_px=huber or None, max_iters=1, return_cost=True,
                                                    return_iters=True)
    r1 = REF.refine(P, det, valid, start, huber, max_iters=1)
    assert np.array_equal(i1, r1[2]) and i1.max() == 1 and np.allclose(one, r1[0], equal_nan=True, **TC.GOLDEN_TOL)
    if kind == "masks":
        n_kept = valid.sum(axis=1)
        assert n_kept[1, 3] == 1 and n_kept[2, 5] == 0 and np.array_equal(iters == 0, n_kept < 2)
        assert np.isnan(X[1, 3]).all() and np.isnan(X[2, 5]).all()
        # the masked views are really left out: moving their detections changes nothing
        det2 = det.copy()
        det2[~valid] = 1e6
        again = REF.refine(P, det2, valid, start, huber)
        assert np.array_equal(again[0], X, equal_nan=True) and np.array_equal(again[2], iters)
    if kind == "huber":
        e = REF.reproject(P, X, det)["err"]
        assert (e > huber).any() and (e <= huber).any()
        if V >= 3:      # the shifted view is beyond the threshold and another view of the same joint is within it
            assert (e[:, RC.SHIFT_VIEW] > huber).mean() > 0.9
            assert ((e > huber).any(axis=1) & (e <= huber).any(axis=1)).any()
        plain = REF.refine(P, det, valid, start, 0.0)[0]
        assert not np.array_equal(plain, X)


def test_the_stopping_rule_fires_and_the_cap_binds():
    """Two views, plain squares: most joints stop by the rule after 2-3 trips; with max_iters = 2 the cap ends the others first."""
    P, det, valid, start, huber = RC.refine_case(2, "plain", seed=1)
    full = REF.refine(P, det, valid, start, huber)
    capped = REF.refine(P, det, valid, start, huber, max_iters=2)
    by_rule = (full[2] > 0) & (full[2] <= 2)
    assert by_rule.any() and (full[2] > 2).any() and full[2].max() < 16
    assert np.array_equal(capped[2][by_rule], full[2][by_rule]) and np.array_equal(capped[0][by_rule], full[0][by_rule])
    bound = full[2] > 2
    assert np.all(capped[2][bound] == 2) and np.all(capped[1][bound][:, 1] >= full[1][bound][:, 1])
    host = reprojection.refine_triangulation(P, det, start, max_iters=2, return_iters=True)
    assert np.array_equal(host[1], capped[2])


def test_a_start_behind_a_camera_or_not_finite_comes_back_unchanged():
    P, det, valid, start, huber = RC.refine_case(4, "plain")
    r3 = P[0, 2, :3]
    start[0, 2] = start[0, 2] - 2.0 * (r3 @ start[0, 2] + P[0, 2, 3]) * r3          # mirrored behind camera 0
    start[1, 4, 1] = np.inf
    start[2, 6] = np.nan
    assert REF.reproject(P, start)["u"][0, 0, 2, 2] < 0
    for X, cost, iters in (REF.refine(P, det, None, start)[:3],
                           reprojection.refine_triangulation(P, det, start, return_cost=True, return_iters=True)):
        still = iters == 0
        assert still.sum() == 3 and still[0, 2] and still[1, 4] and still[2, 6]
        assert np.array_equal(X[still], start[still], equal_nan=True) and not np.array_equal(X[~still], start[~still])
    # float32 in, float32 out, in place
    s32 = torch.as_tensor(start.astype(np.float32))
    keep = s32.clone()
    out = reprojection.refine_triangulation(torch.as_tensor(P), torch.as_tensor(det), s32, out=s32)
    assert out is s32 and s32.dtype == torch.float32 and torch.equal(s32[0, 2], keep[0, 2]) and not torch.equal(s32, keep)


def test_python_refusals():
    P, X, det = RC.scene(4, 17)
    with pytest.raises(ValueError, match="huber_px"):
        reprojection.refine_triangulation(P, det, X, huber_px=-1.0)
    with pytest.raises(ValueError, match="huber_px"):
        reprojection.refine_triangulation(P, det, X, huber_px=float("nan"))
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError, match="max_iters"):
            reprojection.refine_triangulation(P, det, X, max_iters=bad)
    with pytest.raises(ValueError, match="65 views"):
        reprojection.reproject(np.zeros((65, 3, 4)), np.zeros((1, 17, 3)))
    with pytest.raises(ValueError, match="xyz0 must be"):
        reprojection.refine_triangulation(P, det, X[:2])
    with pytest.raises(ValueError, match="valid must be"):
        reprojection.reproject(P, X, det, valid=np.ones((3, 4, 16), bool))
    with pytest.raises(ValueError, match="want"):
        reprojection.reproject(P, X, det, want=("uv", "depth"))
    with pytest.raises(ValueError, match="n_groups"):
        reprojection.evaluate_sequence_reprojection(np.zeros((2, 4, 17)), np.zeros(2, int), n_groups=65)
    from skelsplat_amd._sequence import _checked_refine, _refinement
    assert _refinement(None, None) is None and _refinement(8, 10) == (10.0, 8) and _refinement(16, None) == (0.0, 16)
    with pytest.raises(ValueError, match="set_refinement"):
        _checked_refine((0.0, 16), np.zeros((1, 17, 3)), None, "new_scenes")
    with pytest.raises(ValueError, match="set_refinement"):
        _checked_refine((0.0, 16), None, np.zeros((1, 4, 17, 3)), "new_scenes")


X_ = 0x10000         # a device pointer no refused call touches
REPROJECT = "N V J proj rig_stride xyz xyz_f64 poses_2d poses_2d_f64 valid uv err in_front per_joint per_view per_frame n_used stream".split()
EVAL = "N V J err group_ids n_groups out stream".split()
REFINE = ("N V J proj rig_stride poses_2d poses_2d_f64 valid xyz0 xyz0_f64 huber_px max_iters xyz xyz_f64 cost iters stream").split()
BASE = dict(N=3, V=4, J=17, proj=X_, rig_stride=0, xyz=X_, xyz_f64=None, poses_2d=X_, poses_2d_f64=None, valid=None, uv=None, err=X_,
            in_front=None, per_joint=None, per_view=None, per_frame=None, n_used=None, stream=None, group_ids=None, n_groups=0,
            out=X_, xyz0=X_, xyz0_f64=None, huber_px=0.0, max_iters=16, cost=None, iters=None)
EXACTLY_XYZ = "reproject: give the joints as float (xyz) or as double (xyz_f64), exactly one of the two"
EXACTLY_DET = "triangulate_refine: give the detections as float (poses_2d) or as double (poses_2d_f64), exactly one of the two"
EXACTLY_START = "triangulate_refine: give the start as float (xyz0) or as double (xyz0_f64), exactly one of the two"
REFUSALS = [
    ("sks_reproject", REPROJECT, dict(V=0), -1, "reproject: 0 views, a joint takes 1 .. 64 (SKS_MAX_VIEWS)"),
    ("sks_reproject", REPROJECT, dict(V=65), -1, "reproject: 65 views, a joint takes 1 .. 64 (SKS_MAX_VIEWS)"),
    ("sks_reproject", REPROJECT, dict(N=0), -1, "reproject: N and J must be at least 1"),
    ("sks_reproject", REPROJECT, dict(rig_stride=12), -1, "reproject: rig_stride must be 0 (one rig) or V * 12 (one per frame)"),
    ("sks_reproject", REPROJECT, dict(proj=None), -2, "reproject: missing projection matrices"),
    ("sks_reproject", REPROJECT, dict(xyz_f64=X_), -2, EXACTLY_XYZ),
    ("sks_reproject", REPROJECT, dict(xyz=None), -2, EXACTLY_XYZ),
    ("sks_reproject", REPROJECT, dict(poses_2d_f64=X_), -2,
     "reproject: give the detections as float (poses_2d) or as double (poses_2d_f64), not both (neither: project only)"),
    ("sks_reproject", REPROJECT, dict(err=None), -2, "reproject: no output asked for"),
    ("sks_reproject", REPROJECT, dict(V=65, xyz=None), -1, "reproject: 65 views, a joint takes 1 .. 64 (SKS_MAX_VIEWS)"),
    ("sks_eval_reprojection", EVAL, dict(V=65), -1, "eval_reprojection: 65 views, 1 .. 64 (SKS_MAX_VIEWS)"),
    ("sks_eval_reprojection", EVAL, dict(n_groups=65, group_ids=X_), -1, "eval_reprojection: n_groups = 65, 0 .. 64 (SKS_EVAL_MAX_GROUPS)"),
    ("sks_eval_reprojection", EVAL, dict(n_groups=2), -2, "eval_reprojection: n_groups = 2 without group_ids"),
    ("sks_eval_reprojection", EVAL, dict(err=None), -2, "eval_reprojection: missing err (N,V,J) doubles"),
    ("sks_eval_reprojection", EVAL, dict(out=None), -2, "eval_reprojection: missing out (1 + n_groups, 1 + V + J) doubles"),
    ("sks_triangulate_refine", REFINE, dict(V=0), -1, "triangulate_refine: 0 views, a joint takes 1 .. 64 (SKS_MAX_VIEWS)"),
    ("sks_triangulate_refine", REFINE, dict(V=65), -1, "triangulate_refine: 65 views, a joint takes 1 .. 64 (SKS_MAX_VIEWS)"),
    ("sks_triangulate_refine", REFINE, dict(poses_2d=None), -2, EXACTLY_DET),
    ("sks_triangulate_refine", REFINE, dict(poses_2d_f64=X_), -2, EXACTLY_DET),
    ("sks_triangulate_refine", REFINE, dict(xyz0=None), -2, EXACTLY_START),
    ("sks_triangulate_refine", REFINE, dict(xyz0_f64=X_), -2, EXACTLY_START),
    ("sks_triangulate_refine", REFINE, dict(xyz=None), -2, "triangulate_refine: at least one of xyz / xyz_f64"),
    ("sks_triangulate_refine", REFINE, dict(huber_px=-1.0), -1,
     "triangulate_refine: huber_px must be finite and >= 0 pixels (0: plain squares), got -1"),
    ("sks_triangulate_refine", REFINE, dict(huber_px=float("inf")), -1,
     "triangulate_refine: huber_px must be finite and >= 0 pixels (0: plain squares), got inf"),
    ("sks_triangulate_refine", REFINE, dict(huber_px=float("nan")), -1,
     "triangulate_refine: huber_px must be finite and >= 0 pixels (0: plain squares), got nan"),
    ("sks_triangulate_refine", REFINE, dict(max_iters=0), -1, "triangulate_refine: max_iters = 0, 1 .. 16 (SKS_REFINE_MAX_ITERS)"),
    ("sks_triangulate_refine", REFINE, dict(max_iters=17), -1, "triangulate_refine: max_iters = 17, 1 .. 16 (SKS_REFINE_MAX_ITERS)"),
    ("sks_triangulate_refine", REFINE, dict(huber_px=-1.0, max_iters=0), -1,
     "triangulate_refine: huber_px must be finite and >= 0 pixels (0: plain squares), got -1"),
]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a refusal that went missing would launch on made-up pointers")
def test_library_refusals_before_a_launch():
    lib = _lib.load()
    for symbol, names, change, rc_want, text in REFUSALS:
        assert len(names) == len(_lib.SIGNATURES[symbol][1]) and set(change) <= set(names), symbol
        args = [change[n] if n in change else BASE[n] for n in names]
        lib.sks_set_error_(b"")
        rc = getattr(lib, symbol)(*args)
        assert rc == rc_want, (symbol, change, rc, lib.sks_last_error().decode())
        assert lib.sks_last_error().decode() == text, (symbol, change)


def test_the_header_the_binding_and_the_sources_agree():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "skelsplat_hip.h")).read(), flags=re.S)
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
    for symbol, names in (("sks_reproject", REPROJECT), ("sks_eval_reprojection", EVAL), ("sks_triangulate_refine", REFINE)):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % symbol, hdr).group(1)
        declared = []
        for param in proto.split(","):
            ctype, name = re.fullmatch(r"\s*(.*?)(\w+)\s*", param, flags=re.S).groups()
            declared.append((name, ctypes.c_void_p if "*" in ctype else scalars[ctype.strip()]))
        assert [n for n, _ in declared] == names, symbol
        assert _lib.SIGNATURES[symbol] == (ctypes.c_int, [ct for _, ct in declared]), symbol
    assert re.search(r"#define\s+SKS_REFINE_MAX_ITERS\s+16\b", hdr) and _lib.SKS_REFINE_MAX_ITERS == reprojection.REFINE_MAX_ITERS == 16
    from skelsplat_amd import build
    assert build.SOURCES["sks_reproject.hip"] == [] and _lib.load().sks_version() == 14
    # the constants of k_refine, restated in the host path and in the tests' restatement
    src = open(os.path.join(ROOT, "skelsplat_amd", "csrc", "sks_reproject.hip")).read()
    for name, value in (("LAMBDA0", 1e-3), ("LAMBDA_DOWN", 0.1), ("LAMBDA_UP", 10.0), ("STOP_FRACTION", 1e-6)):
        assert float(re.search(r"REFINE_%s = ([0-9.e+-]+);" % name, src).group(1)) == value == getattr(reprojection, name) == getattr(REF, name)
