"""The aligned pose errors (skelsplat_amd/report.py, csrc/sks_align.hip) without a device: the two float64 textbook solutions the
GPU tests compare against (tests/procrustes_ref.py) agree with each other over the shared case table, are optimal, recover exact
similarities, never return a reflection and follow the mask / empty-frame / NaN rules of include/skelsplat_hip.h; the host
counterparts in skelsplat_amd.io equal them; and the Python surface and the C entry points refuse what they must."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, io, report
from tests import procrustes_cases as pc
from tests import procrustes_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROTATING = ("rigid", "similarity")


def _cases():
    for P in pc.JOINTS:
        for kind in pc.KINDS:
            yield (P, kind) + pc.make_case(P, kind)


def _rotation(axis_angle):
    a = np.linalg.norm(axis_angle)
    k = axis_angle / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def test_case_table_is_the_documented_one():
    assert pc.JOINTS == (1, 2, 3, 4, 17, 19, 64, 65, 130)
    for P in pc.JOINTS:
        pred, gt, valid = pc.batch(P)
        assert pred.dtype == gt.dtype == np.float32 and valid.dtype == bool
        assert pred.shape == gt.shape == (len(pc.KINDS), P, 3) and valid.shape == (len(pc.KINDS), P)
        again = pc.batch(P)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((pred, gt, valid), again))
        k = {kind: i for i, kind in enumerate(pc.KINDS)}
        for n in (0, 1, 2, 3):
            assert valid[k[f"mask_{n}"]].sum() == min(n, P) and (n == 0 or valid[k[f"mask_{n}"]][0])
        assert valid[k["mask_all_but_one"]].sum() == P - 1 and not valid[k["mask_no_root"]][0]
        assert np.isnan(pred[k["nan_valid"]]).sum() == 1 and valid[k["nan_valid"]].all()
        j = np.argwhere(np.isnan(pred[k["nan_masked"]]))
        assert len(j) == 1 and not valid[k["nan_masked"]][j[0][0]]
        assert (gt[k["planar"]][:, 2] == gt[k["planar"]][0, 2]).all() and (pred[k["planar"]][:, 2] == pred[k["planar"]][0, 2]).all()
        if P >= 3:
            c = gt[k["far"]].astype(np.float64)
            assert 4900 < np.linalg.norm(c.mean(axis=0)) < 5100 and pr.extent(c) <= 20
            assert pr.extent(gt[k["tiny"]]) <= 2e-3
            for kind, which in (("collinear_gt", gt), ("collinear_pred", pred)):
                S = np.linalg.svd(which[k[kind]].astype(np.float64) - which[k[kind]].astype(np.float64).mean(axis=0), compute_uv=False)
                assert S[1] < 1e-6 * S[0]
    for N in pc.SEQUENCE_FRAMES:
        for G in pc.SEQUENCE_GROUPS:
            pred, gt, valid, groups = pc.make_sequence(N, G)
            assert pred.shape == (N, 17, 3) and valid.shape == (N, 17) and groups.shape == (N,) and groups.dtype == np.int32
            assert G == 0 or (0 <= groups).all() and (groups < G).all()
            assert G < 2 or not (groups == G - 1).any()          # a group without frames
            assert N == 1 or not valid[N - 1].any()               # a frame without valid joints


def test_the_two_references_agree():
    """On every case and mode, over the outputs the inputs determine: the errors of the valid joints and their mean always; the
    errors of masked joints where the fit is well conditioned (a masked joint of a frame fitted on two joints turns with the
    rotation about their line, which nothing decides).  1e-11 x extent; seen: 1.7e-13."""
    worst = 0.0
    for P, kind, pred, gt, valid in _cases():
        ext = pr.extent(gt, valid)
        for mode in pr.MODES:
            _, eu, mu = pr.errors(pred, gt, valid, mode, pr.umeyama)
            _, eh, mh = pr.errors(pred, gt, valid, mode, pr.horn)
            assert np.array_equal(np.isnan(eu), np.isnan(eh)), (P, kind, mode)
            sel = valid | (pr.conditioning(pred, gt, valid, mode) >= 1e-3)
            sel = sel & ~np.isnan(eu)
            diff = np.abs(eu - eh)[sel].max() if sel.any() else 0.0
            if valid.any() and not np.isnan(mu):
                diff = max(diff, abs(mu - mh))
            # (a frame of extent 0 -- one joint, coincident ground truth -- is held to the size of its own errors)
            scale = ext if ext > 0 else float(np.abs(eu[sel]).max()) if sel.any() else 0.0
            assert diff <= 1e-11 * scale, (P, kind, mode, diff, scale)
            if scale > 0:
                worst = max(worst, diff / scale)
    print(f"largest |umeyama - horn| / extent: {worst:.3g}")
    assert worst < 1e-11


@pytest.mark.parametrize("solver", [pr.umeyama, pr.horn], ids=["umeyama", "horn"])
def test_references_are_optimal(solver):
    """No proper rotation near the returned one and no scale within 1e-3 of the returned one lowers sum ||gt - (s R pred + t)||^2
    (t refitted: the optimal translation for any s, R moves the centroid onto the centroid)."""
    rng = np.random.default_rng(7)
    for P, kind, pred, gt, valid in _cases():
        if kind in pc.POISONED or not valid.any():
            continue
        for mode in ROTATING:
            s, R, t = solver(pred, gt, valid, mode)
            best = pr.objective((s, R, t), pred, gt, valid)
            mx, my = pred[valid].astype(np.float64).mean(axis=0), gt[valid].astype(np.float64).mean(axis=0)
            slack = 1e-9 * max(best, float(np.sum((gt[valid].astype(np.float64) - my) ** 2)), 1e-300)
            for _ in range(6):
                R2 = _rotation(rng.normal(size=3) * 10.0 ** rng.uniform(-4, -1)) @ R
                assert pr.objective((s, R2, my - s * R2 @ mx), pred, gt, valid) >= best - slack, (P, kind, mode)
            if mode == "similarity":
                for ds in (1e-3, -1e-3):
                    s2 = s * (1 + ds)
                    assert pr.objective((s2, R, my - s2 * R @ mx), pred, gt, valid) >= best - slack, (P, kind, mode)


def test_references_recover_exact_similarities():
    rng = np.random.default_rng(11)
    for P in (3, 4, 17, 130):
        for solver in (pr.umeyama, pr.horn):
            x = rng.uniform(-1000, 1000, (P, 3))
            s0, R0, t0 = rng.uniform(0.5, 2.0), _rotation(rng.normal(size=3)), rng.uniform(-3000, 3000, 3)
            y = s0 * x @ R0.T + t0
            s, R, t = solver(x, y, None, "similarity")
            assert abs(s - s0) < 1e-12 * s0 and np.abs(R - R0).max() < 1e-12 and np.abs(t - t0).max() < 1e-8
            s, R, t = solver(x, (y - t0) / s0 + t0, None, "rigid")
            assert s == 1.0 and np.abs(R - R0).max() < 1e-12
            s, R, t = solver(x, 1.7 * (x - x[0]) + x[0] + 5.0, None, "scale")
            assert abs(s - 1.7) < 1e-12 and (R == np.eye(3)).all() and np.abs(t - (x[0] + 5.0 - 1.7 * x[0])).max() < 1e-9
            _, e, m = pr.errors(x, y, None, "similarity", solver)
            assert e.max() < 1e-8 and m < 1e-8


def test_references_return_proper_rotations():
    """det R = +1 and R^T R = I within 1e-12 on every case, the mirrored ones included -- where the best ORTHOGONAL matrix is a
    reflection and the unrepaired SVD solution would have det = -1."""
    mirrored = 0
    for P, kind, pred, gt, valid in _cases():
        if kind in pc.POISONED:
            continue
        for mode in ROTATING:
            for solver in (pr.umeyama, pr.horn):
                s, R, t = solver(pred, gt, valid, mode)
                assert abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12, (P, kind, mode)
                assert np.isfinite(s) and s >= 0 and np.isfinite(t).all()
        if kind == "mirrored" and P >= 4:
            x, y = pred.astype(np.float64), gt.astype(np.float64)
            U, _, Vt = np.linalg.svd((x - x.mean(axis=0)).T @ (y - y.mean(axis=0)))
            mirrored += np.linalg.det(Vt.T @ U.T) < 0
    assert mirrored >= 4        # the table does hold cases whose unconstrained optimum is a reflection


def test_mask_empty_frame_and_nan_semantics():
    for solver in (pr.umeyama, pr.horn):
        pred, gt, valid = pc.make_case(17, "mask_3")
        for mode in pr.MODES:
            # the fit sees the valid joints only: changing a masked joint changes its own outputs and nothing else
            s, R, t = solver(pred, gt, valid, mode)
            p2, g2 = pred.copy(), gt.copy()
            j = int(np.flatnonzero(~valid)[0])
            p2[j] += 500.0
            g2[j] -= 300.0
            s2, R2, t2 = solver(p2, g2, valid, mode)
            assert s2 == s and (R2 == R).all() and (t2 == t).all()
            a, e, m = pr.errors(pred, gt, valid, mode, solver)
            a2, e2, m2 = pr.errors(p2, g2, valid, mode, solver)
            assert m2 == m and (np.delete(e2, j) == np.delete(e, j)).all() and e2[j] != e[j]
            assert np.isclose(m, e[valid].mean(), rtol=1e-15) and a.shape == (17, 3) and np.isfinite(e).all()
            # the same as the fit of the valid joints alone
            s3, R3, t3 = solver(pred[valid], gt[valid], None, mode)
            assert np.isclose(s3, s, rtol=1e-12) and np.abs(R3 - R).max() < 1e-9
        for mode in pr.MODES:       # a frame without a valid joint: identity, aligned = pred, mean NaN
            pred, gt, valid = pc.make_case(19, "mask_0")
            s, R, t = solver(pred, gt, valid, mode)
            assert s == 1.0 and (R == np.eye(3)).all() and (t == 0).all()
            a, e, m = pr.errors(pred, gt, valid, mode, solver)
            assert (a == pred).all() and np.isnan(m) and np.allclose(e, np.linalg.norm(gt.astype(np.float64) - pred, axis=1))
        for mode in pr.MODES:       # NaN in a valid joint: everything NaN; in a masked joint: that joint's outputs only
            pred, gt, valid = pc.make_case(17, "nan_valid")
            a, e, m = pr.errors(pred, gt, valid, mode, solver)
            assert np.isnan(a).all() and np.isnan(e).all() and np.isnan(m)
            pred, gt, valid = pc.make_case(17, "nan_masked")
            a, e, m = pr.errors(pred, gt, valid, mode, solver)
            assert np.isfinite(m) and np.isnan(e[16]) and np.isfinite(e[:16]).all() and np.isfinite(a[:16]).all()
        # "scale" without its root: NaN; the rotating modes do not care
        pred, gt, valid = pc.make_case(17, "mask_no_root")
        s, R, t = solver(pred, gt, valid, "scale")
        assert np.isnan(s) and np.isnan(R).all() and np.isnan(t).all()
        assert np.isnan(pr.errors(pred, gt, valid, "scale", solver)[2])
        assert np.isfinite(pr.errors(pred, gt, valid, "similarity", solver)[2])
        # a frame of coincident joints: s = 1 where the prediction has no extent; with H = 0 every rotation is optimal (the device
        # returns I, the references whatever their decomposition leaves), and the translation puts point on point
        pred, gt, valid = pc.make_case(4, "coincident")
        s, R, t = solver(pred, gt, valid, "similarity")
        assert s == 1.0 and abs(np.linalg.det(R) - 1) < 1e-12
        assert pr.errors(pred, gt, valid, "similarity", solver)[2] < 1e-9
        assert solver(pred, gt, valid, "scale")[0] == 1.0


def test_allowance_is_the_documented_formula():
    assert pr.allowance(100.0, 50.0) == 2.0 ** -23 * 100.0 + 1e-10 * 50.0
    assert pr.allowance(-100.0, 50.0) == pr.allowance(100.0, 50.0)
    gt = np.array([[0.0, 0, 0], [4, 0, 0], [0, 10, 0], [0, 0, 2]])
    assert pr.extent(gt) == 7.5 and pr.extent(gt, [True, True, False, False]) == 2.0 and pr.extent(gt, [False] * 4) == 0.0
    ev = pr.eval_sequence_ref(np.array([[1.0, 2], [3, 4], [5, 6]]), np.array([[1.0, 1], [1, 1], [2, 2]]),
                              np.array([[1, 1], [1, 0], [0, 0]], dtype=bool), np.array([0, 1, 1]), 3)
    assert ev.shape == (4, 2) and (ev[0] == [2.0, 1.0]).all() and (ev[1] == [1.5, 1.0]).all() and (ev[2] == [3.0, 1.0]).all()
    assert np.isnan(ev[3]).all()


def test_host_counterparts_equal_the_references():
    for P, kind, pred, gt, valid in _cases():
        if kind in pc.POISONED:
            continue
        ext = pr.extent(gt, valid)
        for scale, mode in ((True, "similarity"), (False, "rigid")):
            s, R, t = io.similarity_transform(pred, gt, valid, scale=scale)
            rs, rR, rt = pr.umeyama(pred, gt, valid, mode)
            assert abs(np.linalg.det(R) - 1) < 1e-12
            if pr.conditioning(pred, gt, valid, mode) >= 1e-3:
                assert abs(s - rs) <= 1e-12 * rs and np.abs(R - rR).max() < 1e-12 and np.abs(t - rt).max() <= 1e-9 * (1 + np.abs(rt).max())
        for fn, mode in ((io.pa_mpjpe, "similarity"), (io.n_mpjpe, "scale")):
            got = fn(pred, gt, valid)
            want = pr.errors(pred, gt, valid, mode, pr.horn)[2]
            assert np.isnan(got) == np.isnan(want), (P, kind, mode)
            if not np.isnan(want):
                assert abs(got - want) <= 1e-11 * ext + 1e-12 * want, (P, kind, mode, got, want)
    # sequences: the mean over frames and valid joints, as evaluate_sequence_aligned forms it
    pred, gt, valid, _ = pc.make_sequence(257, 15)
    per = [pr.batch_errors(pred, gt, valid, mode)[1] for mode in ("similarity", "scale")]
    ev = pr.eval_sequence_ref(per[0], per[1], valid, None, 0)
    np.testing.assert_allclose(io.pa_mpjpe(pred, gt, valid), ev[0, 0], rtol=1e-12)
    np.testing.assert_allclose(io.n_mpjpe(pred, gt, valid), ev[0, 1], rtol=1e-12)
    np.testing.assert_allclose(io.pa_mpjpe(pred[3], gt[3]), pr.errors(pred[3], gt[3], None, "similarity")[2], rtol=1e-12)
    assert np.isnan(io.pa_mpjpe(pred[:1], gt[:1], np.zeros((1, 17), dtype=bool)))
    # each wider family of transforms fits no worse (in the squared error it minimises): similarity <= rigid <= none
    for f in range(5):
        s, R, t = io.similarity_transform(pred[f], gt[f], scale=False)
        rigid2 = float(np.sum((gt[f] - (pred[f].astype(np.float64) @ R.T + t)) ** 2))
        s, R, t = io.similarity_transform(pred[f], gt[f])
        sim2 = float(np.sum((gt[f] - (s * pred[f].astype(np.float64) @ R.T + t)) ** 2))
        assert sim2 <= rigid2 * (1 + 1e-12) <= float(np.sum((gt[f].astype(np.float64) - pred[f]) ** 2)) * (1 + 1e-12)
    with pytest.raises(ValueError, match=r"\(P,3\)"):
        io.similarity_transform(np.zeros((2, 17, 3)), np.zeros((2, 17, 3)))
    with pytest.raises(ValueError, match="pa_mpjpe"):
        io.pa_mpjpe(np.zeros((17, 3)), np.zeros((16, 3)))


def test_python_refusals():
    a = torch.zeros((2, 17, 3))
    for fn in (report.align_poses, report.aligned_pose_errors, report.evaluate_sequence_aligned):
        with pytest.raises(ValueError, match="ROCm device"):
            fn(a, a)
    for fn in (report.align_poses, report.aligned_pose_errors):
        with pytest.raises(ValueError, match="mode = 'affine'"):
            fn(a, a, mode="affine")
        with pytest.raises(ValueError, match="mode = 1"):
            fn(a, a, mode=1)
    assert report.ALIGN_MODES == {"rigid": 0, "similarity": 1, "scale": 2}


class _OnDevice:
    """A CPU tensor that claims to be on a ROCm device: lets the argument checks behind `is_cuda` run without one."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getitem__(self, i):
        return self._t[i]

    def __getattr__(self, name):
        return getattr(self._t, name)


@pytest.fixture
def on_device(monkeypatch):
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    return _OnDevice


def test_python_refusals_behind_the_device_check(on_device):
    p = on_device(torch.zeros((2, 17, 3)))
    for fn, what in ((report.align_poses, "align_poses"), (report.aligned_pose_errors, "aligned_pose_errors"),
                     (report.evaluate_sequence_aligned, "evaluate_sequence_aligned")):
        with pytest.raises(ValueError, match=what + ": `valid` must be a tensor on the poses' device"):
            fn(p, p, valid=torch.ones((2, 17), dtype=torch.bool))
        with pytest.raises(ValueError, match=what + ": `valid` must be a tensor"):
            fn(p, p, valid=np.ones((2, 17), dtype=bool))
        with pytest.raises(ValueError, match=what + ": `valid` must be bool or uint8"):
            fn(p, p, valid=on_device(torch.ones((2, 17))))
        with pytest.raises(ValueError, match=what + r": `valid` must be \(N,P\) = \(2, 17\), got \(2, 16\)"):
            fn(p, p, valid=on_device(torch.ones((2, 16), dtype=torch.bool)))
        with pytest.raises(ValueError, match=what + ": `pred` must be float32"):
            fn(on_device(torch.zeros((2, 17, 3), dtype=torch.float64)), p)
        with pytest.raises(ValueError, match=what + ": pred and gt must both be"):
            fn(p, on_device(torch.zeros((2, 16, 3))))
    ev = report.evaluate_sequence_aligned
    with pytest.raises(ValueError, match="n_groups without groups"):
        ev(p, p, n_groups=3)
    with pytest.raises(ValueError, match="need n_groups"):
        ev(p, p, groups=on_device(torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="groups must be integers"):
        ev(p, p, groups=np.zeros(2))
    with pytest.raises(ValueError, match=r"groups must be \(N,\) = \(2,\)"):
        ev(p, p, groups=[0, 1, 2])
    with pytest.raises(ValueError, match="n_groups = 65, at most 64"):
        ev(p, p, groups=[0, 64])


def test_abi_tables_and_build():
    hdr = open(os.path.join(ROOT, "include", "skelsplat_hip.h")).read()
    for name, value in (("SKS_ALIGN_RIGID", 0), ("SKS_ALIGN_SIMILARITY", 1), ("SKS_ALIGN_SCALE", 2)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == getattr(_lib, name) == value
    assert "csrc/sks_align.hip; added to sks_version 14: the number did not move" in re.sub(r"\s*\n \*\s*", " ", hdr)
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for symbol, restype in (("sks_align_poses", "int"), ("sks_eval_sequence_aligned", "int"),
                            ("sks_eval_sequence_aligned_scratch_bytes", "size_t")):
        proto = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (restype, symbol), plain).group(1)
        kinds = []
        for param in proto.split(","):
            ctype, _ = re.fullmatch(r"\s*(.*?)(\w+)\s*", param, flags=re.S).groups()
            kinds.append(ctypes.c_void_p if "*" in ctype else scalars[ctype.strip()])
        assert _lib.SIGNATURES[symbol] == (scalars[restype], kinds), symbol
    from skelsplat_amd import build
    assert "sks_align.hip" in build.SOURCES
    lib = _lib.load()
    assert lib.sks_version() == 14
    assert lib.sks_eval_sequence_aligned_scratch_bytes(513, 17) == 2 * 513 * 17 * 4     # host only
    assert lib.sks_eval_sequence_aligned_scratch_bytes(0, 17) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="a refusal that went missing would launch on made-up pointers")
def test_c_refusals():
    """Each refusal happens before any HIP call, with its exact text; every pointer is a placeholder nothing dereferences."""
    lib = _lib.load()
    x = 0x10000

    def refused(fn, args, code, text):
        assert fn(*args) == code, (fn.__name__, args)
        assert lib.sks_last_error().decode() == text

    ok = dict(N=5, P=17, pred=x, gt=x, valid=None, mode=1, aligned=x, transform=x, per_joint=x, mean=x, stream=None)
    call = lambda **change: tuple({**ok, **change}.values())
    al = lib.sks_align_poses
    refused(al, call(N=0), -1, "align_poses: N = 0 frames of P = 17 joints; both must be at least 1")
    refused(al, call(P=0), -1, "align_poses: N = 5 frames of P = 0 joints; both must be at least 1")
    refused(al, call(P=0x7fffffff // 3 + 1), -1, "align_poses: P = 715827883 joints are too many")
    for mode in (-1, 3):
        refused(al, call(mode=mode), -1,
                f"align_poses: mode = {mode}, must be SKS_ALIGN_RIGID (0), SKS_ALIGN_SIMILARITY (1) or SKS_ALIGN_SCALE (2)")
    refused(al, call(pred=None), -2, "align_poses: missing pred")
    refused(al, call(gt=None), -2, "align_poses: missing gt")
    refused(al, call(aligned=None, transform=None, per_joint=None, mean=None), -2,
            "align_poses: no output requested (aligned, transform, per_joint and mean are all NULL)")
    need = 2 * 5 * 17 * 4
    ok = dict(N=5, P=17, pred=x, gt=x, valid=None, group_ids=x, n_groups=3, scratch=x, scratch_bytes=need, out=x, stream=None)
    ev = lib.sks_eval_sequence_aligned
    refused(ev, call(N=0), -1, "eval_sequence_aligned: N = 0 frames of P = 17 joints; both must be at least 1")
    refused(ev, call(P=-1), -1, "eval_sequence_aligned: N = 5 frames of P = -1 joints; both must be at least 1")
    refused(ev, call(P=715827883), -1, "eval_sequence_aligned: P = 715827883 joints are too many")
    for G in (-1, 65):
        refused(ev, call(n_groups=G), -1, f"eval_sequence_aligned: n_groups = {G}, 0 .. 64 (SKS_EVAL_MAX_GROUPS)")
    refused(ev, call(pred=None), -2, "eval_sequence_aligned: missing pred")
    refused(ev, call(gt=None), -2, "eval_sequence_aligned: missing gt")
    refused(ev, call(out=None), -2, "eval_sequence_aligned: missing out (1 + n_groups, 2) doubles")
    refused(ev, call(group_ids=None), -2, "eval_sequence_aligned: n_groups = 3 without group_ids")
    refused(ev, call(scratch=None), -2,
            f"eval_sequence_aligned: scratch of 0 bytes, {need} are needed (sks_eval_sequence_aligned_scratch_bytes)")
    refused(ev, call(scratch_bytes=need - 1), -2,
            f"eval_sequence_aligned: scratch of {need - 1} bytes, {need} are needed (sks_eval_sequence_aligned_scratch_bytes)")
