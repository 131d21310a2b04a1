"""Procrustes-aligned pose errors on the device (csrc/sks_align.hip, skelsplat_amd/report.py): every comparison is against the
float64 textbook solutions of tests/procrustes_ref.py run on the same float32 inputs, over the case table of
tests/procrustes_cases.py.  The allowance of an error, a mean or an aligned coordinate is 2^-23 |ref| + 1e-10 x extent
(procrustes_ref.allowance): one rounding of the float64 result to float32 with a spare unit, plus the float64 fit.

What the inputs do not determine is not compared.  Where the fit is ill conditioned (procrustes_ref.conditioning < 1e-3: planar
only in one pose is fine, collinear or two-joint fits are not) the rotation about the dominant direction is decided by rounding;
the errors of the joints the fit used and their mean do not depend on it, the transform, the aligned coordinates and the errors
of masked joints do.  Those are compared on the well-conditioned cases only."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import procrustes_cases as pc
from tests import procrustes_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WELL = 1e-3
K = {kind: i for i, kind in enumerate(pc.KINDS)}
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _up(a):
    return torch.as_tensor(a, device=_dev())


def _bits_equal(a, b):
    """bit for bit, NaN payloads included"""
    a, b = a.contiguous(), b.contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    raw = {4: torch.int32, 8: torch.int64, 1: torch.uint8}[a.element_size()]
    return torch.equal(a.view(raw), b.view(raw))


def _reference(P, mode):
    """umeyama on the case batch of P joints, once: aligned, per_joint, mean, (s, R, t), extent (K,), conditioning (K,)."""
    key = ("ref", P, mode)
    if key not in _CACHE:
        pred, gt, valid = pc.batch(P)
        aligned, per_joint, mean, tr = pr.batch_errors(pred, gt, valid, mode)
        ext = np.array([pr.extent(gt[f], valid[f]) for f in range(len(pred))])
        cond = np.array([pr.conditioning(pred[f], gt[f], valid[f], mode) for f in range(len(pred))])
        for a in (aligned, per_joint, mean, ext, cond) + tr:
            a.setflags(write=False)
        _CACHE[key] = (aligned, per_joint, mean, tr, ext, cond)
    return _CACHE[key]


def _device(P, mode):
    """The same batch through report.align_poses / aligned_pose_errors, once, as numpy arrays."""
    key = ("dev", P, mode)
    if key not in _CACHE:
        from skelsplat_amd import report
        pred, gt, valid = (_up(a) for a in pc.batch(P))
        aligned, (s, R, t) = report.align_poses(pred, gt, mode=mode, valid=valid, return_transform=True)
        per_joint, mean = report.aligned_pose_errors(pred, gt, mode=mode, valid=valid, per_joint=True)
        assert aligned.dtype == per_joint.dtype == mean.dtype == torch.float32 and s.dtype == R.dtype == t.dtype == torch.float64
        n = len(pc.KINDS)
        assert aligned.shape == (n, P, 3) and per_joint.shape == (n, P) and mean.shape == (n,)
        assert s.shape == (n,) and R.shape == (n, 3, 3) and t.shape == (n, 3)
        _CACHE[key] = tuple(x.cpu().numpy() for x in (aligned, per_joint, mean, s, R, t))
    return _CACHE[key]


CASES = [(P, mode) for P in pc.JOINTS for mode in pr.MODES]


@pytest.mark.parametrize("P,mode", CASES)
def test_errors_and_means(P, mode):
    """|device - ref| <= 2^-23 |ref| + 1e-10 x extent for every per-joint error the inputs determine and for every mean."""
    valid = pc.batch(P)[2]
    _, ref_pj, ref_mean, _, ext, cond = _reference(P, mode)
    _, pj, mean, _, _, _ = _device(P, mode)
    assert np.array_equal(np.isnan(pj), np.isnan(ref_pj)) and np.array_equal(np.isnan(mean), np.isnan(ref_mean))
    worst = 0.0
    for f, kind in enumerate(pc.KINDS):
        sel = (valid[f] | (cond[f] >= WELL)) & ~np.isnan(ref_pj[f])
        allow = pr.allowance(ref_pj[f], ext[f])
        diff = np.abs(pj[f].astype(np.float64) - ref_pj[f])
        ratios = [diff[j] / allow[j] if allow[j] > 0 else (0.0 if diff[j] == 0 else np.inf) for j in np.flatnonzero(sel)]
        if not np.isnan(ref_mean[f]):
            am, dm = pr.allowance(ref_mean[f], ext[f]), abs(float(mean[f]) - ref_mean[f])
            ratios.append(dm / am if am > 0 else (0.0 if dm == 0 else np.inf))
        r = max(ratios, default=0.0)
        worst = max(worst, r)
        assert r <= 1.0, (P, mode, kind, r)
    print(f"aligned errors P={P} {mode}: largest observed / allowed = {worst:.3g}")


@pytest.mark.parametrize("P,mode", CASES)
def test_transform(P, mode):
    """A proper rotation on every case; s, R, t against the reference within 1e-9 relative where the data determine them.
    t = mu_y - s R mu_x inherits the rotation's error times |mu_x|, so its 1e-9 is relative to |mu_y| + s |mu_x| + extent."""
    pred, gt, valid = pc.batch(P)
    _, _, _, (rs, rR, rt), ext, cond = _reference(P, mode)
    _, _, _, s, R, t = _device(P, mode)
    worst = 0.0
    for f, kind in enumerate(pc.KINDS):
        v = valid[f]
        if np.isnan(rs[f]):
            assert np.isnan(s[f]) and np.isnan(R[f]).all() and np.isnan(t[f]).all(), (P, mode, kind)
            continue
        assert np.isfinite(s[f]) and np.isfinite(R[f]).all() and np.isfinite(t[f]).all(), (P, mode, kind)
        assert abs(np.linalg.det(R[f]) - 1.0) <= 1e-12 and np.abs(R[f].T @ R[f] - np.eye(3)).max() <= 1e-12, (P, mode, kind)
        if not v.any():
            assert s[f] == 1.0 and (R[f] == np.eye(3)).all() and (t[f] == 0.0).all(), (P, mode, kind)
            continue
        if mode == "scale":
            assert (R[f] == np.eye(3)).all()
        if mode == "rigid":
            assert s[f] == 1.0
        x = pred[f][v].astype(np.float64)
        y = gt[f][v].astype(np.float64)
        if mode != "scale" and not ((x - x.mean(axis=0)).T @ (y - y.mean(axis=0))).any():
            assert (R[f] == np.eye(3)).all(), (P, mode, kind)             # H = 0 (one joint, coincident joints): R = I
        if cond[f] < WELL:
            continue
        ox, oy = (pred[f][0], gt[f][0]) if mode == "scale" else (x.mean(axis=0), y.mean(axis=0))
        t_scale = np.abs(oy).max() + abs(rs[f]) * np.linalg.norm(ox.astype(np.float64)) + ext[f]
        r = max(abs(s[f] - rs[f]) / abs(rs[f]), np.abs(R[f] - rR[f]).max(), np.abs(t[f] - rt[f]).max() / t_scale) / 1e-9
        worst = max(worst, r)
        assert r <= 1.0, (P, mode, kind, r)
    print(f"transform P={P} {mode}: largest observed / allowed = {worst:.3g}")


@pytest.mark.parametrize("P,mode", CASES)
def test_aligned_and_per_joint(P, mode):
    """The two outputs describe the same fit: ||gt - aligned|| recomputed in float64 from the device's float32 `aligned` equals
    its `per_joint` within the rounding of the three coordinates (half an ulp each) and of the error itself; and on the
    well-conditioned cases `aligned` is the reference's within 2^-23 |coordinate| + 1e-10 x extent."""
    pred, gt, valid = pc.batch(P)
    ref_al, _, _, _, ext, cond = _reference(P, mode)
    al, pj, _, _, _, _ = _device(P, mode)
    assert np.array_equal(np.isnan(al).any(axis=-1), np.isnan(pj))
    again = np.linalg.norm(gt.astype(np.float64) - al.astype(np.float64), axis=-1)
    ok = ~np.isnan(pj)
    bound = pr.U32 * np.abs(al.astype(np.float64)).sum(axis=-1) + 2 * pr.U32 * again
    assert (np.abs(again - pj)[ok] <= bound[ok]).all(), (P, mode, float((np.abs(again - pj)[ok] / np.maximum(bound[ok], 1e-300)).max()))
    worst = 0.0
    for f, kind in enumerate(pc.KINDS):
        if not valid[f].any():
            assert al[f].tobytes() == pred[f].tobytes(), (P, mode, kind)        # no valid joint: aligned IS pred
        if cond[f] < WELL or np.isnan(ref_al[f]).all():
            continue
        sel = ~np.isnan(ref_al[f]).any(axis=-1)           # (a NaN joint -- masked, or it would have poisoned the frame -- is NaN in both)
        assert np.array_equal(~np.isnan(al[f]).any(axis=-1), sel)
        allow = pr.allowance(ref_al[f], ext[f])
        r = float((np.abs(al[f] - ref_al[f])[sel] / allow[sel]).max())
        worst = max(worst, r)
        assert r <= 1.0, (P, mode, kind, r)
    print(f"aligned coordinates P={P} {mode}: largest observed / allowed = {worst:.3g}")


@pytest.mark.parametrize("mode", pr.MODES)
def test_mask_empty_frame_and_nan_semantics(mode):
    from skelsplat_amd import report
    P = 19
    pred, gt, valid = pc.batch(P)

    def run(pred, gt, valid):
        p, g = _up(pred), _up(gt)
        v = None if valid is None else _up(valid)
        al, (s, R, t) = report.align_poses(p, g, mode=mode, valid=v, return_transform=True)
        pj, mean = report.aligned_pose_errors(p, g, mode=mode, valid=v, per_joint=True)
        return al, s, R, t, pj, mean
    base = run(pred, gt, valid)
    # masked joints take no part in the fit or the mean, and are written: moving every masked joint changes its own two
    # outputs and not one bit of anything else
    p2, g2 = pred.copy(), gt.copy()
    p2[~valid] += 250.0
    g2[~valid] -= 125.0
    moved = run(p2, g2, valid)
    for a, b in zip(base[1:4] + base[5:], moved[1:4] + moved[5:]):
        assert _bits_equal(a, b)
    vd = _up(valid)
    assert _bits_equal(base[0][vd], moved[0][vd]) and _bits_equal(base[4][vd], moved[4][vd])
    f = K["mask_3"]
    masked = np.flatnonzero(~valid[f])
    assert np.isfinite(moved[4][f].cpu().numpy()[masked]).all() and (moved[4][f].cpu().numpy()[masked] > 100.0).all()
    # `valid` counts as != 0 (a uint8 mask of 0 / 2 / 255), and None is every joint
    odd = run(pred, gt, valid.astype(np.uint8) * np.where(np.arange(P) % 2, 255, 2).astype(np.uint8))
    assert all(_bits_equal(a, b) for a, b in zip(base, odd))
    full = [k for k, kind in enumerate(pc.KINDS) if valid[k].all()]
    none = run(pred[full], gt[full], None)
    ones = run(pred[full], gt[full], np.ones((len(full), P), dtype=bool))
    assert all(_bits_equal(a, b) for a, b in zip(none, ones))
    assert all(_bits_equal(a, b[_up(np.array(full))]) for a, b in zip(none, base))
    # a frame without a valid joint
    al, s, R, t, pj, mean = (x[K["mask_0"]] for x in base)
    assert _bits_equal(al, _up(pred[K["mask_0"]])) and float(s) == 1.0 and torch.equal(R, torch.eye(3, dtype=torch.float64, device=_dev()))
    assert not t.any() and bool(torch.isnan(mean))
    want = np.linalg.norm(gt[K["mask_0"]].astype(np.float64) - pred[K["mask_0"]], axis=-1)
    assert np.abs(pj.cpu().numpy() - want).max() <= 2 * pr.U32 * want.max()
    # NaN: a valid joint poisons its whole frame, a masked one its own outputs, neither another frame (bits above: `moved`
    # and `base` share the NaN frames); the batch completed
    al, s, R, t, pj, mean = (x.cpu().numpy() for x in base)
    f = K["nan_valid"]
    assert np.isnan(al[f]).all() and np.isnan(pj[f]).all() and np.isnan(mean[f]) and np.isnan(s[f]) and np.isnan(R[f]).all() and np.isnan(t[f]).all()
    f = K["nan_masked"]
    assert np.isnan(pj[f][P - 1]) and np.isnan(al[f][P - 1]).any() and np.isfinite(pj[f][:P - 1]).all() and np.isfinite(mean[f])
    assert np.isfinite(al[f][:P - 1]).all() and np.isfinite(s[f]) and np.isfinite(R[f]).all() and np.isfinite(t[f]).all()
    clean = [k for k, kind in enumerate(pc.KINDS) if kind not in ("nan_valid", "nan_masked")]
    alone = run(pred[clean], gt[clean], valid[clean])
    assert all(_bits_equal(a, b[_up(np.array(clean))]) for a, b in zip(alone, base))
    # an inf poisons like a NaN
    p3 = pred.copy()
    p3[K["noise"], 3, 0] = np.inf
    inf = run(p3, gt, valid)
    assert bool(torch.isnan(inf[5][K["noise"]])) and bool(torch.isnan(inf[0][K["noise"]]).all())
    keep = _up(np.array([k for k in range(len(pc.KINDS)) if k != K["noise"]]))
    assert all(_bits_equal(a[keep], b[keep]) for a, b in zip(inf, base))
    # "scale" without its root: NaN; the rotating modes fit the other joints
    f = K["mask_no_root"]
    if mode == "scale":
        assert np.isnan(mean[f]) and np.isnan(pj[f]).all() and np.isnan(al[f]).all() and np.isnan(s[f])
    else:
        assert np.isfinite(mean[f]) and np.isfinite(pj[f]).all()


@pytest.mark.parametrize("mode", pr.MODES)
def test_frames_are_independent_bit_for_bit(mode):
    """Each frame of a shuffled 513-frame batch equals the same frame run alone, with and without the frame axis; the same on a
    second stream and on a second run."""
    from skelsplat_amd import report
    pred, gt, valid, _ = pc.make_sequence(513, 0)
    N = len(pred)
    perm = np.random.default_rng(3).permutation(N)
    p, g, v = _up(pred), _up(gt), _up(valid)

    def run(p, g, v):
        al, (s, R, t) = report.align_poses(p, g, mode=mode, valid=v, return_transform=True)
        pj, mean = report.aligned_pose_errors(p, g, mode=mode, valid=v, per_joint=True)
        return al, s, R, t, pj, mean
    batch = run(p, g, v)
    pd = _up(perm)
    shuffled = run(p[pd].contiguous(), g[pd].contiguous(), v[pd].contiguous())
    assert all(_bits_equal(a[pd], b) for a, b in zip(batch, shuffled))
    alone = [run(p[f:f + 1], g[f:f + 1], v[f:f + 1]) for f in range(N)]
    for k in range(6):
        assert _bits_equal(torch.cat([a[k] for a in alone]), batch[k]), k
    for f in (0, 100, 512):
        single = run(p[f], g[f], v[f])
        assert all(_bits_equal(a, b[f]) for a, b in zip(single, batch))
    assert all(_bits_equal(a, b) for a, b in zip(run(p, g, v), batch))
    side = torch.cuda.Stream(device=_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        other = run(p, g, v)
    side.synchronize()
    assert all(_bits_equal(a, b) for a, b in zip(other, batch))


def _sequence_reference(N):
    key = ("seq", N)
    if key not in _CACHE:
        pred, gt, valid, _ = pc.make_sequence(N, 0)
        out = {}
        for masked in (True, False):
            v = valid if masked else None
            per = [pr.batch_errors(pred, gt, v, mode)[1] for mode in ("similarity", "scale")]
            ext = np.array([pr.extent(gt[f], None if v is None else v[f]) for f in range(N)])
            out[masked] = (per[0], per[1], ext)
        _CACHE[key] = out
    return _CACHE[key]


@pytest.mark.parametrize("G", pc.SEQUENCE_GROUPS)
@pytest.mark.parametrize("N", pc.SEQUENCE_FRAMES)
def test_sequence_evaluation(N, G):
    """evaluate_sequence_aligned is the fixed-order float64 mean of the device's own per-joint values -- within (N P + 2) 2^-53
    relative of numpy's mean of them: N P - 1 additions and a division, each half an ulp of a partial sum of positive terms --
    and the reference's figure within the mean of the per-joint allowances; per group, with and without `valid`; an empty group
    is NaN; ids from the host and from the device give the same bits."""
    from skelsplat_amd import report
    pred, gt, valid, groups = pc.make_sequence(N, G)
    P = pc.SEQUENCE_JOINTS
    p, g = _up(pred), _up(gt)
    worst = 0.0
    for masked in (True, False):
        v = _up(valid) if masked else None
        vm = valid if masked else np.ones((N, P), dtype=bool)
        kw = dict(groups=groups, n_groups=G) if G else {}
        ev = report.evaluate_sequence_aligned(p, g, valid=v, **kw)
        assert ev["pa_mpjpe"].shape == () and ev["pa_mpjpe_groups"].shape == (G,) and ev["n_mpjpe"].dtype == torch.float64
        got = np.concatenate([[[float(ev["pa_mpjpe"]), float(ev["n_mpjpe"])]],
                              np.stack([ev["pa_mpjpe_groups"].cpu().numpy(), ev["n_mpjpe_groups"].cpu().numpy()], axis=1)])
        if G:
            dev_ids = report.evaluate_sequence_aligned(p, g, groups=_up(groups), n_groups=G, valid=v)
            assert all(_bits_equal(ev[k], dev_ids[k]) for k in ev)
            if G > 1:
                assert np.isnan(got[G]).all()           # group G - 1 has no frames
        pa = report.aligned_pose_errors(p, g, mode="similarity", valid=v, per_joint=True)[0].cpu().numpy()
        nn = report.aligned_pose_errors(p, g, mode="scale", valid=v, per_joint=True)[0].cpu().numpy()
        own = pr.eval_sequence_ref(pa, nn, vm, groups, G)
        assert np.array_equal(np.isnan(got), np.isnan(own))
        ok = ~np.isnan(own)
        assert (np.abs(got - own)[ok] <= (N * P + 2) * 2.0 ** -53 * np.abs(own)[ok]).all(), (N, G, masked)
        ref_pa, ref_n, ext = _sequence_reference(N)[masked]
        ref = pr.eval_sequence_ref(ref_pa, ref_n, vm, groups, G)
        allow = pr.eval_sequence_ref(pr.allowance(ref_pa, ext[:, None]), pr.allowance(ref_n, ext[:, None]), vm, groups, G)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        allow = allow + (N * P + 2) * 2.0 ** -53 * np.abs(ref)
        r = float((np.abs(got - ref)[ok] / allow[ok]).max()) if ok.any() else 0.0
        worst = max(worst, r)
        assert r <= 1.0, (N, G, masked, r)
    print(f"sequence N={N} G={G}: largest observed / allowed = {worst:.3g}")


def test_end_to_end_example(capsys):
    """examples/optimize_sequence.py --report on its synthetic 64-frame sequence: the PA-MPJPE / N-MPJPE it prints are the numbers
    evaluate_sequence_aligned returned, and those equal io.pa_mpjpe / io.n_mpjpe on the downloaded joints within the mean of the
    per-joint allowances; per frame, each wider family of transforms fits no worse.
    The fits minimise the SUM OF SQUARED joint errors, so that is what is ordered: similarity <= rigid <= no alignment, up to
    the rounding of the float32 per-joint values.  (The means of the norms follow the same order on any ordinary frame but no
    theorem makes them: a scale of 1.0003 that lowers the squares by a hair can raise the mean by less than a hair.)"""
    from skelsplat_amd import io, report
    spec = importlib.util.spec_from_file_location("optimize_sequence_example", os.path.join(ROOT, "examples", "optimize_sequence.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    res = example.main(["--report"])
    text = capsys.readouterr().out
    joints, gt, acts, eva = res["joints"], res["gt"], res["activities"], res["aligned"]
    assert joints.shape == gt.shape == (64, 17, 3)
    line = [ln for ln in text.splitlines() if ln.startswith("evaluate_sequence_aligned:")]
    assert len(line) == 1, text
    m = re.fullmatch(r"evaluate_sequence_aligned: PA-MPJPE ([\d.]+) mm, N-MPJPE ([\d.]+) mm; per activity PA ((?:[\d.]+ ?){4}) \| N "
                     r"((?:[\d.]+ ?){4})", line[0])
    assert m, line[0]
    assert m.group(1) == f"{float(eva['pa_mpjpe']):.3f}" and m.group(2) == f"{float(eva['n_mpjpe']):.3f}"
    assert m.group(3).split() == [f"{x:.2f}" for x in eva["pa_mpjpe_groups"].tolist()]
    assert m.group(4).split() == [f"{x:.2f}" for x in eva["n_mpjpe_groups"].tolist()]
    assert text.index("evaluate_sequence: abs MPJPE") < text.index("evaluate_sequence_aligned:")
    hp, hg, ha = joints.cpu().numpy(), gt.cpu().numpy(), acts.cpu().numpy()
    ext = np.array([pr.extent(hg[f]) for f in range(64)])
    rows = [np.ones(64, dtype=bool)] + [ha == a for a in range(4)]
    got = np.concatenate([[[float(eva["pa_mpjpe"]), float(eva["n_mpjpe"])]],
                          np.stack([eva["pa_mpjpe_groups"].cpu().numpy(), eva["n_mpjpe_groups"].cpu().numpy()], axis=1)])
    for r, sel in enumerate(rows):
        for c, (fn, mode) in enumerate(((io.pa_mpjpe, "similarity"), (io.n_mpjpe, "scale"))):
            want = fn(hp[sel], hg[sel])
            per = pr.batch_errors(hp[sel], hg[sel], None, mode)[1]
            allow = float(pr.allowance(per, ext[sel][:, None]).mean()) + (64 * 17 + 2) * 2.0 ** -53 * want
            print(f"example row {r} {mode}: device {got[r, c]:.9f} host {want:.9f} observed / allowed {abs(got[r, c] - want) / allow:.3g}")
            assert abs(got[r, c] - want) <= allow, (r, mode, got[r, c], want)
    sq = {}
    for mode in pr.MODES[:2]:
        sq[mode] = report.aligned_pose_errors(joints, gt, mode=mode, per_joint=True)[0].double().pow(2).sum(dim=1).cpu().numpy()
    sq["none"] = report.pose_errors(joints, gt, per_joint=True)[0][..., 0].double().pow(2).sum(dim=1).cpu().numpy()
    slack = 1 + 8 * pr.U32          # each float32 error is within half an ulp, its square within one, on either side; x 2 spare
    assert (sq["similarity"] <= sq["rigid"] * slack).all() and (sq["rigid"] <= sq["none"] * slack).all()
    assert float(eva["pa_mpjpe"]) < float(report.evaluate_sequence(joints, gt)["abs"])
