"""Outlier rejection by two-view consensus on the host (no GPU): triangulation.triangulate_sequence(reject_px=..) against the
plain numpy oracle of tests/robust_tri_cases.py, the oracle's own decisiveness, and the refusals of every layer."""
import inspect

import numpy as np
import pytest
import torch

from skelsplat_amd import triangulation
from tests import robust_tri_cases as RC
from tests import tri_cases as TC


def _robust(P, x, **kw):
    kw.setdefault("reject_px", RC.TAU)
    return triangulation.triangulate_sequence(P, x, homogeneous=True, return_n_used=True, return_inliers=True, **kw)


def _compare(got, ref, what):
    """masks and counts exactly and joints within TC.GOLDEN_TOL, on the joints where the oracle is decisive"""
    xyzw, n_used, inl, n_cons = got
    ok = ref["decisive"]
    print(what, "joints:", ok.size, "not decisive:", int((~ok).sum()), "decided by the sum:", int(ref["tie"].sum()))
    assert inl.dtype == np.bool_ and n_cons.dtype == np.int32 and n_used.dtype == np.int32
    assert np.array_equal(inl.transpose(0, 2, 1)[ok], ref["inliers"].transpose(0, 2, 1)[ok])
    assert np.array_equal(n_cons[ok], ref["n_consensus"][ok]) and np.array_equal(n_used[ok], ref["n_used"][ok])
    assert np.array_equal(np.isnan(xyzw[ok]), np.isnan(ref["xyzw"][ok]))
    err = np.nanmax(np.abs(xyzw[ok] - ref["xyzw"][ok]), initial=0.0)
    print(what, "max abs difference of the joints to the oracle:", err)
    assert np.allclose(xyzw[ok], ref["xyzw"][ok], equal_nan=True, **TC.GOLDEN_TOL), err


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_the_oracle_is_decisive_and_finds_the_corrupted_views(shape):
    P, x, bad = RC.generated(*shape)
    ref = RC.generated_oracle(*shape)
    assert (~ref["decisive"]).mean() <= RC.MAX_UNDECIDED
    assert np.array_equal(ref["inliers"], ~bad)
    if shape[1] == 4:
        assert (ref["tie"] & ref["decisive"]).any()          # what exercises the tie-break: an equal-count rival set
    if shape[1] >= 3:
        assert (ref["n_consensus"] >= 3).all() and np.array_equal(ref["n_consensus"], ref["n_used"])


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
def test_host_path_equals_the_oracle(shape):
    P, x, bad = RC.generated(*shape)
    got = _robust(P, x)
    _compare(got, RC.generated_oracle(*shape), f"{shape[0]} V={shape[1]}")
    assert np.array_equal(got[2], ~bad)
    # against the ground truth: rejection is what makes these joints usable
    sc, _, gt, _ = TC.sequence(shape[0], shape[1], shape[2], 5, dtype=np.float64)
    gt = gt[:, :shape[3]] if shape[3] else gt
    plain = triangulation.triangulate_sequence(P, x, homogeneous=True)
    e_plain, e_robust = (np.linalg.norm(a[..., :3] - gt, axis=-1) for a in (plain, got[0]))
    print("mean error plain / robust (mm):", e_plain.mean(), e_robust.mean())
    assert e_robust.max() < 60.0 if shape[1] > 2 else np.array_equal(plain, got[0])


@pytest.mark.parametrize("m", [3, 2])
def test_hand_cases(m):
    P, x, valid = RC.hand()
    ref = RC.hand_oracle(m)
    for name, (f, j) in RC.HAND.items():
        assert ref["decisive"][f, j], name
    got = _robust(P, x, valid=valid, min_inliers=m)
    _compare(got, ref, f"hand m={m}")
    xyzw, n_used, inl, n_cons = got
    at = lambda k: (RC.HAND[k][0], slice(None), RC.HAND[k][1])
    cell = lambda k: RC.HAND[k]
    assert inl[at("nan")].tolist() == [True, True, False, True] and n_cons[cell("nan")] == 3
    assert np.isfinite(xyzw[cell("nan")]).all()
    assert not inl[at("none")].any() and n_cons[cell("none")] == 0 and np.isnan(xyzw[cell("none")]).all()
    assert inl[at("one")].sum() == 1 and n_cons[cell("one")] == 1 and np.isnan(xyzw[cell("one")]).all()
    assert inl[at("two")].tolist() == [True, True, False, False] and n_cons[cell("two")] == 2 and n_used[cell("two")] == 2
    assert n_cons[cell("split")] == 2 and n_cons[cell("behind")] == 2
    if m == 3:      # no consensus: what the plain path gives
        assert inl[at("split")].all() and inl[at("behind")].all() and n_used[cell("split")] == 4
        plain = triangulation.triangulate_sequence(P, np.nan_to_num(x), valid=valid, homogeneous=True)
        assert np.array_equal(xyzw[cell("split")], plain[cell("split")])
    else:           # the pair that reprojects exactly lies behind its cameras: the other pair wins
        assert inl[at("behind")].tolist() == [False, False, True, True] and n_used[cell("behind")] == 2
    # a NaN detection among the views of a joint WITHOUT consensus: the fallback is the plain result, NaN
    x2 = x.copy()
    x2[RC.HAND["split"][0], 0, RC.HAND["split"][1]] = np.nan
    xyzw2, _, inl2, n_cons2 = _robust(P, x2, valid=valid, min_inliers=3)
    assert inl2[at("split")].all() and n_cons2[cell("split")] < 3 and np.isnan(xyzw2[cell("split")]).all()
    assert np.isnan(xyzw2).sum() == np.isnan(xyzw).sum() + 4


def test_a_large_threshold_keeps_every_view_and_is_the_plain_path():
    P, x, bad = RC.generated("h36m", 4, 8, None)
    rng = np.random.default_rng(3)
    valid = rng.random(x.shape[:3]) > 0.15
    for v in (None, valid):
        plain, n_plain = triangulation.triangulate_sequence(P, x, valid=v, homogeneous=True, return_n_used=True)
        xyzw, n_used, inl, n_cons = _robust(P, x, valid=v, reject_px=1e9)
        assert np.array_equal(inl, np.ones_like(bad) if v is None else v)
        assert np.array_equal(xyzw, plain, equal_nan=True) and np.array_equal(n_used, n_plain)
        assert np.array_equal(n_cons, n_plain)


def test_return_values_shapes_and_tensors():
    P, x, bad = RC.generated("h36m", 4, 8, None)
    ref = _robust(P, x)
    xyz = triangulation.triangulate_sequence(P, x, reject_px=RC.TAU)
    assert xyz.dtype == np.float32 and np.array_equal(xyz, ref[0][..., :3].astype(np.float32))
    got = triangulation.triangulate_sequence(P, x, reject_px=RC.TAU, return_inliers=True)
    assert len(got) == 3 and np.array_equal(got[1], ref[2]) and np.array_equal(got[2], ref[3])
    one = triangulation.triangulate_sequence(P, x[2], reject_px=RC.TAU, return_inliers=True, return_n_used=True)   # one frame
    assert one[0].shape == (17, 3) and one[1].shape == (17,) and one[2].shape == (4, 17) and one[3].shape == (17,)
    assert np.array_equal(one[2], ref[2][2]) and np.array_equal(one[3], ref[3][2]) and np.array_equal(one[1], ref[1][2])
    t = triangulation.triangulate_sequence(torch.as_tensor(P), torch.as_tensor(x.astype(np.float32)), reject_px=RC.TAU,
                                           return_inliers=True)
    assert torch.is_tensor(t[1]) and t[1].dtype == torch.bool and t[2].dtype == torch.int32
    assert np.array_equal(t[1].numpy(), ref[2])
    rigs = np.repeat(P[None], x.shape[0], 0)            # one rig per frame
    per = _robust(rigs, x)
    assert all(np.array_equal(a, b) for a, b in zip(per, ref))
    buf = (torch.zeros(bad.shape, dtype=torch.bool), torch.zeros(bad.shape[::2], dtype=torch.int32))
    triangulation.triangulate_sequence(torch.as_tensor(P), torch.as_tensor(x), reject_px=RC.TAU, out_inliers=buf)
    assert np.array_equal(buf[0].numpy(), ref[2]) and np.array_equal(buf[1].numpy(), ref[3])


def test_refusals():
    P, x, bad = RC.generated("h36m", 4, 8, None)
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="reject_px"):
            triangulation.triangulate_sequence(P, x, reject_px=tau)
    for m in (1, 65):
        with pytest.raises(ValueError, match="min_inliers"):
            triangulation.triangulate_sequence(P, x, reject_px=RC.TAU, min_inliers=m)
    with pytest.raises(ValueError, match="reject_px"):
        triangulation.triangulate_sequence(P, x, return_inliers=True)
    from skelsplat_amd import loop
    pts, p3d = np.zeros((8, 17, 3), np.float32), np.zeros((8, 4, 17, 3), np.float32)
    on = loop._rejection(RC.TAU, 3)
    assert on == (RC.TAU, 3) and loop._rejection(None, 3) is None
    for tau in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="reject_px"):
            loop._rejection(tau, 3)
    for m in (1, 65):
        with pytest.raises(ValueError, match="min_inliers"):
            loop._rejection(RC.TAU, m)
    for who in ("new_scene", "new_scenes", "optimize_sequence"):
        with pytest.raises(ValueError, match="explicit points"):
            loop._checked_reject(on, pts, None, who)
        with pytest.raises(ValueError, match="poses_3d"):
            loop._checked_reject(on, None, p3d, who)
        assert loop._checked_reject(None, pts, p3d, who) == (None, 3)
        assert loop._checked_reject(on, None, None, who) == on
    # the setting lives on the loops (set_outlier_rejection): the calls keep the signatures they had
    for cls in (loop.MultiViewLoop, loop.FrameBatchLoop, loop.FramePipeline):
        sig = inspect.signature(cls.set_outlier_rejection).parameters
        assert sig["reject_px"].default is None and sig["min_inliers"].default == 3, cls
    for fn in (loop.MultiViewLoop.new_scene, loop.FrameBatchLoop.new_scenes, loop.FrameBatchLoop.optimize_sequence,
               loop.FramePipeline.optimize_sequence):
        assert "reject_px" not in inspect.signature(fn).parameters
