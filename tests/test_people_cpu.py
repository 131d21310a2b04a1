"""The people front end without a GPU (include/skelsplat_hip.h "People"): the host path of skelsplat_amd.people against the
op-by-op restatement of tests/people_ref.py, exactly; the restatement's pair costs against an independent reference (pseudo-inverse
fundamental matrices, plain numpy distances) within a measured bound; generated scenes, whose known permutation the rule recovers in
every frame with every decision farther from its threshold than that bound; hand cases that each reach the branch they are there
for, asserted on the restatement's counters; the tracker's cases; to_tracks; the library's host-only query and refusals."""
import ctypes

import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, people
from tests import people_cases as C
from tests import people_ref as R

# The restatement's costs against reference_costs, as |difference| / max(cost, 1 px), over every case of people_cases (the
# crowd included).  MEASURED on the CPU: the largest value seen is 2.2e-10 (D128_32x4, 32 ring cameras; 3.4e-11 over the seven
# table configurations); the bound is 16 x that.
MEASURED_REL = 2.2e-10
REL_BOUND = 16 * MEASURED_REL


def _keep(c, f):
    return np.ones(c["x"].shape[1:4], dtype=bool) if c["valid"] is None else c["valid"][f]


def _rig(c, f):
    return c["P"] if c["P"].ndim == 3 else c["P"][f]


def _associate(c, x=None, valid=None, **kw):
    args = dict(max_px=c["max_px"], min_joints=c["min_joints"], min_views=c["min_views"], max_people=c["K"])
    args.update(kw)
    return people.associate(c["P"], c["x"] if x is None else x, c["valid"] if valid is None else valid, **args)


def _same(got, ref):
    return all(np.asarray(getattr(got, k)).dtype == ref[k].dtype and np.array_equal(np.asarray(getattr(got, k)), ref[k], equal_nan=True)
               for k in got._fields)


@pytest.mark.parametrize("name", C.NAMES)
def test_host_path_equals_the_restatement(name):
    c, ref = C.case(name), C.reference(name)
    got = _associate(c)
    assert isinstance(got.assign, np.ndarray) and got.poses_2d.dtype == c["x"].dtype and _same(got, ref)
    # CPU tensors in, CPU tensors out; one frame without the frame axis
    t = _associate(c, x=torch.as_tensor(c["x"]), valid=None if c["valid"] is None else torch.as_tensor(c["valid"]))
    assert torch.is_tensor(t.assign) and all(np.array_equal(a.numpy(), b, equal_nan=True) for a, b in zip(t, got))
    one = people.associate(_rig(c, 0), c["x"][0], None if c["valid"] is None else c["valid"][0], c["max_px"], c["min_joints"],
                           c["min_views"], c["K"])
    assert one.assign.shape == got.assign.shape[1:] and all(np.array_equal(a, b[0], equal_nan=True) for a, b in zip(one, got))


def test_per_frame_rigs_on_the_host():
    c, ref = C.case("h36m_4x4_drop"), C.reference("h36m_4x4_drop")
    P = np.repeat(c["P"][None], len(c["x"]), axis=0)
    assert _same(people.associate(P, c["x"], c["valid"], c["max_px"]), ref)
    # a rig of its own per frame: frame 1 seen by the cameras in reverse order
    P[1] = P[1, ::-1]
    x = c["x"].copy()
    x[1] = x[1, ::-1]
    valid = c["valid"].copy()
    valid[1] = valid[1, ::-1]
    got = people.associate(P, x, valid, c["max_px"])
    want = R.associate(P, x, valid, c["max_px"])
    assert _same(got, want) and C.recovered(got.assign[1], c["perm"][1, ::-1])


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_costs_agree_with_the_independent_reference(name):
    c, ref = C.case(name), C.reference(name)
    worst, n = 0.0, 0
    for f, frame in enumerate(ref["frames"]):
        ind = R.reference_costs(_rig(c, f), c["x"][f], _keep(c, f), c["min_joints"])
        for pair, want in ind.items():
            if pair in frame["costs"] and np.isfinite(want):        # (a joint with an infinite distance: the rule drops it)
                worst, n = max(worst, abs(frame["costs"][pair] - want) / max(want, 1.0)), n + 1
    print(f"{name}: {n} pair costs, largest |restatement - reference| / max(cost, 1 px) = {worst:.3e} (bound {REL_BOUND:.3e})")
    assert worst <= REL_BOUND
    assert n > 0 or name == "empty_and_single_view" or not any(fr["costs"] for fr in ref["frames"])


def test_the_determinant_form_is_a_fundamental_matrix():
    """x_b^T F x_a = 0 for the images of one point, and F equals the pseudo-inverse form up to scale."""
    c = C.case("panoptic_5x3")
    X = np.concatenate([c["gt"][0, 0], np.ones((c["gt"].shape[2], 1))], axis=1)
    for a, b in ((0, 1), (1, 4), (2, 3)):
        F, G = R.fundamental(c["P"][a], c["P"][b]), R.reference_fundamental(c["P"][a], c["P"][b])
        xa, xb = X @ c["P"][a].T, X @ c["P"][b].T
        r = np.einsum("nj,ji,ni->n", xb, F, xa) / (np.linalg.norm(xb, axis=1) * np.linalg.norm(F) * np.linalg.norm(xa, axis=1))
        assert np.abs(r).max() < 1e-12
        F, G = F / np.linalg.norm(F), G / np.linalg.norm(G)
        assert min(np.abs(F - G).max(), np.abs(F + G).max()) < 1e-9


@pytest.mark.parametrize("name", list(C.TABLE))
def test_generated_scenes_recover_the_permutation_in_every_frame(name):
    """The issue's table.  Every frame's people are the known permutation; and no decision hangs on rounding: every measured cost is
    farther from max_px, and every two edge costs are farther from each other, than REL_BOUND (relative) -- a condition with cap
    zero, met by the seeds of people_cases.SEEDS."""
    c, ref = C.case(name), C.reference(name)
    K = c["perm"].shape[2]
    for f, frame in enumerate(ref["frames"]):
        assert C.recovered(ref["assign"][f], c["perm"][f]), (name, f)
        assert ref["n_people"][f] == K and ref["n_overflow"][f] == 0 and ref["n_unassigned"][f] == 0
        costs = np.array(sorted(frame["costs"].values()))
        assert (np.abs(costs - c["max_px"]) > REL_BOUND * np.maximum(costs, c["max_px"])).all()
        edges = costs[costs <= c["max_px"]]
        assert (np.diff(edges) > REL_BOUND * edges[1:]).all()
        assert np.isfinite(ref["cost"][f, :K]).all() and (ref["cost"][f, :K] < c["max_px"]).all() and np.isnan(ref["cost"][f, K:]).all()
    # the gathered detections are the hand-ordered ones, NaN where the mask drops a joint
    order = np.stack([[np.nonzero((c["perm"][f].T == row).all(axis=1))[0][0] for row in ref["assign"][f, :K]] for f in range(len(c["x"]))])
    for f in range(len(c["x"])):
        for k in range(K):
            for v in range(c["x"].shape[1]):
                want = c["x"][f, v, c["perm"][f, v, order[f, k]]].copy()
                if c["valid"] is not None:
                    want[~c["valid"][f, v, c["perm"][f, v, order[f, k]]]] = np.nan
                assert np.array_equal(ref["poses_2d"][f, k, v], want, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ hand cases
def test_veto_refuses_what_single_link_merges():
    c, ref = C.case("veto"), C.reference("veto")
    costs = ref["frames"][0]["costs"]
    assert costs[(0, 2)] < costs[(0, 1)] <= c["max_px"] < costs[(1, 2)]            # the ambiguous pair is the last edge
    assert ref["counters"]["veto_refused"] == 1 and ref["counters"]["view_refused"] == 0
    assert ref["frames"][0]["clusters"] == [[0, 2]] and ref["n_unassigned"][0] == 1
    assert ref["assign"][0, 0].tolist() == [0, -1, 0] and np.isnan(ref["poses_2d"][0, 0, 1]).all()
    single = C.reference("veto", link="single")
    assert single["frames"][0]["clusters"] == [[0, 1, 2]] and single["counters"]["veto_refused"] == 0


def test_view_rule_leaves_a_near_duplicate_unassigned():
    ref = C.reference("view_rule")
    assert ref["counters"]["view_refused"] >= 1 and ref["counters"]["veto_refused"] == 0
    assert ref["n_people"][0] == 1 and ref["n_unassigned"][0] == 1
    assert ref["assign"][0, 0].tolist() == [0, 0, 0]                # the exact detection is the cheaper edge: it joins


def test_equal_costs_are_ordered_by_index():
    dup = C.reference("duplicate_tie")
    costs = dup["frames"][0]["costs"]
    assert costs[(0, 2)] == costs[(0, 3)] and costs[(2, 4)] == costs[(3, 4)]          # bit for bit: the slots hold the same numbers
    assert dup["counters"]["index_ties"] == 2 and dup["counters"]["view_refused"] >= 1
    assert dup["assign"][0, 0].tolist() == [0, 0, 0] and dup["n_unassigned"][0] == 1      # the lower slot joins
    mirror = C.reference("mirror_tie")
    costs = mirror["frames"][0]["costs"]
    assert costs[(0, 2)] == costs[(1, 3)] and 0.0 < costs[(0, 2)] < 15.0 and mirror["counters"]["index_ties"] >= 1
    assert costs[(0, 3)] == costs[(1, 2)] and costs[(0, 3)] < costs[(0, 2)]         # the mirror pairing is exact: it goes first
    assert sorted(mirror["frames"][0]["clusters"]) == [[0, 3], [1, 2]] and mirror["counters"]["view_refused"] == 2


def test_an_unmeasured_pair_does_not_veto():
    c, ref = C.case("unmeasured"), C.reference("unmeasured")
    assert ref["counters"]["unmeasured"] == 1 and (1, 2) not in ref["frames"][0]["costs"]
    assert ref["frames"][0]["clusters"] == [[0, 1, 2]] and ref["counters"]["veto_refused"] == 0
    # one joint fewer asked for: the same pair is measured, is a veto, and C stays out
    two = R.associate(c["P"], c["x"], c["valid"], c["max_px"], min_joints=2)
    assert two["frames"][0]["costs"][(1, 2)] > c["max_px"] and two["counters"]["veto_refused"] == 1
    assert two["frames"][0]["clusters"] == [[0, 1]] and two["n_unassigned"][0] == 1
    assert _same(people.associate(c["P"], c["x"], c["valid"], c["max_px"], min_joints=2), two)


def test_empty_frames_single_views_overflow_and_non_finite_detections():
    ref = C.reference("empty_and_single_view")
    assert ref["n_people"].tolist() == [0, 0, 2] and ref["n_unassigned"].tolist() == [0, 1, 0]
    assert (ref["assign"][:2] == -1).all() and np.isnan(ref["cost"][:2]).all() and np.isnan(ref["poses_2d"][:2]).all()
    c, ref = C.case("overflow"), C.reference("overflow")
    V = c["x"].shape[1]
    assert ref["n_people"].tolist() == [2, 2] and ref["n_overflow"].tolist() == [2, 2] and ref["n_unassigned"].tolist() == [2 * V] * 2
    full = R.associate(c["P"], c["x"], c["valid"], c["max_px"], K=8)
    assert np.array_equal(full["assign"][:, :2], ref["assign"]) and all(C.recovered(full["assign"][f], c["perm"][f]) for f in range(2))
    c, ref = C.case("nonfinite"), C.reference("nonfinite")
    assert not np.isfinite(c["x"]).all() and np.isinf(c["x"]).any()
    assert all(C.recovered(ref["assign"][f], c["perm"][f]) for f in range(2)) and np.isfinite(ref["cost"][:, :3]).all()
    assert np.isinf(ref["poses_2d"]).any()              # a kept coordinate is copied as it is


def test_refusals():
    c = C.case("h36m_2x2")
    x = c["x"]
    for kw, match in ((dict(max_px=np.nan), "max_px"), (dict(min_joints=0), "min_joints"), (dict(min_views=1), "min_views"),
                      (dict(max_people=9), "max_people")):
        with pytest.raises(ValueError, match=match):
            _associate(c, **kw)
    with pytest.raises(ValueError, match="SKS_PEOPLE_MAX_DETS"):
        people.associate(np.zeros((9, 3, 4)), np.zeros((1, 9, 15, 3, 2)))
    with pytest.raises(ValueError, match="SKS_PEOPLE_MAX_SLOTS"):
        people.associate(np.zeros((2, 3, 4)), np.zeros((1, 2, 17, 3, 2)))
    with pytest.raises(ValueError, match="detections must be"):
        people.associate(c["P"], x[0, 0])
    with pytest.raises(ValueError, match="valid"):
        people.associate(c["P"], x, np.ones(x.shape[:3], dtype=bool))
    with pytest.raises(ValueError, match="joints must be"):
        people.track(np.zeros((2, 3, 5)))
    with pytest.raises(ValueError, match="SKS_PEOPLE_MAX"):
        people.track(np.zeros((2, 9, 5, 3)))
    with pytest.raises(ValueError, match="groups"):
        people.track(np.zeros((2, 2, 5, 3)), groups=[0])
    with pytest.raises(ValueError, match="max_gap"):
        people.track(np.zeros((2, 2, 5, 3)), max_gap=-1)
    # the library refuses the same limits before it touches the device
    lib = _lib.load()
    rc = lib.sks_associate_people(1, 9, 15, 3, 8, None, 0, None, None, None, 15.0, 3, 2, None, None, None, None, None, None, None, None)
    assert rc != 0 and b"SKS_PEOPLE_MAX_DETS" in lib.sks_last_error()
    rc = lib.sks_associate_people(1, 2, 2, 3, 9, None, 0, None, None, None, 15.0, 3, 2, None, None, None, None, None, None, None, None)
    assert rc != 0 and b"SKS_PEOPLE_MAX" in lib.sks_last_error()
    rc = lib.sks_associate_people(1, 2, 2, 3, 8, None, 0, None, None, None, 15.0, 3, 2, None, None, None, None, None, None, None, None)
    assert rc != 0 and b"proj" in lib.sks_last_error()
    rc = lib.sks_track_people(1, 9, 5, None, None, 1, 200.0, 1, 3, None, None, None, None)
    assert rc != 0 and b"SKS_PEOPLE_MAX" in lib.sks_last_error()
    rc = lib.sks_track_people(1, 8, 5, None, None, 2, 200.0, 1, 3, None, None, None, None)
    assert rc != 0 and b"n_groups" in lib.sks_last_error()


@pytest.mark.parametrize("V,M", [(2, 2), (5, 4), (8, 16), (31, 4), (64, 2), (1, 16)])
def test_launch_claims(V, M):
    """sks_people_launch (host only) against the layout DESIGN.md "People" states; the longest lists fit the 160 KiB of a CU."""
    got = _lib.people_launch(V, M)
    D, entries = V * M, 2
    while entries < M * M * (V * (V - 1) // 2):
        entries *= 2
    lds = 8 * (18 * V + 2 * D + 2 * D + D + entries) + 4 * (3 * D + 8 * V + 8 + 4) + 2 * entries
    assert got == dict(assoc_threads=256, assoc_lds_bytes=-(-lds // 16) * 16, assoc_list_entries=entries, track_threads=64)
    assert got["assoc_lds_bytes"] <= 160 * 1024 and entries <= 8192
    with pytest.raises(RuntimeError, match="people_launch"):
        _lib.people_launch(9, 15)


def test_the_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "skelsplat_hip.h")).read()
    want = dict(re.findall(r"#define\s+(SKS_PEOPLE_[A-Z_]+)\s+(\d+)", hdr))
    for name in ("SKS_PEOPLE_MAX_DETS", "SKS_PEOPLE_MAX_SLOTS", "SKS_PEOPLE_MAX", "SKS_PEOPLE_MAX_GROUPS", "SKS_PEOPLE_LAUNCH_INTS"):
        assert int(want[name]) == getattr(_lib, name), name
    assert (people.MAX_DETS, people.MAX_SLOTS, people.MAX_PEOPLE, people.MAX_GROUPS, people.MAX_JOINTS) == \
        (_lib.SKS_PEOPLE_MAX_DETS, _lib.SKS_PEOPLE_MAX_SLOTS, _lib.SKS_PEOPLE_MAX, _lib.SKS_PEOPLE_MAX_GROUPS, _lib.SKS_MAX_CHANNELS)
    assert R.S == _lib.SKS_PEOPLE_MAX
    assert _lib.SIGNATURES["sks_associate_people"][1][10] is ctypes.c_double and len(_lib.PEOPLE_LAUNCH_FIELDS) == _lib.SKS_PEOPLE_LAUNCH_INTS


# ------------------------------------------------------------------------------------------------------------ tracking
def _track(c, **kw):
    return people.track(c["joints"], c["groups"], c["max_mm"], c["max_gap"], c["min_joints"], n_groups=c["G"], **kw)


@pytest.mark.parametrize("name", list(C.TRACK))
def test_tracker_host_path_equals_the_restatement(name):
    c, ref = C.track_case(name), C.track_reference(name)
    got = _track(c)
    assert all(np.asarray(getattr(got, k)).dtype == np.int32 and np.array_equal(getattr(got, k), ref[k]) for k in got._fields)
    t = people.track(torch.as_tensor(c["joints"]), None if c["groups"] is None else torch.as_tensor(c["groups"]), c["max_mm"],
                     c["max_gap"], c["min_joints"], n_groups=c["G"])
    assert torch.is_tensor(t.track_id) and all(np.array_equal(a.numpy(), b) for a, b in zip(t, got))


def test_tracker_cases_reach_their_branches():
    c, ref = C.track_case("crossing"), C.track_reference("crossing")
    assert np.array_equal(ref["track_id"], c["ident"]) and ref["n_tracks"].tolist() == [2]        # identities survive the crossing
    exact, plus = C.track_reference("gap_exact"), C.track_reference("gap_plus_one")
    assert exact["n_tracks"].tolist() == [1] and exact["counters"]["freed"] == 0 and set(exact["track_id"].ravel()) == {-1, 0}
    assert plus["n_tracks"].tolist() == [2] and plus["counters"]["freed"] == 1 and plus["track_id"][-1].max() == 1
    ninth = C.track_reference("ninth")
    assert ninth["n_dropped"].tolist() == [1] and ninth["track_id"][1, 7] == -1 and ninth["track_id"][2, 7] == 8
    assert ninth["counters"]["reused"] == 1 and ninth["n_tracks"].tolist() == [9]
    g = C.track_reference("groups")
    assert g["n_tracks"].tolist() == [2, 2] and (g["track_id"][4] == -1).all() and g["track_id"][:, 0].tolist() == [0, 0, 0, 0, -1, 0, 0, 0, 0]
    assert g["track_id"][1, 1] == 1 and g["track_id"][5, 1] == 1          # each recording counts its own ids from 0
    tie = C.track_reference("tie")
    assert tie["counters"]["ties"] == 1 and tie["track_id"].tolist() == [[-1, 0, -1], [0, -1, 1]]
    sp = C.track_reference("sparse_joints")
    assert sp["track_id"].tolist() == [[0, -1], [0, -1], [1, -1], [-1, -1]]


def test_to_tracks_scatters_without_reading_back():
    rng = np.random.default_rng(3)
    N, K, V, J = 5, 3, 2, 4
    p2d = rng.normal(size=(N, K, V, J, 2)).astype(np.float32)
    tid = np.array([[0, 1, -1], [1, 0, -1], [-1, 0, 2], [2, -1, 0], [5, 1, 0]], dtype=np.int32)
    tracks, groups = people.to_tracks(tid, p2d, 3)
    assert tracks.shape == (3, N, V, J, 2) and tracks.dtype == np.float32 and groups.dtype == np.int32
    for t in range(3):
        for n in range(N):
            k = np.nonzero(tid[n] == t)[0]
            assert np.array_equal(tracks[t, n], p2d[n, k[0]]) if len(k) else np.isnan(tracks[t, n]).all()
    assert groups.tolist() == [t for t in range(3) for _ in range(N)]
    rec = np.array([0, 0, 1, 1, 1], dtype=np.int32)
    t2, g2 = people.to_tracks(torch.as_tensor(tid), torch.as_tensor(p2d), 3, groups=torch.as_tensor(rec), n_groups=2)
    assert torch.is_tensor(t2) and np.array_equal(t2.numpy(), tracks, equal_nan=True)
    assert g2.reshape(3, N).tolist() == [[2 * t + r for r in rec] for t in range(3)]
    with pytest.raises(ValueError, match="n_groups"):
        people.to_tracks(tid, p2d, 3, groups=rec)
