"""csrc/sks_people.hip on the device: sks_associate_people and sks_track_people against the op-by-op restatement of
tests/people_ref.py on every case of tests/people_cases.py, bit for bit in every output -- both rules are fixed sequences of
+ - x / sqrt in float64 compiled without contraction, and every choice is made on a total order; the invariances the header
promises (detection type, shared and per-frame rigs, N, the place in the batch, the stream, a captured graph); and the front end
through the pipeline: the gathered detections triangulate to the joints of the hand-ordered ones, and a tracked three-person
sequence optimises to the joints of the three single-person runs."""
import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, people
from skelsplat_amd.triangulation import triangulate_sequence
from tests import people_cases as C
from tests import people_ref as R

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _same_bits(got, want):
    """Equal in every bit, except that a NaN may be any NaN (a freshly made NaN carries no promise about its payload)."""
    g, w = _np(got), _np(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if g.dtype.kind != "f":
        return np.array_equal(g, w)
    bits = np.uint32 if g.dtype == np.float32 else np.uint64
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(bits)[~nan], w.view(bits)[~nan])


def _run(c, device, x=None, P=None, valid=None, **kw):
    x = c["x"] if x is None else x
    valid = c["valid"] if valid is None else valid
    args = dict(max_px=c["max_px"], min_joints=c["min_joints"], min_views=c["min_views"], max_people=c["K"])
    args.update(kw)
    return people.associate(torch.as_tensor(c["P"] if P is None else P, device=device), torch.as_tensor(x, device=device),
                            None if valid is None else torch.as_tensor(valid, device=device), **args)


def _equal(got, ref):
    return all(_same_bits(getattr(got, k), ref[k]) for k in got._fields)


@pytest.mark.parametrize("name", C.NAMES)
def test_association_equals_the_restatement(device, name):
    """V x M = 2x2 (h36m_2x2), 3x2 (view_rule, duplicate_tie), 4x3 with J = 17, D = 64, 65 and 128, the crowd at 8x16 whose 7 168
    pairs are nearly all edges, and every hand case: assign, the three counters, cost and the gathered detections."""
    c, ref = C.case(name), C.reference(name)
    got = _run(c, device)
    assert got.assign.dtype == torch.int32 and got.cost.dtype == torch.float64 and got.poses_2d.dtype == torch.as_tensor(c["x"]).dtype
    for k in got._fields:
        assert _same_bits(getattr(got, k), ref[k]), k


def test_the_crowd_is_the_longest_list(device):
    """One sorter for every length: the crowd fills 7 000 of the 8 192 entries the launch reserves for 8 x 16, within a CU's LDS."""
    c, ref = C.case("crowd_8x16"), C.reference("crowd_8x16")
    edges = sum(1 for v in ref["frames"][0]["costs"].values() if v <= c["max_px"])
    launch = _lib.people_launch(8, 16)
    assert 7000 <= edges <= 7168 <= launch["assoc_list_entries"] == 8192 and launch["assoc_lds_bytes"] <= 160 * 1024
    assert ref["counters"]["view_refused"] > 6000 and ref["n_overflow"][0] > 0


@pytest.mark.parametrize("name", ["panoptic_5x3", "h36m_4x4_drop", "nonfinite"])
def test_float32_and_float64_detections(device, name):
    """Each type against the restatement on its own inputs; the float64 run of float32 numbers gives the float32 run's choices."""
    c, ref = C.case(name), C.reference(name)
    x64 = c["x"].astype(np.float64)
    want = R.associate(c["P"], x64, c["valid"], c["max_px"], c["min_joints"], c["min_views"], c["K"])
    got = _run(c, device, x=x64)
    assert got.poses_2d.dtype == torch.float64 and _equal(got, want)
    assert np.array_equal(want["assign"], ref["assign"]) and _same_bits(got.cost, ref["cost"])


def test_per_frame_rigs_that_equal_one_rig(device):
    c, ref = C.case("h36m_4x4_drop"), C.reference("h36m_4x4_drop")
    P = np.repeat(c["P"][None], len(c["x"]), axis=0)
    assert _equal(_run(c, device, P=P), ref)
    P[1] = P[1, ::-1]                                     # and a rig of its own: frame 1 seen by the cameras in reverse order
    x, valid = c["x"].copy(), c["valid"].copy()
    x[1], valid[1] = x[1, ::-1], valid[1, ::-1]
    assert _equal(_run(c, device, x=x, P=P, valid=valid), R.associate(P, x, valid, c["max_px"]))


def test_a_frame_does_not_depend_on_the_batch_or_the_stream(device):
    """The 7 frames of a generated scene: alone (N = 1), together (N = 7), cycled to N = 64 in another order, on a side stream and
    in a captured graph replayed twice -- the same bits every time, and the restatement's."""
    c = C.generated("panoptic", 5, 3, 1500.0, 0.2, 15.0, seed=77, N=7, M=4)
    ref = R.associate(c["P"], c["x"], c["valid"], c["max_px"])
    together = _run(c, device)
    assert _equal(together, ref)
    for f in range(7):
        alone = _run(c, device, x=c["x"][f:f + 1], valid=c["valid"][f:f + 1])
        assert all(_same_bits(a[0], _np(b)[f]) for a, b in zip(alone, together))
    order = (np.arange(64) * 5 + 3) % 7
    args = [torch.as_tensor(a, device=device) for a in (c["P"], c["x"][order], c["valid"][order])]
    want = [_np(t)[order] for t in together]
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        got = people.associate(*args, max_px=c["max_px"])
    side.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(got, want))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        people.associate(*args, max_px=c["max_px"])        # (warm: the allocator's blocks exist before the capture)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            cap = people.associate(*args, max_px=c["max_px"])
    for _ in range(2):
        for t in cap:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(cap, want))


def test_out_tensors_and_refusals(device):
    c, ref = C.case("h36m_2x2"), C.reference("h36m_2x2")
    first = _run(c, device)
    out = people.Association(*(torch.zeros_like(t) for t in first))
    assert _run(c, device, out=out) is out and _equal(out, ref)
    with pytest.raises(ValueError, match="out.cost"):
        _run(c, device, out=out._replace(cost=out.cost.float()))
    lib = _lib.load()
    x = torch.as_tensor(c["x"], device=device)
    rc = lib.sks_associate_people(3, 2, 2, 17, 8, first.cost.data_ptr(), 5, x.data_ptr(), None, None, 15.0, 3, 2, None, None, None, None,
                                  None, None, None, None)
    assert rc != 0 and b"rig_stride" in lib.sks_last_error()
    rc = lib.sks_associate_people(3, 2, 2, 17, 8, first.cost.data_ptr(), 0, x.data_ptr(), None, None, 15.0, 3, 2, first.assign.data_ptr(),
                                  first.n_people.data_ptr(), first.n_overflow.data_ptr(), first.n_unassigned.data_ptr(),
                                  first.cost.data_ptr(), None, first.cost.data_ptr(), None)
    assert rc != 0 and b"input's type" in lib.sks_last_error()


def test_gathered_detections_triangulate_like_the_hand_ordered_ones(device):
    c, ref = C.case("h36m_4x4_drop"), C.reference("h36m_4x4_drop")
    N, V, M, J = c["x"].shape[:4]
    K = c["K"]
    got = _run(c, device)
    P = torch.as_tensor(c["P"], device=device)
    p2d = got.poses_2d.reshape(N * K, V, J, 2)
    joints = triangulate_sequence(P, p2d, valid=people.kept(p2d)).reshape(N, K, J, 3)
    # by hand: person p's detections picked with the known permutation, its masked joints left out through `valid`
    f, v = np.arange(N)[:, None, None], np.arange(V)[None, None, :]
    slot = c["perm"].transpose(0, 2, 1)                                            # (N,people,V)
    hand_x, hand_valid = c["x"][f, v, slot], c["valid"][f, v, slot]               # (N,people,V,J,2), (N,people,V,J)
    n_p = slot.shape[1]
    hand = triangulate_sequence(P, torch.as_tensor(hand_x.reshape(N * n_p, V, J, 2), device=device),
                                valid=torch.as_tensor(hand_valid.reshape(N * n_p, V, J), device=device)).reshape(N, n_p, J, 3).cpu().numpy()
    assign = ref["assign"]
    for n in range(N):
        for k in range(n_p):
            p = int(np.nonzero((slot[n] == assign[n, k]).all(axis=1))[0][0])
            assert _same_bits(joints[n, k], hand[n, p]), (n, k)
        assert bool(torch.isnan(joints[n, n_p:]).all())


# ------------------------------------------------------------------------------------------------------------ tracking
def _track(c, device, **kw):
    return people.track(torch.as_tensor(c["joints"], device=device), None if c["groups"] is None else torch.as_tensor(c["groups"], device=device),
                        c["max_mm"], c["max_gap"], c["min_joints"], n_groups=c["G"], **kw)


@pytest.mark.parametrize("name", list(C.TRACK))
def test_tracker_equals_the_restatement(device, name):
    c, ref = C.track_case(name), C.track_reference(name)
    got = _track(c, device)
    assert all(_same_bits(getattr(got, k), ref[k]) for k in got._fields)


def test_tracker_on_a_long_shuffled_sequence_side_stream_and_graph(device):
    """Six people for 200 frames in two interleaved recordings, rows shuffled per frame, with drop-outs and NaN joints: against
    the restatement, on a side stream, and captured (the memset and the launch) and replayed twice."""
    rng = np.random.default_rng(9)
    N, K, J = 200, 8, 17
    from skelsplat_amd.scene import skeleton_template
    tmpl = skeleton_template("h36m")
    start, vel = rng.uniform(-3000, 3000, (6, 3)) * [1, 1, 0], rng.normal(0, 25.0, (6, 3)) * [1, 1, 0]
    x = np.full((N, K, J, 3), np.nan, dtype=np.float32)
    groups = (np.arange(N) % 2).astype(np.int32)
    for f in range(N):
        rows = rng.permutation(K)
        for p in range(6):
            if rng.uniform() < 0.3:
                continue
            body = tmpl + start[p] + vel[p] * (f // 2) + rng.normal(0, 10.0, tmpl.shape)
            body[rng.uniform(size=J) < 0.1] = np.nan
            x[f, rows[p]] = body
    c = dict(joints=x, groups=groups, G=2, max_mm=250.0, max_gap=2, min_joints=5)
    ref = R.track(x, groups, 2, 250.0, 2, 5)
    assert ref["counters"]["freed"] > 0 and ref["counters"]["reused"] > 0 and ref["n_tracks"].min() > 6
    got = _track(c, device)
    assert all(_same_bits(getattr(got, k), ref[k]) for k in got._fields)
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        again = _track(c, device)
    side.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(again, got))
    graph = torch.cuda.CUDAGraph()
    jd, gd = torch.as_tensor(x, device=device), torch.as_tensor(groups, device=device)
    with torch.cuda.stream(side):
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            cap = people.track(jd, gd, 250.0, 2, 5, n_groups=2)
    for _ in range(2):
        for t in cap:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(cap, got))


# ------------------------------------------------------------------------------------------------------------ end to end
def test_three_people_through_the_pipeline(device):
    """16 frames, 3 people, 4 views, every view's slots shuffled per frame: associate -> triangulate -> track -> to_tracks ->
    FramePipeline.optimize_sequence(None, ..) gives, bit for bit, the joints of the run on the hand-ordered single-person detections."""
    from skelsplat_amd.loop import FramePipeline
    from skelsplat_amd.scene import GaussianModel, SyntheticScene, articulated_motion, project_points
    V, J, N, n_p, M, F, ITERS = 4, 17, 16, 3, 4, 8, 8
    W, H = 160, 128
    sc = SyntheticScene("h36m", n_views=V, seed=9, W=W, H=H, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5, device=device)
    rng = np.random.default_rng(13)
    off = C.grid_offsets(n_p, 1000.0)
    motion = np.stack([articulated_motion("h36m", N, seed=20 + p) + off[p] for p in range(n_p)], axis=1)      # (N,people,J,3)
    hand = np.stack([[[project_points(cam, motion[n, p]) for cam in sc.cameras] for p in range(n_p)] for n in range(N)])
    hand = (hand + rng.normal(0.0, 0.3, hand.shape)).astype(np.float32)            # (N,people,V,J,2)
    x = np.full((N, V, M, J, 2), np.nan, dtype=np.float32)
    perm = np.stack([[rng.permutation(M)[:n_p] for _ in range(V)] for _ in range(N)])      # (N,V,people)
    for n in range(N):
        for v in range(V):
            x[n, v, perm[n, v]] = hand[n, :, v]

    got = people.associate(sc.cameras, torch.as_tensor(x, device=device), max_px=4.0, max_people=M)
    assert got.n_people.tolist() == [n_p] * N and got.n_unassigned.tolist() == [0] * N
    assert all(C.recovered(got.assign[n].cpu().numpy(), perm[n]) for n in range(N))
    flat = got.poses_2d.reshape(N * M, V, J, 2)
    joints = triangulate_sequence(sc.cameras, flat, valid=people.kept(flat)).reshape(N, M, J, 3)
    tracks = people.track(joints, max_mm=200.0, max_gap=2, min_joints=5)
    assert tracks.n_tracks.tolist() == [n_p] and tracks.n_dropped.tolist() == [0]
    p2d, groups = people.to_tracks(tracks.track_id, got.poses_2d, n_p)
    assert tuple(p2d.shape) == (n_p, N, V, J, 2) and groups.tolist() == [t for t in range(n_p) for _ in range(N)]
    # which person is track t: the one whose detections frame 0 holds -- and then every frame does
    who = [int(np.nonzero([_same_bits(p2d[t, 0], hand[0, p]) for p in range(n_p)])[0][0]) for t in range(n_p)]
    assert sorted(who) == list(range(n_p))
    by_hand = torch.as_tensor(np.stack([hand[:, p] for p in who]), device=device)          # (tracks,N,V,J,2)
    assert _same_bits(p2d, by_hand.cpu().numpy())

    def model():
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9, scaling_modifier=1.0,
                                                device=device)
        gm.training_setup()
        return gm

    def run(detections):
        pipe = FramePipeline(model(), sc.cameras, frames=F, streams=2, dataset="h36m")
        return pipe.optimize_sequence(None, detections.reshape(n_p * N, V, J, 2), iterations=ITERS, groups_per_graph=4, interleave=8).clone()
    ours, theirs = run(p2d), run(by_hand)
    assert tuple(ours.shape) == (n_p * N, J, 3) and bool(torch.isfinite(ours).all()) and _same_bits(ours, theirs.cpu().numpy())
