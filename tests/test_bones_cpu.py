"""The restatement of tests/bones_ref.py (what csrc/sks_bones.hip must equal bit for bit) held to independent references, without
a GPU: medians and MADs against np.partition and statistics.median_low; the unit-covariance single-bone projection against its
closed form; every case converged within 16 trips -- the condition under which the GPU test's bit-for-bit comparison says
anything --; the Sigma-cost against scipy's SLSQP; the inactive-bone contract in every bit; skeleton.py's vectorised host functions
against the restatement; the skeleton trees of scene.DATASETS; the forest check and every argument refusal; and the articulated
synthetic motion."""
import statistics

import numpy as np
import pytest
import torch

from skelsplat_amd import skeleton
from skelsplat_amd.scene import DATASETS, articulated_motion, skeleton_template
from tests import bones_cases as BC
from tests import bones_ref as REF

PARENTS = {"h36m": (0, [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15]),
           "panoptic": (2, [2, 0, -1, 0, 3, 4, 2, 6, 7, 0, 9, 10, 2, 12, 13, 1, 15, 1, 17]),
           "occlusion-person": (0, [-1, 0, 1, 2, 0, 4, 5, 0, 7, 7, 9, 10, 7, 12, 13])}


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("dataset", sorted(DATASETS))
def test_skeleton_trees(dataset):
    d = DATASETS[dataset]
    bones, t = d["bones"], skeleton_template(dataset)
    J = t.shape[0]
    root, parents = PARENTS[dataset]
    assert sorted(bones) == sorted((p, j) for j, p in enumerate(parents) if p >= 0) and parents[root] == -1
    # a spanning tree: J - 1 bones without a cycle (the forest check), every joint reached from the root
    assert len(bones) == J - 1 and skeleton.checked_bones(bones, J).shape == (J - 1, 2)
    reached, grew = {root}, True
    while grew:
        new = {c for p, c in bones if p in reached} - reached
        grew = bool(new)
        reached |= new
    assert reached == set(range(J))
    assert all(tuple(l) in bones for l in d["limbs"])
    assert all(np.linalg.norm(t[c] - t[p]) > 0 for p, c in bones)


@pytest.mark.parametrize("name", BC.NAMES)
def test_medians_and_mads(name):
    c, ref = BC.cases()[name], BC.reference(name)
    M, B = ref["measured"], len(c["bones"])
    # the measure against numpy's norm, within the rounding of a sum of three squares
    x = c["xyz"].astype(np.float64)
    bn = np.asarray(c["bones"])
    with np.errstate(invalid="ignore"):
        want = np.linalg.norm(x[:, bn[:, 1]] - x[:, bn[:, 0]], axis=-1)
    seen = ~np.isnan(M)
    assert np.allclose(M[seen], want[seen], rtol=2.0 ** -23, atol=0)
    if c["max_sigma"] is None and c["valid"] is None:
        assert np.array_equal(seen, np.isfinite(want))
    for g in range(c["G"]):
        for b in range(B):
            rows = np.ones(M.shape[0], bool) if c["groups"] is None else c["groups"] == g
            l = M[rows & seen[:, b], b]
            assert ref["n_used"][g, b] == l.size
            if l.size == 0:
                assert np.isnan(ref["length"][g, b]) and np.isnan(ref["mad"][g, b])
                continue
            k = (l.size - 1) // 2
            assert ref["length"][g, b] == np.partition(l, k)[k] == statistics.median_low(l.tolist())
            assert ref["length"][g, b] in l                       # one of the inputs
            dev = np.abs(l - ref["length"][g, b])                    # float32
            assert ref["mad"][g, b] == np.partition(dev, k)[k] == statistics.median_low(dev.tolist())
    assert c["max_sigma"] is None or name == "gate_all" or (0 < ref["n_used"]).all()
    if name == "gate_some":
        assert (ref["n_used"] < M.shape[0]).any() and (ref["n_used"] > 0).all()
    if name == "gate_all":
        assert (ref["n_used"] == 0).all() and np.isnan(ref["length"]).all()
    if name == "groups_3":
        assert (ref["n_used"][1] == 0).all() and (ref["n_used"][0] > 0).all() and ref["n_used"].sum() == 2 * (6 + 6)


@pytest.mark.parametrize("name", BC.NAMES)
def test_every_case_converges_and_meets_its_lengths(name):
    """A condition, not a measurement: every projection case the GPU test runs converges within its trips in the restatement
    (the cases named in UNCONVERGED are about the trip limit), and a converged frame's active bones have the target's length."""
    c, ref = BC.cases()[name], BC.reference(name)
    live = ref["n_active"] > 0
    assert np.isnan(ref["residual"][~live]).all() and (ref["n_trips"][~live] == 0).all()
    assert (ref["n_trips"] <= c["iters"]).all()
    if name in BC.UNCONVERGED:
        assert (ref["n_trips"][live] == c["iters"]).all() and (ref["residual"][live] > c["tol"]).any()
        return
    assert (ref["residual"][live] <= np.float32(c["tol"])).all(), (ref["residual"].max(), ref["n_trips"].max())
    assert (ref["n_trips"] < 16).all()
    # an independent look at the result: the lengths of the projected joints, measured afresh, in the frames whose bones were
    # all active (float32 joints of a few thousand mm: each end rounded by up to 2^-13 mm per coordinate)
    got = REF.measure(ref["joints"], c["bones"])
    T = ref["target"][np.clip(0 if c["groups"] is None else c["groups"], 0, ref["target"].shape[0] - 1)]
    full = ref["n_active"] == len(c["bones"])
    assert (np.abs(got - T)[full] <= c["tol"] + 2 * 3 * 2.0 ** -13).all()


def test_single_bone_closed_form():
    """Unit covariance, one bone: both ends move by half the excess along the bone, in one trip."""
    rng = np.random.default_rng(3)
    y = rng.uniform(-1000, 1000, (6, 2, 3)).astype(np.float32)
    L = np.array([[250.0]], dtype=np.float32)
    joints, res, trips, nact = REF.project(y, ((0, 1),), L)
    d = y[:, 1].astype(np.float64) - y[:, 0]
    n = np.linalg.norm(d, axis=-1, keepdims=True)
    half = 0.5 * (n - 250.0) * d / n
    assert np.allclose(joints[:, 0], y[:, 0] + half, rtol=0, atol=2.0 ** -13) and np.allclose(joints[:, 1], y[:, 1] - half, rtol=0, atol=2.0 ** -13)
    assert (trips == 1).all() and (res <= 1e-3).all() and (nact == 1).all()
    # with a covariance 9 times larger at the child, the child takes nine tenths of the excess
    cov6 = np.zeros((6, 2, 6), dtype=np.float32)
    cov6[:, 0, [0, 3, 5]], cov6[:, 1, [0, 3, 5]] = 1.0, 9.0
    joints = REF.project(y, ((0, 1),), L, cov6)[0]
    assert np.allclose(joints[:, 1], y[:, 1] - 1.8 * half, rtol=0, atol=2.0 ** -12) and np.allclose(joints[:, 0], y[:, 0] + 0.2 * half, rtol=0, atol=2.0 ** -12)


@pytest.mark.parametrize("name", ["h36m_isotropic", "h36m_needles", "panoptic_needles", "occlusion-person_needles", "h36m_unit_sigma"])
def test_sigma_cost_against_slsqp(name):
    """The fit is A pose on the lengths, not the Sigma-closest one: its Sigma-cost is never BELOW what scipy's SLSQP finds from the
    same start beyond rounding (that would make SLSQP, a local minimiser of exactly this cost, or the restatement wrong); how far
    ABOVE it ends is printed and recorded in MEASUREMENTS.md, not asserted."""
    from scipy.optimize import minimize
    c, ref = BC.cases()[name], BC.reference(name)
    bn = np.asarray(c["bones"])
    T = ref["target"][0].astype(np.float64)
    worst = 0.0
    for f in range(2):
        y = c["xyz"][f].astype(np.float64)
        J = y.shape[0]
        cov = None if c["cov6"] is None else c["cov6"][f].astype(np.float64)
        W = np.tile(np.eye(3), (J, 1, 1)) if cov is None else np.linalg.inv(
            np.stack([[[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]] for q in cov]))
        # over the displacement v = x - y, so that the unknowns are a few mm, not a few thousand
        cost = lambda v: float(np.einsum("ja,jab,jb->", v.reshape(-1, 3), W, v.reshape(-1, 3)))
        grad = lambda v: (2.0 * np.einsum("jab,jb->ja", W, v.reshape(-1, 3))).ravel()

        def ends(v):
            x = y + v.reshape(-1, 3)
            return x[bn[:, 1]] - x[bn[:, 0]]

        def jac(v):
            d = ends(v)
            u = d / np.linalg.norm(d, axis=-1, keepdims=True)
            A = np.zeros((len(bn), J, 3))
            for b, (p, ch) in enumerate(bn):
                A[b, ch], A[b, p] = u[b], -u[b]
            return A.reshape(len(bn), -1)
        cons = dict(type="eq", fun=lambda v: np.linalg.norm(ends(v), axis=-1) - T, jac=jac)
        sol = minimize(cost, np.zeros(3 * J), jac=grad, constraints=[cons], method="SLSQP", options=dict(maxiter=400, ftol=1e-9))
        assert sol.success and np.abs(cons["fun"](sol.x)).max() < 1e-6, sol.message
        mine = cost((ref["joints"][f].astype(np.float64) - y).ravel())
        assert abs(mine - REF.sigma_cost(ref["joints"][f], y, cov, c["floor"])) <= 1e-9 * mine
        # float32 joints and SLSQP's own tolerance: 1e-4 relative is far above both and far below the excess seen
        assert mine >= sol.fun * (1.0 - 1e-4), (mine, sol.fun)
        worst = max(worst, mine / sol.fun - 1.0)
    print(f"{name}: Sigma-cost above SLSQP's by at most {100 * worst:.2f} %")


def test_inactive_bone_contract():
    """Bit for bit: a joint that only inactive bones touch comes back with its input's bits, NaN payload and sign included; a frame
    without an active bone is a copy with residual NaN, 0 trips, 0 active."""
    c, ref = BC.cases()["degenerate_rows"], BC.reference("degenerate_rows")
    x, out = c["xyz"], ref["joints"]
    same = lambda f, j: np.array_equal(_bits(out[f, j]), _bits(x[f, j]))
    moved = lambda f, j: not same(f, j)
    # frame 0: joint 13 (a leaf) NaN -> its bone idle, its parent 12 still moved by bone (11, 12)
    assert same(0, 13) and np.isnan(out[0, 13]).all() and moved(0, 12) and ref["n_active"][0] == 15
    # frame 1: one NaN coordinate of joint 2 -> bones (1,2) and (2,3) idle: joint 3 untouched, joint 1 moved by (0,1)
    assert same(1, 2) and same(1, 3) and moved(1, 1) and ref["n_active"][1] == 14
    # frame 2: joint 8 (thorax) masked: its four bones idle; 7 moved by (0,7); 9 by (9,10); 11 by (11,12)
    assert same(2, 8) and moved(2, 7) and moved(2, 9) and ref["n_active"][2] == 12
    # frame 3: zero covariance at 5 and a negative variance at 15: (4,5), (5,6) and (14,15), (15,16) idle
    assert all(same(3, j) for j in (5, 6, 15, 16)) and moved(3, 4) and moved(3, 14) and ref["n_active"][3] == 12
    # frame 4: a NaN covariance entry at joint 11; frame 5: joints 5 and 6 coincide -> bone (5,6) idle, 6 a leaf
    assert same(4, 11) and ref["n_active"][4] == 14 and same(5, 6) and moved(5, 5) and ref["n_active"][5] == 15
    # with a floor of 4 mm^2 the zero covariance is usable again, the negative one (-4 + 4 = 0) still is not
    fl = BC.reference("cov_floor")
    assert ref["n_active"][3] == 12 and fl["n_active"][3] == 14
    # NaN payloads: a quiet NaN with a payload and a set sign bit survives in an untouched joint
    y = c["xyz"][:1].copy()
    y[0, 13] = np.array([0xffc12345, 0x7fc00001, 0x7fffffff], dtype=np.uint32).view(np.float32)
    got = REF.project(y, c["bones"], ref["target"])[0]
    assert np.array_equal(_bits(got[0, 13]), _bits(y[0, 13]))
    host = skeleton.project_host(y, c["bones"], ref["target"]).joints
    assert np.array_equal(_bits(host), _bits(got))
    # targets NaN, 0 and negative: those bones idle; every frame of a gated-out recording a copy
    bt, cb = BC.reference("bad_targets"), BC.cases()["bad_targets"]
    assert (bt["n_active"] == 14 - 3).all()
    ga, cg = BC.reference("gate_all"), BC.cases()["gate_all"]
    assert np.array_equal(_bits(ga["joints"]), _bits(cg["xyz"])) and np.isnan(ga["residual"]).all() and (ga["n_trips"] == 0).all()
    # a frame whose group id is out of range is a copy too
    g3, c3 = BC.reference("groups_3"), BC.cases()["groups_3"]
    assert np.array_equal(_bits(g3["joints"][6]), _bits(c3["xyz"][6])) and g3["n_active"][6] == 0 and g3["n_active"][5] == 2
    # the forest's joint without a bone
    fo, cf = BC.reference("forest"), BC.cases()["forest"]
    assert np.array_equal(_bits(fo["joints"][:, 6]), _bits(cf["xyz"][:, 6])) and not np.array_equal(fo["joints"][:, :6], cf["xyz"][:, :6])


@pytest.mark.parametrize("name", BC.NAMES)
def test_host_functions_equal_the_restatement(name):
    """skeleton.py's float64 numpy functions (what arrays and CPU tensors get), vectorised over the frames, bit for bit."""
    c, ref = BC.cases()[name], BC.reference(name)
    h = skeleton.bone_lengths(c["xyz"], c["bones"], c["cov6"], c["valid"], c["groups"], c["max_sigma"], n_groups=c["G"])
    for key in ("measured", "length", "mad", "n_used"):
        got = getattr(h, key)
        assert got.dtype == ref[key].dtype and np.array_equal(got, ref[key], equal_nan=True), key
    t = lambda a: None if a is None else torch.as_tensor(a)
    p = skeleton.project_to_lengths(t(c["xyz"]), c["bones"], t(ref["target"]), t(c["cov6"]), t(c["valid"]), t(c["groups"]), c["floor"],
                                    c["iters"], c["tol"])
    assert np.array_equal(_bits(p.joints), _bits(ref["joints"])) and np.array_equal(p.residual, ref["residual"], equal_nan=True)
    assert np.array_equal(p.n_trips, ref["n_trips"]) and np.array_equal(p.n_active, ref["n_active"])


def test_symmetrize_and_bone_index():
    bones = DATASETS["h36m"]["bones"]
    idx = skeleton.bone_index(bones, DATASETS["h36m"]["limbs"])
    assert [bones[i] for i in idx] == [tuple(l) for l in DATASETS["h36m"]["limbs"]]
    L = np.arange(32, dtype=np.float32).reshape(2, 16)
    S = skeleton.symmetrize(L, [(idx[0], idx[1])])
    want = np.float32((L[:, idx[0]] + L[:, idx[1]]) * np.float32(0.5))
    assert np.array_equal(S[:, idx[0]], want) and np.array_equal(S[:, idx[1]], want) and S.dtype == np.float32
    keep = [i for i in range(16) if i not in idx[:2]]
    assert np.array_equal(S[:, keep], L[:, keep]) and L[0, idx[0]] != S[0, idx[0]]
    St = skeleton.symmetrize(torch.as_tensor(L), [(idx[0], idx[1])])
    assert np.array_equal(St.numpy(), S)


def test_refusals():
    x = np.zeros((4, 3, 3), dtype=np.float32)
    ok = ((0, 1), (1, 2))
    for bad, text in ((((0, 1), (1, 2), (2, 0)), "forest"), (((0, 1), (0, 1)), "forest"), (((1, 1),), "forest"),
                      (((0, 3),), "outside"), (((-1, 0),), "outside"), ((), "bones"), (((0.0, 1.0),), "integers"),
                      (((0, 1, 2),), "bones")):
        with pytest.raises(ValueError, match=text):
            skeleton.checked_bones(bad, 3)
    with pytest.raises(ValueError, match="forest"):
        skeleton.bone_lengths(x, ((0, 1), (1, 2), (0, 2)))
    with pytest.raises(ValueError, match="joints"):
        skeleton.checked_bones(ok, 33)
    with pytest.raises(ValueError, match="bones"):
        skeleton.checked_bones(tuple((j, j + 1) for j in range(32)), 32)
    assert skeleton.checked_bones(torch.tensor(ok), 3).dtype == np.int32
    with pytest.raises(ValueError, match="integers"):
        skeleton.checked_bones(torch.tensor(ok).float(), 3)
    with pytest.raises(ValueError, match="xyz"):
        skeleton.bone_lengths(x[0], ok)
    with pytest.raises(ValueError, match="cov6"):
        skeleton.bone_lengths(x, ok, cov6=np.zeros((4, 3, 5)), max_sigma_mm=1.0)
    with pytest.raises(ValueError, match="max_sigma_mm"):
        skeleton.bone_lengths(x, ok, max_sigma_mm=1.0)
    with pytest.raises(ValueError, match="max_sigma_mm"):
        skeleton.bone_lengths(x, ok, cov6=np.zeros((4, 3, 6)), max_sigma_mm=-1.0)
    with pytest.raises(ValueError, match="valid"):
        skeleton.bone_lengths(x, ok, valid=np.ones((4, 2), bool))
    with pytest.raises(ValueError, match="groups"):
        skeleton.bone_lengths(x, ok, groups=np.zeros(3, int))
    with pytest.raises(ValueError, match="groups"):
        skeleton.bone_lengths(x, ok, groups=np.zeros(4, int), n_groups=257)
    with pytest.raises(ValueError, match="without groups"):
        skeleton.bone_lengths(x, ok, n_groups=2)
    L = np.ones((1, 2), dtype=np.float32)
    for kw, text in ((dict(max_iters=0), "max_iters"), (dict(max_iters=17), "max_iters"), (dict(cov_floor=-1.0), "cov_floor"),
                     (dict(cov_floor=float("nan")), "cov_floor"), (dict(tol_mm=-1e-3), "tol_mm"), (dict(tol_mm=float("inf")), "tol_mm")):
        with pytest.raises(ValueError, match=text):
            skeleton.project_to_lengths(x, ok, L, **kw)
    with pytest.raises(ValueError, match="lengths"):
        skeleton.project_to_lengths(x, ok, np.ones((1, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="without groups"):
        skeleton.project_to_lengths(x, ok, np.ones((2, 2), dtype=np.float32))
    # a (B,) row of lengths is one recording's
    assert skeleton.project_to_lengths(x + np.arange(3, dtype=np.float32)[None, :, None], ok, L[0]).n_active.tolist() == [2] * 4


@pytest.mark.parametrize("dataset", sorted(DATASETS))
def test_articulated_motion_keeps_the_lengths(dataset):
    gt = articulated_motion(dataset, 40)
    t = skeleton_template(dataset)
    bn = np.asarray(DATASETS[dataset]["bones"])
    l = np.linalg.norm(gt[:, bn[:, 1]] - gt[:, bn[:, 0]], axis=-1)
    want = np.linalg.norm(t[bn[:, 1]] - t[bn[:, 0]], axis=-1)
    # float64 kinematics on coordinates of a few thousand mm: a few ulps of 2^-41 mm
    assert np.abs(l - want[None]).max() < 1e-9
    assert np.abs(gt[1:] - gt[:-1]).max() > 5.0 and np.abs(gt[1:] - gt[:-1]).max() < 80.0       # it moves, and slowly
    # as float32 (what the pipeline sees) the MAD relative to the median is at rounding level, unlike the independent motions
    h = skeleton.bone_lengths(gt.astype(np.float32), DATASETS[dataset]["bones"])
    assert float((h.mad / h.length).max()) < 1e-5
