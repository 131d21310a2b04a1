"""The temporal fit of include/skelsplat_hip.h (sks_smooth_sequence) without a GPU: its two float64 references against each other
and against scipy's Savitzky-Golay filter, the cases of tests/smooth_cases.py reaching what they are there for, the host
counterpart smoothing.smooth_host and the host acceleration figures against the references, the Python argument checks, and the
library's own refusals, which come before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, smoothing
from tests import smooth_cases as SC
from tests import smooth_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND_MAX = 1e9          # every committed case's normal matrix; E64 means what it says only below it


def _host(c, **kw):
    return smoothing.smooth_host(c["xyz"], c["cov6"], c["weights"], c["valid"], c["groups"], c["h"], c["d"], c["taper"], c["floor"], **kw)


def test_the_two_references_agree():
    """(a) np.linalg.lstsq on the whitened design and (b) the fixed LDL^T sequence: the same taps everywhere, and values apart by
    E64 -- printed; on the committed cases 3.1e-4 float32 ulps for positions, 7.5e-8 mm per frame and 2.4e-7 mm^2 -- which has
    to stay far below half a float32 ulp for the device test's one-ulp bar to follow.  The bound asserted is float64's own:
    eps x condition number (at most 1e9, asserted) x a coefficient of at most 1e3 mm, 1.1e-4 mm, against a float32 ulp of 2.4e-4 mm
    at the cases' positions: under a quarter ulp (positions), 1e-4 absolute (velocity, covariance)."""
    worst = 0.0
    for name in SC.NAMES:
        a, b = SC.reference(name, "a"), SC.reference(name, "b")
        assert np.array_equal(a["n_used"], b["n_used"]), name
        for key in ("joints", "velocity", "cov6"):
            assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])), (name, key)
            assert np.array_equal(np.isnan(a[key]).all(-1), a["n_used"] == 0) and not np.isinf(b[key]).any(), (name, key)
        cond = float(np.nanmax(a["cond"], initial=0.0))
        worst = max(worst, cond)
        assert cond <= COND_MAX, (name, cond)
    e = SC.e64()
    print(f"E64: positions {e['joints']:.3g} float32 ulp, velocity {e['velocity']:.3g} mm/frame, covariance {e['cov6']:.3g} mm^2; "
          f"largest condition number {worst:.3g}")
    assert e["joints"] < 0.25 and e["velocity"] < 1e-4 and e["cov6"] < 1e-4, e


@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("h", [1, 3, 8])
def test_interior_frames_are_savitzky_golay(h, d):
    """Unit weights and the box taper: on interior frames (h <= f < N - h) the fit is the Savitzky-Golay filter of window 2h + 1
    and order d, and its velocity the filter's first derivative.  Edge frames are not compared: scipy's `interp` mode fits the
    last full window, this fit clips the window.  Relative to the largest magnitude of the compared block: a derivative crosses
    zero, where an element-wise ratio means nothing."""
    from scipy.signal import savgol_filter
    rng = np.random.default_rng(100 * h + d)
    N, J = 3 * h + 9, 3
    xyz = SC.trajectory(rng, N, J)
    case = dict(xyz=xyz, cov6=None, weights=None, valid=None, groups=None, h=h, d=d, taper="box", floor=0.0)
    x64 = xyz.astype(np.float64)
    want = {"joints": savgol_filter(x64, 2 * h + 1, d, deriv=0, axis=0), "velocity": savgol_filter(x64, 2 * h + 1, d, deriv=1, axis=0)}
    for ref in (REF.fit_lstsq(case), REF.fit_ldl(case)):
        assert (ref["n_used"][h:N - h] == 2 * h + 1).all()
        for key in ("joints", "velocity"):
            got, sg = ref[key][h:N - h], want[key][h:N - h]
            assert np.abs(got - sg).max() <= 1e-9 * max(np.abs(sg).max(), 1e-300), (key, np.abs(got - sg).max() / np.abs(sg).max())
    if d == 0:
        assert not REF.fit_ldl(case)["velocity"].any()


def test_every_case_reaches_its_branch():
    C, b = SC.cases(), lambda name: SC.reference(name, "b")
    T = SC.tile(17, 2)
    assert {C[f"seam_N{N}"]["xyz"].shape[0] for N in (T - 1, T, T + 1, 2 * T, 2 * T + 1)} == {T - 1, T, T + 1, 2 * T, 2 * T + 1}
    assert C["h32_joint_runs"]["h"] == C["h32_one_joint"]["h"] == 32 and C["h1"]["h"] == 1
    # 17 joints at h = 32 do not fit one stage: the kernel splits the joints into runs there (more workgroups than frame tiles)
    la = _lib.smooth_launch(20, 17, 32)
    assert la["groups"] > -(-20 // la["tile"]) and _lib.smooth_launch(20, 17, 2)["groups"] == -(-20 // T)
    for name in SC.NAMES:
        c, r = C[name], b(name)
        assert r["n_used"].max() <= 2 * c["h"] + 1 and np.array_equal(r["n_used"] == 0, np.isnan(r["joints"]).all(-1)), name
        if "reduced" in c["expect"]:
            assert ((r["deff"] >= 0) & (r["deff"] < c["d"])).any(), name
        if "empty" not in c["expect"]:
            assert (r["n_used"] > 0).all(), name
    r = b("short_N1")
    assert (r["deff"] == 0).all() and np.array_equal(r["joints"], C["short_N1"]["xyz"].astype(np.float64)) and not r["velocity"].any()
    assert np.allclose(r["cov6"], C["short_N1"]["cov6"], rtol=1e-5, atol=1e-6)       # (one tap: the fit's covariance is the tap's)
    assert (b("short_N2")["deff"] == 1).all() and (b("short_N5")["deff"] == 2).all() and (b("short_N5")["n_used"] == 5).all()
    r = b("degree_reduction")
    assert (r["deff"][3] == 0).all() and (r["n_used"][3] == 1).all() and not r["velocity"][3].any()
    assert (r["deff"][4:6] == 1).all() and (r["n_used"][4:6] == 2).all() and (r["deff"][:3] == 2).all()
    r = b("groups")
    assert (r["n_used"][T] == 3).all() and (r["n_used"][T - 1] == 3).all() and (r["n_used"][T // 2] == 3).all()
    assert (r["n_used"][2 * T + 1] == 3).all() and (r["n_used"][2 * T] == 3).all() and (r["n_used"][2 * T - 1] == 4).all() and (r["n_used"][T + 2] == 5).all()
    r = b("gaps")
    assert (r["n_used"][8:11, 1] == [4, 4, 4]).all() and np.isfinite(r["joints"][8:11, 1]).all()
    assert (r["n_used"][8:15, 2] == 0).all() and np.isnan(r["joints"][8:15, 2]).all() and np.isnan(r["cov6"][8:15, 2]).all()
    assert r["n_used"][7, 2] == 1 and r["n_used"][5, 2] == 3 and np.isfinite(r["joints"][5:8, 2]).all()
    r = b("nan_rows")
    assert r["n_used"][5, 2] == 4 and r["n_used"][7, 3] == 4 and r["n_used"][0, 4] == 2
    assert np.isfinite(r["joints"][[5, 7, 0], [2, 3, 4]]).all()
    r = b("bad_covariances")
    for f, j in C["bad_covariances"]["bad"]:
        assert r["n_used"][f, j] == 4 and np.isfinite(r["joints"][f, j]).all(), (f, j)
    assert b("cov_floor")["n_used"][4, 1] == 5
    r = b("weights")
    assert r["n_used"][3, 0] == 3 and r["n_used"][6, 1] == 4 and r["n_used"][7, 2] == 4 and np.isfinite(r["joints"]).all()


@pytest.mark.parametrize("name", SC.NAMES)
def test_smooth_host_against_the_references(name):
    """The host counterpart against (a): the same taps, positions within one float32 ulp (E64 is far below half an ulp, so the
    rounding to float32 moves the result by one ulp at most), velocity and covariance within one float32 ulp plus 16 x E64.  It is
    written apart from restatement (b) and vectorised, yet runs the same IEEE sequence: it equals (b) bit for bit, which is
    asserted too; and the optional outputs change nothing."""
    c, a, b = SC.cases()[name], SC.reference(name, "a"), SC.reference(name, "b")
    got = _host(c)
    e = SC.e64()
    assert got.n_used.dtype == np.int32 and np.array_equal(got.n_used, a["n_used"])
    for key, extra in (("joints", 0.0), ("velocity", 16 * e["velocity"]), ("cov6", 16 * e["cov6"])):
        g = getattr(got, key)
        assert g.dtype == np.float32 and np.array_equal(np.isnan(g), np.isnan(a[key])), key
        with np.errstate(invalid="ignore"):
            assert np.all(np.nan_to_num(np.abs(g - a[key])) <= np.nan_to_num(SC.ulp32(a[key])) + extra), key
        assert np.array_equal(g, b[key].astype(np.float32), equal_nan=True), key
    only = _host(c, want=("joints",))
    assert only.velocity is None and only.cov6 is None and only.n_used is None and np.array_equal(only.joints, got.joints, equal_nan=True)
    # smooth_sequence hands arrays and CPU tensors to the host path
    opt = lambda k: None if c[k] is None else torch.as_tensor(c[k])
    via = smoothing.smooth_sequence(torch.as_tensor(c["xyz"]), opt("cov6"), opt("weights"), opt("valid"), opt("groups"), c["h"], c["d"],
                                    c["taper"], c["floor"])
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(via, got))


@pytest.mark.parametrize("N", [1, 2, 3, 40, 300])
def test_sequence_accel_host_against_the_reference(N):
    xyz, gt, groups = SC.accel_case(N)
    ref, cnt = REF.accel_ref(xyz, gt, groups, 3)
    got = smoothing.sequence_accel(xyz, gt, groups, n_groups=3)
    table = got["table"]
    assert table.shape == (4, 2, 18) and np.array_equal(np.isnan(table), cnt == 0)
    # a mean of at most N x J positive terms summed in another order: that many roundings of the running sum on either side
    assert np.allclose(table, ref, rtol=2 * (N * 17 + 1) * np.finfo(np.float64).eps, atol=0, equal_nan=True)
    assert np.array_equal(got["accel"], table[0, 0, 0], equal_nan=True) and np.array_equal(got["accel_error_joints"], table[0, 1, 1:], equal_nan=True)
    assert got["accel_groups"].shape == (3,) and np.array_equal(got["accel_error_groups"], table[1:, 1, 0], equal_nan=True)
    if N >= 40:
        assert cnt[0, 0, 0] > cnt[0, 1, 0] > 0 and cnt[2].sum() == 0 and cnt[1, 0, 0] + cnt[3, 0, 0] < cnt[0, 0, 0]
        assert np.isnan(table[:, :, 1 + 5]).all()
    plain = smoothing.sequence_accel(torch.as_tensor(xyz))
    assert plain["table"].shape == (1, 2, 18) and np.isnan(plain["table"][0, 1]).all() and plain["accel_groups"].shape == (0,)
    ref0, cnt0 = REF.accel_ref(xyz)
    assert np.array_equal(np.isnan(plain["table"]), cnt0 == 0)
    assert np.allclose(plain["table"], ref0, rtol=2 * (N * 17 + 1) * np.finfo(np.float64).eps, atol=0, equal_nan=True)


def test_python_argument_checks():
    xyz = np.zeros((6, 17, 3), dtype=np.float32)
    for kw, text in ((dict(half_window=0), "half_window"), (dict(half_window=33), "half_window"), (dict(degree=3), "degree"),
                     (dict(degree=-1), "degree"), (dict(taper="gauss"), "taper"), (dict(cov_floor=-1.0), "cov_floor"),
                     (dict(cov_floor=float("nan")), "cov_floor"), (dict(want=("velocity",)), "want"), (dict(want=("joints", "x")), "want"),
                     (dict(cov6=np.zeros((6, 17, 3))), "cov6"), (dict(weights=np.zeros((6, 16))), "weights"),
                     (dict(valid=np.ones((5, 17), bool)), "valid"), (dict(groups=np.zeros(7, int)), "groups")):
        with pytest.raises(ValueError, match=text):
            smoothing.smooth_sequence(xyz, **kw)
    with pytest.raises(ValueError, match="xyz"):
        smoothing.smooth_sequence(np.zeros((6, 17)))
    with pytest.raises(ValueError, match="n_groups"):
        smoothing.sequence_accel(xyz, n_groups=65)
    with pytest.raises(ValueError, match="without groups"):
        smoothing.sequence_accel(xyz, n_groups=2)
    with pytest.raises(ValueError, match="gt"):
        smoothing.sequence_accel(xyz, gt=np.zeros((6, 17, 2)))


X_ = 0x10000         # a device pointer no refused call touches
SMOOTH = "N J xyz cov6 weights valid group_ids half_window degree taper cov_floor out_xyz out_vel out_cov6 n_used stream".split()
LAUNCH = "N J half_window out".split()
ACCEL = "N J xyz gt group_ids n_groups out stream".split()
BASE = dict(N=40, J=17, xyz=X_, cov6=None, weights=None, valid=None, group_ids=None, half_window=8, degree=2, taper=1, cov_floor=0.0,
            out_xyz=0x20000, out_vel=None, out_cov6=None, n_used=None, stream=None, gt=None, n_groups=0, out=X_)
REFUSALS = [
    ("sks_smooth_sequence", SMOOTH, dict(N=0), -1, "smooth_sequence: N = 0 frames, 1 .. 2^30"),
    ("sks_smooth_sequence", SMOOTH, dict(J=0), -1, "smooth_sequence: J = 0 joints, 1 .. 256 (SKS_SMOOTH_MAX_JOINTS)"),
    ("sks_smooth_sequence", SMOOTH, dict(J=257), -1, "smooth_sequence: J = 257 joints, 1 .. 256 (SKS_SMOOTH_MAX_JOINTS)"),
    ("sks_smooth_sequence", SMOOTH, dict(half_window=0), -1, "smooth_sequence: half_window = 0, 1 .. 32 (SKS_SMOOTH_MAX_HALF_WINDOW)"),
    ("sks_smooth_sequence", SMOOTH, dict(half_window=33), -1, "smooth_sequence: half_window = 33, 1 .. 32 (SKS_SMOOTH_MAX_HALF_WINDOW)"),
    ("sks_smooth_sequence", SMOOTH, dict(degree=-1), -1, "smooth_sequence: degree = -1, 0 .. 2"),
    ("sks_smooth_sequence", SMOOTH, dict(degree=3), -1, "smooth_sequence: degree = 3, 0 .. 2"),
    ("sks_smooth_sequence", SMOOTH, dict(taper=2), -1, "smooth_sequence: taper = 2, SKS_SMOOTH_BOX (0) or SKS_SMOOTH_TRICUBE (1)"),
    ("sks_smooth_sequence", SMOOTH, dict(cov_floor=-1.0), -1, "smooth_sequence: cov_floor must be finite and >= 0 mm^2, got -1"),
    ("sks_smooth_sequence", SMOOTH, dict(cov_floor=float("inf")), -1, "smooth_sequence: cov_floor must be finite and >= 0 mm^2, got inf"),
    ("sks_smooth_sequence", SMOOTH, dict(cov_floor=float("nan")), -1, "smooth_sequence: cov_floor must be finite and >= 0 mm^2, got nan"),
    ("sks_smooth_sequence", SMOOTH, dict(xyz=None), -2, "smooth_sequence: missing xyz (N,J,3) floats"),
    ("sks_smooth_sequence", SMOOTH, dict(out_xyz=None), -2, "smooth_sequence: missing out_xyz (N,J,3) floats"),
    ("sks_smooth_sequence", SMOOTH, dict(out_xyz=X_), -2,
     "smooth_sequence: out_xyz overlaps xyz (a tile reads its neighbours' frames: not in place)"),
    ("sks_smooth_sequence", SMOOTH, dict(out_xyz=X_ + 40 * 17 * 12 - 4), -2,
     "smooth_sequence: out_xyz overlaps xyz (a tile reads its neighbours' frames: not in place)"),
    ("sks_smooth_launch", LAUNCH, dict(J=257), -1, "smooth_launch: J = 257 joints, 1 .. 256 (SKS_SMOOTH_MAX_JOINTS)"),
    ("sks_smooth_launch", LAUNCH, dict(half_window=33), -1, "smooth_launch: half_window = 33, 1 .. 32 (SKS_SMOOTH_MAX_HALF_WINDOW)"),
    ("sks_smooth_launch", LAUNCH, dict(out=None), -2, "smooth_launch: missing out (SKS_SMOOTH_LAUNCH_INTS ints)"),
    ("sks_eval_accel", ACCEL, dict(N=0), -1, "eval_accel: N = 0 frames (1 .. 2^30) of J = 17 joints (at least 1)"),
    ("sks_eval_accel", ACCEL, dict(n_groups=65, group_ids=X_), -1, "eval_accel: n_groups = 65, 0 .. 64 (SKS_EVAL_MAX_GROUPS)"),
    ("sks_eval_accel", ACCEL, dict(n_groups=2), -2, "eval_accel: n_groups = 2 without group_ids"),
    ("sks_eval_accel", ACCEL, dict(xyz=None), -2, "eval_accel: missing xyz (N,J,3) floats"),
    ("sks_eval_accel", ACCEL, dict(out=None), -2, "eval_accel: missing out (1 + n_groups, 2, 1 + J) doubles"),
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


def test_the_launch_shape_is_the_librarys_answer():
    """sks_smooth_launch is host only: one (frame, joint) per lane of 256, all joints in a tile while T + 2h frames of them fit
    the 64 KiB stage (64 bytes a staged item plus the frames' group ids), the joints in equal runs beyond."""
    for N, J, h in ((1, 1, 1), (40, 17, 8), (1000, 19, 8), (20, 17, 32), (7, 256, 32), (16384, 15, 1)):
        la = _lib.smooth_launch(N, J, h)
        T = la["tile"]
        assert la["threads"] == 256 and T >= 1 and la["lds_bytes"] <= 65536
        runs = la["groups"] // -(-N // T)
        assert la["groups"] == runs * -(-N // T) and runs >= 1
        Jc = -(-J // runs)
        assert T == 256 // Jc and la["lds_bytes"] == (T + 2 * h) * (Jc * 64 + 4)
        if (256 // J + 2 * h) * J <= 1000:
            assert runs == 1 and T == 256 // J
    assert _lib.smooth_launch(40, 17, 8) == dict(tile=15, groups=3, threads=256, lds_bytes=31 * (17 * 64 + 4))


def test_the_header_the_binding_and_the_documents_agree():
    raw = open(os.path.join(ROOT, "include", "skelsplat_hip.h")).read()
    assert "csrc/sks_smooth.hip; added to sks_version 14: the number did not move" in re.sub(r"\s*\n \*\s*", " ", raw)
    hdr = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    scalars = {"int": ctypes.c_int, "double": ctypes.c_double}
    doc = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "INTEGRATION.md")).read(), flags=re.S)
    for symbol, names in (("sks_smooth_sequence", SMOOTH), ("sks_smooth_launch", LAUNCH), ("sks_eval_accel", ACCEL)):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % symbol, hdr)
        declared = []
        for param in proto.group(1).split(","):
            ctype, name = re.fullmatch(r"\s*(.*?)(\w+)\s*", param, flags=re.S).groups()
            declared.append((name, ctypes.c_void_p if "*" in ctype else scalars[ctype.strip()]))
        assert [n for n, _ in declared] == names, symbol
        assert _lib.SIGNATURES[symbol] == (ctypes.c_int, [ct for _, ct in declared]), symbol
        flat = lambda s: " ".join(s.split())
        assert flat(proto.group(0)) in flat(doc), f"INTEGRATION.md's ABI listing lacks {symbol} as the header declares it"
    for name in ("MAX_JOINTS", "MAX_HALF_WINDOW", "BOX", "TRICUBE", "LAUNCH_INTS"):
        assert int(re.search(r"#define\s+SKS_SMOOTH_%s\s+(\d+)" % name, hdr).group(1)) == getattr(_lib, "SKS_SMOOTH_" + name)
    assert [int(re.search(r"#define\s+SKS_SMOOTH_%s\s+(\d+)" % n.upper(), hdr).group(1)) for n in _lib.SMOOTH_LAUNCH_FIELDS] == [0, 1, 2, 3]
    from skelsplat_amd import build
    assert build.SOURCES["sks_smooth.hip"] == [] and _lib.load().sks_version() == 14
    # the feature is described with what has not been measured
    for path in ("README.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().split())
        assert "Temporal smoothing" in text and "has not been measured" in text, path
