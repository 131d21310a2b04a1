"""The uncertainty report (skelsplat_amd/uncertainty.py, csrc/sks_uncertainty.hip) without a device: the float64 references the
GPU tests compare against reproduce what the reference's own code computed (tests/golden/reference_uncertainty.npz), their
whitening form of the Mahalanobis distance and their analytic eigenvalues agree with numpy's inverse and eigen-solver, the cases
keep their distance from the k-sigma thresholds, the argument checks of the Python surface and of the C entry points refuse, and
save_ply_arrays writes save_ply's bytes."""
import ctypes
import os
import re

import numpy as np
import pytest

from skelsplat_amd import _lib, io
from tests import uncertainty_cases as uc
from tests import uncertainty_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture_refs(i):
    fx = uc.fixture()
    mod = fx["modifiers"][i]
    scales = np.exp(fx["scaling_raw"].astype(np.float64))
    return fx, mod, scales


@pytest.mark.parametrize("i", [0, 1], ids=["modifier-1", "modifier-1.3"])
def test_references_reproduce_the_reference(i):
    """The covariance: the reference computes it in float32 (build_scaling_rotation, `R @ L`, `L @ L^T`), so the float64 reference
    can only be held to it within the float32 arithmetic's own error -- the allowance counted for the kernel's float sequence of
    the same formula (uncertainty_ref) plus torch.exp's float32 result (1 ulp of the scale, 2u of its square) -- and is; against
    an independent float64 evaluation (numpy's eigen-decomposition put back together) it holds to float64 rounding.  The
    fractions: exactly."""
    fx, mod, scales = _fixture_refs(i)
    cov = ur.covariance_ref(scales, fx["rotation_raw"], mod)
    want = fx[f"cov_m{i}"].astype(np.float64)
    allow = ur.matrices_of(ur.cov6_allowance(scales, fx["rotation_raw"], mod)) + 4.0 * ur.U32 * np.abs(cov) \
        + 4.0 * ur.U32 * ur.trace_ref(scales, mod)[..., None, None]
    assert (np.abs(cov - want) <= allow).all(), float((np.abs(cov - want) / allow).max())
    assert float((np.abs(cov - want) / np.abs(cov).max(axis=(-1, -2), keepdims=True)).max()) < 2e-6
    assert np.array_equal(ur.matrices_of(ur.cov6_of(cov)), cov)          # symmetric to the bit, and the two packings invert
    lam, vec = np.linalg.eigh(cov)
    back = np.einsum("...ik,...k,...jk->...ij", vec, lam, vec)
    assert float((np.abs(back - cov) / ur.trace_ref(scales, mod)[..., None, None]).max()) < 64 * 2.0 ** -52
    d2 = ur.d2_ref(fx["xyz"], fx["gt"], scales, fx["rotation_raw"], mod)
    counts = ur.calibration_counts_ref(d2, fx["ks"])
    overall, per_joint = ur.fractions_of(counts)
    assert np.array_equal(overall, fx[f"overall_m{i}"]) and np.array_equal(per_joint, fx[f"per_joint_m{i}"])
    assert 0.05 < overall[0] < overall[1] < overall[2] <= 1.0             # the levels separate the sample


@pytest.mark.parametrize("i", [0, 1], ids=["modifier-1", "modifier-1.3"])
def test_no_fixture_joint_sits_near_a_threshold(i):
    """The fractions of the fixture are compared EXACTLY with what the kernels count from their float d2, so no joint's reference
    d2 may be within GAP_FACTOR x its rounding allowance of a k^2: asserted on the reference alone, nothing left out."""
    fx, mod, scales = _fixture_refs(i)
    d2 = ur.d2_ref(fx["xyz"], fx["gt"], scales, fx["rotation_raw"], mod)
    # the GPU path's scales are torch.exp's float32 results: their rounding (u each, 2u of every B_k^2) joins the allowance
    allow = ur.d2_allowance(fx["xyz"], fx["gt"], scales, mod) + 2.0 * ur.U32 * ur.d2_basis(fx["xyz"], fx["gt"], scales, mod)
    assert d2.shape == (37, 17)
    gap = np.min([np.abs(d2 - float(k) ** 2) for k in fx["ks"]], axis=0)
    assert (gap > uc.GAP_FACTOR * allow).all(), float((gap / allow).min())
    print(f"\n[fixture gap, modifier {mod}] smallest |d2 - k^2| = {float((gap / (ur.U32 * ur.d2_basis(fx['xyz'], fx['gt'], scales, mod))).min()):.0f} units of 2^-24 sum_k (|delta|_1 / sigma_k)^2")


def test_whitening_is_the_inverse_form():
    """d2 by whitening against delta^T inv(cov) delta on the fixture's 629 joints (condition numbers up to 16): both float64, the
    inverse form is the worse conditioned one."""
    fx, mod, scales = _fixture_refs(0)
    d2 = ur.d2_ref(fx["xyz"], fx["gt"], scales, fx["rotation_raw"], mod)
    inv = ur.d2_inverse_ref(fx["xyz"], fx["gt"], ur.covariance_ref(scales, fx["rotation_raw"], mod))
    rel = float((np.abs(d2 - inv) / d2).max())
    print(f"\n[whitening vs inverse] {d2.size} joints, largest relative difference {rel:.1e}")
    assert d2.size == 629 and rel < 1e-12
    # and it is what the generator planted: Mahalanobis distances in [0.05, 4] up to the float32 rounding of gt
    assert 0.04 ** 2 < d2.min() and d2.max() < 4.05 ** 2


def test_analytic_eigenvalues_against_eigvalsh():
    """On the well-conditioned cases the sorted squared scales are numpy's eigenvalues within 64 eps l1; on a needle the solver
    is the one that loses the small ones."""
    fx, mod, scales = _fixture_refs(1)
    lam = ur.eigenvalues_ref(scales, mod)
    got = np.linalg.eigvalsh(ur.covariance_ref(scales, fx["rotation_raw"], mod))[..., ::-1]
    assert (np.abs(got - lam) <= 64 * 2.0 ** -52 * lam[..., :1]).all()
    assert (lam[..., 0] >= lam[..., 1]).all() and (lam[..., 1] >= lam[..., 2]).all()
    np.testing.assert_allclose(lam.sum(-1), ur.trace_ref(scales, mod), rtol=1e-15)
    np.testing.assert_allclose(lam.prod(-1), ur.det_ref(scales, mod), rtol=1e-15)
    c = uc.joint_case(3, 17)
    # (1e4, 1e-2, 1e-2) in float32, the kernel's precision: the nine entries are rounded at 6e-8 of l1, 1e-12 of it is gone
    needle = np.linalg.eigvalsh(ur.covariance_ref(c["scales"][0, 2], c["rot"][0, 2]).astype(np.float32)).astype(np.float64)
    exact = ur.eigenvalues_ref(c["scales"][0, 2])
    assert exact[0] / exact[2] > 0.9e12 and abs(needle[0] - exact[2]) > 0.5 * exact[2]
    assert np.array_equal(ur.eigenvalues_f32(c["scales"][0, 2]).astype(np.float64), exact.astype(np.float32).astype(np.float64))


def test_cases_are_what_they_claim():
    assert [n * p for n, p in uc.JOINT_SHAPES[:6]] == [1, 255, 255, 256, 256, 257]
    ratios, lo, hi = [], np.inf, 0.0
    for N, P in uc.JOINT_SHAPES:
        c = uc.joint_case(N, P)
        s = c["scales"].astype(np.float64)
        lo, hi = min(lo, s.min()), max(hi, s.max())
        ratios.append((s.max(-1) / s.min(-1)).max())
        assert s.min() >= 0.999e-3 and s.max() <= 1.001e4 and (s.max(-1) / s.min(-1)).max() <= 1.001e6
        for mod in uc.MODIFIERS:        # the ground truth sits where it was put, up to the float32 rounding of gt and xyz
            d2 = ur.d2_ref(c["xyz"], c["gt"], c["scales"], c["rot"], mod)
            assert np.isfinite(d2).all() and (d2 >= 0).all()
        qn = np.linalg.norm(c["rot"].astype(np.float64), axis=-1)
        assert qn.min() > 0.9e-3 and qn.max() < 1.1e3
    assert lo < 1.001e-3 and hi > 0.999e4 and max(ratios) > 0.999e6
    for N in uc.CAL_N:
        for P in uc.CAL_P:
            d2, valid = uc.calibration_case(N, P)
            assert d2.dtype == np.float32 and d2.shape == (N, P) and valid.shape == (N,)
            counts = ur.calibration_counts_ref(d2, uc.CAL_LEVELS, valid)
            assert counts.shape == (1 + P, 9) and (counts[1:].sum(0) == counts[0]).all()
            assert (counts[:, :8] <= counts[:, 8:]).all()
    d2, valid = uc.calibration_case(1000, 19)
    assert np.isnan(d2).sum() == 2 and np.isinf(d2).sum() == 1 and 0 < valid.sum() < 1000
    t = np.float32(2.5) * np.float32(2.5)
    assert (d2 == t).any() and (d2 == np.nextafter(t, np.float32(np.inf))).any()


def test_python_refusals():
    import torch
    from skelsplat_amd import uncertainty as un
    a3, a4 = torch.zeros((2, 17, 3)), torch.zeros((2, 17, 4))
    with pytest.raises(ValueError, match="ROCm device"):
        un.joint_uncertainty(a3, a3, a4)
    with pytest.raises(ValueError, match="ROCm device"):
        un.calibration(torch.zeros((2, 17)))
    with pytest.raises(ValueError, match="ROCm device"):
        un.view_footprints(a3[0], a3[0], a4[0], cameras=[])
    with pytest.raises(ValueError, match="either cameras= or views="):
        un.view_footprints(a3[0], a3[0], a4[0])
    with pytest.raises(ValueError, match=r"\(\.\.,6\)"):
        un.covariance_matrices(torch.zeros((2, 5)))
    c6 = torch.arange(12.0).reshape(2, 6)
    m = un.covariance_matrices(c6)
    assert tuple(m.shape) == (2, 3, 3) and torch.equal(m, m.transpose(1, 2))
    assert np.array_equal(m.numpy(), ur.matrices_of(c6.numpy()))
    assert un.JointUncertainty._fields == ("cov6", "eigenvalues", "trace", "det", "anisotropy", "d2")


def test_abi_tables_and_c_refusals():
    hdr = open(os.path.join(ROOT, "include", "skelsplat_hip.h")).read()
    assert int(re.search(r"#define\s+SKS_CALIBRATION_MAX_K\s+(\d+)", hdr).group(1)) == _lib.SKS_CALIBRATION_MAX_K == 8
    assert "csrc/sks_uncertainty.hip; added to sks_version 14: the number did not move" in re.sub(r"\s*\n \*\s*", " ", hdr)
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for symbol in ("sks_joint_uncertainty", "sks_view_footprints", "sks_calibration"):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % symbol, plain).group(1)
        kinds = [ctypes.c_void_p if "*" in p else ctypes.c_float if "float" in p else ctypes.c_int for p in proto.split(",")]
        assert _lib.SIGNATURES[symbol] == (ctypes.c_int, kinds), symbol
        assert symbol not in _lib.STEP_PARAMS
    from skelsplat_amd import build
    assert "sks_uncertainty.hip" in build.SOURCES
    lib = _lib.load()
    assert lib.sks_version() == 14
    x = 0x1000      # (never dereferenced: every call below is refused before anything is launched)

    def refused(fn, name, args, text):
        rc = fn(*args)
        assert rc < 0, (name, args)
        msg = lib.sks_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, (name, text, msg)

    one = ctypes.c_float(1.0)
    ok = dict(N=2, P=17, xyz=x, scales=x, rotations=x, scale_modifier=one, gt=x, cov6=x, spectrum=x, d2=x, stream=None)
    for change, text in ((dict(N=0), "at least 1"), (dict(P=0), "at least 1"), (dict(N=1 << 20, P=1 << 10), "too many"),
                         (dict(scales=None), "scales"), (dict(rotations=None), "rotations"), (dict(xyz=None), "xyz"),
                         (dict(d2=None), "d2"), (dict(gt=None), "without gt"), (dict(cov6=None), "cov6"),
                         (dict(spectrum=None), "spectrum")):
        refused(lib.sks_joint_uncertainty, "joint_uncertainty", tuple({**ok, **change}.values()), text)
    tan = ctypes.cast((ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0), ctypes.c_void_p)
    wh = ctypes.cast((ctypes.c_int * 8)(16, 16, 16, 16, 16, 16, 16, 17), ctypes.c_void_p)
    ok = dict(V=4, J=17, W=16, H=16, means3D=x, scales=x, rotations=x, scale_modifier=one, viewmatrix=x, tanfovx=tan, tanfovy=tan,
              view_wh=None, views_dev=None, frames=1, lambdas=x, stream=None)
    for change, text in ((dict(V=0), "bad shape"), (dict(V=65), "bad shape"), (dict(J=0), "bad shape"), (dict(W=0), "bad shape"),
                         (dict(H=0), "bad shape"), (dict(J=1 << 27), "too many"), (dict(frames=0), "frames"),
                         (dict(frames=3), "frames"), (dict(means3D=None), "missing"), (dict(scales=None), "missing"),
                         (dict(rotations=None), "missing"), (dict(viewmatrix=None), "missing"), (dict(lambdas=None), "missing"),
                         (dict(views_dev=x), "both view forms"), (dict(tanfovx=None, tanfovy=None), "no view form"),
                         (dict(tanfovy=None), "no view form"), (dict(tanfovx=None, tanfovy=None, view_wh=wh, views_dev=x), "both"),
                         (dict(view_wh=wh), "within")):
        refused(lib.sks_view_footprints, "view_footprints", tuple({**ok, **change}.values()), text)

    def levels(*v):
        return ctypes.cast((ctypes.c_float * 8)(*v), ctypes.c_void_p)
    ok = dict(N=5, P=17, d2=x, valid=None, K=3, k_sigma=levels(1, 2, 3), counts=x, stream=None)
    for change, text in ((dict(N=0), "at least 1"), (dict(P=0), "at least 1"), (dict(N=1 << 20, P=1 << 12), "too many"),
                         (dict(K=0), "SKS_CALIBRATION_MAX_K"), (dict(K=9), "SKS_CALIBRATION_MAX_K"), (dict(d2=None), "d2"),
                         (dict(k_sigma=None), "k_sigma"), (dict(counts=None), "counts"),
                         (dict(k_sigma=levels(1, 0, 3)), "finite and > 0"), (dict(k_sigma=levels(1, 2, -3)), "finite and > 0"),
                         (dict(k_sigma=levels(float("nan"), 2, 3)), "finite and > 0"),
                         (dict(k_sigma=levels(1, float("inf"), 3)), "finite and > 0")):
        refused(lib.sks_calibration, "calibration", tuple({**ok, **change}.values()), text)


def test_save_ply_arrays_writes_save_plys_bytes(tmp_path):
    """One frame's arrays over a template model = save_ply of a model that holds them; host arrays and tensors alike.  The
    template's own parameters do not reach the file."""
    import torch
    G = np.load(os.path.join(ROOT, "tests", "golden", "reference_next.npz"))
    rng = np.random.default_rng(3)
    gm = type("GM", (), {})()
    for f in ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"):
        setattr(gm, "_" + f, torch.tensor(G["ply_h36m_" + f]))
    P = gm._xyz.shape[0]
    frame = [rng.normal(0, 1.0, (P, k)).astype(np.float32) for k in (3, 3, 4, 1)]
    before = [t.detach().clone() for t in (gm._xyz, gm._scaling, gm._rotation, gm._opacity)]
    a, b, c = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "c.ply")
    io.save_ply_arrays(a, gm, *frame)
    io.save_ply_arrays(b, gm, *[torch.from_numpy(f) for f in frame])
    for t, old in zip((gm._xyz, gm._scaling, gm._rotation, gm._opacity), before):
        assert torch.equal(t.detach(), old)
    with torch.no_grad():
        for t, f in zip((gm._xyz, gm._scaling, gm._rotation, gm._opacity), frame):
            t.copy_(torch.from_numpy(f))
    io.save_ply(c, gm)
    want = open(c, "rb").read()
    assert open(a, "rb").read() == want and open(b, "rb").read() == want
    assert np.array_equal(io.read_ply_xyz(a), frame[0].astype(np.float64))
    with pytest.raises(ValueError, match="one frame"):
        io.save_ply_arrays(a, gm, frame[0][None], *frame[1:])
    with pytest.raises(ValueError, match="template"):
        io.save_ply_arrays(a, gm, *[f[:5] for f in frame])
