"""triangulation.triangulate_sequence on the host (no GPU): the batched-SVD path that GPU-less users run and that the
device kernel is compared with in tests/test_triangulate_gpu.py, plus the kernel's arithmetic restated in numpy."""
import ctypes

import numpy as np
import pytest
import torch

from skelsplat_amd import triangulation
from tests import tri_cases as TC


def test_sequence_equals_triangulate_poses_per_frame_and_the_reference_golden():
    sc, P, gt, p2d = TC.sequence("h36m", 4, frames=6, seed=2)
    got = triangulation.triangulate_sequence(P, p2d, homogeneous=True)
    assert isinstance(got, np.ndarray) and got.shape == (6, sc.n_points, 4) and got.dtype == np.float64
    for f in range(6):
        ref = triangulation.triangulate_poses(P, p2d[f])
        assert np.allclose(got[f], ref, **TC.SVD_TOL), np.abs(got[f] - ref).max()
    assert np.all(got[..., 3] == 1.0)
    assert 1.0 < np.linalg.norm(got[..., :3] - gt, axis=-1).mean() < 40.0
    xyz = triangulation.triangulate_sequence(sc.cameras, p2d)               # a camera list, float32 joints
    assert xyz.dtype == np.float32 and np.array_equal(xyz, got[..., :3].astype(np.float32))
    for tag in TC.GOLDEN_TAGS:
        Pg, x2d, X = TC.golden(tag)
        got = triangulation.triangulate_sequence(Pg, x2d[None], homogeneous=True)[0]
        assert got.shape == X.shape and np.all(got[:, 3] == 1.0)
        assert np.allclose(got, X, **TC.GOLDEN_TOL), (tag, np.abs(got - X).max())


def test_valid_mask_equals_the_kept_views_alone():
    sc, P, gt, p2d = TC.sequence("h36m", 4, frames=3, seed=5, dtype=np.float64)
    J = sc.n_points
    rng = np.random.default_rng(7)
    valid = np.ones((3, 4, J), dtype=bool)
    for f in range(3):
        for j in range(J):
            valid[f, rng.choice(4, size=rng.integers(0, 3), replace=False), j] = False      # 2 .. 4 views kept
    valid[1, 1:, 3] = False         # one view kept
    valid[2, :, 5] = False          # none
    x = p2d.copy()
    x[~valid] = np.nan              # a left-out detection is never read into the result
    got, n_used = triangulation.triangulate_sequence(P, x, valid=valid, homogeneous=True, return_n_used=True)
    assert n_used.dtype == np.int32 and np.array_equal(n_used, valid.sum(1))
    assert n_used[1, 3] == 1 and n_used[2, 5] == 0
    for f in range(3):
        ref = TC.kept_views_reference(P, p2d[f], valid[f])
        assert np.array_equal(np.isnan(got[f]), np.isnan(ref))
        assert np.allclose(got[f], ref, equal_nan=True, **TC.SVD_TOL), np.nanmax(np.abs(got[f] - ref))
    assert np.isnan(got[1, 3]).all() and np.isnan(got[2, 5]).all() and np.isnan(got).sum() == 8
    xyz = triangulation.triangulate_sequence(P, x, valid=torch.as_tensor(valid))
    assert np.array_equal(xyz, got[..., :3].astype(np.float32), equal_nan=True)


def test_shapes_dtypes_rigs_and_refusals():
    sc, P, gt, p2d = TC.sequence("h36m", 4, frames=4, seed=9)
    J = sc.n_points
    ref = triangulation.triangulate_sequence(P, p2d, homogeneous=True)
    # tensors in, tensors out; extra components (confidences) are ignored
    t = triangulation.triangulate_sequence(torch.as_tensor(P), torch.as_tensor(np.concatenate([p2d, p2d[..., :1]], -1)))
    assert torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == (4, J, 3)
    assert np.array_equal(t.numpy(), ref[..., :3].astype(np.float32))
    # one frame without a frame axis
    one = triangulation.triangulate_sequence(P, p2d[2], homogeneous=True)
    assert one.shape == (J, 4) and np.array_equal(one, ref[2])
    one, n_used = triangulation.triangulate_sequence(P, p2d[2], valid=np.ones((4, J), bool), return_n_used=True)
    assert one.shape == (J, 3) and n_used.shape == (J,) and (n_used == 4).all()
    # one rig per frame: frame f seen by frame f's own cameras
    rigs = np.stack([TC.sequence("h36m", 4, frames=1, seed=20 + f)[1] for f in range(4)])
    per = triangulation.triangulate_sequence(rigs, p2d, homogeneous=True)
    for f in range(4):
        assert np.allclose(per[f], triangulation.triangulate_poses(rigs[f], p2d[f]), **TC.SVD_TOL)
    # `out`
    out = torch.empty((4, J, 4), dtype=torch.float64)
    assert triangulation.triangulate_sequence(P, torch.as_tensor(p2d), out=out, homogeneous=True) is out
    assert np.array_equal(out.numpy(), ref)
    with pytest.raises(ValueError, match="out"):
        triangulation.triangulate_sequence(P, torch.as_tensor(p2d), out=out)              # float32 (N,J,3) wanted
    # refusals
    sc65, P65, _, p65 = TC.sequence("panoptic", 65, frames=1, seed=1)
    with pytest.raises(ValueError, match="65 views"):
        triangulation.triangulate_sequence(P65, p65)
    with pytest.raises(ValueError, match="projection matrices"):
        triangulation.triangulate_sequence(rigs[:3], p2d)                                 # 3 rigs, 4 frames
    with pytest.raises(ValueError, match="valid"):
        triangulation.triangulate_sequence(P, p2d, valid=np.ones((3, 4, J), bool))
    with pytest.raises(ValueError, match="poses_2d"):
        triangulation.triangulate_sequence(P, p2d[..., :1])


def test_kernel_arithmetic_restated_in_numpy_meets_the_golden_bar():
    """tests/tri_cases.jacobi_dlt is sks_triangulate's arithmetic, operation for operation.  It must sit inside the
    project's bar against the reference's golden X on all three cases, two views included, and converge well inside the
    kernel's cap of 16 sweeps (the last sweep only confirms that nothing rotates any more)."""
    for tag in TC.GOLDEN_TAGS:
        P, x2d, X = TC.golden(tag)
        got, sweeps = TC.jacobi_dlt(P, x2d)
        assert np.allclose(got, X, **TC.GOLDEN_TOL), (tag, np.abs(got - X).max())
        assert sweeps <= 8, (tag, sweeps)
    for ds, V in (("h36m", 2), ("h36m", 4), ("panoptic", 31), ("panoptic", 64)):
        sc, P, gt, p2d = TC.sequence(ds, V, frames=2, seed=3, dtype=np.float64)
        valid = np.ones((V, sc.n_points), bool)
        valid[0, 1] = False
        for f in range(2):
            got, sweeps = TC.jacobi_dlt(P, p2d[f], valid if V > 2 else None)
            ref = TC.kept_views_reference(P, p2d[f], valid) if V > 2 else triangulation.triangulate_poses(P, p2d[f])
            assert np.allclose(got, ref, **TC.GOLDEN_TOL), (ds, V, np.abs(got - ref).max())
            assert sweeps <= 8, (ds, V, sweeps)


def test_loops_keep_the_projection_matrices_and_refuse_what_cannot_be_triangulated():
    """device_projection_matrices is what the loops build at construction; the CPU statement of it."""
    sc, P, gt, p2d = TC.sequence("h36m", 4, frames=1, seed=4)
    t = triangulation.device_projection_matrices(sc.cameras, "cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (4, 3, 4) and t.is_contiguous() and np.array_equal(t.numpy(), P)

    class Bare:
        pass
    assert triangulation.device_projection_matrices([Bare()], "cpu") is None


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """sks_triangulate checks its arguments on the host: these calls return before anything is enqueued (no GPU needed)."""
    from skelsplat_amd import _lib
    lib = _lib.load()
    assert lib.sks_version() >= 13
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    for args, word in (((1, 65, 1, p, 0, p, None, None, p, None, None, None), "65 views"),
                       ((0, 4, 17, p, 0, p, None, None, p, None, None, None), "at least 1"),
                       ((2, 4, 17, p, 7, p, None, None, p, None, None, None), "rig_stride"),
                       ((2, 4, 17, p, 0, p, p, None, p, None, None, None), "not both"),
                       ((2, 4, 17, p, 0, None, None, None, p, None, None, None), "not both"),
                       ((2, 4, 17, p, 0, p, None, None, None, None, None, None), "xyz / xyzw"),
                       ((2, 4, 17, None, 0, p, None, None, p, None, None, None), "projection")):
        assert lib.sks_triangulate(*args) < 0
        assert word in lib.sks_last_error().decode(), (word, lib.sks_last_error())
