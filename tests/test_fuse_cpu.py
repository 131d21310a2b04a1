"""The fused initial guess on the host (initial_guess.fuse_predictions with arrays / CPU tensors) against the reference's own
results (tests/golden/reference_fuse.npz), by the counted tolerances of tests/fuse_cases.py; the `valid` mask against the
restatement there; shapes, `out=` and every refusal.  No GPU."""
import numpy as np
import pytest
import torch

from tests import fuse_cases as fc
from skelsplat_amd.initial_guess import fuse_predictions

NORM = {"64": torch.float64, "32": torch.float32}
NP_NORM = {"64": np.float64, "32": np.float32}


def test_fixture_is_the_documented_one():
    """Six cases, half stored as float32; every |u_ic - x_c| >= the generator's 0.5 px on the stored values."""
    import os
    assert tuple(fc.names()) == fc.NAMES
    assert os.path.getsize(fc.GOLDEN) < 100 * 1024
    dtypes = []
    for name in fc.NAMES:
        c = fc.case(name)
        N, V, J = c["p3d"].shape[:3]
        assert name == f"v{V}j{J}n{N}" and c["p2d"].shape == (N, V, J, 2) and c["proj"].shape == (V, 3, 4)
        assert c["p3d"].dtype == c["p2d"].dtype and c["err64"].dtype == np.float64 and c["err32"].dtype == np.float32
        assert np.abs(c["p3d"]).max() <= 1e4
        dtypes.append(c["p3d"].dtype)
        X = np.concatenate([c["p3d"].astype(np.float64), np.ones((N, V, J, 1))], -1)
        h = np.einsum("ckm,nijm->nicjk", c["proj"], X)
        e = np.linalg.norm(h[..., :2] / h[..., 2:3] - c["p2d"].astype(np.float64)[:, None], axis=-1)
        assert e.min() >= 0.5, (name, e.min())
    assert dtypes.count(np.dtype("float32")) == dtypes.count(np.dtype("float64")) == 3


@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("name", fc.NAMES)
def test_restatement_equals_golden(name, variant):
    """With `valid` all true (or None) the restatement the mask tests lean on is the reference's result."""
    c = fc.case(name)
    for valid in (None, np.ones(c["p3d"].shape[:3], dtype=bool)):
        fused, ebar, n_used = fc.restate(c["proj"], c["p3d"], c["p2d"], valid, NP_NORM[variant])
        fc.check_case(name, variant, fused, ebar, tag="restatement")
        assert (n_used == c["p3d"].shape[1]).all()


@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("name", fc.NAMES)
def test_host_path_against_golden(name, variant):
    c = fc.case(name)
    out = torch.empty(c["fused64"].shape, dtype=torch.float64)
    ret, ebar, n_used = fuse_predictions(c["proj"], torch.from_numpy(c["p3d"]), torch.from_numpy(c["p2d"]),
                                         norm_dtype=NORM[variant], out=out, return_errors=True, return_n_used=True)
    assert ret is out and ebar.dtype == torch.float64 and n_used.dtype == torch.int32
    fc.check_case(name, variant, out.numpy(), ebar.numpy(), tag="host")
    assert (n_used == c["p3d"].shape[1]).all()
    # the default result is the float64 one rounded to nearest: what the loops take as `points`
    f32 = fuse_predictions(c["proj"], c["p3d"], c["p2d"], norm_dtype=NORM[variant])
    assert isinstance(f32, np.ndarray) and f32.dtype == np.float32 and np.array_equal(f32, out.numpy().astype(np.float32))


def test_single_view_is_the_candidate():
    c = fc.case("v1j3n1")
    for variant in fc.VARIANTS:
        out = torch.empty((1, 3, 3), dtype=torch.float64)
        fuse_predictions(c["proj"], torch.from_numpy(c["p3d"]), torch.from_numpy(c["p2d"]), norm_dtype=NORM[variant], out=out)
        assert np.array_equal(out.numpy(), c["p3d"][:, 0].astype(np.float64))


@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("name", ("v4j17n3", "v5j19n2", "v2j5n2", "v33j2n1"))
def test_valid_against_restatement(name, variant):
    """A left-out view is out in both roles; no kept view -> NaN; one kept view -> that candidate, exactly."""
    c = fc.case(name)
    N, V, J = c["p3d"].shape[:3]
    valid = fc.masks(N, V, J, seed=3)
    want, want_e, want_n = fc.restate(c["proj"], c["p3d"], c["p2d"], valid, NP_NORM[variant])
    out = torch.empty((N, J, 3), dtype=torch.float64)
    _, ebar, n_used = fuse_predictions(c["proj"], torch.from_numpy(c["p3d"]), torch.from_numpy(c["p2d"]), valid=valid,
                                       norm_dtype=NORM[variant], out=out, return_errors=True, return_n_used=True)
    got = out.numpy()
    assert np.array_equal(n_used.numpy(), want_n) and np.array_equal(want_n, valid.sum(1))
    assert (want_n[:, 0] == 0).all() and np.isnan(got[:, 0]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(ebar.numpy()), ~valid)
    al = fc.allowance(c, variant, result=want)
    ok = want_n > 0
    assert (np.abs(got - want)[ok] <= np.broadcast_to(al["fused"], got.shape)[ok]).all()
    rel = np.abs(ebar.numpy() - want_e)[valid] / want_e[valid]
    assert (rel <= al["err"][valid]).all()
    one = want_n == 1
    assert one[:, 1].all()
    cand = np.einsum("nvj,nvjk->njk", (valid & one[:, None]).astype(np.float64), c["p3d"].astype(np.float64))
    assert np.array_equal(got[one], cand[one])
    # the kept views alone, as a smaller problem, give the same joint
    n, j = 0, J - 1
    k = np.flatnonzero(valid[n, :, j])
    if k.size:
        alone = fc.restate(c["proj"][k], c["p3d"][n:n + 1, k, j:j + 1], c["p2d"][n:n + 1, k, j:j + 1], None, NP_NORM[variant])[0]
        assert np.array_equal(alone[0, 0], want[n, j])


def test_forms_and_out():
    c = fc.case("v4j17n3")
    P, X, x = c["proj"], c["p3d"], c["p2d"]
    ref = fuse_predictions(P, X, x)
    assert isinstance(ref, np.ndarray) and ref.shape == (3, 17, 3) and ref.dtype == np.float32
    # one frame without the N axis; a third detection column (a confidence) is ignored
    one, e1, n1 = fuse_predictions(P, X[1], np.concatenate([x[1], np.ones((4, 17, 1))], -1), return_errors=True, return_n_used=True)
    assert one.shape == (17, 3) and e1.shape == (4, 17) and n1.shape == (17,) and np.array_equal(one, ref[1])
    # tensors in, tensors out; per-frame matrices (N,V,3,4); cameras through projection_matrices
    t = fuse_predictions(torch.from_numpy(P), torch.from_numpy(X), torch.from_numpy(x))
    assert torch.is_tensor(t) and np.array_equal(t.numpy(), ref)
    assert np.array_equal(fuse_predictions(np.broadcast_to(P, (3, 4, 3, 4)).copy(), X, x), ref)
    assert np.array_equal(fuse_predictions([p for p in P], X, x), ref)
    from skelsplat_amd import scene, triangulation
    sc = scene.SyntheticScene("h36m", n_views=4, seed=0, device="cpu")
    assert np.array_equal(fuse_predictions(sc.cameras, X, x), fuse_predictions(triangulation.projection_matrices(sc.cameras), X, x),
                          equal_nan=True)
    # out=: float32 or float64, with or without the frame axis for one frame
    o32 = torch.empty((3, 17, 3), dtype=torch.float32)
    assert fuse_predictions(P, X, x, out=o32) is o32 and np.array_equal(o32.numpy(), ref)
    o1 = torch.empty((17, 3), dtype=torch.float64)
    assert fuse_predictions(P, X[1], x[1], out=o1) is o1 and np.array_equal(o1.numpy().astype(np.float32), ref[1])
    # numpy dtypes name the variant too
    assert np.array_equal(fuse_predictions(P, X, x, norm_dtype=np.float32), fuse_predictions(P, X, x, norm_dtype=torch.float32))


def test_refusals():
    c = fc.case("v4j17n3")
    P, X, x = c["proj"], c["p3d"], c["p2d"]
    bad = [
        dict(poses_3d=X[..., :2]),                                   # not (.., 3)
        dict(poses_3d=X[0, 0]),                                      # too few axes
        dict(poses_2d=x[:, :3]),                                     # another V than the predictions
        dict(poses_2d=x[..., :1]),                                   # fewer than two columns
        dict(poses_2d=x[:2]),                                        # another N
        dict(proj_or_cameras=P[:3]),                                 # another V
        dict(proj_or_cameras=np.broadcast_to(P, (2, 4, 3, 4)).copy()),      # another N
        dict(valid=np.ones((3, 4, 16), dtype=bool)),
        dict(norm_dtype=torch.float16),
        dict(norm_dtype="float32"),
        dict(out=torch.empty((3, 17, 4), dtype=torch.float32)),
        dict(out=torch.empty((3, 17, 3), dtype=torch.float16)),
        dict(out=np.empty((3, 17, 3), dtype=np.float32)),
        dict(out=torch.empty((3, 3, 17), dtype=torch.float32).permute(0, 2, 1)),      # not contiguous
        dict(poses_3d=np.zeros((1, 65, 2, 3)), poses_2d=np.zeros((1, 65, 2, 2)), proj_or_cameras=np.zeros((65, 3, 4))),
        dict(poses_3d=X.astype(np.int64)),
    ]
    for kw in bad:
        args = dict(proj_or_cameras=P, poses_3d=X, poses_2d=x)
        args.update(kw)
        with pytest.raises(ValueError):
            fuse_predictions(**args)


def test_entry_checks_its_arguments_on_the_host():
    """sks_fuse_predictions refuses bad arguments before anything is enqueued (no GPU needed), with sks_last_error's text."""
    from skelsplat_amd import _lib
    lib = _lib.load()
    p = 4096       # never dereferenced: every call below returns before the launch
    good = [1, 4, 17, p, 0, p, None, p, None, None, 0, p, None, None, None, None]
    for slot, value in ((0, 0), (2, 0), (1, 0), (1, 65), (4, 12), (3, None), (5, None), (6, p), (7, None), (8, p), (11, None)):
        args = list(good)
        args[slot] = value
        assert lib.sks_fuse_predictions(*args) < 0, (slot, value)
        assert b"fuse_predictions" in lib.sks_last_error()
    args = list(good)
    args[0], args[2] = 1 << 20, 1 << 12
    assert lib.sks_fuse_predictions(*args) < 0 and b"too many" in lib.sks_last_error()


def test_loops_take_the_keyword():
    """`poses_3d=None` is the LAST keyword of every layer that takes `points=None`: no existing position moved."""
    import inspect
    from skelsplat_amd import loop
    for fn, before in ((loop.MultiViewLoop.new_scene, "dropout"), (loop.FrameBatchLoop.new_scenes, "rig_ids"),
                       (loop.FrameBatchLoop.optimize_sequence, "rig_ids"), (loop.FramePipeline.optimize_sequence, "rig_ids")):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == [before, "poses_3d"] and inspect.signature(fn).parameters["poses_3d"].default is None
    with pytest.raises(ValueError):
        loop._sequence_predictions(np.zeros((2, 17, 3)), np.zeros((2, 4, 17, 3)), 2)        # with explicit points
    with pytest.raises(ValueError):
        loop._sequence_predictions(None, np.zeros((3, 4, 17, 3)), 2)                        # another N
    assert loop._sequence_predictions(None, None, 2) is None
