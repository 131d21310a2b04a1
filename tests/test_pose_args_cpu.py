"""_pose_args, the argument handling the four pose entry points share (triangulate_sequence, fuse_predictions, reproject,
refine_triangulation): the forms it accepts give the same tensors and pointers, and one table of bad inputs is refused by every
entry point that takes the argument, each for its own reason."""
import types

import numpy as np
import pytest
import torch

from skelsplat_amd import _pose_args, initial_guess, reprojection, triangulation

N, V, J = 2, 4, 5


def test_the_four_projection_forms_give_the_identical_float64_tensor():
    rng = np.random.default_rng(0)
    cams = [types.SimpleNamespace(K=rng.normal(size=(3, 3)), R=rng.normal(size=(3, 3)), T=rng.normal(size=3)) for _ in range(V)]
    P = triangulation.projection_matrices(cams)
    want = torch.as_tensor(P)
    assert want.dtype == torch.float64 and tuple(want.shape) == (V, 3, 4)
    for form in (want, P, [p for p in P], cams, tuple(cams)):
        got = _pose_args.projections(form, torch.device("cpu"))
        assert got.dtype == torch.float64 and torch.equal(got, want), type(form)
    rigs = np.stack([P, 2 * P])                                              # one rig per frame
    assert torch.equal(_pose_args.projections(rigs, torch.device("cpu")), torch.as_tensor(rigs))
    assert _pose_args.rig_stride(torch.as_tensor(rigs), V) == V * 12 and _pose_args.rig_stride(want, V) == 0
    assert _pose_args.projections(want.to(torch.float32), torch.device("cpu")).dtype == torch.float64


def test_pointer_pairs_and_the_two_real_forms():
    f32, f64 = torch.zeros(3, dtype=torch.float32), torch.zeros(3, dtype=torch.float64)
    assert _pose_args.pointers(f32) == (f32.data_ptr(), None)
    assert _pose_args.pointers(f64) == (None, f64.data_ptr())
    assert _pose_args.pointers(None) == (None, None)
    assert _pose_args.as_real(f64) is f64 and _pose_args.as_real(f32) is f32            # nothing is copied that is ready
    half = _pose_args.as_real(torch.ones((2, 3), dtype=torch.float16).t())
    assert half.dtype == torch.float32 and half.is_contiguous()
    mask = torch.ones(4, dtype=torch.bool)
    assert _pose_args.byte_pointer(mask) == mask.data_ptr() and _pose_args.byte_pointer(None) is None
    assert reprojection._as_real is _pose_args.as_real


def test_arrays_in_arrays_out_and_the_one_frame_form():
    t, was_array = _pose_args.as_tensor(np.zeros((2, 3)))
    assert torch.is_tensor(t) and was_array
    same = torch.zeros(2)
    assert _pose_args.as_tensor(same)[0] is same and _pose_args.as_tensor(same)[1] is False
    res, extra = torch.arange(6.0).reshape(1, 2, 3), torch.arange(2).reshape(1, 2)
    got = _pose_args.results(res, None, True, True, [extra])
    assert isinstance(got[0], np.ndarray) and got[0].shape == (2, 3) and got[1].shape == (2,)
    assert _pose_args.results(res, None, False, False) is res
    out = torch.empty((2, 3))
    assert _pose_args.results(res, out, True, True) is out                               # a given `out` goes back as it is
    view = _pose_args.check_out(out, (1, 2, 3), (torch.float32,), torch.device("cpu"), single=True)
    assert tuple(view.shape) == (1, 2, 3) and view.data_ptr() == out.data_ptr()
    valid = _pose_args.check_valid(np.ones((V, J), bool), True, torch.device("cpu"), (1, V, J))
    assert valid.dtype == torch.bool and tuple(valid.shape) == (1, V, J)
    assert _pose_args.check_valid(None, True, torch.device("cpu"), (1, V, J)) is None


def _inputs(views=V):
    rng = np.random.default_rng(1)
    t = lambda *s: torch.as_tensor(rng.normal(size=s).astype(np.float32))
    return dict(P=torch.as_tensor(rng.normal(size=(views, 3, 4))), x=t(N, views, J, 2), X=t(N, J, 3), X3=t(N, views, J, 3), valid=None,
                out=None)


ENTRIES = {     # name -> (the call on _inputs' names, does it take `out`?)
    "triangulate_sequence": (lambda d: triangulation.triangulate_sequence(d["P"], d["x"], valid=d["valid"], out=d["out"]), True),
    "fuse_predictions": (lambda d: initial_guess.fuse_predictions(d["P"], d["X3"], d["x"], valid=d["valid"], out=d["out"]), True),
    "refine_triangulation": (lambda d: reprojection.refine_triangulation(d["P"], d["x"], d["X"], valid=d["valid"], out=d["out"]), True),
    "reproject": (lambda d: reprojection.reproject(d["P"], d["X"], d["x"], valid=d["valid"]), False),
}
BAD = [         # (what, the inputs, the refusal, is it about `out`?)
    ("65 views", _inputs(65), "65 views", False),
    ("a (V,4,3) projection", dict(_inputs(), P=torch.zeros((V, 4, 3), dtype=torch.float64)), "projection matrices must be", False),
    ("a valid of the wrong shape", dict(_inputs(), valid=torch.ones((N, V, J + 1), dtype=torch.bool)), "valid must be", False),
    ("an out that is not contiguous", dict(_inputs(), out=torch.zeros((N, 3, J)).permute(0, 2, 1)), "`out` must be a contiguous", True),
    ("an out of the wrong dtype", dict(_inputs(), out=torch.zeros((N, J, 3), dtype=torch.float16)), "`out` must be a contiguous", True),
]


@pytest.mark.parametrize("name", list(ENTRIES))
def test_one_table_of_bad_inputs_is_refused_by_every_entry_point(name):
    call, takes_out = ENTRIES[name]
    good = dict(_inputs(), valid=torch.ones((N, V, J), dtype=torch.bool), out=torch.zeros((N, J, 3)))
    got = call(good)                                                        # the table's base is accepted ...
    if takes_out:
        assert got is good["out"]
    for _, inputs, text, about_out in BAD:                               # ... and every change to it refused for its reason
        if about_out and not takes_out:
            continue
        with pytest.raises(ValueError, match=text):
            call(inputs)
