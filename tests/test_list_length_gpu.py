"""The binned path against the CPU oracle at every regime of a tile list's length (tests/list_length_cases.py: the six ways a list
is ordered or walked, the scenes that reach each, and the claims -- asserted on the oracle, through the host-only sks_list_regime,
before anything runs here).

Per case: the forward bit for bit (colour, inverse depth, radii, final_T, n_contrib, the ranges and the exported point_list: the
export reads the lists as the compositor left them, so it pins every sorter) into outputs that held NaN, and all seven gradients at
the standing tolerance (util.assert_close: rtol 1e-3 + 1e-5 of the largest entry).  Then, on the long scenes: the clamped forward and
the backward that re-composites (against fp64 autograd), run-to-run bits, the one call against the two calls in every grouping (the
global-memory sort borrows rows the backward writes later), and an arena that cuts the long list in half."""
import numpy as np
import pytest
import torch

from tests import geometry_cases as G, list_length_cases as LC, util
from skelsplat_amd import _lib, rasterizer as R

pytestmark = pytest.mark.gpu


def _release():
    R.reset_scratch()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=LC.names())
def run(request, device):
    r = LC.Run(LC.get(request.param), device)
    yield r
    del r
    _release()


def test_forward_bits(run):
    G.check_forward_bits(run)


def test_gradients(run):
    G.check_gradients(run, want_dfeatures=run.c.name != LC.NOFEAT())


# ------------------------------------------------------------------------------------------------------------
# the long scenes through the other switches
# ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def longest(device):
    r = LC.Run(LC.get(LC.LONGEST()), device)
    yield r
    del r
    _release()


@pytest.mark.parametrize("which", list(LC.clamp_cases()))
def test_clamped_forward_and_the_backward_that_recomposites(device, which):
    """clamp01: the forward is clip(oracle) exactly; the backward composites again to find the clamped pixels, and is held to what
    the project's clamped tests are (fp64 autograd of the PyTorch restatement, test_render_functions_drop_in_like_train_py's rtol
    2e-3 + 2e-4 of the largest entry)."""
    c = LC.clamp_cases()[which]()
    run = LC.Run(c, device)
    ws = run.nan_workspace()
    color, inv, radii, st = run.forward(ws, clamp01=True)
    o = run.fwd[0]
    assert np.array_equal(radii[0].cpu().numpy(), o["radii"])
    got = color[0].cpu().numpy()
    assert np.array_equal(got, np.clip(o["color"], 0.0, 1.0)), f"{c.name}: {int((got != np.clip(o['color'], 0.0, 1.0)).sum())} pixels differ from clip(oracle)"
    assert np.array_equal(inv[0].cpu().numpy(), o["invdepth"])
    g = run.backward(st, ws, want_dfeatures=True)
    torch.cuda.synchronize()
    want, col = LC.clamped_autograd(c)
    outside = (col > 1) | (col < 0)
    assert 0.02 < outside.mean() < 0.98, "the clamp does not bite"
    failures = []
    for key, w in want.items():
        a = g[key][0].cpu().numpy()
        if key == "means2D":
            a, w = a[:, :2], w[:, :2]
        try:
            util.assert_close(f"{c.name} {key}", a, w.reshape(a.shape), rtol=2e-3, atol_scale=2e-4)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    del run
    _release()


def test_two_backwards_give_the_same_bits(longest):
    """No float atomics on the binned path but the feature gradient's (documented): every other gradient repeats bit for bit."""
    run = longest
    _, _, _, st = run.forward()
    a = {k: None if x is None else x.clone() for k, x in run.backward(st, want_dfeatures=True).items()}
    b = run.backward(st, want_dfeatures=True)
    torch.cuda.synchronize()
    for k in a:
        if k != "features" and a[k] is not None:
            assert torch.equal(a[k], b[k]), f"{run.c.name}: gradient {k} differs between two backward calls"
    util.assert_close("features, run to run", b["features"].cpu().numpy(), a["features"].cpu().numpy(), rtol=1e-4)


@pytest.mark.parametrize("join", [True, False], ids=["join", "nojoin"])
@pytest.mark.parametrize("groups", [0, 3], ids=["default-groups", "3-groups"])
def test_one_call_equals_the_two_calls(device, groups, join):
    """sks_forward_backward on three views of the lds + 52 scene: the sort of a list beyond the LDS network's capacity keeps its keys
    in the rows the backward fills later -- with view groups, the backward of one group runs beside the forward of the next."""
    c = LC.one_call_case()
    run = LC.Run(c, device)
    tf = _lib.SKS_BIN_GROUPS(groups) if groups else 0
    color, inv, radii, st = run.forward(tune_flags=tf)
    g = run.backward(st, tune_flags=tf)
    torch.cuda.synchronize()
    for v in range(c.V):
        assert np.array_equal(color[v].cpu().numpy(), run.fwd[v]["color"]), f"view {v}: the two calls' colour differs from the oracle"
    ref, gref = (color.clone(), inv.clone(), radii.clone()), {k: None if x is None else x.clone() for k, x in g.items()}
    ws = run.nan_workspace(prefill=0)
    for rep in range(3):      # (the first round IS the two calls and records them; the later ones replay them as one call)
        for t_ in G.held_nan(ws, c, device):
            t_.fill_(G.NAN)
        out = R.forward_backward_views(run.views, *run.args, run.dLc, run.dLi, bg=run.bg, force_binned=c.force_binned, workspace=ws,
                                       tune_flags=tf, join=join)
        if not join:
            ws.join(device.index)
        assert out[0].data_ptr() == G.held_nan(ws, c, device)[0].data_ptr()
        for name, a, b in zip(("colour", "inverse depth", "radii"), out[:3], ref):
            assert torch.equal(a, b), f"{c.name} one call, round {rep}: {name} differs"
        for k, x in gref.items():
            if x is not None:
                assert torch.equal(out[4][k], x), f"{c.name} one call, round {rep}: gradient {k} differs"
    assert "bwd" in ws._plans and "fwd" in ws._plans, "the later rounds did not replay the records"
    del run, ws
    _release()


def test_an_arena_that_cuts_the_long_list_in_half(device):
    """bin_capacity ends inside the middle tile's list: the first pass sorts and composites a clipped list, the capacity check
    (check_capacity=True) grows the arena and redoes the forward -- which equals the oracle bit for bit, lists included."""
    c = LC.get(f"dense17-{LC.BIG()}")
    run = LC.Run(c, device)
    a, b = (int(x) for x in run.fwd[0]["ranges"].reshape(c.gy, c.gx, 2)[1, 1])
    cap = a + (b - a) // 2
    assert a < cap < b <= run.fwd[0]["R"]
    R.reset_scratch()
    G.check_forward_bits(run, bin_capacity=cap, check_capacity=True)
    del run
    _release()
