"""Both rasterizer paths against the CPU oracle at the limits of the image geometry (tests/geometry_cases.py: what each case holds
and which launch regime it is there for -- asserted here too, through sks_launch_regime, before anything runs).

Per case: the forward bit for bit (colour, inverse depth, radii, final_T, n_contrib; the tile lists on the binned path) into
outputs that held NaN, so an unzeroed pixel and a pixel zeroed over the compositor's store both show; all seven gradients at the
standing tolerance (util.assert_close: rtol 1e-3 + 1e-5 of the largest entry) -- the two tallest images, whose pixel coordinates
near 2**19 leave fp32 ~0.03 px, at the oracle's computed rounding bound instead (util.assert_close_bound, BOUND_KAPPA as it
stands); and the same bits from every launch form: two calls and sks_forward_backward, with and without the early fill,
non-temporal and plain stores, the small path and the binned one (forward), run to run.  The oracle and the upstream gradients of
a case are computed once and shared by its tests (a module-scoped fixture: pytest groups the tests by case)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import geometry_cases as G
from skelsplat_amd import _lib, rasterizer as R

pytestmark = pytest.mark.gpu

NAN = G.NAN


@pytest.fixture(scope="module", params=G.names())
def run(request, device):
    r = G.Run(G.get(request.param), device)
    yield r
    del r
    R.reset_scratch()
    torch.cuda.empty_cache()


def test_forward_bits(run):
    G.check_forward_bits(run)


def test_gradients(run):
    G.check_gradients(run)


def same_image(what, got, ref):
    for name, a, b in zip(("colour", "inverse depth", "radii"), got, ref):
        assert torch.equal(a, b), f"{what}: {name} differs"


def same_grads(what, got, ref):
    for key in ref:
        if ref[key] is not None:
            assert torch.equal(got[key], ref[key]), f"{what}: gradient {key} differs"


def test_launch_forms(run):
    c, dev = run.c, run.dev
    color, inv, radii, st = run.forward()
    g = run.backward(st)
    torch.cuda.synchronize()
    for v in range(c.V):      # (the plain forward takes the early fill where test_forward_bits' debug planes turn it off)
        assert np.array_equal(color[v].cpu().numpy(), run.fwd[v]["color"]) and np.array_equal(inv[v].cpu().numpy(), run.fwd[v]["invdepth"]), \
            f"{c.name} view {v}: the plain forward differs from the oracle"
    ref, gref = (color.clone(), inv.clone(), radii.clone()), {k: None if x is None else x.clone() for k, x in g.items()}
    # run to run, and the fill variants: no early fill, plain stores, both
    small = run.regime["path"] == _lib.PATH_SMALL
    # (the early fill's field is the binned path's view-group count: every plane early on the small path, two view groups on the binned)
    groups = _lib.SKS_EARLY_FILL(7) if small else _lib.SKS_BIN_GROUPS(2)
    for tf in (0, _lib.SKS_NO_EARLY_FILL, _lib.SKS_NO_NT_STORES, _lib.SKS_NO_EARLY_FILL | _lib.SKS_NO_NT_STORES, groups):
        ws = run.nan_workspace(prefill=0)
        out = run.forward(ws, tune_flags=tf)
        assert out[0].data_ptr() == G.held_nan(ws, c, dev)[0].data_ptr()
        same_image(f"{c.name} flags {tf:#x}", out[:3], ref)
        same_grads(f"{c.name} flags {tf:#x}", run.backward(out[3], ws), gref)
    # two calls against the one call: the first call through a workspace IS the two calls and records them, the second replays them
    # through sks_forward_backward -- into outputs refilled with NaN
    ws = run.nan_workspace(prefill=0)
    for rep in range(2):
        for t_ in G.held_nan(ws, c, dev):
            t_.fill_(NAN)
        out = R.forward_backward_views(run.views, *run.args, run.dLc, run.dLi, bg=run.bg, force_binned=c.force_binned, workspace=ws)
        assert out[0].data_ptr() == G.held_nan(ws, c, dev)[0].data_ptr()
        same_image(f"{c.name} one call, round {rep}", out[:3], ref)
        same_grads(f"{c.name} one call, round {rep}", out[4], gref)
    assert "bwd" in ws._plans and "fwd" in ws._plans, "the second round did not replay the records"
    if small:      # the small path against the binned one (forward only)
        same_image(f"{c.name} forced onto the binned path", run.forward(force_binned=True)[:3], ref)


# ------------------------------------------------------------------------------------------------------------
# outputs that are 16-byte aligned and no more: only a direct C-ABI caller can make them
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [5, 80])
@pytest.mark.parametrize("W,H", G.ALIGN_SHAPES, ids=lambda v: str(v))
def test_outputs_16_bytes_past_a_line(device, W, H, P):
    c = G.align_case(W, H, P, seed=W + P)
    G.check_claims(c, aligned=False)
    dev, V, C, off = device, c.V, c.C, 4
    t = lambda a: torch.tensor(a, device=dev)
    means, feat, opac, scales, quats = t(c.means), t(c.feat), t(c.opac), t(c.scales), t(c.quats)
    views = R.ViewBatch.from_cameras([cam.to(dev) for cam in c.cams])
    gbytes = _lib.scratch_bytes(V, P, C, W, H, 0)[0]
    want = [G.oracle_forward(c, v) for v in range(V)]
    for flags in (0, _lib.SKS_NO_EARLY_FILL, _lib.SKS_NO_NT_STORES, _lib.SKS_EARLY_FILL(7), _lib.SKS_FILL_LINEAR, _lib.SKS_FILL_ROWS):
        color = torch.full((V * C * H * W + off + 32,), NAN, device=dev)
        inv = torch.full((V * H * W + off + 32,), NAN, device=dev)
        assert color.data_ptr() % 128 == 0 and inv.data_ptr() % 128 == 0
        radii = torch.full((V, P), -7, dtype=torch.int32, device=dev)
        geom = torch.zeros((gbytes,), dtype=torch.uint8, device=dev)
        args = [V, P, C, W, H, views.viewmatrix.data_ptr(), views.projmatrix.data_ptr(), views.tanfovx, views.tanfovy, means.data_ptr(),
                feat.data_ptr(), opac.data_ptr(), scales.data_ptr(), quats.data_ptr(), None, 1.0, int(flags),
                color.data_ptr() + 4 * off, inv.data_ptr() + 4 * off, radii.data_ptr(), geom.data_ptr(), None, 0, None, None, None,
                torch.cuda.current_stream(dev).cuda_stream]
        _lib.check(_lib.load().sks_forward(*args), "sks_forward")
        torch.cuda.synchronize()
        # nothing in front of the outputs or behind them was touched
        for buf, n in ((color, V * C * H * W), (inv, V * H * W)):
            assert torch.isnan(buf[:off]).all() and torch.isnan(buf[off + n:]).all(), f"flags {flags:#x}: a store outside the outputs"
        col = color[off:off + V * C * H * W].view(V, C, H, W).cpu().numpy()
        iv = inv[off:off + V * H * W].view(V, 1, H, W).cpu().numpy()
        for v in range(V):
            assert np.array_equal(radii[v].cpu().numpy(), want[v]["radii"])
            assert np.array_equal(col[v], want[v]["color"]), f"flags {flags:#x} view {v}: colour ({int(np.isnan(col[v]).sum())} left NaN)"
            assert np.array_equal(iv[v], want[v]["invdepth"]), f"flags {flags:#x} view {v}: inverse depth"


def test_images_beyond_the_limits_are_refused(device):
    lib = _lib.load()
    fwd_n, bwd_n = len(_lib.FORWARD_PARAMS), len(_lib.BACKWARD_PARAMS)
    for W, H in ((G.MAX_W + 1, 16), (16, G.MAX_H + 1)):
        for fn, n in ((lib.sks_forward, fwd_n), (lib.sks_backward, bwd_n)):
            args = [None] * n
            args[:5] = [1, 5, 3, W, H]
            for i, (_, ct) in enumerate(_lib.FORWARD_PARAMS if n == fwd_n else _lib.BACKWARD_PARAMS):
                if i >= 5 and ct is not ctypes.c_void_p:
                    args[i] = 0
            assert fn(*args) != 0 and b"out of range" in lib.sks_last_error()
        with pytest.raises(RuntimeError, match="out of range"):
            _lib.scratch_bytes(1, 5, 3, W, H)
        with pytest.raises(RuntimeError, match="out of range"):
            _lib.launch_regime(1, 5, 3, W, H)
    assert _lib.scratch_bytes(1, 5, 3, G.MAX_W, 16)[0] > 0 and _lib.scratch_bytes(1, 5, 3, 4, G.MAX_H)[0] > 0
