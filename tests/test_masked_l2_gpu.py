"""GPU tests of k_masked_l2 and the fused criterion (csrc/sks_ops.hip) at their launch regimes: the cases of
tests/masked_l2_cases.py, which tests/test_masked_l2_cpu.py shows to reach the kernel's unrolled loop, its remainder loop and its
scalar tail, against a float64 reference.

Held to, per view: N exactly; S within S_BAR_U = 8 x 2^-24 of the float64 sum (counted in masked_l2_cases.reference, never
measured); the gradient bit for bit, also with the three base pointers at every 4-byte phase between guards (tests/guarded.py).
Every test prints its figures before it asserts; MEASUREMENTS.md "masked L2 at its launch regimes" has the MI355X run."""
import numpy as np
import pytest
import torch

from tests import guarded
from tests import masked_l2_cases as mc
from tests import util

pytestmark = pytest.mark.gpu

_CASE = {}


def case(name):
    """Inputs and float64 reference of one case, computed once and shared."""
    if name not in _CASE:
        r, g = mc.make_inputs(name)
        _CASE[name] = (r, g) + mc.reference(r, g)
    return _CASE[name]


def call(V, n, r_ptr, g_ptr, dL_ptr, sums, device):
    """sks_masked_l2 through the C ABI on raw pointers; `sums` (V, 2) float64 on the device is filled."""
    from skelsplat_amd import _lib
    with torch.cuda.device(device):
        rc = _lib.load().sks_masked_l2(V, n, r_ptr, g_ptr, dL_ptr, sums.data_ptr(), torch.cuda.current_stream(device).cuda_stream)
    _lib.check(rc, "sks_masked_l2")


def hold_sums(what, sums, N, S64):
    S, got_N = sums[:, 0].cpu().numpy(), sums[:, 1].cpu().numpy()
    dev = mc.s_deviation_u(S, S64)
    print(f"{what}: S off by {dev.max():.3e} x 2^-24 of itself (bar {mc.S_BAR_U:g})")
    assert np.array_equal(got_N, N.astype(np.float64)), what
    assert np.all(dev <= mc.S_BAR_U), what
    return float(dev.max())


@pytest.mark.parametrize("name", list(mc.CASES))
def test_masked_l2_at_every_launch_regime(device, name):
    """ops.masked_l2 on (V, 1, 1, n): N, S and the gradient's bits; then the same call with `sums` holding garbage on entry (the
    entry clears it) and without a gradient."""
    from skelsplat_amd.ops import masked_l2
    r, g, N, S64, dL = case(name)
    V, n = mc.CASES[name]
    rd, gd = torch.from_numpy(r).to(device).view(V, 1, 1, n), torch.from_numpy(g).to(device).view(V, 1, 1, n)
    got_dL, S, N_ = masked_l2(rd, gd)
    hold_sums(name, torch.stack([S, N_], dim=1), N, S64)
    got = got_dL.view(V, n).cpu().numpy()
    assert got.dtype == np.float32
    bad = np.flatnonzero(got.view(np.int32) != dL.view(np.int32))
    assert bad.size == 0, f"{name}: {bad.size} gradient elements differ, the first at {int(bad[0])} of {V} x {n}"

    stale = torch.full((V, 2), 1.0e300, dtype=torch.float64, device=device)
    stale[:, 1] = float("nan")
    out = torch.empty_like(rd)
    call(V, n, rd.data_ptr(), gd.data_ptr(), out.data_ptr(), stale, device)
    hold_sums(name + " (stale sums)", stale, N, S64)
    assert torch.equal(out, got_dL)

    none, S2, N2 = masked_l2(rd, gd, want_grad=False)
    assert none is None
    hold_sums(name + " (no gradient)", torch.stack([S2, N2], dim=1), N, S64)


@pytest.mark.parametrize("name", mc.PHASE_CASES)
def test_gradient_is_written_exactly_once_at_every_phase(device, name):
    """render, gt and dL handed in 0..3 floats past a 16-byte boundary (masked_l2_cases.PHASE_TRIPLES): the kernel's 16-byte
    groups are relative to the pointers it is given, so it must write the n floats from `dL` on and nothing else.  dL lies between
    guards in a buffer of sentinels; the interior equals the reference's bits at every phase and both guards stay untouched."""
    r, g, N, S64, dL = case(name)
    V, n = mc.CASES[name]
    total = V * n
    size = guarded.buffer_floats(total)
    want = dL.reshape(-1).view(np.int32)
    src = {}
    for what, a in (("r", r), ("g", g)):
        for p in guarded.PHASES:
            if any(t[0 if what == "r" else 1] == p for t in mc.PHASE_TRIPLES):
                buf = torch.zeros(size, dtype=torch.float32, device=device)
                buf[guarded.interior(p, total)] = torch.from_numpy(a.reshape(-1)).to(device)
                src[what, p] = buf
    sentinel = torch.full((size,), int(guarded.SENTINEL), dtype=torch.int32, device=device)
    worst = 0.0
    for pr, pg, pd in mc.PHASE_TRIPLES:
        out = sentinel.clone()
        for t in (src["r", pr], src["g", pg], out):
            assert t.data_ptr() % 16 == 0
        sums = torch.empty((V, 2), dtype=torch.float64, device=device)
        call(V, n, src["r", pr].data_ptr() + 4 * (guarded.GUARD + pr), src["g", pg].data_ptr() + 4 * (guarded.GUARD + pg),
             out.data_ptr() + 4 * (guarded.GUARD + pd), sums, device)
        worst = max(worst, hold_sums(f"{name} phases {pr}{pg}{pd}", sums, N, S64))
        guarded.check(f"{name} phases {pr}{pg}{pd}", out.cpu().numpy(), pd, total, want)
    print(f"{name}: largest S deviation over {len(mc.PHASE_TRIPLES)} phase triples {worst:.3e} x 2^-24")


def test_fused_criterion_on_two_unrolled_trips(device):
    """ops.l2_loss_gaussian on `main2` as one view of 7.3 million elements: 'mean' and 'sum' within LOSS_BAR_U = 10 x 2^-24 of the
    float64 value (S's 8, the division in fp64, the cast to float), the gradient under (3 loss).backward() at
    test_fused_l2_loss_gaussian_criterion's rtol = 1e-5, atol_scale = 1e-6."""
    from skelsplat_amd.ops import l2_loss_gaussian
    r, g, N, S64, dL = case("main2")
    rd, gd = torch.from_numpy(r[0]).to(device), torch.from_numpy(g[0]).to(device)
    for reduction in ("mean", "sum"):
        x = rd.clone().requires_grad_(True)
        out = l2_loss_gaussian(x, gd, None, 1.0, reduction=reduction)
        loss = out[0] if reduction == "mean" else out
        assert reduction == "sum" or out[1] is None
        want = S64[0] / N[0] if reduction == "mean" else S64[0]
        (3.0 * loss).backward()
        dev = abs(float(loss.item()) - want) / (mc.U * want)
        print(f"main2 '{reduction}': value off by {dev:.3f} x 2^-24 of itself (bar {mc.LOSS_BAR_U:g})")
        assert loss.dtype == torch.float32 and dev <= mc.LOSS_BAR_U
        want_g = 3.0 * dL[0].astype(np.float64) / (N[0] if reduction == "mean" else 1.0)
        util.assert_close(f"grad ({reduction})", x.grad.cpu().numpy(), want_g, rtol=1e-5, atol_scale=1e-6)


def test_fused_criterion_of_an_empty_mask(device):
    """An all-zero pair: nothing is in the mask.  'mean' is NaN like the reference's mean of nothing, 'sum' is 0."""
    from skelsplat_amd.ops import l2_loss_gaussian
    z = torch.zeros(mc.CASES["one_block"][1], device=device)
    mean, err = l2_loss_gaussian(z, z.clone(), None, 1.0, reduction="mean")
    assert err is None and torch.isnan(mean).item()
    assert l2_loss_gaussian(z, z.clone(), None, 1.0, reduction="sum").item() == 0.0
