"""The float64 references of tests/tail_ref.py held to their sources (no GPU): scipy for the impulse response, the reference's
golden LR schedules and early-stopping decisions, the library's own limb loss and activation chain (which the goldens pin)."""
import os

import numpy as np
import torch

from tests import tail_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_python.npz"))
NEXT = os.path.join(ROOT, "tests", "golden", "reference_next.npz")


def impulse_cases():
    """(n, p, sigma, radius) over the axis lengths of the GPU test's images and radius in {0, 1, n-1, n, n+1, 3n, 10n}, the
    impulse at 0, n-1 and in the middle; 4 sigma + 0.5 sits a quarter above its integer."""
    for n in (1, 16, 24, 40, 130):
        for r in sorted({0, 1, 3, n - 1, n, n + 1, 3 * n, 10 * n}):
            for p in sorted({0, n - 1, n // 2}):
                yield n, p, ((r + 0.25) / 4.0 if r else 0.1), r


def test_impulse_ref_is_scipy_gaussian_filter1d():
    from scipy.ndimage import gaussian_filter1d
    beyond = 0.0
    for n, p, sigma, r in impulse_cases():
        got, radius = tail_ref.impulse_ref(n, p, sigma)
        assert radius == r
        line = np.zeros(n)
        line[p] = 1.0
        want = gaussian_filter1d(line, sigma, mode="reflect", truncate=4.0)
        assert np.abs(got - want).max() <= 4e-16, (n, p, sigma)
        assert abs(got.sum() - 1.0) < 1e-12            # (a reflecting boundary loses nothing)
        # the impulse and one mirror per side are not enough once radius > n: this is what the longer sum is for
        idx = np.arange(n)
        j = np.arange(-r, r + 1)
        tap = lambda s: np.exp(-0.5 * (idx - s) ** 2 / sigma ** 2) * (np.abs(idx - s) <= r)
        three = (tap(p) + tap(-1 - p) + tap(2 * n - 1 - p)) / np.exp(-0.5 * j * j / sigma ** 2).sum()
        if r <= n:
            assert np.abs(three - want).max() <= 4e-16, (n, p, sigma)
        else:
            beyond = max(beyond, np.abs(three - want).max() / want.max())
    assert beyond > 0.1


def test_oracle_twin_impulse_response_is_impulse_ref_at_any_radius():
    """oracle/heatmaps_ref.py's closed form (what sks_heatmap_factors is held to on the GPU) against the definition, past
    radius == n too: to its float32 output rounding."""
    from oracle import heatmaps_ref
    for n, p, sigma, r in impulse_cases():
        got = heatmaps_ref._impulse_response_1d(torch.tensor([p]), torch.tensor([sigma], dtype=torch.float64), n, "cpu")[0]
        want, _ = tail_ref.impulse_ref(n, p, sigma)
        assert np.abs(got.double().numpy() - want).max() <= 2.0 ** -24 * want.max() + 1e-45, (n, p, r)


def test_reflect_index_is_numpy_symmetric_padding():
    for n in (1, 2, 5, 16):
        line = np.arange(n)
        assert np.array_equal(np.pad(line, 7 * n, mode="symmetric"), line[tail_ref.reflect_index(np.arange(-7 * n, 8 * n), n)])


def test_lr_ref_is_the_golden_schedules():
    steps = [int(s) for s in GOLD["lr_steps"]]
    a = [tail_ref.lr_ref((0.0005 * 5500.0, 0.000005 * 5500.0, 0.0, 0.0, 4000.0), s) for s in steps]
    b = [tail_ref.lr_ref((0.01, 0.001, 0.1, 100.0, 500.0), s) for s in steps]
    np.testing.assert_allclose(a, GOLD["lr_values"], rtol=4.5e-16, atol=0)
    np.testing.assert_allclose(b, GOLD["lr2_values"], rtol=4.5e-16, atol=0)
    assert any(0 < s < 100 for s in steps)              # the golden visits the delay ramp
    assert tail_ref.lr_ref((0.0, 0.0, 0.01, 1000.0, 4000.0), 10) == 0.0
    assert tail_ref.lr_ref((0.0, 0.02, 0.01, 0.0, 4000.0), 10) == 0.0          # exp(-inf): one zero end point with weight


def test_es_ref_is_the_golden_decisions():
    G = np.load(NEXT)
    fired = 0
    for name in ("plateau", "period4", "period4_drift", "edge", "noise", "short"):
        seq = [float(x) for x in G[f"es_{name}_loss"]]
        for key, w, tol in ((f"es_{name}_opt", 4, 1e-6), (f"es_{name}_opt_w3", 3, 1e-3)):
            want = G[key].tolist()
            first = want.index(True) + 1 if any(want) else 0
            assert tail_ref.es_ref(seq, w, tol) == first, (name, w)
            fired += first > 0
    assert fired >= 3
    # the loss the criterion sees: fp32 quotient, clamp of N, fp32 sum
    assert tail_ref.es_losses((3.0, 0.0)) == 3.0 and tail_ref.es_losses((1.0, 3.0)) == float(np.float32(1.0 / 3.0))
    assert tail_ref.es_losses((1.0, 3.0), 1e-9) == float(np.float32(np.float32(1.0 / 3.0) + np.float32(1e-9)))
    assert np.isnan(tail_ref.es_losses((float("nan"), 5.0)))
    assert tail_ref.es_ref([0.5, float("nan"), 0.5, 0.5], 1, 1e-3) == 4     # a NaN never fires; the pair behind it does


def test_limb_loss_is_the_library_limb_loss():
    from skelsplat_amd import loop
    from skelsplat_amd.scene import DATASETS
    for key in ("h36m", "panoptic", "occlusion-person"):
        limb = [i for pair in DATASETS[key]["limbs"] for i in pair]
        if key == "h36m":
            assert tuple(limb) == tail_ref.H36M_LIMB
        x = torch.tensor(GOLD[f"limb_{key}_xyz"], dtype=torch.float64, requires_grad=True)
        y = x.detach().clone().requires_grad_(True)
        a, b = tail_ref.limb_loss(x, limb), loop.limb_3d_consistency_loss(y, key)
        a.backward()
        b.backward()
        assert a.item() == b.item() and torch.equal(x.grad, y.grad)
        assert abs(a.item() - GOLD[f"limb_{key}_loss"]) <= 1e-6 * GOLD[f"limb_{key}_loss"]


def test_pack_ref_is_the_activation_chain_in_float64():
    import types
    from skelsplat_amd import loop
    g = torch.Generator().manual_seed(0)
    V, P = 3, 5
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    raw_s, raw_q, raw_o = r(P, 3), r(P, 4), r(P, 1)
    gm = types.SimpleNamespace(get_scaling=torch.exp(raw_s), get_opacity=torch.sigmoid(raw_o), _rotation=raw_q)
    grads = {"scales": r(V, P, 3), "rotations": r(V, P, 4), "opacities": r(V, P, 1)}
    means = r(V, P, 3)
    sums = torch.tensor([[1.0, 4.0], [2.0, 0.0], [3.0, 7.0]], dtype=torch.float64)
    d_s, d_q, d_o = loop.activation_chain(gm, grads)
    sc = torch.tensor([0.25, 1.0, 1.0 / 7.0], dtype=torch.float64)[:, None, None]
    want = torch.cat([means, d_s, d_q, d_o], dim=2) * sc
    got, allow = tail_ref.pack_ref(means, grads["scales"], grads["rotations"], grads["opacities"], raw_s, raw_q, raw_o, sums)
    torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-15)
    assert bool((allow >= got.abs()).all())            # a sum of |terms| is never below the value


def test_adam_step_ref_is_the_loop_of_the_source():
    """One call of adam_step_ref against the formulas written out (slots, mean, last view's rows, schedule, Adam), in a case
    small enough to follow by hand: V = 2, one view in the mask, a joint in both limb pairs of the arm term."""
    g = torch.Generator().manual_seed(1)
    V, P = 2, 4
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    grads, slots, m0 = r(V, P, 11), r(V, P, 3), r(P, 11) * 0.1
    v0 = (r(P, 11) * 0.1) ** 2
    prm = [r(P, 3) * 100.0, r(P, 3), r(P, 4), r(P, 1)]
    limb = (0, 1, 0, 2, 1, 3, 2, 3)
    sched, lrs, adam = (2.0, 0.02, 0.01, 1000.0, 4000.0), (0.005, 0.001, 0.05), (0.9, 0.999, 1e-15)
    out = tail_ref.adam_step_ref(grads, slots, 0b10, 1, prm, m0, v0, (8, 2), 4, sched, lrs, adam, 0.5, limb)
    x = prm[0].clone().requires_grad_(True)
    (gc,) = torch.autograd.grad(0.5 * tail_ref.limb_loss(x, limb), x)
    want_slots = torch.stack([slots[0], grads[1, :, :3] + gc])
    assert torch.equal(out["slots"][0], want_slots) and out["counters"] == (12, 3)
    gx = want_slots.mean(0)
    lr = tail_ref.lr_ref(sched, 12)
    assert 0.01 * 2.0 * 0.98 < lr < 0.1                 # inside the delay ramp: the sine factor is at work
    m1 = 0.9 * m0[:, :3] + 0.1 * gx
    v1 = 0.999 * v0[:, :3] + 0.001 * gx * gx
    want_xyz = prm[0] - lr / (1 - 0.9 ** 3) * m1 / (v1.sqrt() / (1 - 0.999 ** 3) ** 0.5 + 1e-15)
    torch.testing.assert_close(out["xyz"][0], want_xyz, rtol=1e-12, atol=0)
    torch.testing.assert_close(out["m"][0][:, 3:], 0.9 * m0[:, 3:] + 0.1 * grads[1, :, 3:], rtol=1e-13, atol=1e-16)
    for name in ("slots", "m", "v", "xyz", "scaling", "rotation", "opacity"):
        assert bool(torch.isfinite(out[name][1]).all()) and bool((out[name][1] >= 0).all())
