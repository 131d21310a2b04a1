"""The fused-SSIM CPU oracle (oracle/sks_ssim_oracle.c) held to SSIM, and the derivation the GPU tests' bounds rest on.

  * The double build against an independent float64 conv2d SSIM with autograd, on every input class: both sides are
    float64 and differ in the order of their sums, so the allowance is computed, not chosen (see _allowances).
  * The float build on uniform noise at the tolerances the GPU tests use against float64, and on the reference's own
    golden values.
  * The input classes' conditions: which classes reach quotients outside the division sequence's exact range.
  * The kernels' division sequence restated with a reciprocal seed at -1 / 0 / +1 ulp: where it is IEEE `/`.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ssim_ref
from tests import ssim_cases as sc
from tests import util

U = 2.0 ** -53
N_SUM = 121 + 22   # roundings on the way of one term: <= 121 in the 11 x 11 sum, 11 + 11 in the separable one


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _conv(x):
    return F.conv2d(x, sc.ssim_window(x.size(-3), x, sc.TAPS32), padding=5, groups=x.size(-3))


def _outputs(leaves, C1, C2):
    """map and partial derivatives as a function of the moments, every occurrence of a product of means its own leaf
    (a11, a22 inside A; c12 inside Cn; s11, s22, s12 inside the sigmas), so that a rounding inside one sum can be
    attributed to a leaf that feeds nothing else."""
    mu1, mu2, a11, a22, c12, s11, s22, s12, e11, e22, e12 = leaves
    Cn, D = 2 * c12 + C1, 2 * (e12 - s12) + C2
    A, B = a11 + a22 + C1, (e11 - s11) + (e22 - s22) + C2
    q = [2 * mu2 * D / (A * B), 2 * mu2 * Cn / (A * B), 2 * mu1 * Cn * D / (A * A * B), 2 * mu1 * Cn * D / (A * B * B)]
    return dict(map=Cn * D / (A * B), dm_dmu1=q[0] - q[1] - q[2] + q[3], dm_dsigma1_sq=-Cn * D / (A * B * B),
                dm_dsigma12=2 * Cn / (A * B)), sum(x.abs() for x in q)


def _allowances(img1, img2, mom, C1, C2):
    """How far two float64 evaluations of SSIM that differ in the order of their sums may sit apart, first order:

      sum over leaves of |d out / d leaf| x (the leaf's own allowance)  +  k x 2^-53 x sum |terms of out|,   all x 2.

    A moment's allowance is (number of roundings a term passes) x 2^-53 x sum |terms|: N_SUM for the two filters, + 2 for
    the rounded products under E[.]; a product of means adds its factors' allowances and one rounding per side.  The
    roundings of the sums A, B, Cn, D and of the sigmas (one per operation and side, each at most 2^-53 x the sum of the
    operands' magnitudes) are attributed to the leaf of that sum.  What is left are products and quotients: at most 16
    relative roundings per term and side (the oracle's expression, autograd's chain), k = 32.  The final factor 2
    covers the second-order terms, which are 2^-53 times smaller.
    """
    mu1, mu2, e11, e22, e12 = mom
    a1, a2 = img1.abs(), img2.abs()
    d_mu1, d_mu2 = N_SUM * U * _conv(a1), N_SUM * U * _conv(a2)
    p11, p22, p12 = mu1 * mu1, mu2 * mu2, (mu1 * mu2).abs()
    d_p11 = 2 * mu1.abs() * d_mu1 + 2 * U * p11
    d_p22 = 2 * mu2.abs() * d_mu2 + 2 * U * p22
    d_p12 = mu1.abs() * d_mu2 + mu2.abs() * d_mu1 + 2 * U * p12
    Aabs, Babs = p11 + p22 + C1, (e11 + p11) + (e22 + p22) + C2
    Dabs = 2 * (e12.abs() + p12) + C2
    delta = [d_mu1, d_mu2,
             d_p11 + 4 * U * Aabs, d_p22, d_p12 + 2 * U * (2 * p12 + C1),                      # a11 (A's sums), a22, c12 (Cn's sum)
             d_p11, d_p22, d_p12,                                                              # s11, s22, s12
             (N_SUM + 2) * U * _conv(a1 * a1) + 2 * U * (e11 + p11) + 4 * U * Babs,            # e11 (sigma1's, B's sums)
             (N_SUM + 2) * U * _conv(a2 * a2) + 2 * U * (e22 + p22),                           # e22
             (N_SUM + 2) * U * _conv(a1 * a2) + 2 * U * (e12.abs() + p12) + 2 * U * Dabs]      # e12 (sigma12's, D's sums)
    leaves = [x.detach().clone().requires_grad_(True) for x in (mu1, mu2, p11, p22, mu1 * mu2, p11, p22, mu1 * mu2, e11, e22, e12)]
    outs, qsum = _outputs(leaves, C1, C2)
    allow = {}
    for k, o in outs.items():
        grads = torch.autograd.grad(o.sum(), leaves, retain_graph=True, allow_unused=True)
        grads = [torch.zeros_like(o) if g is None else g for g in grads]
        terms = qsum if k == "dm_dmu1" else o.abs()
        allow[k] = 2 * (sum(g.abs() * d for g, d in zip(grads, delta)) + 32 * U * terms).detach()
    return allow


@functools.lru_cache(maxsize=None)
def _float64_reference(name, shape):
    """The independent side, once per case: conv2d moments, the map from ssim_torch, the partial derivatives from
    autograd of that map with respect to the moments."""
    c = sc.make(name, shape)
    img1, img2 = _t(c.img1), _t(c.img2)
    mom = sc.ssim_moments(img1, img2, sc.TAPS32)
    lv = [m.detach().clone().requires_grad_(True) for m in mom]
    mu1, mu2, e11, e22, e12 = lv
    m = ((2 * mu1 * mu2 + c.C1) * (2 * (e12 - mu1 * mu2) + c.C2)) / \
        ((mu1.pow(2) + mu2.pow(2) + c.C1) * ((e11 - mu1.pow(2)) + (e22 - mu2.pow(2)) + c.C2))
    g = torch.autograd.grad(m.sum(), [mu1, e11, e12])
    x = img1.clone().requires_grad_(True)
    mr = sc.ssim_torch(x, img2, c.C1, c.C2, sc.TAPS32)     # keeps its graph: dL_dimg1 under any upstream gradient
    ref = dict(map=mr.detach(), dm_dmu1=g[0], dm_dsigma1_sq=g[1], dm_dsigma12=g[2])
    return c, img1, img2, ref, _allowances(img1, img2, mom, c.C1, c.C2), (mr, x)


@functools.lru_cache(maxsize=None)
def _oracle(name, shape, real):
    c = sc.make(name, shape)
    return ssim_ref.forward(c.img1, c.img2, c.C1, c.C2, real=real)


def _assert_within(tag, got, want, allow, crop=0):
    got, want, allow = (np.asarray(a, dtype=np.float64) for a in (got, want, allow))
    if crop:
        got, want, allow = (a[:, :, crop:-crop, crop:-crop] for a in (got, want, allow))
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), f"{tag}: the non-finite pixels differ"
    err = np.abs(got[fin] - want[fin])
    bad = ~(err <= allow[fin])
    assert not bad.any(), (f"{tag}: {bad.sum()} / {bad.size} outside the allowance; worst error / allowance "
                           f"{np.max(err / np.maximum(allow[fin], 1e-300)):.2f}")


CASES = sc.case_list()


@pytest.mark.parametrize("name,shape", CASES, ids=sc.case_id)
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_double_build_is_ssim(name, shape, padding):
    """Map, the three partial derivatives and dL_dimg1 under a random upstream gradient: the oracle's text in double
    against conv2d SSIM with autograd, within the computed allowance."""
    c, img1, img2, ref, allow, (mr, x) = _float64_reference(name, shape)
    o = _oracle(name, shape, "f64")
    crop = 5 if padding == "valid" else 0
    H, W = c.shape[2:]
    if H <= 2 * crop or W <= 2 * crop:
        assert mr[:, :, 5:-5, 5:-5].numel() == 0
        assert np.isnan(ssim_ref.mean(o["map"], crop, real="f64"))
        return
    for k in ("map", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12"):
        _assert_within(f"{name} {k}", o[k], ref[k].numpy(), allow[k].numpy(), crop)
    # dL_dimg1: the upstream gradient of the ("valid"-cropped) map, zero outside the crop
    w = np.zeros(c.shape)
    inner = (slice(None), slice(None), slice(crop, H - crop), slice(crop, W - crop))
    w[inner] = np.random.default_rng(5).uniform(-1, 1, w[inner].shape)
    want = torch.autograd.grad(mr, x, grad_outputs=_t(w), retain_graph=True)[0]
    got = ssim_ref.backward(c.img1, c.img2, w, o["dm_dmu1"], o["dm_dsigma1_sq"], o["dm_dsigma12"], real="f64")
    # allowance: the partial maps' own, filtered, plus the filters' (N_SUM + the products' and the three final operations'
    # roundings) x 2^-53 x sum |terms|; x 2 as above
    wa = _t(np.abs(w))
    with np.errstate(invalid="ignore"):
        fz = lambda t: torch.nan_to_num(t, nan=float("inf"), posinf=float("inf"))
        d = {k: fz(ref[k].abs()) for k in ref}
        al = {k: fz(allow[k]) for k in allow}
        a1, a2 = fz(img1.abs()), fz(img2.abs())
        g_allow = (_conv(wa * al["dm_dmu1"]) + 2 * a1 * _conv(wa * al["dm_dsigma1_sq"]) + a2 * _conv(wa * al["dm_dsigma12"]) +
                   2 * (N_SUM + 8) * U * (_conv(wa * d["dm_dmu1"]) + 2 * a1 * _conv(wa * d["dm_dsigma1_sq"]) +
                                          a2 * _conv(wa * d["dm_dsigma12"])))
    _assert_within(f"{name} dL_dimg1", got, want.numpy(), torch.nan_to_num(g_allow, nan=float("inf")).numpy())


def test_float_build_on_noise_at_todays_gpu_tolerances():
    """The float oracle passes what the kernels pass today (tests/test_ops_gpu.py): float64 conv2d SSIM with the
    reference's own window at 2e-5 on the map, 1e-3 / 1e-4 max on the gradient."""
    for shape in sc.MAIN_SHAPES:
        c = sc.make("noise", shape)
        o = _oracle("noise", shape, "f32")
        w = np.random.default_rng(6).random(c.shape).astype(np.float32)
        x = _t(c.img1).requires_grad_(True)
        mr = sc.ssim_torch(x, _t(c.img2))
        (mr * _t(w)).sum().backward()
        util.assert_close("ssim_map", o["map"], mr.detach().numpy(), rtol=2e-5, atol_scale=5e-6)
        got = ssim_ref.backward(c.img1, c.img2, w, o["dm_dmu1"], o["dm_dsigma1_sq"], o["dm_dsigma12"])
        util.assert_close("dL_dimg1", got, x.grad.numpy(), rtol=1e-3, atol_scale=1e-4)


def test_float_build_reproduces_the_reference_wrapper():
    """tests/golden/reference_ssim.npz at the tolerances of test_fused_ssim_wrapper_reproduces_the_reference_wrapper."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_ssim.npz"))
    for tag in ("a", "b", "c"):
        img1, img2 = G[tag + "_img1"], G[tag + "_img2"]
        o = ssim_ref.forward(img1, img2)
        B, CH, H, W = img1.shape
        for padding, crop in (("same", 0), ("valid", 5)):
            key = f"{tag}_{padding}_train"
            val = float(ssim_ref.mean(o["map"], crop))
            for mode in ("train", "infer"):
                want = float(G[f"{tag}_{padding}_{mode}_value"])
                assert abs(val - want) <= 1e-5 * abs(want), key
            count = B * CH * (H - 2 * crop) * (W - 2 * crop)
            g = ssim_ref.backward_uniform(img1, img2, 3.0, 1.0 / count, crop, o["dm_dmu1"], o["dm_dsigma1_sq"], o["dm_dsigma12"])
            util.assert_close(key, g, G[key + "_grad"], rtol=1e-3, atol_scale=1e-4)


def test_uniform_backward_is_the_backward_of_the_materialised_gradient():
    c = sc.make("heatmaps", sc.SHAPE_SCALAR)
    o = _oracle("heatmaps", sc.SHAPE_SCALAR, "f32")
    parts = (o["dm_dmu1"], o["dm_dsigma1_sq"], o["dm_dsigma12"])
    for crop in (0, 5):
        dL = np.zeros(c.shape, np.float32)
        dL[:, :, crop:c.shape[2] - crop, crop:c.shape[3] - crop] = np.float32(0.75) * np.float32(1.0 / 77)
        assert np.array_equal(ssim_ref.backward_uniform(c.img1, c.img2, 0.75, 1.0 / 77, crop, *parts),
                              ssim_ref.backward(c.img1, c.img2, dL, *parts))


# ---- the input classes' conditions ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", CASES, ids=sc.case_id)
def test_class_conditions(name, shape):
    """Every class except the tails and the non-finite one keeps every quotient inside the range in which the kernels'
    division sequence is exact, so every pixel pins bits; the tails reach outside it on some pixels and stay inside on
    most; no class is vacuous."""
    c = sc.make(name, shape)
    o = _oracle(name, shape, "f32")
    flagged = o["flags"] != 0
    if name not in sc.MAY_BE_FLAGGED:
        assert not flagged.any(), f"{flagged.sum()} flagged pixels"
    if name == "tails":
        assert flagged.any() and 2 * flagged.sum() < flagged.size, (flagged.sum(), flagged.size)
        assert (c.img1[c.img1 > 0] < 2.0 ** -126).any(), "the tails must run down to denormals"
    if name == "heatmaps":
        px = np.concatenate([c.img1.ravel(), c.img2.ravel()])
        assert ((px == 0) | (px >= 2.0 ** -16)).all() and (px == 0).mean() > 0.3 and (px > 0.25).any()
    if name == "blobs255":
        assert o["outside_documented"] > 0   # beyond d < 2^8: what this class is for
    if name in ("noise", "signed", "checker-shift"):
        assert np.unique(o["map"]).size > o["map"].size // 4 or name == "checker-shift"
    if name == "checker-shift" and min(c.shape[2:]) > 8:
        assert (o["map"] < 0).any()
    if name == "signed":
        assert (2 * o["dm_dsigma12"] < 0).any()   # Cn < 0
    if name == "seams":
        assert ((o["map"] != 1).reshape(c.shape[0], -1).sum(1) >= min(c.shape[2], 6) * min(c.shape[3], 6)).all()
    if name == "nonfinite" and shape == sc.SHAPE_VEC:
        bad = ~np.isfinite(o["map"])
        assert 0 < bad.sum() <= 2 * 121


# ---- the division sequence --------------------------------------------------------------------------------------

def _fmaf(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum is rounded to odd there (two-sum's error term
    decides), and the final rounding to float32 is then the single rounding of the exact a*b + c."""
    with np.errstate(invalid="ignore", over="ignore"):   # an overflowed operand gives inf - inf = nan, as fmaf does
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64).copy()
        inexact = (e != 0) & np.isfinite(s)
        away = inexact & ((e > 0) == (s > 0))            # the exact sum lies beyond s: truncation is s itself
        toward = inexact & ~away                         # ... short of s: truncation is the value before s
        bits[toward] -= 1
        bits[inexact] |= 1
    with np.errstate(over="ignore", under="ignore"):
        return bits.view(np.float64).astype(np.float32)


def _div_by(n, d, seed_ulps):
    """sks_ssim.hip's refined_rcp / div_by with the reciprocal seed `seed_ulps` away from the correctly rounded 1 / d."""
    one = np.float32(1)
    r = one / d
    if seed_ulps:
        r = np.nextafter(r, np.float32(np.inf if seed_ulps > 0 else -np.inf), dtype=np.float32)
    r = _fmaf(_fmaf(-d, r, np.broadcast_to(one, d.shape)), r, r)
    q = n * r
    q = _fmaf(_fmaf(-d, q, n), r, q)
    return _fmaf(_fmaf(-d, q, n), r, q)


def _pow2_sample(rng, lo, hi, size):
    return (np.exp2(rng.uniform(lo, hi, size))).astype(np.float32)


def test_fmaf_restatement_is_fmaf():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(20000).astype(np.float32), rng.standard_normal(20000).astype(np.float32)
    c = (-(a.astype(np.float64) * b)).astype(np.float32)   # a*b + c cancels to the product's rounding error
    got = _fmaf(a, b, c)
    from fractions import Fraction
    for i in range(0, 20000, 40):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert float(got[i]) == float(exact), i   # the error of a float32 product is itself a float32


@pytest.mark.parametrize("seed_ulps", [-1, 0, 1])
def test_division_sequence_is_ieee_division_in_its_range(seed_ulps):
    """d in [2^-100, 2^100), |n| in [2^-100, 2^100): equal to n / d on 1.2 x 10^6 seeded pairs per seed offset; with
    |n| or d below 2^-100 within one ulp of it.  This is what the GPU tests' "exact here, bounded there" rests on."""
    rng = np.random.default_rng(10 + seed_ulps)
    N = 1_200_000
    with np.errstate(over="ignore", under="ignore"):
        d = _pow2_sample(rng, -100, 100, N)
        n = _pow2_sample(rng, -100, 100, N) * rng.choice(np.float32([-1, 1]), N)
        want = n / d
        ok = np.isfinite(want) & (np.abs(want) >= 2.0 ** -126)     # the quotient itself a normal number
        got = _div_by(n, d, seed_ulps)
        assert ok.sum() > N // 2
        assert np.array_equal(got[ok], want[ok]), f"{(got[ok] != want[ok]).sum()} of {ok.sum()} differ"
        for lo_n, hi_n, lo_d, hi_d in ((-149, -100, -100, 100), (-100, 0, -126, -100)):
            d = _pow2_sample(rng, lo_d, hi_d, N // 4)
            n = _pow2_sample(rng, lo_n, hi_n, N // 4) * rng.choice(np.float32([-1, 1]), N // 4)
            want = n / d
            got = _div_by(n, d, seed_ulps)
            fin = np.isfinite(want)
            err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
            assert np.isfinite(got[fin]).all() and (err <= np.spacing(np.abs(want[fin])).astype(np.float64)).all(), \
                f"worst {np.max(err / np.spacing(np.abs(want[fin])))} ulp"
