"""Shared by tests/test_fuse_cpu.py and tests/test_fuse_gpu.py: the reference's fused initial guesses of
tests/golden/reference_fuse.npz (made by tests/golden/make_golden_fuse.py from the reference's own two scripts), a numpy
restatement of the masked formula, and the COUNTED tolerances the results are held to.

The tolerances.  u = 2^-53, u32 = 2^-24, per (frame, joint):
  A     = max over i, c of (|u_ic| + |x_c|) / e_ic     the amplification of the cancellation in u - x (>= 1 by the triangle inequality)
  kappa = max over i, c, k of sum_m |P_c[k,m] [X_i;1]_m| / |(P_c [X_i;1])_k|       the conditioning of the three 4-term dot products
  S     = max_i |X_i - result|,   M = max_i |X_i|        (Euclidean norms, which bound every coordinate)
all from the fixture's INPUTS and golden result, never from the code under test.  One side's operation chain, first order:
  the dot products   4 roundings each (3 products and 3 additions, or FMAs): relative 4 kappa u on each h_k
  u_k = h_k / h_2    (4 kappa + 4 kappa + 1) u relative, so |du| <= (8 kappa + 1) u |u|
  d = u - x          one rounding: |dd| <= (8 kappa + 1) u |u| + u |d|
  e = |d|            two squares, one addition, one root: 2 u, plus |dd| / e  ->  relative ((8 kappa + 1) A + 3) u
  ebar_i             a sum of V positive terms and a division: + V u
  1 / ebar_i, the sum of V of them, the division by it: + (1 + (V - 1) + 1) u       -> weights: ((8 kappa + 1) A + 2 V + 4) u
  the result moves by at most that times S (the weights sum to one); with A >= 1:  <= (8 kappa + 2 V + 5) u A S
  the average        V products, V - 1 additions, the weight sum's V - 1 additions, one division: <= (2 V + 1) u M
  ->  one side <= (8 kappa + 2 V + 5) u (A S + M).  The golden went through the same chain in numpy's / BLAS's order, so
  C64 = 2 (8 kappa + 2 V + 5) = 16 kappa + 4 V + 10   and   |got - golden| <= C64 u (A S + M).
The float32 variant rounds d to float32 (a step function: either side may land one float32 ulp apart, u32 |d| each), then the
norm (2 u32), the mean (V u32) and the three weight operations ((V + 1) u32) are float32:  (2 V + 4) u32 per side on the weights,
  C32 = 2 (2 V + 4) = 4 V + 8   and   |got - golden| <= C32 u32 S + C64 u (A S + M).
ebar itself: relative 2 ((8 kappa + 1) A + 3 + V) u, and 2 (3 + V) u32 more in the float32 variant."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fuse.npz")
U64, U32 = 2.0 ** -53, 2.0 ** -24
VARIANTS = ("64", "32")             # the H36M script (all float64) / the Panoptic script (float32 weight chain)
_G = None


def _golden():
    global _G
    if _G is None:
        with np.load(GOLDEN) as f:
            _G = {k: f[k] for k in f.files}
    return _G


def names():
    return [str(n) for n in _golden()["names"]]


NAMES = ("v4j17n3", "v5j19n2", "v2j5n2", "v1j3n1", "v31j19n2", "v33j2n1")      # (test ids; held to the file by test_fuse_cpu)


def case(name):
    """dict(proj (V,3,4) f64, p3d (N,V,J,3), p2d (N,V,J,2) as stored -- float32 or float64 --, err64 / fused64 / err32 / fused32)."""
    G = _golden()
    return {k: G[f"{name}_{k}"] for k in ("proj", "p3d", "p2d", "err64", "fused64", "err32", "fused32")}


def restate(P, p3d, p2d, valid=None, norm=np.float64):
    """The masked formula in this project's words, in numpy's order (cameras, then candidates, one after the other): P (V,3,4) or
    (N,V,3,4), p3d (N,V,J,3), p2d (N,V,J,>=2), valid (N,V,J) bool or None, norm = dtype of the weight chain
    -> (fused (N,J,3) float64, ebar (N,V,J) float64 with NaN for a view left out, n_used (N,J))."""
    X, x = np.asarray(p3d, dtype=np.float64), np.asarray(p2d, dtype=np.float64)[..., :2]
    N, V, J = X.shape[:3]
    P = np.broadcast_to(np.asarray(P, dtype=np.float64), (N, V, 3, 4))
    keep = np.ones((N, V, J), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    n_used = keep.sum(axis=1)
    with np.errstate(all="ignore"):
        ebar = np.zeros((N, V, J), dtype=norm)
        for i in range(V):
            s = np.zeros((N, J), dtype=norm)
            for c in range(V):
                h = [((P[:, c, k, 0, None] * X[:, i, :, 0] + P[:, c, k, 1, None] * X[:, i, :, 1]) + P[:, c, k, 2, None] * X[:, i, :, 2])
                     + P[:, c, k, 3, None] for k in range(3)]
                dx, dy = (h[0] / h[2] - x[:, c, :, 0]).astype(norm), (h[1] / h[2] - x[:, c, :, 1]).astype(norm)
                s = np.where(keep[:, c], s + np.sqrt(dx * dx + dy * dy), s)
            ebar[:, i] = s / n_used.astype(norm)
        r = (1 / ebar).astype(norm)
        wsum = np.zeros((N, J), dtype=norm)
        for i in range(V):
            wsum = np.where(keep[:, i], wsum + r[:, i], wsum)
        w = (r / wsum[:, None]).astype(norm).astype(np.float64)
        num, scl = np.zeros((N, J, 3)), np.zeros((N, J))
        for i in range(V):
            num = np.where(keep[:, i, :, None], num + X[:, i] * w[:, i, :, None], num)
            scl = np.where(keep[:, i], scl + w[:, i], scl)
        fused = np.where((n_used > 0)[..., None], num / scl[..., None], np.nan)
    return fused, np.where(keep, ebar.astype(np.float64), np.nan), n_used.astype(np.int32)


def allowance(c, variant, result=None):
    """The counted bounds of the module docstring for one golden case: dict(C64, C32, unit (N,J,1) = u (A S + M), fused (N,J,1) =
    the bound on |got - golden| per coordinate, fused64 = the float64 variant's bound (the condition test_fuse_* assert on),
    err (N,V,J) = the bound on |ebar - golden| as a fraction of ebar).  `result`: the witness to take S from instead of the
    golden (a masked run against the restatement: the maxima then run over ALL views, a superset of the kept ones)."""
    P, X, x = c["proj"], c["p3d"].astype(np.float64), c["p2d"].astype(np.float64)
    N, V, J = X.shape[:3]
    Xh = np.concatenate([X, np.ones((N, V, J, 1))], -1)
    terms = np.abs(P[None, None, :, None, :, :] * Xh[:, :, None, :, None, :]).sum(-1)        # (N,Vi,Vc,J,3)
    h = np.einsum("ckm,nijm->nicjk", P, Xh)
    kappa = (terms / np.abs(h)).max(axis=(1, 2, 4))                                          # (N,J)
    u = h[..., :2] / h[..., 2:3]
    e = np.linalg.norm(u - x[:, None], axis=-1)                                              # (N,Vi,Vc,J)
    A = ((np.linalg.norm(u, axis=-1) + np.linalg.norm(x, axis=-1)[:, None]) / e).max(axis=(1, 2))
    S = np.nanmax(np.linalg.norm(X - (c["fused64"] if result is None else np.nan_to_num(result))[:, None], axis=-1), axis=1)
    M = np.linalg.norm(X, axis=-1).max(axis=1)
    C64, C32 = 16 * kappa + 4 * V + 10, 4 * V + 8
    unit = U64 * (A * S + M)
    fused64 = C64 * unit
    fused = fused64 + (C32 * U32 * S if variant == "32" else 0.0)
    err = 2 * ((8 * kappa + 1) * A + 3 + V)[:, None] * U64 + (2 * (3 + V) * U32 if variant == "32" else 0.0)
    return dict(C64=C64, C32=C32, unit=unit[..., None], fused=fused[..., None], fused64=fused64[..., None],
                err=np.broadcast_to(err, (N, V, J)), S=S[..., None])


def check_case(name, variant, fused, ebar=None, tag=""):
    """Holds one result to the golden by the counted bounds; prints the measured need before it asserts.  Returns (need in
    units of u (A S + M) -- or, for the float32 variant, in float32 ulps of S -- , bound in the same units)."""
    c = case(name)
    al = allowance(c, variant)
    assert float(al["fused64"].max()) < 1e-6, f"{name}: the float64 allowance {al['fused64'].max():.3g} mm must stay below 1e-6 mm"
    diff = np.abs(np.asarray(fused, dtype=np.float64) - c[f"fused{variant}"])
    if variant == "64":
        need, bound = float((diff / al["unit"]).max()), float(al["C64"].min())
    else:
        need, bound = float((diff / np.maximum(U32 * al["S"], 1e-300)).max()), float(al["C32"])      # (V = 1: S is 0 and so is diff)
    print(f"fuse {tag} {name} variant {variant}: max |got - golden| = {diff.max():.3e} mm, need {need:.3f} of {bound:.0f} "
          f"{'u (A S + M)' if variant == '64' else 'float32 ulps of S'}; allowance <= {al['fused'].max():.3e} mm")
    assert (diff <= al["fused"]).all(), (name, variant, float(diff.max()), float(al["fused"].max()))
    if ebar is not None:
        g = c[f"err{variant}"].astype(np.float64)
        rel = np.abs(np.asarray(ebar, dtype=np.float64) - g) / g
        print(f"fuse {tag} {name} variant {variant}: ebar relative error {rel.max():.3e}, allowance {al['err'].max():.3e}")
        assert (rel <= al["err"]).all(), (name, variant, float(rel.max()))
    return need, bound


def masks(N, V, J, seed=0):
    """A (N,V,J) bool `valid` in which joint 0 of every frame keeps NO view, joint 1 keeps exactly one, joint 2 (if any) exactly
    two (when V allows), and the rest lose a random third of their views."""
    rng = np.random.default_rng(seed)
    valid = rng.random((N, V, J)) > 1 / 3
    for n in range(N):
        for j, kept in ((0, 0), (1, 1), (2, 2)):
            if j < J:
                valid[n, :, j] = False
                valid[n, rng.permutation(V)[:min(kept, V)], j] = True
    return valid
