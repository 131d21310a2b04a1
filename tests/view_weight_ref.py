"""TEST INFRASTRUCTURE -- the view-agreement weighting of the optimiser step (include/skelsplat_hip.h, DESIGN.md "View
agreement") restated on the CPU: op by op in numpy float32, in the order the kernel takes (`*32`: what the GPU tests compare
bits with), and in float64 (`*64`).  Nothing here loads the HIP library.

g: (V,P,3) slots, view-major.  similarity: (P,V,V).  weights: (V,P).  merged: (P,3) -- the xyz gradient of the step.
MODES: the C ABI's vw_mode numbers."""
import numpy as np

MODES = {None: 0, "scale": 1, "select": 2}
F = np.float32
SLOT_LDS = 8192       # floats of the kernel's slot mirror in LDS (adam_block_finish)

# fp32 roundings between a slot and a cosine: 3 squares + 2 additions, sqrtf, + 1e-8f (7 on the norm, each a relative 2**-24);
# u = g / n (1); c = 3 products + 2 additions (5).  To first order every one of them moves c by at most 2**-24 x a quantity
# <= 1 (|u| <= 1, |c| <= 1), the norm's and the division's once per operand: 2 x (7 + 1) + 5.
K_COS = 2 * (7 + 1) + 5
# s: V - 2 additions that round (the first adds to 0) and the division, of quantities <= 1 in size -- plus the cosines' own
K_S = lambda V: (V - 2) + 1
# w (scale): the log branch has slope 0.54 / ((2 + s) ln 3) <= 0.25, the linear one 0.8 (< 1: the allowance takes 1); then one
# rounding of the double result to float (the log branch), or the addition and the product (the linear branch): 2
K_W = 2


def regime(V, P):
    """Which walk of adam_block_finish a shape takes with the weighting on ('lds': the slots are parked in LDS and the pairwise
    work is spread over the workgroup; 'walk': they do not fit, one thread per joint) and with it off ('narrow' / 'wide' / 'walk')."""
    fits = V * P * 3 <= SLOT_LDS
    return ("lds" if fits else "walk"), ("wide" if V > 8 and fits else ("narrow" if V <= 8 else "walk"))


def similarity32(g):
    g = np.asarray(g, dtype=F)
    V, P = g.shape[:2]
    with np.errstate(all="ignore"):
        n = np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]) + F(1e-8)      # (V,P)
        u = g / n[..., None]
        c = np.empty((P, V, V), dtype=F)
        for a in range(V):
            for b in range(V):
                c[:, a, b] = (u[a, :, 0] * u[b, :, 0] + u[a, :, 1] * u[b, :, 1]) + u[a, :, 2] * u[b, :, 2] if a != b else F(1.0)
    return c


def _row_sums32(c):
    P, V = c.shape[:2]
    s = np.zeros((V, P), dtype=F)
    with np.errstate(all="ignore"):
        for a in range(V):
            for b in range(V):
                if b != a:
                    s[a] = s[a] + c[:, a, b]
    return s


def scale_weights32(c):
    """compute_scaling_weights with the divisor V - 1 and the clamp; the log branch in double, rounded once."""
    c = np.asarray(c, dtype=F)
    P, V = c.shape[:2]
    if V < 2:
        return np.ones((V, P), dtype=F)
    with np.errstate(all="ignore"):
        s = _row_sums32(c) / F(V - 1)
        nan = np.isnan(s)
        s = np.where(s < F(-1.0), F(-1.0), np.where(s > F(1.0), F(1.0), s)).astype(F)
        lin = F(0.8) * (s + F(1.0))
        log = (0.54 * (np.log(2.0 + s.astype(np.float64)) / np.log(3.0)) + 0.46).astype(F)
        w = np.where(s < F(0.0), lin, log).astype(F)
    return np.where(nan, F(0.0), w).astype(F)


def select_weights32(c, threshold):
    """identify_consistent_views: 1.0 where at least two OTHER views reach the threshold (fp32 comparison), else 0.0."""
    c = np.asarray(c, dtype=F)
    P, V = c.shape[:2]
    k = np.zeros((V, P), dtype=np.int64)
    with np.errstate(all="ignore"):
        for a in range(V):
            for b in range(V):
                if b != a:
                    k[a] += c[:, a, b] >= F(threshold)
    return (k >= 2).astype(F)


def merged32(g, w, mode):
    """The step's xyz gradient from the slots and the weights the kernel exported, in the kernel's order."""
    g, w = np.asarray(g, dtype=F), np.asarray(w, dtype=F)
    V, P = g.shape[:2]
    acc = np.zeros((P, 3), dtype=F)
    with np.errstate(all="ignore"):
        if mode == "scale":
            for a in range(V):
                acc = acc + w[a][:, None] * g[a]
            return acc / F(V)
        plain = np.zeros((P, 3), dtype=F)
        n = np.zeros(P, dtype=np.int64)
        for a in range(V):
            plain = plain + g[a]
            keep = w[a] != 0
            acc = np.where(keep[:, None], acc + g[a], acc)
            n += keep
        return np.where((n >= 1)[:, None], acc / np.maximum(n, 1).astype(F)[:, None], plain / F(V)).astype(F)


def view_weighting32(g, mode, threshold=0.5):
    c = similarity32(g)
    w = scale_weights32(c) if mode == "scale" else select_weights32(c, threshold)
    return {"similarity": c, "weights": w, "merged": merged32(g, w, mode)}


def view_weighting64(g, mode, threshold=0.5):
    """The same definition in float64 (threshold compared as the float32 number the C argument is)."""
    g = np.asarray(g, dtype=np.float64)
    V, P = g.shape[:2]
    with np.errstate(all="ignore"):
        n = np.sqrt((g * g).sum(-1)) + 1e-8
        u = g / n[..., None]
        c = np.einsum("apk,bpk->pab", u, u)
        c[:, np.arange(V), np.arange(V)] = 1.0
        off = c.sum(2) - 1.0                                  # (P,V)
        if mode == "scale":
            if V < 2:
                w = np.ones((V, P))
            else:
                s = np.clip(off / (V - 1), -1.0, 1.0).T
                w = np.where(s < 0, 0.8 * (s + 1.0), 0.54 * (np.log(2.0 + np.maximum(s, 0.0)) / np.log(3.0)) + 0.46)
                w = np.where(np.isnan(s), 0.0, w)
            merged = (w[..., None] * g).sum(0) / V
        else:
            k = (c >= float(F(threshold))).sum(2) - 1         # (P,V)
            w = (k >= 2).T.astype(np.float64)
            cnt = w.sum(0)
            merged = np.where((cnt >= 1)[:, None], (w[..., None] * g).sum(0) / np.maximum(cnt, 1)[:, None], g.mean(0))
    return {"similarity": c, "weights": w, "merged": merged}


def weight_allowance(c64, V):
    """Units of 2**-24 a float32 `scale` weight may differ from the float64 one by: the cosines' roundings summed into s
    (their mean: K_COS each, averaged), s's own, and the weight's."""
    return K_COS + K_S(V) + K_W
