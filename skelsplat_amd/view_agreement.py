"""View agreement in tensor ops: the definition of include/skelsplat_hip.h ("View agreement") -- the reference's
utils/similarity_utils.py pairwise_cosine_similarity, compute_scaling_weights / weight_function and identify_consistent_views, with
the divisor V - 1 and the clamp -- one fp32 operation per line of it and in its order, so that on the CPU it gives the bits the
device kernel gives (up to the device's double log).  What the loops' tensor-op tail runs (custom loss_grad, view_grad_fn, no
device_tail); the device tail runs it inside sks_loop_adam_step_vw / sks_loop_fused_step_vw."""
import math

import torch

MODES = ("scale", "select")


def check_mode(view_weighting):
    if view_weighting is not None and view_weighting not in MODES:
        raise ValueError(f"view_weighting = {view_weighting!r}: expected None, 'scale' or 'select'")
    return view_weighting


def pairwise_cosine_similarity(slots):
    """slots (V,P,3) float32 -> (P,V,V): c_ab = (u_a0 u_b0 + u_a1 u_b1) + u_a2 u_b2 of u = g / (|g| + 1e-8), diagonal 1."""
    g = slots
    V = g.shape[0]
    # (torch's float32 sqrt on the CPU is not correctly rounded; the double one rounded to float is: 53 >= 2 x 24 + 2 bits)
    n = torch.sqrt(((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]).double()).to(g.dtype) + 1e-8
    u = g / n[..., None]
    prod = u[:, None] * u[None]                                    # (V,V,P,3)
    c = (prod[..., 0] + prod[..., 1]) + prod[..., 2]
    eye = torch.eye(V, dtype=torch.bool, device=g.device)[:, :, None]
    return torch.where(eye, torch.ones_like(c), c).permute(2, 0, 1).contiguous()


def scaling_weights(similarity):
    """(P,V,V) -> (V,P): weight_function of the mean cosine with the OTHER views (divisor V - 1, clamped to [-1, 1])."""
    c = similarity
    P, V = c.shape[0], c.shape[1]
    if V < 2:
        return torch.ones((V, P), dtype=c.dtype, device=c.device)
    s = torch.zeros((P, V), dtype=c.dtype, device=c.device)
    own = torch.eye(V, dtype=torch.bool, device=c.device)
    for b in range(V):                                             # ascending b, b != a (adding 0.0 where b == a is exact)
        s = s + torch.where(own[:, b][None], torch.zeros_like(s), c[:, :, b])
    s = s / float(V - 1)
    nan = torch.isnan(s)
    s = torch.where(s < -1.0, torch.full_like(s, -1.0), torch.where(s > 1.0, torch.full_like(s, 1.0), s))
    lin = 0.8 * (s + 1.0)
    log = (0.54 * (torch.log(2.0 + s.double()) / math.log(3.0)) + 0.46).to(c.dtype)
    w = torch.where(s < 0.0, lin, log)
    return torch.where(nan, torch.zeros_like(w), w).t().contiguous()


def consistent_views(similarity, threshold=0.5):
    """(P,V,V) -> (V,P) of 1.0 / 0.0: a view is kept when at least two OTHER views reach the threshold with it."""
    c = similarity
    V = c.shape[1]
    thr = torch.tensor(threshold, dtype=c.dtype, device=c.device)
    own = torch.eye(V, dtype=torch.bool, device=c.device)[None]
    k = ((c >= thr) & ~own).sum(dim=2)
    return (k >= 2).to(c.dtype).t().contiguous()


def merge(slots, weights, mode):
    """The step's xyz gradient (P,3): scale -- (sum_a w_a g_a) / V; select -- the mean of the kept views, the plain mean of all
    where none is kept.  Views in ascending order."""
    V = slots.shape[0]
    acc = torch.zeros_like(slots[0])
    if mode == "scale":
        for a in range(V):
            acc = acc + weights[a][:, None] * slots[a]
        return acc / float(V)
    plain = torch.zeros_like(slots[0])
    n = torch.zeros(slots.shape[1], dtype=slots.dtype, device=slots.device)
    for a in range(V):
        plain = plain + slots[a]
        keep = weights[a] != 0
        acc = torch.where(keep[:, None], acc + slots[a], acc)
        n = n + keep.to(n.dtype)
    return torch.where((n >= 1)[:, None], acc / n.clamp_min(1.0)[:, None], plain / float(V))


def weighted_mean(slots, mode, threshold=0.5):
    """slots (V,P,3) -> (xyz gradient (P,3), weights (V,P), similarity (P,V,V))."""
    c = pairwise_cosine_similarity(slots)
    w = scaling_weights(c) if mode == "scale" else consistent_views(c, threshold)
    return merge(slots, w, mode), w, c
