"""TEST INFRASTRUCTURE -- float64 references for ONE call of the loop's device tail and of the heat-map factors' impulse
response, CPU only.  Nothing here loads the HIP library; the pieces are the ones the CPU suite already pins to the
reference's goldens (loop.limb_3d_consistency_loss, scene.get_expon_lr_func, loop.OptEarlyStopping, torch.optim.Adam,
scipy's `reflect` rule), and tests/test_tail_ref_cpu.py holds what is restated here to them.

Every reference returns, next to its float64 values, the ROUNDING ALLOWANCE of the fp32 kernel it stands for, in units of
2**-24: (number of fp32 roundings on the path, counted from the kernel source) x (the reference's own sum of |terms| of the
output), with the allowances of a stage's inputs carried forward to first order.  The counts are the K_* constants below;
a kernel is held to `|got - want| <= 2**-24 * allowance`, and the tests print the largest observed / allowed ratio.

Transcendentals: the HIP math API reference (ROCm documentation, "HIP math API", table of single-precision functions,
column "Maximum ULP difference") states 1 ulp for expf; one fp32 ulp is at most 2 x 2**-24 of the value, so an expf counts
as 2.  The double-precision exp / sin / pow / sqrt / log of the LR schedule and the bias corrections (1-2 ulp of a double
in the same reference) are 2**-29 of a unit and count as 0; the rounding of their result to float counts as 1.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24
H36M_LIMB = (12, 13, 15, 16, 5, 6, 2, 3)     # l_arm, r_arm, l_leg, r_leg pairs of a 17-joint skeleton (scene.DATASETS)

# ---- k_loop_pack (csrc/sks_loop.hip), roundings per output -------------------------------------------------------------
K_SC = 1          # sc = (float)(1.0 / n): one rounding of a double quotient
K_EXPF = 2        # expf: 1 ulp (HIP math API reference) = 2 units of 2**-24
K_PACK_XYZ = K_SC + 1                    # g * sc
K_PACK_SCALING = K_EXPF + 2 + K_SC       # g * expf(raw) * sc
# nn = sum of 4 squares (4 mul + 3 add), sqrtf, q / nrm, dot (4 mul + 3 add), q * dot, gq - ., / nrm, * sc, sc
K_PACK_ROTATION = 7 + 1 + 1 + 7 + 1 + 1 + 1 + 1 + K_SC
# s = 1 / (1 + expf(-x)): expf, add, divide; 1 - s; s * (1 - s); g * .; * sc; sc.  Term scale |g| * s (1 - s cancels)
K_PACK_OPACITY = K_EXPF + 1 + 1 + 1 + 1 + 1 + 1 + K_SC

# ---- adam_block_finish / adam_update (csrc/sks_loop_dev.h) ---------------------------------------------------------------
# limb gradient of one pair at one joint: d = x0 - x1 (1), len^2 = 3 mul + 2 add (5), sqrtf (1), d / len (1), w * dir (1);
# gc += (1 per pair the joint sits in, at most 2); slot = gr + gc (1)
K_LIMB = 1 + 5 + 1 + 1 + 1
K_SLOT = K_LIMB + 2 + 1
# mean: V - 1 additions that round (the first one adds to 0) and the division by (float)V
K_MEAN = lambda V: (V - 1) + 1
K_M = 3 + 1       # m + w1 * (g - m): subtract, multiply, add -- and w1 = (float)(1 - beta1)
K_V = 4 + 2       # v * b2 + w2 * (g * g): three multiplies, one add -- and b2, w2 rounded to float
K_SQRT = 1
K_Q = 1 + 1       # sqrtf(v) / bc2_sqrt: bc2_sqrt rounded to float, the division
K_DENOM = 1 + 1   # + eps: the addition, eps rounded to float
K_T = 1           # m / denom
K_U = 1 + 1       # step_size * .: the step size rounded to float, the multiplication
K_P = 1           # param - .


def pairs_kept(limb, missing=()):
    """Which of the two limb-symmetry pairs (arms: limb[0:4], legs: limb[4:8]) the loss keeps: a pair that touches an
    UNOBSERVED joint (`missing`; DESIGN.md "Unobserved joints") is left out of the loss and of every gradient."""
    missing = set(int(p) for p in missing)
    return tuple(not (set(limb[4 * h:4 * h + 4]) & missing) for h in range(2))


def limb_loss(xyz, limb, missing=()):
    """loop.limb_3d_consistency_loss (utils/loss_utils.py:226-250) for any four joint pairs `limb` (8 indices); the CPU suite
    holds it to that function on the datasets' own pairs.  `missing`: see pairs_kept; the lengths of a pair that is left out
    are never formed (its rows of `xyz` may hold NaN)."""
    n = lambda a, b: torch.norm(xyz[a] - xyz[b], dim=-1)
    if not missing:
        return torch.norm(n(limb[0], limb[1]) - n(limb[2], limb[3])) + torch.norm(n(limb[4], limb[5]) - n(limb[6], limb[7]))
    total = torch.zeros((), dtype=xyz.dtype)
    for h, kept in enumerate(pairs_kept(limb, missing)):
        if kept:
            total = total + torch.norm(n(limb[4 * h], limb[4 * h + 1]) - n(limb[4 * h + 2], limb[4 * h + 3]))
    return total


def _limb_grad(xyz64, lam32, limb, missing=()):
    """(gradient of float32(lambda) x limb loss wrt xyz, its sum of |terms|), (P,3) float64 each."""
    P = xyz64.shape[0]
    kept = pairs_kept(limb, missing) if limb is not None else (False, False)
    if limb is None or float(lam32) == 0.0 or not any(kept):
        return torch.zeros((P, 3), dtype=torch.float64), torch.zeros((P, 3), dtype=torch.float64)
    x = xyz64.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(limb_loss(x, limb, missing) * float(lam32), x)
    # |terms|: a joint's gradient is a sum of +-lambda * unit vectors, one per pair it ends; same sum with every sign +
    mag = torch.zeros((P, 3), dtype=torch.float64)
    for k in range(4):
        if not kept[k // 2]:
            continue
        d = xyz64[limb[2 * k]] - xyz64[limb[2 * k + 1]]
        ln = d.norm()
        if float(ln) > 0.0:
            mag[limb[2 * k]] += abs(float(lam32)) * (d / ln).abs()
            mag[limb[2 * k + 1]] += abs(float(lam32)) * (d / ln).abs()
    return g, mag


def pack_ref(g_means, g_scales, g_rots, g_opac, raw_scaling, raw_rotation, raw_opacity, sums=None):
    """sks_loop_pack_grads in float64: autograd through exp / F.normalize / sigmoid of sum(g_act * activated), times
    1 / max(N_v, 1).  g_*: (V,P,.) gradients wrt the activated tensors, raw_*: (P,.), sums: (V,2) {S, N} or None.
    Returns (packed (V,P,11), allowance (V,P,11) in units of 2**-24)."""
    d = lambda t: torch.as_tensor(t).detach().cpu().to(torch.float64)
    gm, gs, gr, go = d(g_means), d(g_scales), d(g_rots), d(g_opac)
    V, P = gm.shape[0], gm.shape[1]
    go = go.reshape(V, P)
    # (one copy of the raw parameters per view, so that one backward gives every view's own gradient)
    rs = d(raw_scaling).reshape(1, P, 3).repeat(V, 1, 1).requires_grad_(True)
    rq = d(raw_rotation).reshape(1, P, 4).repeat(V, 1, 1).requires_grad_(True)
    ro = d(raw_opacity).reshape(1, P).repeat(V, 1).requires_grad_(True)
    sc = torch.ones(V, dtype=torch.float64) if sums is None else 1.0 / d(sums)[:, 1].clamp_min(1.0)
    L = ((gs * torch.exp(rs)).sum(dim=(1, 2)) + (gr * F.normalize(rq, dim=-1)).sum(dim=(1, 2)) + (go * torch.sigmoid(ro)).sum(dim=1)) * sc
    d_s, d_q, d_o = torch.autograd.grad(L.sum(), (rs, rq, ro))
    packed = torch.cat([gm * sc[:, None, None], d_s, d_q, d_o[:, :, None]], dim=2)
    # sums of |terms|
    scv = sc[:, None, None]
    ksc = K_SC if sums is not None else 0          # (sc is the constant 1.0f without sums: its products are exact)
    q = d(raw_rotation)
    nrm = q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    qh = (q / nrm)[None]
    t_rot = (gr.abs() + qh.abs() * (qh * gr).abs().sum(-1, keepdim=True)) / nrm[None] * scv
    t_opa = (go.abs() * torch.sigmoid(d(raw_opacity).reshape(1, P)))[:, :, None] * scv
    allow = torch.cat([(K_PACK_XYZ - K_SC + ksc) * (gm * scv).abs(), (K_PACK_SCALING - K_SC + ksc) * d_s.abs(),
                       (K_PACK_ROTATION - K_SC + ksc) * t_rot, (K_PACK_OPACITY - K_SC + ksc) * t_opa], dim=2)
    return packed.detach(), allow


def lr_ref(sched, iteration):
    """The xyz learning rate of sks_loop_adam_step's `lr_sched` (init, final, delay_mult, delay_steps, max_steps) at
    `iteration`: scene.get_expon_lr_func, the function the CPU suite pins to the reference's golden schedules."""
    from skelsplat_amd.scene import get_expon_lr_func
    with np.errstate(divide="ignore", invalid="ignore"):
        return get_expon_lr_func(sched[0], sched[1], lr_delay_steps=int(sched[3]), lr_delay_mult=sched[2],
                                 max_steps=int(sched[4]))(int(iteration))


def adam_step_ref(grads, slots, group_mask, last_view, params, exp_avg, exp_avg_sq, counters, acc_steps, sched, lrs, adam,
                  lam, limb, missing=()):
    """ONE sks_loop_adam_step call in float64 from the state BEFORE it.  grads (V,P,11), slots (V,P,3), params = (xyz (P,3),
    scaling (P,3), rotation (P,4), opacity (P,1)), exp_avg / exp_avg_sq (P,11), counters = (iteration, adam steps); `lam` is
    rounded to float32 like the C argument.  Returns a dict of (value, allowance in units of 2**-24) pairs for
    "slots", "m", "v", "xyz", "scaling", "rotation", "opacity", and "counters" (ints).
    `missing`: unobserved joints (pairs_kept) -- their rows of xyz hold NaN and stay NaN (compared as such), a limb pair that
    touches one adds nothing to any joint's gradient; the rounding counts of every other row are what they are without it."""
    d = lambda t: torch.as_tensor(t).detach().cpu().to(torch.float64)
    grads, slots, m0, v0 = d(grads), d(slots).clone(), d(exp_avg), d(exp_avg_sq)
    prm = [d(p) for p in params]
    V, P = grads.shape[0], grads.shape[1]
    lam32 = np.float32(lam)
    # slots of the views in the mask <- this group's xyz gradient + the limb gradient (train.py:150-152,175)
    gc, gc_mag = _limb_grad(prm[0], lam32, limb, missing)
    slot_allow = torch.zeros_like(slots)
    for v in range(V):
        if (group_mask >> v) & 1:
            slots[v] = grads[v, :, :3] + gc
            slot_allow[v] = K_SLOT * (grads[v, :, :3].abs() + gc_mag) if float(gc_mag.abs().sum()) > 0.0 else 0.0
    # gradient of the step: mean of the V slots; the last view's scaling / rotation / opacity rows (quirk Q7)
    g = torch.cat([slots.mean(0), grads[last_view, :, 3:]], dim=1)                              # (P,11)
    g_allow = torch.zeros_like(g)
    g_allow[:, :3] = slot_allow.sum(0) / V + K_MEAN(V) * slots.abs().sum(0) / V
    # torch.optim.Adam in float64 with the moments and the step count loaded into its state
    it1, step0 = int(counters[0]) + int(acc_steps), int(counters[1])
    lr_xyz = lr_ref(sched, it1)
    leaves = [p.clone().requires_grad_(True) for p in prm]
    opt = torch.optim.Adam([{"params": [leaves[0]], "lr": lr_xyz}, {"params": [leaves[1]], "lr": lrs[0]},
                            {"params": [leaves[2]], "lr": lrs[1]}, {"params": [leaves[3]], "lr": lrs[2]}],
                           betas=(adam[0], adam[1]), eps=adam[2], foreach=False)
    cols = [(0, 3), (3, 6), (6, 10), (10, 11)]
    for leaf, (a, b) in zip(leaves, cols):
        leaf.grad = g[:, a:b].clone()
        opt.state[leaf] = {"step": torch.tensor(float(step0)), "exp_avg": m0[:, a:b].clone(), "exp_avg_sq": v0[:, a:b].clone()}
    opt.step()
    m1 = torch.cat([opt.state[l]["exp_avg"] for l in leaves], dim=1)
    v1 = torch.cat([opt.state[l]["exp_avg_sq"] for l in leaves], dim=1)
    p0, p1 = torch.cat(prm, dim=1), torch.cat([l.detach() for l in leaves], dim=1)
    # allowances, first-order propagation through adam_update (absolute, units of 2**-24)
    step = step0 + 1
    w1, b2, w2, eps = 1.0 - adam[0], adam[1], 1.0 - adam[1], adam[2]
    bc1, bc2s = 1.0 - adam[0] ** step, math.sqrt(1.0 - adam[1] ** step)
    ss = torch.tensor([lr_xyz] * 3 + [lrs[0]] * 3 + [lrs[1]] * 4 + [lrs[2]], dtype=torch.float64) / bc1
    e_m = K_M * (m0.abs() + w1 * (g.abs() + m0.abs())) + w1 * g_allow
    e_v = K_V * (b2 * v0 + w2 * g * g) + w2 * 2.0 * g.abs() * g_allow
    r = v1.sqrt()
    e_r = torch.where(r > 0, e_v / (2.0 * r).clamp_min(1e-300), torch.zeros_like(r)) + K_SQRT * r
    qd = r / bc2s
    e_q = e_r / bc2s + K_Q * qd
    den = qd + eps
    e_d = e_q + K_DENOM * den
    t = m1 / den
    e_t = e_m / den + t.abs() * e_d / den + K_T * t.abs()
    u = ss * t
    e_u = ss.abs() * e_t + K_U * u.abs()
    e_p = e_u + K_P * (p0.abs() + u.abs())
    finite = lambda x: torch.nan_to_num(x, nan=0.0, posinf=0.0)       # (a NaN / inf reference is compared as such, not by bound)
    out = {"slots": (slots, slot_allow), "m": (m1, finite(e_m)), "v": (v1, finite(e_v)), "counters": (it1, step)}
    for name, (a, b) in zip(("xyz", "scaling", "rotation", "opacity"), cols):
        out[name] = (p1[:, a:b], finite(e_p[:, a:b]))
    return out


def es_losses(sums, cons=0.0):
    """The fp32 loss the criterion sees for a view's {S, N} (float64) and the limb term lambda x loss:
    float32(S / max(N, 1)) + float32(cons), added in fp32."""
    S, N = float(sums[0]), float(sums[1])
    with np.errstate(invalid="ignore"):
        return float(np.float32(np.float32(S / max(N, 1.0)) + np.float32(cons)))


class EsRef:
    """The host OptEarlyStopping (the class the CPU suite pins to the reference's golden decisions), fed one loss at a time;
    `stopped_at` is the 1-based iteration at which it first fired, or 0."""

    def __init__(self, window, tol):
        from skelsplat_amd.loop import OptEarlyStopping
        self.crit = OptEarlyStopping(window_size=window, repeat_tolerance=tol)
        self.n, self.stopped_at = 0, 0

    def feed(self, loss):
        self.n += 1
        if not self.stopped_at and self.crit(float(loss)):
            self.stopped_at = self.n
        return self.stopped_at


def es_ref(losses, window, tol):
    """EsRef over a whole sequence: the 1-based iteration at which the criterion first fires, or 0."""
    ref = EsRef(window, tol)
    for x in losses:
        if ref.feed(x):
            break
    return ref.stopped_at


def reflect_index(i, n):
    """scipy.ndimage's `reflect` extension (d c b a | a b c d | d c b a): the sample of a length-n line that position i of
    the infinitely extended line shows, for any integer i."""
    i = np.asarray(i, dtype=np.int64) % (2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def impulse_ref(n, p, sigma):
    """scipy.ndimage.gaussian_filter1d(unit impulse at p of a length-n line, sigma, mode='reflect', truncate=4.0) by its
    definition in float64: extend the line by the reflect index map as far as the kernel reaches -- however many bounces that
    takes -- and correlate with the normalised truncated kernel of radius floor(4 sigma + 0.5).  Returns ((n,) float64, radius)."""
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5)
    j = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 * j * j / (sigma * sigma)) if radius > 0 else np.ones(1)
    w = w / w.sum()
    line = np.zeros(n, dtype=np.float64)
    line[p] = 1.0
    ext = line[reflect_index(np.arange(-radius, n + radius), n)]          # ext[k] = extended line at k - radius
    out = np.array([np.dot(w, ext[i:i + 2 * radius + 1]) for i in range(n)])
    return out, radius
