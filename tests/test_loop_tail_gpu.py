"""The loop's device tail (sks_loop_pack_grads, sks_loop_adam_step, the early-stopping criterion) and sks_heatmap_factors, ONE
call at a time against the float64 references of tests/tail_ref.py, at the shapes, schedules and edges the loop tests never
visit.  Allowances are computed (tail_ref: roundings counted from the kernel x the reference's own sum of |terms|), never
chosen; every test prints the largest observed / allowed ratio per output (MEASUREMENTS.md, "loop tail against fp64")."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import tail_ref, util

pytestmark = pytest.mark.gpu

EPS32 = tail_ref.EPS32
LRS = (0.005, 0.001, 0.05)
ADAM = (0.9, 0.999, 1e-15)


def _dbl(vals):
    return (ctypes.c_double * len(vals))(*[float(v) for v in vals])


def _ints(vals):
    return None if vals is None else (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _held(name, got, want, allow, seen):
    """|got - want| <= 2**-24 * allow elementwise (allow == 0: equal; a non-finite reference: the same non-finite value);
    records the largest observed / allowed ratio under `name`."""
    got = got.detach().cpu().to(torch.float64).reshape(want.shape)
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{name}: NaNs differ"
    assert torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)]), f"{name}: infinities differ"
    err = (got - want).abs()[fin]
    tol = (EPS32 * allow)[fin]
    exact = tol == 0
    assert float(err[exact].sum()) == 0.0 if bool(exact.any()) else True, f"{name}: differs where nothing rounds"
    ratio = float((err[~exact] / tol[~exact]).max()) if bool((~exact).any()) else 0.0
    seen[name] = max(seen.get(name, 0.0), ratio)
    assert ratio <= 1.0, f"{name}: error is {ratio:.2f} x the counted rounding allowance"


def _report(title, seen):
    print(f"\n[{title}] observed / allowed: " + ", ".join(f"{k} {v:.3f}" for k, v in seen.items()))


# ------------------------------------------------------------------------------------------------ sks_loop_pack_grads
@pytest.mark.parametrize("with_sums", [True, False], ids=["sums", "no-sums"])
@pytest.mark.parametrize("V,P", [(1, 1), (4, 17), (64, 4), (3, 256)])
def test_pack_grads_against_fp64_autograd(device, V, P, with_sums):
    from skelsplat_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 * V + P)
    r = lambda *s: torch.randn(s, generator=g)
    gm, gs, gr, go = r(V, P, 3), r(V, P, 3), r(V, P, 4), r(V, P)
    raw_s = (torch.rand((P, 3), generator=g) * 16.0 - 8.0)
    raw_s.view(-1)[0], raw_s.view(-1)[-1] = 8.0, -8.0
    raw_o = r(P) * 4.0
    for k, x in enumerate((15.0, -15.0, 0.0)):
        if k < P:
            raw_o[(k * 7) % P] = x
    if P == 1:
        raw_o[0] = 15.0 if with_sums else -15.0
    # quaternion norms from 1e-3 to 1e3 (their fp32 squares stay normal numbers), one exactly zero quaternion
    q = r(P, 4)
    q = q / q.norm(dim=1, keepdim=True) * (10.0 ** torch.linspace(-3.0, 3.0, P))[:, None]
    if P > 1:
        q[P // 2] = 0.0
    sums = None
    if with_sums:
        sums = torch.stack([r(V).abs().double() * 50.0, torch.tensor([float((3 + 997 * v) % 1500 + 1) for v in range(V)]).double()], 1)
        sums[V // 2, 1] = 0.0            # a view without a live pixel: N < 1 clamps to 1
    want, allow = tail_ref.pack_ref(gm, gs, gr, go, raw_s, q, raw_o, sums)
    dv = lambda t: t.contiguous().to(device)
    d = [dv(t) for t in (gm, gs, gr, go, raw_s, q, raw_o)]
    d_sums = None if sums is None else dv(sums)
    out = torch.full((V, P, 11), float("nan"), device=device)
    _lib.check(lib.sks_loop_pack_grads(V, P, *[t.data_ptr() for t in d], _lib.ptr(d_sums), out.data_ptr(),
                                       torch.cuda.current_stream(device).cuda_stream), "sks_loop_pack_grads")
    seen = {}
    for name, (a, b), k in (("xyz", (0, 3), tail_ref.K_PACK_XYZ), ("scaling", (3, 6), tail_ref.K_PACK_SCALING),
                            ("rotation", (6, 10), tail_ref.K_PACK_ROTATION), ("opacity", (10, 11), tail_ref.K_PACK_OPACITY)):
        _held(f"{name} (K {k})", out[:, :, a:b], want[:, :, a:b], allow[:, :, a:b], seen)
    _report(f"pack V={V} P={P} {'sums' if with_sums else 'no sums'}", seen)
    # the cases are what they claim: the zero quaternion's row is g / 1e-12, the saturated logits barely pass anything
    if P > 1:
        assert float(want[:, P // 2, 6:10].abs().max()) > 1e6 and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------ sks_loop_adam_step
SCHEDULES = {"plain": (2.0, 0.02, 0.0, 0.0, 4000.0), "delay": (2.0, 0.02, 0.01, 1000.0, 4000.0),
             "off": (0.0, 0.0, 0.0, 0.0, 4000.0), "zero-init": (0.0, 0.02, 0.01, 0.0, 4000.0)}
# (mask, last view) kind, counters at the start, schedule, lambda, limb kind: every value of every axis, the delay ramp from
# inside (iterations 4 .. 12) and from past its end, lambda 1 with every skeleton
CONFIGS = [("full", (0, 0), "plain", 0.0, "none"), ("missing", (0, 0), "delay", 1e-5, "h36m"),
           ("lastbit", (3990, 997), "delay", 1.0, "twice"), ("full", (3990, 997), "plain", 1.0, "coincident"),
           ("missing", (0, 0), "off", 1.0, "equal"), ("lastbit", (0, 0), "zero-init", 1e-5, "twice"),
           ("full", (0, 0), "delay", 1.0, "h36m"), ("missing", (3990, 997), "plain", 1e-5, "none"),
           # an UNOBSERVED joint (DESIGN.md "Unobserved joints": its xyz row is NaN, its gradient rows and slots are 0, as the
           # rasterizer and new_scene(s) leave them) on an arm, on a leg, on no limb: the row keeps its NaN and its zero moments,
           # every other row is held to tail_ref.adam_step_ref(missing=) at the allowances counted above -- a NaN adds no rounding
           ("full", (0, 0), "plain", 1.0, "nan-arm"), ("missing", (0, 0), "delay", 1e-5, "nan-leg"),
           ("lastbit", (0, 0), "plain", 1.0, "nan-none")]
NAN_JOINT = {"nan-arm": 12, "nan-leg": 5, "nan-none": 9}
SHAPES = [(1, 1), (4, 17), (8, 64), (9, 64), (31, 19), (64, 4), (64, 64), (2, 256)]
ACC = 4


def _mask_of(kind, V):
    if kind == "full" or V == 1:
        return (1 << V) - 1, 0
    if kind == "missing":
        return (1 << V) - 1 - (1 << (1 % V)), V // 2
    return 1 << (V - 1), V - 1


def _missing_of(kind, P):
    """the unobserved joints of a limb kind: () or one index"""
    return (NAN_JOINT[kind] % P,) if kind in NAN_JOINT else ()


def _bits(t):
    """a tensor's bits (NaN == NaN where the bits agree)"""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _skeleton(kind, P, g):
    """(limb or None, xyz (P,3) fp32 at limb scale: hundreds of mm)"""
    xyz = torch.randn((P, 3), generator=g) * 300.0
    if kind == "none":
        return None, xyz
    if kind == "h36m" or kind in NAN_JOINT:
        limb = tail_ref.H36M_LIMB if P >= 17 else tuple(i % P for i in (0, 1, 2, 3, 1, 2, 3, 0))
        if kind in NAN_JOINT:
            xyz[_missing_of(kind, P)[0]] = float("nan")
    elif kind == "twice":        # joint 0 starts both arm pairs, joint 3 ends both leg pairs
        limb = tuple(i % P for i in (0, 1, 0, 2, 1, 3, 2, 3))
    else:
        limb = tuple(i % P for i in range(8))
        if kind == "coincident" and P >= 2:       # a limb of length 0: its direction is taken as 0
            xyz[limb[1]] = xyz[limb[0]]
        if kind == "equal" and P >= 8:            # mirrored arms with exactly representable coordinates: len[0] == len[1]
            xyz[limb[0]], xyz[limb[1]] = torch.tensor([10.0, 20.0, 30.0]), torch.tensor([110.0, 60.0, 5.0])
            xyz[limb[2]], xyz[limb[3]] = torch.tensor([-10.0, 20.0, 30.0]), torch.tensor([-110.0, 60.0, 5.0])
    return limb, xyz


class _State:
    """The buffers of one optimiser on the device; `snap()` = their values on the host."""

    def __init__(self, device, V, P, xyz, counters, g, es_window=0):
        r = lambda *s: torch.randn(s, generator=g)
        warm = counters[1] > 0
        host = [xyz, r(P, 3), r(P, 4), r(P, 1), r(V, P, 3), (r(P, 11) * 0.1) if warm else torch.zeros(P, 11),
                (r(P, 11) * 0.1) ** 2 if warm else torch.zeros(P, 11)]
        self.t = [x.contiguous().to(device) for x in host]
        self.cnt = torch.tensor(counters, dtype=torch.int32, device=device)
        self.es = torch.zeros(2 + 2 * es_window, dtype=torch.int32, device=device) if es_window else None
        self.flag = torch.zeros(1, dtype=torch.int32).pin_memory() if es_window else None

    def snap(self):
        torch.cuda.synchronize()
        return [x.cpu().clone() for x in self.t] + [self.cnt.cpu().clone()]

    def ptrs(self):          # slots | xyz scaling rotation opacity exp_avg exp_avg_sq counters
        xyz, sc, ro, op, slots, m, v = self.t
        return (slots.data_ptr(),), (xyz.data_ptr(), sc.data_ptr(), ro.data_ptr(), op.data_ptr(), m.data_ptr(), v.data_ptr(),
                                     self.cnt.data_ptr())


def _check_step(before, after, grads, mask, last, acc, sched, lam, limb, seen, V, missing=()):
    """one call's outputs (`after`) against adam_step_ref run from the state `before`"""
    xyz, sc, ro, op, slots, m, v, cnt = before
    ref = tail_ref.adam_step_ref(grads, slots, mask, last, (xyz, sc, ro, op), m, v, (int(cnt[0]), int(cnt[1])), acc, sched,
                                 LRS, ADAM, lam, limb, missing=missing)
    for j in missing:       # the unobserved row: still NaN, moments exactly 0, scaling / rotation / opacity untouched
        assert bool(torch.isnan(after[0][j]).all()) and not after[5][j].any() and not after[6][j].any()
        assert all(torch.equal(after[i][j], before[i][j]) for i in (1, 2, 3))
    assert (int(after[7][0]), int(after[7][1])) == ref["counters"]
    for name, i in (("slots", 4), ("m", 5), ("v", 6), ("xyz", 0), ("scaling", 1), ("rotation", 2), ("opacity", 3)):
        _held(name, after[i], ref[name][0], ref[name][1], seen)
    for vv in range(V):     # a view outside the mask keeps its slot, bit for bit
        if not (mask >> vv) & 1:
            assert torch.equal(after[4][vv], before[4][vv])
    return ref


@pytest.mark.parametrize("cfg", range(len(CONFIGS)), ids=["-".join(str(x) for x in (c[0], c[1][0], c[2], c[3], c[4])) for c in CONFIGS])
@pytest.mark.parametrize("V,P", SHAPES)
def test_adam_step_against_fp64_torch_adam(device, V, P, cfg):
    """Three consecutive sks_loop_adam_step calls on one state, each held to tail_ref.adam_step_ref from the state before it;
    then the same three calls through sks_loop_adam_step_es with the criterion disarmed (tolerance 0): the same bits."""
    from skelsplat_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream(device).cuda_stream
    mask_kind, counters, sched_name, lam, limb_kind = CONFIGS[cfg]
    sched = SCHEDULES[sched_name]
    g = torch.Generator().manual_seed(1000 * cfg + 10 * V + P)
    limb, xyz = _skeleton(limb_kind, P, g)
    missing = _missing_of(limb_kind, P)
    mask, last = _mask_of(mask_kind, V)
    grads_h = torch.randn((V, P, 11), generator=g)
    grads_h[:, list(missing)] = 0.0
    grads = grads_h.to(device)
    c_sched, c_lrs, c_adam, c_limb = _dbl(sched), _dbl(LRS), _dbl(ADAM), _ints(limb)
    g_state = torch.Generator().manual_seed(7 + cfg)
    seen, finals = {}, []
    for entry in ("plain", "es"):
        g_state.manual_seed(7 + cfg)
        st = _State(device, V, P, xyz.clone(), counters, g_state, es_window=4 if entry == "es" else 0)
        st.t[4][:, list(missing)] = 0.0
        slots_p, rest_p = st.ptrs()
        sums = torch.tensor([[float(v + 1), 10.0] for v in range(V)], dtype=torch.float64, device=device)
        lrs_seen = []
        for call in range(3):
            before = st.snap() if entry == "plain" else None
            if entry == "plain":
                rc = lib.sks_loop_adam_step(V, P, grads.data_ptr(), *slots_p, mask, last, *rest_p, ACC, c_sched, c_lrs, c_adam,
                                            lam, c_limb, 1, stream)
            else:
                rc = lib.sks_loop_adam_step_es(V, P, grads.data_ptr(), *slots_p, mask, last, *rest_p, ACC, c_sched, c_lrs,
                                               c_adam, lam, c_limb, 1, sums.data_ptr(), st.es.data_ptr(), 4, 0.0,
                                               st.flag.data_ptr(), stream)
            _lib.check(rc, "sks_loop_adam_step")
            if entry == "plain":
                after = st.snap()
                _check_step(before, after, grads_h, mask, last, ACC, sched, lam, limb, seen, V, missing)
                lrs_seen.append(tail_ref.lr_ref(sched, int(after[7][0])))
        finals.append(st.snap())
        if entry == "plain":      # the case is what it claims
            if sched_name == "delay":
                full = [tail_ref.lr_ref(SCHEDULES["plain"], counters[0] + ACC * (k + 1)) for k in range(3)]
                inside = counters[0] == 0
                assert all((a < 0.1 * b) if inside else (a == b) for a, b in zip(lrs_seen, full)), (lrs_seen, full)
            if sched_name in ("off", "zero-init"):
                assert lrs_seen == [0.0, 0.0, 0.0] and torch.equal(finals[0][0], xyz)     # xyz stays; the moments moved
                assert not torch.equal(finals[0][5], torch.zeros(P, 11))
            if counters[0]:
                assert counters[0] + 2 * ACC < sched[4] < counters[0] + 3 * ACC           # the clip at t = 1 is crossed
        else:
            assert int(st.es[1]) == 0 and int(st.flag[0]) == 0 and int(st.es[0]) == 3 * ACC
    for k, (a, b) in enumerate(zip(*finals)):
        assert torch.equal(_bits(a), _bits(b)), ("xyz scaling rotation opacity slots m v counters".split()[k])
    wide = V > 8 and V * P * 3 <= 8192
    assert wide == ((V, P) in ((9, 64), (31, 19), (64, 4)))          # which slot path these shapes take (sks_loop_dev.h)
    _report(f"adam V={V} P={P} {CONFIGS[cfg]}", seen)


# ------------------------------------------------------------------------------------------------ the criterion
ES_TOL = 2.0 ** -10          # exactly representable: a pair of fp32 losses can differ by exactly the tolerance
ES_GROUPS = 40


def _loss_sequence(kind, w, n):
    """per-iteration target losses (float64, exactly representable where the case needs it)"""
    i = np.arange(n, dtype=np.float64)
    settle = 0.5 + 0.3 * np.exp(-i / 6.0)
    half = (np.arange(n) // w) % 2           # period 2w: every loss faces the other level one window earlier
    if kind in ("settle", "n0", "nan", "nan-limb"):
        return settle
    if kind == "oscillate":                  # 1.5 tolerances apart for five windows, then flat
        return np.where(np.arange(n) < 5 * w, 0.5 + 1.5 * ES_TOL * half, 0.5)
    assert kind == "tie"                     # exactly one tolerance apart, for ever: `<` never fires, `<=` fires at once
    return 0.5 + ES_TOL * half


@pytest.mark.parametrize("V,acc", [(4, 4), (4, 5), (7, 4), (7, 5)])
@pytest.mark.parametrize("w", [1, 3, 4, 16])
def test_early_stopping_against_the_host_criterion(device, w, V, acc):
    """sks_loop_adam_step_es over 40 groups of synthetic {S, N} against tail_ref.es_ref (the host OptEarlyStopping, one loss at a
    time): the stopping iteration, es_state[1], the host flag, the cut of the group it fires in (which views refreshed their
    slots, whose scaling / rotation / opacity rows won, the iteration counter), and nothing moves afterwards."""
    from skelsplat_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream(device).cuda_stream
    P = 17
    sched = (2e-3, 2e-4, 0.0, 0.0, 4000.0)            # (small steps: the limb term of the loss barely moves)
    c_sched, c_lrs, c_adam = _dbl(sched), _dbl(LRS), _dbl(ADAM)
    seen, stops = {}, {}
    for kind in ("settle", "oscillate", "tie", "n0", "nan", "nan-limb"):
        lam, limb = (1e-5, tail_ref.H36M_LIMB) if kind in ("settle", "nan-limb") else (0.0, None)
        # nan-limb: finite sums, lambda != 0 and an unobserved arm joint -- the arm pair is out of the loss the criterion sees as
        # it is out of the gradient, so the losses stay finite and the criterion fires where the host's does on the masked loss
        missing = (12,) if kind == "nan-limb" else ()
        g = torch.Generator().manual_seed(w * 100 + V * 10 + acc)
        xyz = torch.randn((P, 3), generator=g) * 300.0
        xyz[list(missing)] = float("nan")
        grads_h = torch.randn((V, P, 11), generator=g) * 1e-3
        grads_h[:, list(missing)] = 0.0
        grads = grads_h.to(device)
        st = _State(device, V, P, xyz, (0, 0), g, es_window=w)
        st.t[4][:, list(missing)] = 0.0
        slots_p, rest_p = st.ptrs()
        target = _loss_sequence(kind, w, ES_GROUPS * acc)
        N = 1024.0
        crit, stop, snap_after = tail_ref.EsRef(w, ES_TOL), 0, None
        after = st.snap()
        for k in range(ES_GROUPS):
            it0 = k * acc + 1
            views = [(it0 + j - 1) % V for j in range(acc)]
            sums = torch.zeros((V, 2), dtype=torch.float64)
            sums[:, 1] = N
            for j, v in enumerate(views):
                sums[v, 0] = N * target[it0 + j - 1]              # (a view seen twice in a group keeps its later sum)
            if kind == "n0":
                sums[1] = torch.tensor([0.25, 0.0])               # a view without a live pixel: the loss is S / 1
            if kind == "nan" and k == (2 * w + 3) // acc + 1:
                sums[views[0], 0] = float("nan")                  # one NaN loss: no window that holds it may fire
            mask = 0
            for v in views:
                mask |= 1 << v
            before = after
            # the limb term of every loss of the group, from the joints before the step: float32(lambda x limb loss)
            cons = np.float32(np.float32(lam) * float(tail_ref.limb_loss(before[0].double(), limb, missing))) if limb else 0.0
            assert np.isfinite(cons)
            d_sums = sums.to(device)
            _lib.check(lib.sks_loop_adam_step_es(V, P, grads.data_ptr(), *slots_p, mask, views[-1], *rest_p, acc, c_sched, c_lrs,
                                                 c_adam, lam, _ints(limb), 1, d_sums.data_ptr(), st.es.data_ptr(), w, ES_TOL,
                                                 st.flag.data_ptr(), stream), "sks_loop_adam_step_es")
            after = st.snap()
            if stop:                                              # launches behind the stop change nothing
                for a, b in zip(snap_after, after):
                    assert torch.equal(_bits(a), _bits(b)), (kind, k)
                assert int(st.es[1]) == int(st.flag[0]) == stop
                continue
            want = 0
            for v in views:
                want = want or crit.feed(tail_ref.es_losses(sums[v], cons))
            assert int(st.flag[0]) == int(st.es[1]) == want, (kind, k, int(st.flag[0]), want)
            if want:
                stop, n_it = want, want - it0 + 1
                assert 1 <= n_it <= acc and int(after[7][0]) == stop and int(st.es[0]) == stop
                cut_mask = 0
                for v in views[:n_it]:
                    cut_mask |= 1 << v
                _check_step(before, after, grads_h, cut_mask, views[n_it - 1], n_it, sched, lam, limb, seen, V, missing)
                snap_after = after
            else:
                assert int(after[7][0]) == it0 + acc - 1 and int(st.es[0]) == it0 + acc - 1
                if k % 13 == 0:
                    _check_step(before, after, grads_h, mask, views[-1], acc, sched, lam, limb, seen, V, missing)
        stops[kind] = stop
        if kind == "tie" and acc <= V:
            assert stop == 0              # |h1 - h2| == tolerance in every pair: strictly-less never holds
        if kind in ("settle", "oscillate", "nan-limb"):
            assert stop >= 2 * w
        if kind == "nan":
            assert stop == 0 or stop >= 2 * w
    assert stops["settle"] > 0 and stops["nan-limb"] > 0, stops        # (a NaN limb term would never let the criterion fire)
    print(f"\n[es w={w} V={V} acc={acc}] stopped at {stops}")
    _report(f"es cut w={w} V={V} acc={acc}", seen)


# ------------------------------------------------------------------------------------------------ the delay ramp, production paths
def test_delay_ramp_through_the_fused_step_and_the_rig_bank(device):
    """No configuration ships a delayed schedule, so the bit-identity tests of the production paths never ran the sine ramp of
    adam_block_begin: 8 groups of the smallest scene those tests use (160x128, 4 views) with delay_steps 1000, delay_mult 0.01
    through sks_loop_fused_step and -- schedule rows from a rig bank -- sks_loop_fused_step_dv, each bit for bit the separate
    sks_loop_adam_step sequence."""
    from skelsplat_amd.loop import MultiViewLoop, FrameBatchLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.rigs import RigBank
    from tests.test_ops_gpu import _make_loop_scene
    sc, model = _make_loop_scene(device, seed=17)
    iters = 32
    p2d = torch.tensor(sc.poses_2d, device=device)

    def delayed(gm, on=True):
        if on:
            gm.opt_cfg["lr_delay_steps"], gm.opt_cfg["lr_delay_mult"] = 1000, 0.01
        return gm

    def state(xyz, scaling, rotation, opacity, counters):
        torch.cuda.synchronize()
        return [t.detach().reshape(-1).clone() for t in (xyz, scaling, rotation, opacity, counters)]

    res = {}
    for name, fused, delay in (("separate", False, True), ("fused", True, True), ("fused-plain", True, False)):
        gm = delayed(model(device), delay)
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(), p2d, sc.cameras)
        loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", sparse=True, fused_tail=fused)
        assert loop.fused_tail == fused and loop._sched[3] == (1000.0 if delay else 0.0)
        loop.run(iters)
        res[name] = state(gm._xyz, gm._scaling, gm._rotation, gm._opacity, loop.counters)
    pts = np.asarray(sc.pose_3d_init, dtype=np.float32)[None]
    p2 = np.asarray(sc.poses_2d, dtype=np.float32)[None]
    for name, rigs in (("frame", False), ("frame-dv", True)):
        gm = delayed(model(device))
        if rigs:
            bank = RigBank([sc.cameras])
            for rows in (bank.sched, bank.sched_log):            # the bank's schedule rows carry the ramp
                rows[:, 2], rows[:, 3] = 0.01, 1000.0
            assert bank.sched[0, 0].item() == gm.opt_cfg["lr_init"]
            fb = FrameBatchLoop(gm, rigs=bank.to(device), frames=1, dataset="h36m")
            fb.new_scenes(pts, poses_2d=p2, rig_ids=[0])
        else:
            fb = FrameBatchLoop(gm, sc.cameras, 1, dataset="h36m")
            fb.new_scenes(pts, poses_2d=p2)
        fb.run(iters)
        if rigs:
            fb.check_rigs()
            assert fb._sel.sched.cpu()[0].tolist()[2:4] == [0.01, 1000.0]
        res[name] = state(fb.xyz[0], fb.scaling[0], fb.rotation[0], fb.opacity[0], fb.counters[0])
    for a, b in (("fused", "separate"), ("frame-dv", "frame")):
        for k, (x, y) in enumerate(zip(res[a], res[b])):
            assert torch.equal(x, y), (a, b, "xyz scaling rotation opacity counters".split()[k])
    assert res["fused"][4].tolist() == [iters, iters // 4]
    # the ramp is at work: through iteration 32 the factor is 0.01 + 0.99 sin(pi/2 * it/1000) <= 0.06, and an Adam step is
    # proportional to the learning rate, so the joints have moved a small fraction of what the plain schedule moves them
    init = torch.tensor(sc.pose_3d_init, device=device).float().reshape(-1)
    moved = lambda r: float((r[0] - init).reshape(-1, 3).norm(dim=1).mean())
    assert 0.0 < moved(res["fused"]) < 0.25 * moved(res["fused-plain"])
    assert 0.0 < moved(res["frame-dv"]) < 0.25 * moved(res["fused-plain"])


# ------------------------------------------------------------------------------------------------ sks_heatmap_factors
def _solve_scales(cam, means, W, H, targets, modifier):
    """Per joint an isotropic scale such that floor(4 sigma + 0.5) of the targeted axis is the wanted radius, with 4 sigma + 0.5
    in the middle of its integer interval, by bisection on the twin's own fp32 lambdas in `cam`.  targets: [(axis, radius)]."""
    from oracle import heatmaps_ref
    J = means.shape[0]
    lo, hi = torch.full((J,), 1e-3), torch.full((J,), 1e5)
    want = torch.tensor([r / 4.0 if r else 0.0625 for _, r in targets])       # 4 sigma + 0.5 = r + 0.5 (radius 0: 0.75)
    axis = torch.tensor([a for a, _ in targets])
    ident = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(J, 1)
    for _ in range(60):
        mid = torch.sqrt(lo * hi)
        cov = heatmaps_ref.covariance_from_scaling_rotation(mid[:, None].repeat(1, 3), ident, modifier)
        l1, l2 = heatmaps_ref.ewa_lambdas_views(means, cov, [cam], W, H)
        sig = torch.where(axis == 0, l1[0], l2[0]).clamp_min(0).sqrt()
        small = sig < want
        lo, hi = torch.where(small, mid, lo), torch.where(small, hi, mid)
    return torch.sqrt(lo * hi)


def _heatmap_case(W, H, mixed):
    """Everything of a case that needs no GPU: cameras, inputs, the twin's factors per view, and the CPU-side assertions that
    the case visits the radii it is meant to and that no 4 sigma + 0.5 sits within 1e-3 of an integer."""
    from skelsplat_amd.scene import SyntheticScene
    from oracle import heatmaps_ref
    V, modifier = 2, 1.3
    sc = SyntheticScene("h36m", n_views=V, seed=4, W=W, H=H, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5)
    cams = list(sc.cameras)
    if mixed:
        small = SyntheticScene("h36m", n_views=V, seed=4, W=W - 4, H=H - 4, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5)
        cams[1] = small.cameras[1]
    J = sc.n_joints
    means = torch.tensor(sc.pose_3d_init, dtype=torch.float32)
    # lambda1 (rows) is at least 0.3 + sqrt(0.1): its radius starts at 3, and lambda2 = lambda1 - 2 sqrt(0.1) must stay positive,
    # so the rows start at 4; lambda2 (columns) reaches down to radius 0
    classes = lambda n: [n - 1, n, n + 1, 3 * n, 10 * n]
    targets = [(0, max(r, 4)) for r in classes(H)] + [(1, max(r, 1)) for r in classes(W)]
    targets = (targets + [(1, 0), (1, 1), (0, 4), (1, 2), (0, max(2 * H, 4)), (1, 5 * W), (0, max(H, 4))])[:J]
    assert len(targets) == J
    scales = _solve_scales(cams[0], means, W, H, targets, modifier)[:, None].repeat(1, 3).contiguous()
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(J, 1)
    p2d = torch.tensor(sc.poses_2d, dtype=torch.float32).clone()
    for j in range(J):                  # the detection at 0, at n - 1 and in the middle
        p2d[:, j] = torch.tensor([[0.3, 0.7], [W - 0.5, H - 0.5], [W / 2.0, H / 2.0]][j % 3])
    want, radii = [], {0: set(), 1: set()}
    for v, cam in enumerate(cams):
        w_v, h_v = int(cam.image_width), int(cam.image_height)
        want.append([t[0] for t in heatmaps_ref.heatmap_factors(means, scales, rot, p2d[v:v + 1], [cam], scaling_modifier=modifier)])
        cov = heatmaps_ref.covariance_from_scaling_rotation(scales, rot, modifier)
        l1, l2 = heatmaps_ref.ewa_lambdas_views(means, cov, [cam], w_v, h_v)
        for ax, lam in ((0, l1[0]), (1, l2[0])):
            x = 4.0 * lam.sqrt().double() + 0.5          # (sigma as the kernel forms it: fp32 sqrt, then double)
            assert bool(torch.isfinite(x).all())
            assert float((x - x.round()).abs().min()) > 1e-3, "a truncation radius sits on a rounding step"
            if v == 0:
                radii[ax] |= {int(r) for r in x.floor().tolist()}
    for ax, n in ((0, H), (1, W)):        # every class of radius is visited in the full-size view
        assert min(radii[ax]) <= (4 if ax == 0 else 0), (ax, radii[ax])
        for r in classes(n):
            assert (r in radii[ax] if r <= n + 1 else any(0.7 * r <= x <= 1.3 * r for x in radii[ax])) or r < (4 if ax == 0 else 1), \
                (ax, n, r, sorted(radii[ax]))
    return V, J, modifier, cams, means, scales, rot, p2d, want


@pytest.mark.parametrize("W,H,mixed", [(16, 16, False), (40, 24, False), (130, 1, False), (40, 24, True)],
                         ids=["16x16", "40x24", "130x1", "40x24+36x20"])
def test_heatmap_factors_at_any_radius(device, W, H, mixed):
    """sks_heatmap_factors against the oracle twin (which tests/test_tail_ref_cpu.py and tests/test_cpu.py hold to scipy at
    these radii) at the twin's existing tolerance, with Gaussians sized so that the truncation radius of an axis of n samples
    is its smallest, n - 1, n, n + 1, about 3n and about 10n -- past n the impulse bounces more than once -- and the detection
    at 0, n - 1 and in the middle; one case with per-view sizes.  Then the planes of sks_heatmaps are (row * col - cmin) / den
    bit for bit."""
    from skelsplat_amd import _lib
    from skelsplat_amd import heatmaps as hmod
    from skelsplat_amd.rasterizer import ViewBatch
    lib = _lib.load()
    V, J, modifier, cams, means, scales, rot, p2d, want = _heatmap_case(W, H, mixed)
    views = ViewBatch.from_cameras([c.to(device) for c in cams], allow_mixed=mixed)
    d = lambda t: t.contiguous().to(device)
    d_means, d_scales, d_rot, d_p2d = d(means), d(scales), d(rot), d(p2d)
    row = torch.full((V, J, H), float("nan"), device=device)
    col = torch.full((V, J, W), float("nan"), device=device)
    cmin, den = torch.empty((V, J), device=device), torch.empty((V, J), device=device)
    _lib.check(lib.sks_heatmap_factors(V, J, W, H, d_means.data_ptr(), d_scales.data_ptr(), d_rot.data_ptr(), modifier,
                                       d_p2d.data_ptr(), views.viewmatrix.data_ptr(), views.tanfovx, views.tanfovy,
                                       row.data_ptr(), col.data_ptr(), cmin.data_ptr(), den.data_ptr(), 1, views.wh,
                                       torch.cuda.current_stream(device).cuda_stream), "sks_heatmap_factors")
    torch.cuda.synchronize()
    for v, cam in enumerate(cams):
        w_v, h_v = int(cam.image_width), int(cam.image_height)
        for name, a, b in (("row", row[v, :, :h_v], want[v][0]), ("col", col[v, :, :w_v], want[v][1]),
                           ("cmin", cmin[v], want[v][2]), ("den", den[v], want[v][3])):
            util.assert_close(f"{name} view {v}", a.cpu(), b, rtol=2e-5, atol_scale=1e-6)
        if (w_v, h_v) != (W, H):      # beyond a smaller view's own size nothing is written
            assert bool(torch.isnan(row[v, :, h_v:]).all()) and bool(torch.isnan(col[v, :, w_v:]).all())
        # cmin / den follow from the rows the kernel wrote
        r_, c_ = row[v, :, :h_v], col[v, :, :w_v]
        lo = r_.amin(dim=1) * c_.amin(dim=1)
        assert torch.equal(cmin[v], lo) and torch.equal(den[v], (r_.amax(dim=1) * c_.amax(dim=1) - lo) + 1e-8)
    if (W, H) == (40, 24) and not mixed:
        out = hmod.heatmap_planes(row, col, cmin, den)
        ref = (row[:, :, :, None] * col[:, :, None, :] - cmin[:, :, None, None]) / den[:, :, None, None]
        assert out.shape == (V, J, H, W) and torch.equal(out, ref)
