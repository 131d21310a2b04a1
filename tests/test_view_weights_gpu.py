"""View agreement on the device (include/skelsplat_hip.h "View agreement"): sks_loop_adam_step_vw one call at a time against the
op-by-op restatement of tests/view_weight_ref.py (bits) and a float64 reference (counted allowance); the fused step's _vw forms
against the separate calls, frame batches against single frames, the _dv twin against the by-value one; the loops."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tail_ref, view_weight_ref as REF
from tests.test_loop_tail_gpu import ACC, ADAM, EPS32, LRS, SCHEDULES, _State, _bits, _dbl, _held, _ints, _mask_of, _report, _skeleton

pytestmark = pytest.mark.gpu

MODE = {"scale": 1, "select": 2}
THR = 0.5
SHAPES = [(2, 1), (3, 17), (4, 17), (8, 64), (9, 64), (31, 19), (64, 4), (64, 64), (2, 256),
          (42, 64), (43, 64)]       # (the last two: 8 064 and 8 256 floats of slots, either side of the LDS mirror's 8 192)
# (the weighted step parks the slots in LDS whenever they fit, the plain one only with more than 8 views)
REGIMES = {(2, 1): ("lds", "narrow"), (3, 17): ("lds", "narrow"), (4, 17): ("lds", "narrow"), (8, 64): ("lds", "narrow"),
           (9, 64): ("lds", "wide"), (31, 19): ("lds", "wide"), (64, 4): ("lds", "wide"), (64, 64): ("walk", "walk"), (42, 64): ("lds", "wide"), (43, 64): ("walk", "walk"),
           (2, 256): ("lds", "narrow")}        # (2 x 256 x 3 = 1 536 floats: by the rule V * P * 3 <= 8192 it fits)
SETS = ("random", "identical", "opposed", "zero", "unobserved", "inf")


def _same_bits(a, b):
    """float32 arrays equal in every bit, a NaN matching a NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32).reshape(np.shape(a))
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def _slot_set(kind, V, P, g):
    """(V,P,3) xyz gradients of a set, magnitudes 1e-6 .. 1e-2, and the unobserved joint or None"""
    mag = 10.0 ** (torch.rand((V, P, 1), generator=g) * 4.0 - 6.0)
    rnd = torch.randn((V, P, 3), generator=g)
    common = torch.randn((1, P, 3), generator=g)
    agree = common + 0.3 * rnd
    if kind in ("random", "inf"):
        s = rnd * mag
    elif kind == "identical":
        s = (common * mag[:1]).repeat(V, 1, 1)
    else:
        s = agree * mag
    missing = None
    if kind == "opposed":
        s[V - 1] = -s[0]
    elif kind == "zero":
        s[1 % V] = 0.0
    elif kind == "unobserved":
        missing = P // 2
        s[:, missing] = 0.0
    elif kind == "inf":
        s[0, 0, 1] = float("inf")
    return s.contiguous(), missing


def _call_vw(lib, st, V, P, grads, mask, last, sched, lam, limb, mode, out_w, out_c, stream, es=None, sums=None, tol=0.0):
    slots_p, rest_p = st.ptrs()
    es_args = (None, None, 0, 0.0, None) if es is None else (sums.data_ptr(), es.data_ptr(), 4, tol, st.flag.data_ptr())
    return lib.sks_loop_adam_step_vw(V, P, grads.data_ptr(), *slots_p, mask, last, *rest_p, ACC, _dbl(sched), _dbl(LRS), _dbl(ADAM),
                                     lam, _ints(limb), 1, *es_args, mode, THR, None if out_w is None else out_w.data_ptr(),
                                     None if out_c is None else out_c.data_ptr(), stream)


def _update_ref(monkeypatch, ref1, grads_h, last, before, w, mode, V, sched):
    """The complete update in float64 from the float64 slots of tail_ref.adam_step_ref (`ref1`) merged with the kernel's own
    weights `w`; allowances in units of 2**-24: the slots' carried through the weights, plus per view one product and one
    addition that round and the final division.  The merged gradient then goes through adam_step_ref as the one slot of a
    one-view step, with that allowance in the place of the mean's (K_MEAN)."""
    slots, slot_allow = ref1["slots"]
    w = torch.as_tensor(w, dtype=torch.float64)[..., None]
    if mode == "scale":
        g = (w * slots).sum(0) / V
        allow = (w * slot_allow).sum(0) / V + (2 * V + 1) * (w * slots.abs()).sum(0) / V
    else:
        n = w.sum(0)
        kept = (w * slots).sum(0) / n.clamp_min(1.0)
        kept_allow = (w * slot_allow).sum(0) / n.clamp_min(1.0) + (V + 1) * (w * slots.abs()).sum(0) / n.clamp_min(1.0)
        plain_allow = slot_allow.sum(0) / V + (V + 1) * slots.abs().sum(0) / V
        g = torch.where(n >= 1, kept, slots.mean(0))
        allow = torch.where(n >= 1, kept_allow, plain_allow)
    ratio = torch.where(g.abs() > 0, allow / g.abs().clamp_min(1e-300), torch.zeros_like(g))
    monkeypatch.setattr(tail_ref, "K_MEAN", lambda _v: ratio)
    xyz, sc, ro, op, _, m, v, cnt = before
    one = torch.cat([g, grads_h[last, :, 3:].to(torch.float64)], dim=1)[None]
    ref = tail_ref.adam_step_ref(one, torch.zeros((1, g.shape[0], 3)), 1, 0, (xyz, sc, ro, op), m, v, (int(cnt[0]), int(cnt[1])), ACC,
                                 sched, LRS, ADAM, 0.0, None)
    monkeypatch.undo()
    return ref


@pytest.mark.parametrize("mode", ["scale", "select"])
@pytest.mark.parametrize("V,P", SHAPES)
def test_adam_step_vw_against_the_restatement(device, monkeypatch, V, P, mode):
    """One sks_loop_adam_step_vw call from zero moments per (mask, gradient set): the slots as the plain step leaves them; the
    cosines equal the restatement's in every bit, `select` weights exactly, `scale` weights within one fp32 ulp (the device's double
    log); exp_avg's xyz columns equal (1 - beta1) x the restatement's merge of the kernel's slots with the kernel's weights in
    every bit; the complete update within the counted allowance of a float64 reference; an unobserved joint keeps its NaN and
    zero moments and changes no other row's bits."""
    from skelsplat_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream(device).cuda_stream
    assert REF.regime(V, P) == REGIMES[(V, P)]
    sched = SCHEDULES["plain"]
    w1 = np.float32(1.0 - ADAM[0])
    seen, off_by_ulp, total_w = {}, 0, 0
    for mk, mask_kind in enumerate(("full", "missing", "lastbit")):
        mask, last = _mask_of(mask_kind, V)
        for sk, kind in enumerate(SETS):
            g = torch.Generator().manual_seed(100000 * mk + 1000 * sk + 10 * V + P)
            s, missing = _slot_set(kind, V, P, g)
            lam, limb_kind = (1e-5, "h36m") if kind == "random" and P >= 4 else (0.0, "none")
            limb, xyz = _skeleton(limb_kind, P, g)
            grads_h = torch.randn((V, P, 11), generator=g)
            grads_h[:, :, :3] = s
            stale = torch.randn((V, P, 3), generator=g) * 1e-3 if kind == "random" else s.clone()
            runs = []
            for observed in ((True,) if missing is None else (False, True)):
                x0 = xyz.clone()
                if missing is not None:
                    grads_h[:, missing] = 0.0
                    if not observed:
                        x0[missing] = float("nan")
                st = _State(device, V, P, x0, (0, 0), torch.Generator().manual_seed(7 + sk))
                st.t[4].copy_(stale)
                out_w = torch.full((V, P), -7.0, device=device)
                out_c = torch.full((P, V, V), -7.0, device=device)
                before = st.snap()
                _lib.check(_call_vw(lib, st, V, P, grads_h.to(device), mask, last, sched, lam, limb, MODE[mode], out_w, out_c, stream),
                           "sks_loop_adam_step_vw")
                after = st.snap()
                runs.append((before, after, out_w.cpu().numpy(), out_c.cpu().numpy()))
            before, after, got_w, got_c = runs[0]
            miss = () if missing is None else (missing,)
            if missing is not None:     # the NaN row stays NaN with zero moments; nobody else's bits depend on it
                assert bool(torch.isnan(after[0][missing]).all()) and not after[5][missing].any() and not after[6][missing].any()
                keep = [p for p in range(P) if p != missing]
                for k in range(7):
                    a, b = after[k], runs[1][1][k]
                    a, b = (a[:, keep], b[:, keep]) if k == 4 else (a[keep], b[keep])
                    assert torch.equal(_bits(a), _bits(b)), ("unobserved joint changed another row", k)
                assert np.array_equal(got_w, runs[1][2]) and np.array_equal(got_c, runs[1][3])
            slots = after[4].numpy()
            # the slots are the plain step's: this group's gradient (+ the limb gradient) where the mask says, stale elsewhere
            ref1 = tail_ref.adam_step_ref(grads_h, before[4], mask, last, before[:4], before[5], before[6], (0, 0), ACC, sched, LRS,
                                          ADAM, lam, limb, missing=miss)
            if kind != "inf":
                _held("slots", after[4], ref1["slots"][0], ref1["slots"][1], seen)
            for v in range(V):
                src = grads_h[v, :, :3] if (mask >> v) & 1 and lam == 0.0 else (None if (mask >> v) & 1 else before[4][v])
                assert src is None or _same_bits(slots[v], src.numpy()), (kind, mask_kind, v)
            want = REF.view_weighting32(slots, mode, THR)
            assert _same_bits(got_c, want["similarity"]), (kind, mask_kind, "similarity")
            if mode == "select":
                assert _same_bits(got_w, want["weights"]), (kind, mask_kind, "weights")
            else:
                ulp = np.spacing(np.abs(want["weights"]).astype(np.float32))
                assert np.array_equal(np.isnan(got_w), np.isnan(want["weights"]))
                assert (np.abs(got_w - want["weights"]) <= ulp).all(), (kind, mask_kind, "weights beyond one ulp")
                off_by_ulp += int((got_w != want["weights"]).sum())
                total_w += got_w.size
            merged = REF.merged32(slots, got_w, mode)
            with np.errstate(all="ignore"):
                m_want = np.float32(0.0) + w1 * (merged - np.float32(0.0))
            assert _same_bits(after[5][:, :3].numpy(), m_want), (kind, mask_kind, "merged gradient")
            if kind != "inf":
                ref = _update_ref(monkeypatch, ref1, grads_h, last, before, got_w, mode, V, sched)
                for name, i in (("m", 5), ("v", 6), ("xyz", 0), ("scaling", 1), ("rotation", 2), ("opacity", 3)):
                    _held(name, after[i], ref[name][0], ref[name][1], seen)
                assert (int(after[7][0]), int(after[7][1])) == (ACC, 1)
    if mode == "scale":
        print(f"\nV={V} P={P}: {off_by_ulp} of {total_w} scale weights differ from the restatement (by one ulp)")
    _report(f"vw {mode} V={V} P={P}", seen)


@pytest.mark.parametrize("V,P", SHAPES)
def test_vw_mode_0_is_the_plain_step(device, V, P):
    """vw_mode = 0 through sks_loop_adam_step_vw equals sks_loop_adam_step (es_state NULL) and sks_loop_adam_step_es (criterion
    given) in every output bit over three calls, writes neither optional output, and an unknown mode is an error string."""
    from skelsplat_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream(device).cuda_stream
    sched = SCHEDULES["delay"]
    g = torch.Generator().manual_seed(31 * V + P)
    limb, xyz = _skeleton("h36m" if P >= 4 else "none", P, g)
    grads = torch.randn((V, P, 11), generator=g).to(device)
    mask, last = _mask_of("missing", V)
    sums = torch.tensor([[float(v + 1), 10.0] for v in range(V)], dtype=torch.float64, device=device)
    for es in (False, True):
        finals = []
        for entry in ("old", "vw"):
            st = _State(device, V, P, xyz.clone(), (0, 0), torch.Generator().manual_seed(5), es_window=4 if es else 0)
            out_w = torch.full((V, P), -7.0, device=device)
            out_c = torch.full((P, V, V), -7.0, device=device)
            slots_p, rest_p = st.ptrs()
            for _ in range(3):
                if entry == "vw":
                    rc = _call_vw(lib, st, V, P, grads, mask, last, sched, 1e-5, limb, 0, out_w, out_c, stream, es=st.es, sums=sums)
                elif es:
                    rc = lib.sks_loop_adam_step_es(V, P, grads.data_ptr(), *slots_p, mask, last, *rest_p, ACC, _dbl(sched), _dbl(LRS),
                                                   _dbl(ADAM), 1e-5, _ints(limb), 1, sums.data_ptr(), st.es.data_ptr(), 4, 0.0,
                                                   st.flag.data_ptr(), stream)
                else:
                    rc = lib.sks_loop_adam_step(V, P, grads.data_ptr(), *slots_p, mask, last, *rest_p, ACC, _dbl(sched), _dbl(LRS),
                                                _dbl(ADAM), 1e-5, _ints(limb), 1, stream)
                _lib.check(rc, entry)
            finals.append(st.snap() + ([st.es.cpu().clone()] if es else []))
            assert bool((out_w == -7.0).all()) and bool((out_c == -7.0).all())
        for k, (a, b) in enumerate(zip(*finals)):
            assert torch.equal(_bits(a), _bits(b)), (es, k)
    st = _State(device, V, P, xyz.clone(), (0, 0), torch.Generator().manual_seed(5))
    assert _call_vw(lib, st, V, P, grads, mask, last, sched, 0.0, None, 3, None, None, stream) != 0
    assert b"vw_mode" in lib.sks_last_error()
    # either output may be NULL: the other one and the step do not change
    res = []
    for outs in ((True, True), (False, True), (True, False), (False, False)):
        st = _State(device, V, P, xyz.clone(), (0, 0), torch.Generator().manual_seed(5))
        out_w = torch.full((V, P), -7.0, device=device) if outs[0] else None
        out_c = torch.full((P, V, V), -7.0, device=device) if outs[1] else None
        _lib.check(_call_vw(lib, st, V, P, grads, mask, last, sched, 1e-5, limb, 1, out_w, out_c, stream), "vw")
        res.append((st.snap(), out_w, out_c))
    for snap, out_w, out_c in res[1:]:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(snap, res[0][0]))
        assert out_w is None or torch.equal(out_w, res[0][1])
        assert out_c is None or torch.equal(out_c, res[0][2])


# ------------------------------------------------------------------------------------------------ the fused step
FV, FW, FH, FACC = 4, 64, 48, 4


def _fused_scene(device, F):
    """The recipe of tests/fused_loss_cases.py (one 17-joint skeleton, its own cameras) at 4 views of 64 x 48, F frames: frame f's
    joints are the scene's plus noise, its heat-maps random planes; raw leaf parameters as the fused step takes them."""
    from skelsplat_amd import rasterizer as R
    from tests import fused_loss_cases as FC
    c = FC._base("view-weights", 4242, FW, FH, FV)
    assert c.P == 17 and c.V == FV
    rng = np.random.default_rng(77)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=device)
    xyz = torch.stack([t(c.means + (rng.normal(0, 15.0, c.means.shape) if f else 0.0)) for f in range(F)]).contiguous()
    scaling = t(np.log(c.scales))[None].repeat(F, 1, 1).contiguous()
    rotation = t(c.quats)[None].repeat(F, 1, 1).contiguous()
    op = np.clip(c.opac, 1e-3, 1 - 1e-3)
    opacity = t(np.log(op / (1 - op)))[None].repeat(F, 1, 1).contiguous()
    planes = torch.stack([t(p) for _ in range(F) for p in FC._planes(rng, c.C, c.sizes)])
    cams = [cam.to(device) for cam in c.cams]
    views = R.ViewBatch.from_cameras([cams[k % FV] for k in range(F * FV)])
    return c, views, R.gt_tile_stats(planes), t(c.feat), [xyz, scaling, rotation, opacity]


class _Frames:
    def __init__(self, device, F, params, es=False):
        P = params[0].shape[1]
        self.p = [x.clone() for x in params]
        self.m, self.v = torch.zeros((F, P, 11), device=device), torch.zeros((F, P, 11), device=device)
        self.cnt = torch.zeros((F, 2), dtype=torch.int32, device=device)
        self.slots = torch.zeros((F, FV, P, 3), device=device)
        self.packed = torch.zeros((F * FV, P, 11), device=device)
        self.sums = torch.zeros((F * FV, 2), dtype=torch.float64, device=device)
        self.w = torch.full((F, FV, P), -7.0, device=device)
        self.c = torch.full((F, P, FV, FV), -7.0, device=device)
        self.es = torch.zeros((F, 2 + 2 * 4), dtype=torch.int32, device=device) if es else None

    def state(self, f=None):
        torch.cuda.synchronize()
        sl = slice(None) if f is None else slice(f, f + 1)
        return [x[sl].clone() for x in self.p + [self.m, self.v, self.cnt, self.slots, self.w, self.c]]


OPT = None


def _opt_arrays():
    return _dbl(SCHEDULES["plain"]), _dbl(LRS), _dbl(ADAM), _ints(tail_ref.H36M_LIMB)


def _fused_steps(device, F, mode, n_groups, es_tol=None, frames_of=None, separate=False):
    """n_groups accumulation groups of F frames through sks_loop_fused_step_vw (or, `separate`, sks_geometry +
    sks_backward_fused_loss + one sks_loop_adam_step_vw per frame); `frames_of`: run only these frames of the F-frame scene."""
    from skelsplat_amd import _lib, rasterizer as R
    lib = _lib.load()
    c, views, stats, feat, params = _fused_scene(device, F)
    if frames_of is not None:
        f = frames_of
        params = [x[f:f + 1].contiguous() for x in params]
        views = R.ViewBatch.from_cameras([cam.to(device) for cam in c.cams])
        stats = R.gt_tile_stats(stats.gt[f * FV:(f + 1) * FV].contiguous())
        F = 1
    fr = _Frames(device, F, params, es=es_tol is not None)
    sched, lrs, adam, limb = _opt_arrays()
    stream = torch.cuda.current_stream(device).cuda_stream
    mask, last = (1 << FV) - 1, FV - 1
    st = None
    for _ in range(n_groups):
        st = R.geometry_views(views, fr.p[0], c.C, fr.p[3], fr.p[1], fr.p[2], None, raw_params=True, out=st, frames=F)
        if not separate:
            kw = {} if es_tol is None else dict(es_state=fr.es, es_window=4, es_tolerance=es_tol)
            R.loop_fused_step(st, stats, feat, fr.packed, fr.sums, fr.slots, mask, last, *fr.p, fr.m, fr.v, fr.cnt, FACC, sched, lrs,
                              adam, 1e-5, limb, view_weights=(MODE[mode], THR, fr.w, fr.c), **kw)
            continue
        assert F == 1
        R.backward_fused_loss(st, stats, fr.p[0][0], feat, fr.p[3][0], fr.p[1][0], fr.p[2][0], None, packed_out=fr.packed,
                              sums_out=fr.sums)
        es_args = (None, None, 0, 0.0, None) if es_tol is None else (fr.sums.data_ptr(), fr.es.data_ptr(), 4, es_tol, None)
        _lib.check(lib.sks_loop_adam_step_vw(FV, c.P, fr.packed.data_ptr(), fr.slots.data_ptr(), mask, last,
                                             *[x.data_ptr() for x in fr.p], fr.m.data_ptr(), fr.v.data_ptr(), fr.cnt.data_ptr(), FACC,
                                             sched, lrs, adam, 1e-5, limb, 1, *es_args, MODE[mode], THR, fr.w.data_ptr(),
                                             fr.c.data_ptr(), stream), "sks_loop_adam_step_vw")
    return fr


@pytest.mark.parametrize("mode", ["scale", "select"])
def test_fused_step_vw_equals_the_separate_calls_and_frames_equal_single_frames(device, mode):
    """sks_loop_fused_step_vw over three groups == sks_geometry + sks_backward_fused_loss + sks_loop_adam_step_vw in every bit
    (parameters, moments, counters, slots, weights, cosines); frames = 3 == each frame alone; the weights are not all alike."""
    one = _fused_steps(device, 1, mode, 3).state()
    sep = _fused_steps(device, 1, mode, 3, separate=True).state()
    for k, (a, b) in enumerate(zip(one, sep)):
        assert torch.equal(_bits(a), _bits(b)), k
    assert not bool((one[-2] == -7.0).any()) and not bool((one[-1] == -7.0).any())
    assert len(torch.unique(one[-2])) > 1
    batch = _fused_steps(device, 3, mode, 3)
    for f in range(3):
        alone = _fused_steps(device, 3, mode, 3, frames_of=f).state()
        for k, (a, b) in enumerate(zip(batch.state(f), alone)):
            assert torch.equal(_bits(a), _bits(b)), (f, k)


def test_fused_step_vw_with_the_criterion(device):
    """With the criterion on (a tolerance that fires as soon as it has its two windows, iteration 8) the fused step and the
    separate calls stop at the same iteration with the same bits; afterwards a stopped frame's weight rows stay unwritten."""
    from skelsplat_amd import rasterizer as R
    fused = _fused_steps(device, 1, "scale", 3, es_tol=1e9)
    sep = _fused_steps(device, 1, "scale", 3, es_tol=1e9, separate=True)
    assert int(fused.es[0, 1]) == 8 == int(sep.es[0, 1]) and int(fused.cnt[0, 0]) == 8
    for k, (a, b) in enumerate(zip(fused.state(), sep.state())):
        assert torch.equal(_bits(a), _bits(b)), k
    for fr in (fused, sep):
        assert not bool((fr.w == -7.0).any())
        fr.w.fill_(-7.0)
        fr.c.fill_(-7.0)
    more = _fused_steps_continue(device, fused)
    assert bool((more.w == -7.0).all()) and bool((more.c == -7.0).all())


def _fused_steps_continue(device, fr):
    """one more fused launch on a state whose frame has stopped"""
    from skelsplat_amd import rasterizer as R
    c, views, stats, feat, _ = _fused_scene(device, 1)
    sched, lrs, adam, limb = _opt_arrays()
    st = R.geometry_views(views, fr.p[0], c.C, fr.p[3], fr.p[1], fr.p[2], None, raw_params=True, frames=1)
    R.loop_fused_step(st, stats, feat, fr.packed, fr.sums, fr.slots, (1 << FV) - 1, FV - 1, *fr.p, fr.m, fr.v, fr.cnt, FACC, sched, lrs,
                      adam, 1e-5, limb, view_weights=(1, THR, fr.w, fr.c), es_state=fr.es, es_window=4, es_tolerance=1e9)
    torch.cuda.synchronize()
    return fr


# ------------------------------------------------------------------------------------------------ the loops
LV, LJ, LW, LH, LITERS = 4, 17, 64, 48, 24


def _loop_scene(dev):
    from skelsplat_amd.scene import GaussianModel, SyntheticScene
    sc = SyntheticScene("h36m", n_views=LV, seed=9, W=LW, H=LH, ring=2500.0, fx=1145.0 * (LW / 1000) * 1.5, device=dev)

    def model():
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9, scaling_modifier=1.0,
                                                device=dev)
        gm.training_setup()
        return gm
    rng = np.random.default_rng(11)
    base3, base2 = np.asarray(sc.pose_3d_init, np.float32), np.asarray(sc.poses_2d, np.float32)
    pts = np.stack([base3 + rng.normal(0, 10.0 * (f + 1), base3.shape) for f in range(3)]).astype(np.float32)
    p2d = np.stack([base2 + rng.normal(0, 1.0 * f, base2.shape) for f in range(3)]).astype(np.float32)
    p2d[:, 1] += rng.normal(0, 6.0, p2d[:, 1].shape).astype(np.float32)        # one view's detections are off
    return sc, model, pts, p2d


def _single(dev, sc, model, pt, p2d_f, mode, **kw):
    """MultiViewLoop on one frame, on the heat-map planes generate_heatmaps draws for it"""
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.loop import MultiViewLoop
    gm = model()
    loop = MultiViewLoop(gm, sc.cameras, torch.zeros((LV, LJ, LH, LW), device=dev), dataset="h36m", view_weighting=mode,
                         view_threshold=THR, **kw)
    gm.reset_from_points(torch.tensor(pt, device=dev))
    for slots, vb, gt, stats, idx in loop.size_groups:
        generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(), torch.tensor(p2d_f[slots], device=dev),
                          [sc.cameras[k] for k in slots], out=gt, views=vb, totals=None if stats is None else stats.totals)
    return loop, gm


@pytest.mark.parametrize("mode", ["scale", "select"])
def test_loops_with_view_weighting(device, mode):
    """MultiViewLoop(view_weighting=mode): the fused tail == the separate tail == use_graph in every bit; the device tail follows
    the tensor-op tail within the loop tests' standing tolerance (rtol 1e-3 of the movement's scale); FrameBatchLoop frames ==
    single frames in every bit, weights included; a pipeline's view_weights rows are the loops'; the weighting changes the result."""
    from skelsplat_amd.loop import FrameBatchLoop, FramePipeline, masked_l2_grad_torch
    sc, model, pts, p2d = _loop_scene(device)
    res = {}
    for name, kw in (("fused", dict(sparse=True)), ("separate", dict(sparse=True, fused_tail=False)),
                     ("graph", dict(sparse=True, use_graph=True)), ("host", dict(loss_grad=masked_l2_grad_torch)),
                     ("plain", dict(sparse=True))):
        loop, gm = _single(device, sc, model, pts[0], p2d[0], None if name == "plain" else mode, **kw)
        assert name in ("host", "plain") or (loop.device_tail and loop.fused_tail == (name != "separate"))
        loop.run(LITERS, groups_per_graph=3)
        torch.cuda.synchronize()
        res[name] = (gm._xyz.detach().clone(), None if name == "plain" else loop.view_weights.clone(),
                     None if name == "plain" else loop.view_similarity.clone())
    for name in ("separate", "graph"):
        for a, b in zip(res["fused"], res[name]):
            assert torch.equal(_bits(a), _bits(b)), name
    # (tests/test_ops_gpu.py test_device_tail_loop_matches_tensor_op_tail: xyz within 0.2 % of the mean distance moved)
    start = torch.tensor(pts[0], device=device)
    moved = float((res["host"][0] - start).norm(dim=1).mean())
    gap = float((res["fused"][0] - res["host"][0]).norm(dim=1).max())
    print(f"\n{mode}: device tail vs tensor-op tail: {gap:.3e} of {2e-3 * moved:.3e} allowed (moved {moved:.3f})")
    assert moved > 0 and gap < 2e-3 * moved
    assert not torch.equal(res["fused"][0], res["plain"][0])
    fb = FrameBatchLoop(model(), sc.cameras, 3, dataset="h36m", view_weighting=mode, view_threshold=THR)
    fb.new_scenes(pts, poses_2d=p2d)
    fb.run(LITERS, groups_per_graph=3)
    torch.cuda.synchronize()
    singles = []
    for f in range(3):
        loop, gm = _single(device, sc, model, pts[f], p2d[f], mode, sparse=True)
        loop.run(LITERS, groups_per_graph=3)
        torch.cuda.synchronize()
        singles.append(loop.view_weights.clone())
        assert torch.equal(fb.xyz[f], gm._xyz.detach()), f
        assert torch.equal(fb.view_weights[f], loop.view_weights) and torch.equal(fb.view_similarity[f], loop.view_similarity), f
    pipe = FramePipeline(model(), sc.cameras, frames=2, streams=2, dataset="h36m")
    assert pipe.set_view_weighting(mode, THR) is pipe
    out = pipe.optimize_sequence(pts, p2d, iterations=LITERS, groups_per_graph=3, interleave=8)
    torch.cuda.synchronize()
    assert tuple(pipe.view_weights.shape) == (3, LV, LJ)
    for f in range(3):
        assert torch.equal(out[f], fb.xyz[f]) and torch.equal(pipe.view_weights[f], singles[f]), f


def test_dv_twin_equals_the_by_value_step(device):
    """A frame batch over a rig bank (sks_loop_fused_step_vw_dv) == the same batch on the cameras by value, weights included."""
    from skelsplat_amd.loop import FrameBatchLoop
    from skelsplat_amd.rigs import RigBank
    sc, model, pts, p2d = _loop_scene(device)
    res = []
    for rigs in (False, True):
        if rigs:
            fb = FrameBatchLoop(model(), rigs=RigBank([sc.cameras]).to(device), frames=3, dataset="h36m", view_weighting="scale")
            fb.new_scenes(pts, poses_2d=p2d, rig_ids=[0, 0, 0])
        else:
            fb = FrameBatchLoop(model(), sc.cameras, 3, dataset="h36m", view_weighting="scale")
            fb.new_scenes(pts, poses_2d=p2d)
        fb.run(LITERS, groups_per_graph=3)
        torch.cuda.synchronize()
        res.append([fb.xyz.clone(), fb.exp_avg.clone(), fb.view_weights.clone(), fb.view_similarity.clone()])
    for k, (a, b) in enumerate(zip(*res)):
        assert torch.equal(_bits(a), _bits(b)), k
