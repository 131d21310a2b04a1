"""Prefill: the small-path backward's two launches zero the last planes of the output set the NEXT forward renders into
(sks_backward_prefill), and that forward takes them as zero (sks_forward_prefilled).  No result bit may depend on it.

C ABI: with the other set NaN-filled, sks_backward_prefill gives the gradients of sks_backward bit for bit, leaves exactly the
promised planes exactly zero and every other element still NaN; sks_forward_prefilled into that set equals a plain sks_forward into
NaN (torch.equal on colour, inverse depth, radii, geometry records) for plane counts 0, 1, a boundary inside a view, a view
boundary, half and all planes, with every early-fill field value, SKS_NO_EARLY_FILL, plain stores and forced-linear fill, outputs
offset by 4 floats, features that put covered tiles into prefilled planes, and a view with every Gaussian culled.

Workspace: two-call steps through a Workspace (two output sets) equal fresh-tensor calls bit for bit through every hand-over the
invariant in its docstring names.

Shapes are those of tests/test_early_fill_gpu.py, the smallest at which plane hand-overs go wrong: (64, 48) 16-byte stores,
(66, 48) the pair-masked HALF mode, (67, 45) 4-byte stores (no prefill by the backward: the forward still takes a promise),
(1000, 40) linear passes that are not whole rows, (1024, 24) row-aligned fill blocks in the main launch."""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_early_fill_gpu import SIZES, VC, Scene
from skelsplat_amd import _lib, rasterizer as R

pytestmark = pytest.mark.gpu

OFF = _lib.SKS_NO_EARLY_FILL
LINEAR = 1 << 21          # SKS_FILL_LINEAR
FWD_FLAGS = [_lib.SKS_EARLY_FILL(n) for n in range(8)] + [OFF, _lib.SKS_NO_NT_STORES, LINEAR, LINEAR | _lib.SKS_EARLY_FILL(3)]
NAN = float("nan")


def can_prefill(W, H):
    return W % 4 == 0 or (W % 4 == 2 and H % 2 == 0)


def plane_counts(V, C):
    """0, 1, a boundary inside a view, a view boundary, half, all -- of the (C + 1) * V planes."""
    planes = (C + 1) * V
    return sorted({0, 1, (C + 1) // 2 + (C + 1 if V > 1 else 0), C + 1, planes // 2, planes})


class PScene(Scene):
    """tests/test_early_fill_gpu.py's scene plus the backward and the prefill pair through the C ABI."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        g = torch.Generator(device="cpu").manual_seed(5)
        self.dLc = torch.randn((self.V, self.C, self.H, self.W), generator=g).to(self.dev)
        self.dLi = torch.randn((self.V, 1, self.H, self.W), generator=g).to(self.dev)
        self.accum = torch.empty((_lib.scratch_bytes(self.V, self.P, self.C, self.W, self.H, 0)[2],), dtype=torch.uint8, device=self.dev)

    def outputs(self, off=0):
        """A NaN-filled output set that starts `off` floats into its allocations."""
        V, C, H, W = self.V, self.C, self.H, self.W
        color = torch.full((V * C * H * W + off,), NAN, device=self.dev)[off:].view(V, C, H, W)
        inv = torch.full((V * H * W + off,), NAN, device=self.dev)[off:].view(V, 1, H, W)
        return color, inv

    def planes_of(self, color, inv):
        """(planes, H * W) in the library's plane order: view-major, a view's colour planes, then its inverse depth."""
        V, C = self.V, self.C
        return torch.cat([color.reshape(V, C, -1), inv.reshape(V, 1, -1)], dim=1).reshape((C + 1) * V, -1)

    def forward_prefilled(self, flags, color, inv, n):
        V, C, H, W, P, dev = self.V, self.C, self.H, self.W, self.P, self.dev
        radii = torch.full((V, P), -7, dtype=torch.int32, device=dev)
        geom = torch.zeros((self.gbytes,), dtype=torch.uint8, device=dev)
        means, feat, opac, scales, quats = self.params
        vw = self.views
        args = [V, P, C, W, H, vw.viewmatrix.data_ptr(), vw.projmatrix.data_ptr(), vw.tanfovx, vw.tanfovy, means.data_ptr(),
                feat.data_ptr(), opac.data_ptr(), scales.data_ptr(), quats.data_ptr(), None, 1.0, int(flags),
                color.data_ptr(), inv.data_ptr(), radii.data_ptr(), geom.data_ptr(), None, 0, None, None, None, int(n),
                torch.cuda.current_stream(dev).cuda_stream]
        _lib.check(_lib.load().sks_forward_prefilled(*args), "sks_forward_prefilled")
        return color, inv, radii, geom

    def backward(self, fwd, nxt=None, nw=0, ng=0, want_mean=True, dfeat=False, rc_only=False):
        """sks_backward (nxt None) or sks_backward_prefill through the C ABI into NaN-filled gradients."""
        V, C, H, W, P, dev = self.V, self.C, self.H, self.W, self.P, self.dev
        new = lambda *s: torch.full(s, NAN, device=dev)
        g = dict(m3=new(V, P, 3), m2=new(V, P, 3), op=new(V, P, 1), sc=new(V, P, 3), rot=new(V, P, 4), cov=new(V, P, 6),
                 feat=new(V, P, C) if dfeat else None, mean=new(P, 3) if want_mean else None)
        means, feat, opac, scales, quats = self.params
        vw = self.views
        p = lambda t: None if t is None else t.data_ptr()
        args = [V, P, C, W, H, vw.viewmatrix.data_ptr(), vw.projmatrix.data_ptr(), vw.tanfovx, vw.tanfovy, None, means.data_ptr(),
                feat.data_ptr(), opac.data_ptr(), scales.data_ptr(), quats.data_ptr(), None, 1.0, 0, fwd[2].data_ptr(),
                fwd[3].data_ptr(), None, 0, self.dLc.data_ptr(), self.dLi.data_ptr(), self.accum.data_ptr(), p(g["m3"]), p(g["m2"]),
                p(g["op"]), p(g["sc"]), p(g["rot"]), p(g["cov"]), p(g["feat"]), p(g["mean"])]
        st = torch.cuda.current_stream(dev).cuda_stream
        if nxt is None:
            rc = _lib.load().sks_backward(*args, st)
        else:
            rc = _lib.load().sks_backward_prefill(*args, nxt[0].data_ptr(), nxt[1].data_ptr(), int(nw), int(ng), st)
        if rc_only:
            return rc
        _lib.check(rc, "sks_backward(_prefill)")
        return g


def same(got, ref, what):
    for name, g, r in zip(("out_color", "out_invdepth", "radii", "geom"), got, ref):
        assert torch.equal(g, r), f"{what}: {name} differs from the plain forward into NaN"


def same_grads(got, ref, what):
    for k, r in ref.items():
        if r is None:
            assert got[k] is None
            continue
        assert not torch.isnan(r).any(), f"{what}: the reference left {k} unwritten"
        assert torch.equal(got[k], r), f"{what}: gradient {k} differs from sks_backward's"


def check_prefill(sc, what, counts=None, offs=(0, 4), flag_list=FWD_FLAGS, dfeat=False):
    """Every plane count: the backward prefills a NaN-filled set (where the shape allows it; else the test zeroes the planes itself),
    the planes are checked, and the forward into copies of that set, under every flag variant, equals the plain forward."""
    V, C, W, H = sc.V, sc.C, sc.W, sc.H
    planes = (C + 1) * V
    ref = sc.forward(OFF)
    assert not torch.isnan(ref[0]).any() and not torch.isnan(ref[1]).any(), f"{what}: the reference left elements unwritten"
    gref = sc.backward(ref, dfeat=dfeat)
    for k, r in gref.items():
        assert r is None or not torch.isnan(r).any(), f"{what}: sks_backward left {k} unwritten"
    possible = can_prefill(W, H)
    # the rule answers only where its constants were measured (and never where the call would be refused)
    ruled = possible and W % 4 == 0 and C <= 20 and 51 <= V * sc.P <= 85
    assert (sum(_lib.prefill_planes(V, sc.P, C, W, H, 0)) > 0) == ruled, f"{what}: the rule"
    for i, n in enumerate(plane_counts(V, C) if counts is None else counts):
        nw, ng = (n + 1) // 2, n // 2
        if i % 3 == 1:
            nw, ng = ng, nw                      # (the geometry launch takes the larger share / the only plane)
        want_mean = i % 4 != 2                   # (without the mean over the views the compositing launch carries both shares)
        for off in offs:                         # off = 4: 16-byte aligned, not 128-byte aligned (the passes' `shift` is not 0)
            tag = f"{what}, {n} planes ({nw} + {ng}), outputs offset by {off} floats"
            color, inv = sc.outputs(off)
            if possible:
                g = sc.backward(ref, (color, inv), nw, ng, want_mean, dfeat)
                same_grads(g, gref if want_mean else {**gref, "mean": None}, tag)
            else:
                if n:
                    assert sc.backward(ref, (color, inv), nw, ng, want_mean, dfeat, rc_only=True) != 0, f"{tag}: not refused"
                    assert torch.isnan(color).all() and torch.isnan(inv).all(), f"{tag}: a refused call wrote"
                for zid in range(planes - n, planes):      # (what a backward would have left)
                    v, pl = divmod(zid, C + 1)
                    (inv[v, 0] if pl == C else color[v, pl]).zero_()
            pl = sc.planes_of(color, inv)
            assert (pl[planes - n:] == 0).all(), f"{tag}: a promised plane is not exactly zero"
            assert torch.isnan(pl[: planes - n]).all(), f"{tag}: an element outside the promised planes was written"
            for flags in flag_list:
                c2, i2 = sc.outputs(off)
                c2.copy_(color), i2.copy_(inv)
                same(sc.forward_prefilled(flags, c2, i2, n), ref, f"{tag}, forward flags {flags:#x}")
    return ref


@pytest.mark.parametrize("V,C", VC, ids=lambda v: str(v))
@pytest.mark.parametrize("W,H", SIZES, ids=lambda v: str(v))
def test_prefill_changes_no_bit(device, W, H, V, C):
    sc = PScene(device, W, H, V, C, "dense")
    ref = check_prefill(sc, f"{W}x{H} V={V} C={C}", dfeat=(C == 3))
    assert (ref[2] > 0).any(), "the case renders nothing"
    assert (ref[0][-1] != 0).any(), "no covered tile in the prefilled region"


@pytest.mark.parametrize("feat", ["onehot", "last"])
@pytest.mark.parametrize("W,H", SIZES[:4], ids=lambda v: str(v))
def test_covered_tiles_in_prefilled_planes(device, W, H, feat):
    """Per-plane cover rows: a composite block stores only the planes its list has features on.  The last view's last channel and
    its inverse-depth plane -- the first planes a backward prefills -- hold covered tiles."""
    for V, C in ((2, 3), (5, 17)):
        sc = PScene(device, W, H, V, C, feat)
        ref = check_prefill(sc, f"{feat} {W}x{H} V={V} C={C}", offs=(0,))
        assert (ref[0][-1, C - 1] != 0).any() and (ref[1][-1] != 0).any()
        if feat == "last":
            assert not ref[0][:, : C - 1].any()


@pytest.mark.parametrize("culled", [(1,), (3,), (0, 1, 2, 3, 4)], ids=lambda v: "culled" + "".join(map(str, v)))
def test_view_with_every_gaussian_culled(device, culled):
    V = 2 if culled == (1,) else 5
    for W, H in ((64, 48), (67, 45)):
        sc = PScene(device, W, H, V, 17, "dense", culled=culled)
        ref = check_prefill(sc, f"{W}x{H} V={V} culled {culled}")
        for v in culled:
            assert not ref[2][v].any() and not ref[0][v].any() and not ref[1][v].any()


def test_bad_counts_are_refused(device):
    sc = PScene(device, 64, 48, 2, 3, "dense")
    ref = sc.forward(OFF)
    color, inv = sc.outputs()
    for nw, ng in ((-1, 0), (0, -1), (5, 4), (9, 0)):
        assert sc.backward(ref, (color, inv), nw, ng, rc_only=True) != 0
    with pytest.raises(RuntimeError):
        sc.forward_prefilled(0, color, inv, 9)
    with pytest.raises(RuntimeError):
        sc.forward_prefilled(0, color, inv, -1)
    assert torch.isnan(color).all() and torch.isnan(inv).all()
    assert _lib.prefill_planes(2, 300, 3, 64, 48, 0) == (0, 0)                        # the binned path
    assert _lib.prefill_planes(2, 17, 3, 64, 48, _lib.SKS_NO_NT_STORES) == (0, 0)     # plain stores
    assert _lib.prefill_planes(4, 17, 17, 1000, 1000, 0) == (14, 7)                   # H36M: 56 MB + 28 MB in planes of 4 MB
    assert 14 + 7 + 9 <= 36                                                           # (with the early region at most half)
    # outside what the constants were measured on: the pair-masked 1002-wide images, other V * P, more than 20 channels
    assert _lib.prefill_planes(4, 17, 17, 1002, 1000, 0) == (0, 0)
    assert _lib.prefill_planes(2, 17, 17, 1000, 1000, 0) == (0, 0) and _lib.prefill_planes(8, 17, 17, 1000, 1000, 0) == (0, 0)
    assert _lib.prefill_planes(4, 17, 24, 1000, 1000, 0) == (0, 0)


# ------------------------------------------------------------------------------------------------------------ Workspace
class Steps:
    """Two-call steps of one case through a Workspace, each checked against the same calls on fresh tensors."""

    def __init__(self, device, prefill=(5, 3), W=160, H=128, V=3, seed=3):
        c = util.make_case(seed=seed, W=W, H=H, scale_log=4.0, n_views=V)
        t = lambda a: torch.tensor(a, device=device)
        self.dev = device
        self.views = R.ViewBatch.from_cameras([cam.to(device) for cam in c.cams])
        self.args = (t(c.means), t(c.feat), t(c.opac), t(c.scales), t(c.quats), None)
        self.dLc, self.dLi = t(c.dL_color), t(c.dL_inv)
        self.ws = R.Workspace(prefill=prefill)
        self.n = 0

    def change(self):
        """Parameters and upstream gradient changed IN PLACE: the recorded calls stay the recorded calls."""
        self.n += 1
        self.args[0].add_(0.003 * self.n)
        self.args[2].mul_(0.97)
        self.dLc.mul_(-1.01), self.dLi.add_(0.01)

    def reference(self):
        color, inv, radii, st = R.forward_views(self.views, *self.args)
        g = R.backward_views(st, *self.args, self.dLc, self.dLi, want_mean=True)
        return color, inv, radii, g

    def forward(self, **kw):
        return R.forward_views(self.views, *self.args, workspace=self.ws, **kw)

    def backward(self, st):
        return R.backward_views(st, *self.args, self.dLc, self.dLi, workspace=self.ws, want_mean=True)

    def poison_unpromised(self):
        """NaN over everything of the set the next forward renders into that no note promises to be zero."""
        pf = self.ws._pf
        if pf is None or pf.sets[1] is None:
            return
        color, inv = pf.sets[1 - pf.cur] if pf.note is not None else pf.sets[pf.cur]
        n = pf.note[0] if pf.note is not None else 0
        V, C = color.shape[:2]
        for zid in range((C + 1) * V - n):
            v, pl = divmod(zid, C + 1)
            (inv[v, 0] if pl == C else color[v, pl]).fill_(NAN)

    def check_fwd(self, out, ref, tag):
        for k, name in enumerate(("color", "invdepth", "radii")):
            assert torch.equal(out[k], ref[k]), f"{tag}: {name} differs from the fresh-tensor call"

    def check_bwd(self, g, ref, tag):
        for k, r in ref[3].items():
            if r is not None:
                assert torch.equal(g[k], r), f"{tag}: gradient {k} differs from the fresh-tensor call"

    def step(self, tag, poison=True):
        self.change()
        ref = self.reference()
        if poison:
            self.poison_unpromised()
        out = self.forward()
        self.check_fwd(out, ref, tag)
        g = self.backward(out[3])
        self.check_bwd(g, ref, tag)
        self.check_fwd(out, ref, tag + " (the image after its own backward)")
        return out, g, ref


@pytest.mark.parametrize("prefill", [None, (5, 3), (0, 4), (20, 7), (27, 27)], ids=str)
def test_workspace_steps_equal_fresh_calls(device, prefill):
    s = Steps(device, prefill)
    seen = set()
    for i in range(8):
        out, _, _ = s.step(f"prefill={prefill} step {i}")
        seen.add(out[0].data_ptr())
    torch.cuda.synchronize(device)
    assert len(seen) == 2, "the forwards did not alternate between two output sets"
    assert s.ws._pf.note is not None


def test_prefill_off_is_one_set_and_equal(device):
    s0, s1 = Steps(device, 0), Steps(device, None)
    for i in range(4):
        o0, g0, _ = s0.step(f"prefill=0 step {i}")
        o1, g1, _ = s1.step(f"default step {i}")
        s0.check_fwd(o0, o1, "prefill=0 against the default")
        s0.check_bwd(g0, (None, None, None, g1), "prefill=0 against the default")
    assert s0.ws._pf is None and ("fwd", "color2") not in {k[0] for k in s0.ws._t}
    assert ("fwd", "color2") in {k[0] for k in s1.ws._t}


def test_workspace_hand_overs(device):
    """Two forwards in a row with everything poisoned in between, two backwards in a row, a one-call step between two-call steps,
    a want_aux forward, a forward on another stream, flags patched in the live record -- each followed by ordinary steps."""
    s = Steps(device)
    for i in range(3):
        s.step(f"warm {i}")
    # two forwards in a row, everything poisoned in between
    s.change()
    ref = s.reference()
    s.forward()
    for t in s.ws._pf.sets:
        t[0].fill_(NAN), t[1].fill_(NAN)
    out = s.forward()
    s.check_fwd(out, ref, "second of two forwards")
    # two backwards in a row
    g = s.backward(out[3])
    g = s.backward(out[3])
    s.check_bwd(g, ref, "second of two backwards")
    s.step("after two backwards")
    # a one-call step between two-call steps
    s.change()
    ref = s.reference()
    r = R.forward_backward_views(s.views, *s.args, s.dLc, s.dLi, workspace=s.ws, want_mean=True)
    s.check_fwd(r, ref, "one-call step")
    s.check_bwd(r[4], ref, "one-call step")
    s.step("after the one-call step")
    s.step("second after the one-call step")
    # a want_aux forward (the validating path: it writes the first set)
    s.change()
    ref = s.reference()
    aux = s.forward(want_aux=True)
    s.check_fwd(aux, ref, "want_aux forward")
    s.step("after the want_aux forward", poison=False)
    s.step("second after the want_aux forward")
    # a forward on another stream: the note is for the stream of the backward
    s.change()
    ref = s.reference()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        out = s.forward()
    torch.cuda.current_stream(device).wait_stream(side)
    s.check_fwd(out, ref, "forward on another stream")
    s.check_bwd(s.backward(out[3]), ref, "backward after the forward on another stream")
    s.step("after the side-stream forward")
    # flags patched in the live record between calls (what bench.py and Workspace.tune do)
    base = s.ws._plans["fwd"].args[_lib.FWD["flags"]]
    for bits in (3 << 8, _lib.SKS_NO_NT_STORES, _lib.SKS_EARLY_FILL(7), OFF, 0):
        s.ws._plans["fwd"][2][_lib.FWD["flags"]] = base | bits
        s.step(f"flags | {bits:#x}")
        s.step(f"flags | {bits:#x}, second")
    torch.cuda.synchronize(device)


def test_backward_recorded_with_plain_stores(device):
    """The backward's recorded flags carry the forward's store kind as it was when the step was recorded (here: a tuned plain-stores
    pick); the forward's live flags are re-tuned to non-temporal stores afterwards.  The counts follow the forward's live flags,
    and the backward's own SKS_NO_NT_STORES bit is no reason to refuse them."""
    s = Steps(device, None)
    key = (s.args[0].device.index, 3, s.args[0].shape[0], s.args[1].shape[-1], 160, 128, "workspace")
    had = R._FILL_TUNE.get(key)
    R._FILL_TUNE[key] = _lib.SKS_NO_NT_STORES
    try:
        for i in range(3):
            s.step(f"plain stores {i}")
        live = s.ws._plans["fwd"].args
        assert live[_lib.FWD["flags"]] & _lib.SKS_NO_NT_STORES and s.ws._plans["bwd"].args[_lib.BWD["flags"]] & _lib.SKS_NO_NT_STORES
        assert s.ws._pf.note is None and s.ws._pf.sets[1] is None          # (plain stores: the rule answers 0 / 0)
        live[_lib.FWD["flags"]] &= ~_lib.SKS_NO_NT_STORES
        seen = set()
        for i in range(4):
            out, _, _ = s.step(f"re-tuned to non-temporal {i}")
            seen.add(out[0].data_ptr())
        assert len(seen) == 2 and s.ws._pf.note is not None
    finally:
        if had is None:
            R._FILL_TUNE.pop(key, None)
        else:
            R._FILL_TUNE[key] = had
    torch.cuda.synchronize(device)


def test_feature_gradient_does_not_prefill_by_rule(device):
    s = Steps(device, None)
    for i in range(3):
        s.change()
        out = s.forward()
        R.backward_views(out[3], *s.args, s.dLc, s.dLi, workspace=s.ws, want_dfeatures=True)
    assert s.ws._pf.sets[1] is None and s.ws._pf.note is None
    torch.cuda.synchronize(device)


def test_workspace_shape_change(device):
    a, b = Steps(device, (5, 3)), Steps(device, (4, 2), W=96, H=64, V=2, seed=4)
    b.ws = a.ws
    for i in range(3):
        a.step(f"first shape {i}")
    for i in range(3):
        b.step(f"second shape {i}", poison=i > 0)
    for i in range(3):
        a.step(f"first shape again {i}", poison=i > 0)
    torch.cuda.synchronize(device)


def test_capture_with_a_note_pending(device):
    """A step captured while a note is pending: the captured calls neither prefill nor take the planes, the replays (into
    poisoned outputs) and the eager steps behind them are bit-equal to fresh-tensor calls, and the workspace has stopped."""
    s = Steps(device)
    for i in range(3):
        s.step(f"warm {i}")
    assert s.ws._pf.note is not None
    s.change()
    ref = s.reference()
    side = torch.cuda.Stream(device)            # (the side-stream warm-up of tests/test_early_fill_gpu.py's graph test)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        o = s.forward()
        s.backward(o[3])
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = s.forward()
        grads = s.backward(out[3])
    assert s.ws._pf_off
    for rep in range(2):
        for t in s.ws._pf.sets:
            t[0].fill_(NAN), t[1].fill_(NAN)
        out[2].fill_(-7)
        for v in grads.values():
            if v is not None:
                v.fill_(NAN)
        g.replay()
        torch.cuda.synchronize(device)
        s.check_fwd(out, ref, f"graph replay {rep}")
        s.check_bwd(grads, ref, f"graph replay {rep}")
    for i in range(3):
        o, _, _ = s.step(f"eager step {i} behind the graph", poison=False)
        assert o[0].data_ptr() == out[0].data_ptr()
    assert s.ws._pf.note is None


def test_hook_counts_one_sample_per_forward(device):
    s = Steps(device)
    _lib.prof_enable(True, every=1)
    _lib.prof_read(0), _lib.prof_read(1)
    try:
        for i in range(6):
            s.step(f"hooked step {i}", poison=False)
        torch.cuda.synchronize(device)
        n_fwd = 6 * 2                            # (each step: the fresh-tensor reference's forward and the workspace's)
        assert _lib.prof_count(0) == n_fwd
        ms, n = _lib.prof_read(0)
        assert n == n_fwd and ms > 0
        _lib.prof_enable(True, every=3)          # a stride: the backward in front of a sampled forward brackets its launches
        ws_only = 0
        for i in range(6):
            s.change()
            out = s.forward()
            s.backward(out[3])
            ws_only += 1
        torch.cuda.synchronize(device)
        assert _lib.prof_count(0) == (ws_only + 2) // 3
        ms, n, q = _lib.prof_read_quantiles(0)
        assert n == (ws_only + 2) // 3 and q[0] > 0
        _lib.prof_enable(True, every=1)          # every launch, no other forward in between: every sample is two intervals
        for i in range(4):
            s.change()
            out = s.forward()
            s.backward(out[3])
        torch.cuda.synchronize(device)
        assert _lib.prof_count(0) == 4
        assert _lib.prof_read(0)[1] == 4
        # The sample holds BOTH intervals.  The same steps through a prefilling workspace and through one that does not prefill:
        # the first one's kind-0 sample spans the forward and the backward's two launches, the second one's the forward alone, so
        # it is longer by at least the compositing backward's own duration (kind 1, the first of the two launches in the bracket)
        # less what the forward saves -- and at 160 x 128 the whole image is 0.2 MB per plane, 30 ns of HBM time each.  Half of
        # the kind-1 median leaves room for event granularity; a sample without the parked interval differs by about nothing.
        off = Steps(device, 0)
        med = {}
        for name, x in (("prefill", s), ("off", off)):
            for i in range(3):
                x.step(f"{name} warm {i}", poison=False)
            torch.cuda.synchronize(device)
            _lib.prof_enable(True, every=1)
            _lib.prof_read(0), _lib.prof_read(1)
            for i in range(16):
                x.change()
                out = x.forward()
                x.backward(out[3])
            torch.cuda.synchronize(device)
            f, b = _lib.prof_read_quantiles(0), _lib.prof_read_quantiles(1)
            assert f[1] == 16 and b[1] == 16
            med[name] = (f[2][1] * 1e3, b[2][1] * 1e3)
        print(f"kind-0 median us: prefilling {med['prefill'][0]:.2f}, off {med['off'][0]:.2f}; kind-1 median us: "
              f"{med['prefill'][1]:.2f}, {med['off'][1]:.2f}")
        assert med["prefill"][0] >= med["off"][0] + 0.5 * med["off"][1]
    finally:
        _lib.prof_enable(False)
        _lib.prof_read(0), _lib.prof_read(1)
