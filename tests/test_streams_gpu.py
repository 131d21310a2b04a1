"""The one-call forward + backward (sks_forward_backward, rasterizer.forward_backward_views) held to its stream-ordering contract
(include/skelsplat_hip.h) on every path it can take, not only to its numbers.

A missing wait between two streams only shows when the stream that should have been waited for is still busy.  The probes below
make one stream deliberately late with the library's own bounded idle kernel (sks_prof_spin: one wavefront that spins on the
wall clock and ends by itself, so a broken ordering gives wrong numbers, never a hang), poison every tensor the call will write
with NaN first (workspace tensors are reused: a stale result could equal the right one), and read the results at once from the
stream the contract names:
  join=True   the second stream is late; the results are cloned on the current stream right behind the call;
  join=False  the current stream is late; the gradients are cloned on Workspace.aux_stream right behind the call, before the
              caller's Workspace.join -- or the next call through the workspace makes the join itself (Workspace.settle).
The reference is forward_views + backward_views on fresh tensors, bit for bit (the binned path's feature gradient is summed with
float atomics: the tolerance test_view_groups_on_the_binned_path_change_no_bit uses)."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from tests import util
from skelsplat_amd import _lib, rasterizer as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# How late the skewed stream is.  The calls under test take tens of microseconds on the GPU (the 31-view scene at its size
# ~0.1 ms) and at most a couple of milliseconds of host time (a first, recording call validates and allocates); 20 ms leaves
# an order of magnitude over both, so the probe's clones are enqueued while the late stream is still spinning, and it costs
# ~20 ms per probe.
SPIN_US = 20000.0
CALLS = 4           # the first (recording) call, a replay, then two replays with the parameters and dL changed in place
BIG_CAP = 1 << 15   # binned rows: an arena no scene here fills (asserted), so the probes can skip the capacity read-back


def t(a, dev):
    return torch.tensor(a, device=dev)


def spin(stream):
    _lib.check(_lib.load().sks_prof_spin(SPIN_US, ctypes.c_void_p(stream.cuda_stream)), "sks_prof_spin")


def poison(tensors):
    for x in tensors:
        if x is not None:
            x.fill_(float("nan") if x.is_floating_point() else -7)


class PoisonedWorkspace(R.Workspace):
    """A Workspace whose output tensors come out of allocation filled with NaN (-7 for radii), on the current stream: the first,
    recording call of a shape writes into them, and the caching allocator could otherwise hand it memory that already holds the
    right numbers (the reference's own, just freed)."""
    OUTPUTS = {("fwd", "color"), ("fwd", "invdepth"), ("fwd", "radii"), ("bwd", "m3"), ("bwd", "m2"), ("bwd", "op"), ("bwd", "cov"),
               ("bwd", "sc"), ("bwd", "rot"), ("bwd", "feat"), ("bwd", "m3mean")}

    def get(self, name, shape, dtype, device):
        fresh = (name, tuple(shape), dtype, device) not in self._t
        x = super().get(name, shape, dtype, device)
        if fresh and name in self.OUTPUTS:
            poison([x])
        return x


def written(out):
    """Every tensor a forward_backward_views result holds that the call writes."""
    return [out[0], out[1], out[2]] + [v for v in out[4].values() if v is not None]


def same(got, ref, binned, tag):
    for k, v in ref.items():
        if v is None:
            assert got.get(k) is None, (tag, k)
        elif binned and k == "features":
            torch.testing.assert_close(got[k], v, rtol=1e-4, atol=1e-5 * float(v.abs().max()), msg=lambda m: f"{tag} {k}: {m}")
        else:
            assert torch.equal(got[k], v), (tag, k, float((got[k] - v).abs().nan_to_num(float("inf")).max()))


class Scene:
    """A case on the device plus the switches of one matrix row; reference() = the two calls on fresh tensors."""

    def __init__(self, c, dev, fb_kw, fwd_kw=None, shard=False):
        self.c, self.dev = c, dev
        self.views = R.ViewBatch.from_cameras([cam.to(dev) for cam in c.cams])
        self.args = tuple(t(a, dev) for a in (c.means, c.feat, c.opac, c.scales, c.quats)) + (None,)
        self.dL, self.dLi = t(c.dL_color, dev), t(c.dL_inv, dev)
        self.fb_kw = dict(fb_kw)
        self.fwd_kw = dict(fwd_kw or {})      # what forward_views needs to take the same path (force_binned, tune_flags, ...)
        self.binned = c.P > _lib.SKS_SMALL_P or self.fwd_kw.get("force_binned", False)
        self.shard = torch.zeros((len(c.cams) + 1, c.P, 3), device=dev) if shard else None

    def change(self):
        """Between replays: the parameters move in place, dL flips sign and shrinks (the same arithmetic on the host copies)."""
        with torch.no_grad():
            self.args[0].add_(2.0)
            self.args[3].mul_(1.0625)
            self.dL.mul_(-0.5)
            self.dLi.mul_(-0.5)
        self.c.means = (self.c.means + np.float32(2.0)).astype(np.float32)
        self.c.scales = (self.c.scales * np.float32(1.0625)).astype(np.float32)
        self.c.dL_color = (self.c.dL_color * np.float32(-0.5)).astype(np.float32)
        self.c.dL_inv = (self.c.dL_inv * np.float32(-0.5)).astype(np.float32)

    def bkw(self):
        return {k: v for k, v in self.fb_kw.items() if k in ("bg", "want_dfeatures", "want_mean")}

    def reference(self, dL=None):
        tf = self.fb_kw.get("tune_flags", 0)
        col, inv, rad, st = R.forward_views(self.views, *self.args, tune_flags=tf, **self.fwd_kw)
        g = R.backward_views(st, *self.args, self.dL if dL is None else dL, self.dLi, tune_flags=tf, **self.bkw())
        torch.cuda.synchronize()
        return col, inv, rad, g

    def call(self, ws, dL=None, **kw):
        extra = dict(out_means3D=self.shard[:-1]) if self.shard is not None else {}
        return R.forward_backward_views(self.views, *self.args, self.dL if dL is None else dL, self.dLi, workspace=ws,
                                        **extra, **self.fb_kw, **kw)


def probe_join(s, ws, prev, tag):
    """join=True with the second stream late: every output and gradient cloned on the current stream right behind the call."""
    ref = s.reference()
    if prev is not None:
        poison(written(prev))
    if s.shard is not None:
        poison([s.shard])
    spin(ws.aux_stream(s.dev.index))
    out = s.call(ws, join=True)
    col, inv, rad = out[0].clone(), out[1].clone(), out[2].clone()
    g = {k: (None if v is None else v.clone()) for k, v in out[4].items()}
    shard = s.shard.clone() if s.shard is not None else None
    torch.cuda.synchronize()
    assert torch.equal(col, ref[0]) and torch.equal(inv, ref[1]) and torch.equal(rad, ref[2]), (tag, "forward")
    same(g, ref[3], s.binned, tag)
    if shard is not None:
        assert torch.equal(shard[:-1], ref[3]["means3D"]), (tag, "out_means3D")
    return out


def probe_no_join(s, ws, prev, tag, settle=False):
    """join=False with the current stream late: the gradients (and the exchange rows) cloned on the second stream right behind
    the call, then the caller's join -- or, settle=True, no join: the next call through the workspace, with another dL, makes it."""
    ref = s.reference()
    if settle:     # (the second call's reference first: computing it later would synchronise what the probe looks at)
        dL2 = s.dL * -1.5
        ref2 = s.reference(dL2)
    cur, aux = torch.cuda.current_stream(s.dev), ws.aux_stream(s.dev.index)
    if prev is not None:
        poison(written(prev))
    if s.shard is not None:
        poison([s.shard])
    aux.wait_stream(cur)          # (the poison is in place on both streams before anything is late)
    spin(cur)
    out = s.call(ws, join=False)
    with torch.cuda.stream(aux):
        g = {k: (None if v is None else v.clone()) for k, v in out[4].items()}
        shard = s.shard.clone() if s.shard is not None else None
    if settle:
        out2 = s.call(ws, dL=dL2, join=True)
        torch.cuda.synchronize()
        same(out2[4], ref2[3], s.binned, tag + " (the call that settles)")
        assert torch.equal(out2[0], ref2[0]), (tag, "the call that settles: forward")
    else:
        ws.join(s.dev.index)
        torch.cuda.synchronize()
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2]), (tag, "forward")
    same(g, ref[3], s.binned, tag + " (on the second stream)")
    if shard is not None:
        assert torch.equal(shard[:-1], ref[3]["means3D"]), (tag, "out_means3D on the second stream")
    return out


def run_row(s, join, label, check_oracle=False):
    ws = PoisonedWorkspace()
    torch.cuda.synchronize()
    prev = None
    for rep in range(CALLS):
        if rep >= 2:
            s.change()
        tag = f"{label} join={join} call {rep}"
        prev = probe_join(s, ws, prev, tag) if join else probe_no_join(s, ws, prev, tag)
        if check_oracle:
            torch.cuda.synchronize()
            hold_to_oracle(s, prev, tag)
    assert "fwd" in ws._plans and "bwd" in ws._plans, label      # (the later calls were replays through the combined entry point)
    if not join:      # the caller who never joins: the next call settles
        probe_no_join(s, ws, prev, f"{label} join=False, settled by the next call", settle=True)
    torch.cuda.synchronize()


def hold_to_oracle(s, out, tag):
    """The high-precision restatement: forward bit for bit, every gradient within the tolerance the oracle tests use."""
    c = s.c
    for v in range(len(c.cams)):
        o = util.oracle_forward(c, v)
        b = util.oracle_backward(c, v, o)
        assert np.array_equal(out[2][v].cpu().numpy(), o["radii"]), (tag, v, "radii")
        assert np.array_equal(out[0][v].cpu().numpy(), o["color"]), (tag, v, "color")
        g = out[4]
        for k, ko in (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
                      ("rotations", "dL_drotations"), ("cov3D", "dL_dcov3D"), ("features", "dL_dcolors")):
            if g.get(k) is not None:
                util.assert_close(f"{tag} view {v} {k}", g[k][v].cpu(), b[ko], rtol=1e-3, atol_scale=1e-5)


def binned_case(n_views, seed=35, W=152, H=120):
    return util.make_case(seed=seed, W=W, H=H, scale_log=3.6, n_skeletons=16, pitch=150.0, n_views=n_views)   # P = 272


def binned_kw(s):
    """The binned rows skip the synchronous capacity read-back (it would hold the host until the late stream's forward is through
    and shrink the window the probe looks through) and take an arena the reference shows is big enough."""
    col, inv, rad, st = R.forward_views(s.views, *s.args, bin_capacity=BIG_CAP, **s.fwd_kw)
    torch.cuda.synchronize()
    assert st.bin_capacity == BIG_CAP and int(st.num_rendered_dev[:len(s.c.cams)].max()) <= BIG_CAP // 2
    s.fb_kw.update(bin_capacity=BIG_CAP, check_capacity=False)
    s.fwd_kw.update(bin_capacity=BIG_CAP)


ROWS = {
    # small path, backward beside the forward on the second stream: V x P = 51 <= 400
    "small-overlapped": lambda dev: Scene(util.make_case(seed=4, W=208, H=160, scale_log=4.2, n_views=3), dev,
                                          dict(want_mean=True, want_dfeatures=True), shard=True),
    # small path, 31 Panoptic-shaped views (V x P = 589 > 400): sequential when joined, overlapped with join=False
    "small-crowded": lambda dev: Scene(util.make_case(seed=7, W=64, H=48, scale_log=3.4, n_views=31, dataset="panoptic"), dev,
                                       dict(want_mean=True)),
    "overlap=False": lambda dev: Scene(util.make_case(seed=5, W=120, H=96, scale_log=4.0, n_views=3), dev,
                                       dict(overlap=False, want_mean=True, want_dfeatures=True)),
    # the debug switch: a synchronising stage check, so the call runs its halves one after the other on the current stream.  (Its
    # last stage check synchronises that stream behind the backward, so a missing hand-over to the second stream has no window
    # to show in here: these rows hold the results, the stream order on that branch is held by the P == 0 and binned rows.)
    "debug": lambda dev: Scene(util.make_case(seed=6, W=120, H=96, scale_log=4.0, n_views=3), dev,
                               dict(tune_flags=_lib.SKS_DEBUG_SYNC, want_mean=True)),
    # binned path (P > 256) in view groups asked for by the caller: group g's backward beside group g + 1's forward
    "binned-groups2": lambda dev: Scene(binned_case(5), dev, dict(tune_flags=_lib.SKS_BIN_GROUPS(2), want_dfeatures=True)),
    "binned-groups3": lambda dev: Scene(binned_case(5), dev, dict(tune_flags=_lib.SKS_BIN_GROUPS(3), want_mean=True)),
    "binned-debug": lambda dev: Scene(binned_case(3), dev, dict(tune_flags=_lib.SKS_DEBUG_SYNC)),
}


@pytest.mark.parametrize("join", [True, False], ids=["join", "no_join"])
@pytest.mark.parametrize("row", list(ROWS))
def test_one_call_keeps_its_stream_order(device, row, join):
    s = ROWS[row](device)
    if s.binned:
        binned_kw(s)
    run_row(s, join, row)


@pytest.mark.parametrize("join", [True, False], ids=["join", "no_join"])
def test_one_call_on_the_binned_path_in_one_group_keeps_its_stream_order_and_the_oracle(device, join):
    """The binned path's default (one view group: the forward, then the backward, on the current stream) at four views, held to the
    stream contract and to the CPU oracle -- the one-call binned path at more than one view against the high-precision
    restatement, not only against the two calls."""
    s = Scene(binned_case(4, seed=36), device, dict(want_dfeatures=True))
    binned_kw(s)
    run_row(s, join, "binned-one-group", check_oracle=True)


@pytest.mark.parametrize("join", [True, False], ids=["join", "no_join"])
def test_one_call_redoes_an_overflowed_replay_in_stream_order(device, join):
    """The synchronous capacity check with an arena sized for the first calls: the parameters grow between replays, the replay's
    pair counts overflow the recorded arena, and the call redoes itself through the two calls with a grown one -- in stream order
    for both kinds of caller, with the right numbers."""
    c = binned_case(3, seed=37, W=148, H=116)          # (a shape no other test uses: the arena hints are per shape)
    s = Scene(c, device, dict(want_mean=True), fwd_kw=dict(bin_capacity=BIG_CAP))    # (the reference never uses the hint)
    col, inv, rad, st = R.forward_views(s.views, *s.args, bin_capacity=BIG_CAP)
    torch.cuda.synchronize()
    need = int(st.num_rendered_dev[:len(c.cams)].max())
    key = (device.index, len(c.cams), c.P, c.C, c.W, c.H)
    R._BIN_CAP_HINT[key] = need + 64                    # as if this scene had sized the arena: room for the first calls only
    ws = PoisonedWorkspace()
    prev = None
    for rep in range(CALLS):
        if rep == 2:
            with torch.no_grad():
                s.args[3].mul_(1.5)                     # larger splats: more (Gaussian, tile) pairs than the arena holds
            s.c.scales = (s.c.scales * np.float32(1.5)).astype(np.float32)
        tag = f"overflow join={join} call {rep}"
        prev = probe_join(s, ws, prev, tag) if join else probe_no_join(s, ws, prev, tag)
        if rep == 2:
            assert R._BIN_CAP_HINT[key] > need + 64, "the replay did not overflow: the row tests nothing"
    R._BIN_CAP_HINT.pop(key, None)


@pytest.mark.parametrize("join", [True, False], ids=["join", "no_join"])
def test_one_call_with_no_gaussians_keeps_its_stream_order(device, join):
    """P == 0: forward_backward_views (the two calls under the hood), then the C entry point itself -- it runs its two halves on
    `stream` one after the other, and with SKS_FB_NO_JOIN must leave what it wrote ordered on aux_stream as well."""
    c = util.make_case(seed=8, W=96, H=64, n_views=3)
    V, C, W, H = len(c.cams), c.C, c.W, c.H
    views = R.ViewBatch.from_cameras([cam.to(device) for cam in c.cams])
    empty = lambda *s: torch.zeros(s, device=device)
    args = (empty(0, 3), empty(0, C), empty(0, 1), empty(0, 3), empty(0, 4), None)
    dL, dLi = t(c.dL_color, device), t(c.dL_inv, device)
    ws = R.Workspace()
    cur, aux = torch.cuda.current_stream(device), ws.aux_stream(device.index)
    for rep in range(3):
        out = R.forward_backward_views(views, *args, dL, dLi, workspace=ws, want_mean=True, join=join)
        with torch.cuda.stream(cur if join else aux):
            col, g = out[0].clone(), {k: (None if v is None else v.clone()) for k, v in out[4].items()}
        ws.join(device.index)
        torch.cuda.synchronize()
        assert torch.equal(col, torch.zeros((V, C, H, W), device=device)) and g["means3D"].shape == (V, 0, 3), rep
    # the C entry point: outputs poisoned, the late stream spinning, what the call wrote read on the stream the contract names
    lib = _lib.load()
    color, inv = torch.empty((V, C, H, W), device=device), torch.empty((V, 1, H, W), device=device)
    for rep in range(3):
        poison([color, inv])
        aux.wait_stream(cur)
        spin(aux if join else cur)
        rc = lib.sks_forward_backward(V, 0, C, W, H, views.viewmatrix.data_ptr(), views.projmatrix.data_ptr(), views.tanfovx,
                                      views.tanfovy, None, None, None, None, None, None, 1.0, 0, color.data_ptr(), inv.data_ptr(),
                                      None, None, None, 0, None, None, dL.data_ptr(), dLi.data_ptr(), None,
                                      *[None] * 8, cur.cuda_stream, aux.cuda_stream, 0 if join else _lib.SKS_FB_NO_JOIN)
        _lib.check(rc, "sks_forward_backward")
        with torch.cuda.stream(cur if join else aux):
            col, iv = color.clone(), inv.clone()
        ws.join(device.index)
        torch.cuda.synchronize()
        assert torch.equal(col, torch.zeros_like(col)) and torch.equal(iv, torch.zeros_like(iv)), (join, rep)


_GROUPS_CHILD = textwrap.dedent("""
    import sys, torch
    sys.path.insert(0, sys.argv[1])
    from tests import util
    from tests.test_streams_gpu import binned_case, t, same
    from skelsplat_amd import _lib, rasterizer as R
    dev = torch.device("cuda:0")
    ref = {k: (v.to(dev) if torch.is_tensor(v) else {n: (None if x is None else x.to(dev)) for n, x in v.items()})
           for k, v in torch.load(sys.argv[2]).items()}
    c = binned_case(5, seed=38)
    views = R.ViewBatch.from_cameras([cam.to(dev) for cam in c.cams])
    args = tuple(t(a, dev) for a in (c.means, c.feat, c.opac, c.scales, c.quats)) + (None,)
    dL, dLi, dL2 = t(c.dL_color, dev), t(c.dL_inv, dev), t(c.dL_color, dev) * -0.75
    ws = R.Workspace()
    for rep in range(3):        # the recording call, then replays through the combined entry point
        out = R.forward_backward_views(views, *args, dL, dLi, workspace=ws, want_dfeatures=True)
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref["color"]), "one call: forward"
    same(out[4], ref["g1"], True, "one call")
    st = out[3]
    g2 = R.backward_views(st, *args, dL2, dLi, want_dfeatures=True)
    torch.cuda.synchronize()
    same(g2, ref["g2"], True, "backward_views on the one call's state")
    # sks_backward through the state's recorded plan, dL swapped for dL2, into fresh tensors
    a = list(ws._plans["bwd"].args)
    g3 = {k: torch.full_like(v, float("nan")) for k, v in ref["g2"].items() if v is not None}
    a[_lib.BWD["dL_dout_color"]] = dL2.data_ptr()
    for k, name in (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
                    ("rotations", "dL_drotations"), ("cov3D", "dL_dcov3D"), ("features", "dL_dfeatures")):
        a[_lib.BWD[name]] = g3[k].data_ptr()
    a[_lib.BWD["dL_dmeans3D_mean"]] = None
    _lib.check(R._replay(_lib.load().sks_backward, a, 0), "sks_backward")
    torch.cuda.synchronize()
    same(g3, ref["g2"], True, "sks_backward through the recorded plan")
    print("groups child ok")
""")


def test_view_group_count_is_the_same_for_every_entry_point(device, tmp_path):
    """SKS_BIN_GROUPS in the environment (read once per process: this runs in a child process of its own) lays the binned forward
    of sks_forward_backward out in three view groups; a later backward_views / sks_backward on the state it returned must walk
    the same three groups -- it used to walk group 0 alone and drop the other views' gradients.  The reference, computed here
    without groups: the two calls, with the second upstream gradient."""
    c = binned_case(5, seed=38)
    views = R.ViewBatch.from_cameras([cam.to(device) for cam in c.cams])
    args = tuple(t(a, device) for a in (c.means, c.feat, c.opac, c.scales, c.quats)) + (None,)
    dL, dLi, dL2 = t(c.dL_color, device), t(c.dL_inv, device), t(c.dL_color, device) * -0.75
    col, inv, rad, st = R.forward_views(views, *args)
    g1 = R.backward_views(st, *args, dL, dLi, want_dfeatures=True)
    g2 = R.backward_views(st, *args, dL2, dLi, want_dfeatures=True)
    torch.cuda.synchronize()
    assert (rad > 0).sum() > 0 and g2["means3D"][4].abs().max() > 0      # (the last group's views see the scene)
    cpu = lambda g: {k: (None if v is None else v.cpu()) for k, v in g.items()}
    torch.save(dict(color=col.cpu(), g1=cpu(g1), g2=cpu(g2)), str(tmp_path / "ref.pt"))
    env = dict(os.environ, SKS_BIN_GROUPS="3")
    r = subprocess.run([sys.executable, "-c", _GROUPS_CHILD, ROOT, str(tmp_path / "ref.pt")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "groups child ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
