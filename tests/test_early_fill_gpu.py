"""The early fill of the small-path forward (k_geom_fwd_fill: the geometry launch zeroes the call's last E planes, the fill +
composite launch streams the rest) changes no result bit: with SKS_NO_EARLY_FILL and with every value of the E field,
out_color, out_invdepth, radii and the geometry records are the same bits (torch.equal).  Every forward here writes into outputs
pre-filled with NaN, so a tile nobody wrote shows; the flag-off call is the reference (the oracle tests hold it to the CPU
oracle).

Shapes: the smallest at which the two-launch layout can go wrong -- (64, 48) 16-byte stores, (66, 48) the pair-masked HALF mode,
(67, 45) 4-byte stores and a last band of 13 rows, (1000, 40) linear passes that are not whole rows, (1024, 24) row-aligned
fill blocks in the main launch beside the linear ones of the early region; V = 1, 2, 5 with C = 3, 17 put the first early plane
inside a view, on a view boundary ((V, C) = (5, 3): E = 4 and 8 of 20 planes) and so far forward that the composite blocks
(4 * P * V of them) outnumber the rows left to the main launch."""
import numpy as np
import pytest
import torch

from tests import util
from skelsplat_amd import _lib, rasterizer as R

pytestmark = pytest.mark.gpu

OFF = _lib.SKS_NO_EARLY_FILL
SIZES = [(64, 48), (66, 48), (67, 45), (1000, 40), (1024, 24)]
VC = [(1, 3), (2, 17), (5, 3), (5, 17)]


class Scene:
    """A seeded skeleton case on the device with features of C channels of one of three kinds."""

    def __init__(self, dev, W, H, V, C, feat="dense", culled=()):
        # (wide and flat images: a short focal length keeps the skeleton inside the few rows)
        c = util.make_case(seed=7, W=W, H=H, n_views=V, scale_log=4.3, fxmul=0.2 * 1000.0 / W if W >= 1000 else 1.0, with_dL=False)
        self.W, self.H, self.V, self.C, self.P = W, H, V, C, c.P
        rng = np.random.default_rng(11)
        if feat == "dense":
            f = rng.uniform(0.1, 1.0, (c.P, C))
        elif feat == "onehot":      # what the skeleton configs use, a channel per Gaussian: Gaussian j has channel (C - 1 - j) % C
            f = np.zeros((c.P, C))  # (Gaussian 0, in sight of every view of these cases, has the last one)
            f[np.arange(c.P), (C - 1 - np.arange(c.P)) % C] = 1.0
        else:                       # "last": the only non-zero feature is the LAST channel of Gaussian 0 -- and every Gaussian
            f = np.zeros((c.P, C))  # covers its tiles on the inverse-depth plane, the last plane of each view
            f[0, C - 1] = 0.7
        t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
        self.params = (t(c.means), t(f), t(c.opac), t(c.scales), t(c.quats))
        vm, pm, tanx, tany, _ = R.ViewBatch.camera_rows([cam.to(dev) for cam in c.cams])
        vm = vm.clone()
        for v in culled:            # the whole skeleton far behind this view's camera: every Gaussian culled
            vm[v, 14] -= 1.0e6
        self.views = R.ViewBatch(vm, pm, tanx, tany, W, H)
        self.dev = dev
        self.gbytes = _lib.scratch_bytes(V, c.P, C, W, H, 0)[0]

    def forward(self, flags, off=0):
        """One sks_forward through the C ABI into NaN-filled outputs that start `off` floats into their allocation."""
        V, C, H, W, P, dev = self.V, self.C, self.H, self.W, self.P, self.dev
        nan = float("nan")
        color = torch.full((V * C * H * W + off,), nan, device=dev)[off:].view(V, C, H, W)
        inv = torch.full((V * H * W + off,), nan, device=dev)[off:].view(V, 1, H, W)
        radii = torch.full((V, P), -7, dtype=torch.int32, device=dev)
        geom = torch.zeros((self.gbytes,), dtype=torch.uint8, device=dev)
        means, feat, opac, scales, quats = self.params
        vw = self.views
        args = [V, P, C, W, H, vw.viewmatrix.data_ptr(), vw.projmatrix.data_ptr(), vw.tanfovx, vw.tanfovy, means.data_ptr(),
                feat.data_ptr(), opac.data_ptr(), scales.data_ptr(), quats.data_ptr(), None, 1.0, int(flags),
                color.data_ptr(), inv.data_ptr(), radii.data_ptr(), geom.data_ptr(), None, 0, None, None, None,
                torch.cuda.current_stream(dev).cuda_stream]
        _lib.check(_lib.load().sks_forward(*args), "sks_forward")
        return color, inv, radii, geom


def same(got, ref, what):
    for name, g, r in zip(("out_color", "out_invdepth", "radii", "geom"), got, ref):
        assert torch.equal(g, r), f"{what}: {name} differs from the call without the early fill"


def check_every_E(sc, what, offs=(0, 4)):
    ref = sc.forward(OFF)
    assert not torch.isnan(ref[0]).any() and not torch.isnan(ref[1]).any(), f"{what}: the reference left elements unwritten"
    for off in offs:                      # off = 4: 16-byte aligned, not 128-byte aligned (the passes' `shift` is not 0)
        if off:
            same(sc.forward(OFF, off), ref, f"{what}, outputs offset by {off} floats, no early fill")
        for n in range(8):                # 0 = the default rule, 1..6 sixteenths of the planes, 7 = every plane
            same(sc.forward(_lib.SKS_EARLY_FILL(n), off), ref, f"{what}, E field {n}, outputs offset by {off} floats")
    return ref


@pytest.mark.parametrize("V,C", VC, ids=lambda v: str(v))
@pytest.mark.parametrize("W,H", SIZES, ids=lambda v: str(v))
def test_every_E_equals_no_early_fill(device, W, H, V, C):
    sc = Scene(device, W, H, V, C, "dense")
    ref = check_every_E(sc, f"{W}x{H} V={V} C={C}")
    assert (ref[2] > 0).any(), "the case renders nothing"
    assert (ref[0][-1] != 0).any(), "no covered tile in the early region"


@pytest.mark.parametrize("feat", ["onehot", "last"])
@pytest.mark.parametrize("W,H", SIZES[:4], ids=lambda v: str(v))
def test_covered_tiles_in_the_early_region(device, W, H, feat):
    """Per-plane cover rows: a composite block stores only the planes its list has features on.  The last view's last channel
    and its inverse-depth plane -- the first planes to move into the early region -- hold covered tiles."""
    for V, C in ((2, 3), (5, 17)):
        sc = Scene(device, W, H, V, C, feat)
        ref = check_every_E(sc, f"{feat} {W}x{H} V={V} C={C}", offs=(0,))
        assert (ref[0][-1, C - 1] != 0).any() and (ref[1][-1] != 0).any()
        if feat == "last":
            assert not ref[0][:, : C - 1].any()


@pytest.mark.parametrize("culled", [(1,), (3,), (0, 1, 2, 3, 4)], ids=lambda v: "culled" + "".join(map(str, v)))
def test_view_with_every_gaussian_culled(device, culled):
    V = 2 if culled == (1,) else 5
    for W, H in ((64, 48), (67, 45)):
        sc = Scene(device, W, H, V, 17, "dense", culled=culled)
        ref = check_every_E(sc, f"{W}x{H} V={V} culled {culled}")
        for v in culled:
            assert not ref[2][v].any() and not ref[0][v].any() and not ref[1][v].any()


def test_graph_replay_equals_eager(device):
    sc = Scene(device, 66, 48, 2, 17, "onehot")
    ref = sc.forward(OFF)
    for flags in (0, _lib.SKS_EARLY_FILL(4)):
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            sc.forward(flags)
        torch.cuda.current_stream(device).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = sc.forward(flags)
        for rep in range(2):
            out[0].fill_(float("nan")), out[1].fill_(float("nan")), out[2].fill_(-7), out[3].zero_()
            g.replay()
            torch.cuda.synchronize(device)
            same(out, ref, f"graph replay {rep}, flags {flags:#x}")


def test_one_call_form_and_debug_planes(device):
    """sks_forward_backward keeps its launch layout (no early fill) and equals the two calls, whose forward uses the early fill by
    default; a forward asked for final_T / n_contrib falls back and its debug planes equal the flag-off call's."""
    c = util.make_case(seed=3, W=160, H=128, scale_log=4.0, n_views=3)
    t = lambda a: torch.tensor(a, device=device)
    views = R.ViewBatch.from_cameras([cam.to(device) for cam in c.cams])
    args = (t(c.means), t(c.feat), t(c.opac), t(c.scales), t(c.quats), None)
    dLc, dLi = t(c.dL_color), t(c.dL_inv)
    outs = {}
    for name, tf in (("default", 0), ("off", OFF), ("quarter", _lib.SKS_EARLY_FILL(4))):
        color, inv, radii, st = R.forward_views(views, *args, tune_flags=tf)
        g = R.backward_views(st, *args, dLc, dLi)
        col1, inv1, rad1, _, g1 = R.forward_backward_views(views, *args, dLc, dLi, tune_flags=tf, workspace=R.Workspace())
        aux = R.forward_views(views, *args, tune_flags=tf, want_aux=True)
        torch.cuda.synchronize(device)
        outs[name] = (color, inv, radii, g, col1, inv1, rad1, g1, aux)
    ref = outs["off"]
    for name, o in outs.items():
        for k in (0, 1, 2):
            assert torch.equal(o[k], ref[k]) and torch.equal(o[4 + k], ref[k]), f"{name}: output {k} of the two forms differs"
        for key in ref[3]:
            if ref[3][key] is None:
                continue
            assert torch.equal(o[3][key], ref[3][key]) and torch.equal(o[7][key], ref[3][key]), f"{name}: gradient {key} differs"
        for k in (0, 1, 2, 4, 5):
            assert torch.equal(o[8][k], ref[8][k]), f"{name}: want_aux output {k} differs"
        assert torch.equal(o[8][0], ref[0])
