"""The HIP rasterizer held to the REFERENCE's own rasterizer sources compiled for the host (oracle/ref.py), with no oracle in
between: sks_forward + sks_backward on the small and on the binned path, and sks_forward_backward.

The reference side is oracle/_ref/libref_raster_{17,19,15}.so, built by __graft_entry__.build() where the reference tree is
present; this file only loads them.  Forward: torch.equal on the images, the inverse depth, radii, contributor counts, final T
and (binned path) the tile lists.  Backward: the project's standing tolerance against the reference's fp32 sums (rtol 1e-3,
atol 1e-5 x max).  Deviations as in tests/test_ref_cpu.py: dL_dsh is not compared, the
background is zero-padded to the channel count on both sides (backward.cu:613-614)."""
import functools

import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, rasterizer as R
from tests import ref_cases

pytestmark = pytest.mark.gpu

HAND = ref_cases.hand_cases()
OURS = (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
        ("rotations", "dL_drotations"), ("cov3D", "dL_dcov3D"), ("features", "dL_dcolors"))
MODES = ("small", "binned", "one-call")


_ref = ref_cases.compiled_reference


def _reference(rc):
    """The reference's forward and backward of a case, computed once and left unchanged."""
    ref = _ref()
    r = rc.forward(ref)
    return r, rc.backward(ref, r)


@functools.lru_cache(maxsize=None)
def _hand(name):
    rc = HAND[name]()
    return (rc,) + _reference(rc)


def run_kernels(rc, dev, mode):
    """-> (color, invdepth, radii, final_T or None, n_contrib or None, state, grads) of one view through the HIP kernels."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    views = R.ViewBatch.from_cameras([rc.scene_cam.to(dev)])
    args = tuple(t(a) for a in rc.args[:6])
    dLc, dLi = t(rc.dL_color[None]), t(None if rc.dL_inv is None else rc.dL_inv[None])
    bg = None if rc.bg is None else torch.tensor(rc.bg, dtype=torch.float32, device=dev)
    if mode == "one-call":
        ws = R.Workspace()
        for _ in range(2):      # (a workspace's first call of a shape is the two calls; the second goes through sks_forward_backward)
            col, inv, radii, st, g = R.forward_backward_views(views, *args, dLc, dLi, bg=bg, scale_modifier=rc.smod,
                                                              antialiasing=rc.aa, want_dfeatures=True, workspace=ws)
        torch.cuda.synchronize()
        return col, inv, radii, None, None, st, g
    col, inv, radii, st, fT, nC = R.forward_views(views, *args, scale_modifier=rc.smod, antialiasing=rc.aa, want_aux=True,
                                                  force_binned=mode == "binned", check_capacity=True)
    g = R.backward_views(st, *args, dLc, dLi, bg=bg, want_dfeatures=True)
    return col, inv, radii, fT, nC, st, g


def check(rc, r, br, dev, mode, ratios=None):
    col, inv, radii, fT, nC, st, g = run_kernels(rc, dev, mode)
    eq = lambda got, want: torch.equal(got.cpu(), torch.from_numpy(want))
    assert eq(radii[0], r["radii"]), f"{rc.name} {mode}: radii"
    assert eq(col[0], r["color"]), f"{rc.name} {mode}: colour image"
    assert eq(inv[0], r["invdepth"]), f"{rc.name} {mode}: inverse-depth image"
    if fT is not None:
        assert eq(fT[0], r["final_T"]), f"{rc.name} {mode}: final T"
        assert np.array_equal(nC[0].cpu().numpy().astype(np.uint32), r["n_contrib"]), f"{rc.name} {mode}: n_contrib"
    if mode == "binned":
        pl, rg, nr = R.export_lists(st)
        assert int(nr[0]) == r["R"], f"{rc.name}: num_rendered"
        assert np.array_equal(rg[0].cpu().numpy().astype(np.uint32), r["ranges"]), f"{rc.name}: tile ranges"
        assert np.array_equal(pl[0, :r["R"]].cpu().numpy().astype(np.uint32), r["point_list"]), f"{rc.name}: point_list"
    got = {theirs: g[ours][0].cpu().numpy() for ours, theirs in OURS if g.get(ours) is not None}
    want = {k: br[k] for k in got}
    return ref_cases.grad_ratios(rc, got, want, ratios)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(HAND))
def test_kernels_against_the_compiled_reference(device, name, mode):
    rc, r, br = _hand(name)
    ratios = check(rc, r, br, device, mode)
    print(f"{rc.name} {mode}: observed / allowed " + ", ".join(f"{k[3:]} {v:.3f}" for k, v in ratios.items()))
    assert {"dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dcov3D", "dL_dcolors"} <= set(ratios)
    assert rc.precomp or {"dL_dscales", "dL_drotations"} <= set(ratios)


@pytest.mark.parametrize("channels", [17, 19, 15])
def test_random_cases_against_the_compiled_reference(device, channels):
    """Twenty seeded scenes per rasterizer build (image <= 160 x 128, P <= 300, every switch drawn), all three ways."""
    ratios, drawn = {}, 0
    for seed in range(9000 + 100 * channels, 9000 + 100 * channels + 20):
        rc = ref_cases.random_case(seed, channels)
        r, br = _reference(rc)
        drawn += int(r["n_contrib"].max() > 0)
        for mode in MODES:
            check(rc, r, br, device, mode, ratios)
    print(f"C={channels}: observed / allowed " + ", ".join(f"{k[3:]} {v:.3f}" for k, v in ratios.items()))
    assert drawn >= 15


@pytest.mark.parametrize("name", ["seed0-plain", "culled", "seed4-plain", "seed5-plain"])
def test_mark_visible_against_the_compiled_reference(device, name):
    rc = HAND[name]()
    want = _ref().mark_visible(rc.means, rc.cam, channels=rc.C)
    cam = rc.scene_cam.to(device)
    pos = torch.from_numpy(rc.means).to(device)
    present = torch.zeros(rc.P, dtype=torch.bool, device=device)
    view = cam.world_view_transform.contiguous().float()
    proj = cam.full_proj_transform.contiguous().float()
    rcode = _lib.load().sks_mark_visible(rc.P, pos.data_ptr(), view.data_ptr(), proj.data_ptr(), present.data_ptr(),
                                         torch.cuda.current_stream(device).cuda_stream)
    _lib.check(rcode, "sks_mark_visible")
    torch.cuda.synchronize()
    assert np.array_equal(present.cpu().numpy(), want)
    assert want.any() and (name != "culled" or not want.all())
