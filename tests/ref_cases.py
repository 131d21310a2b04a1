"""Cases that hold the CPU oracle (tests/test_ref_cpu.py) and the HIP kernels (tests/test_ref_gpu.py) to the REFERENCE's
own rasterizer sources compiled for the host (oracle/ref.py): one view of one scene each, small enough for the host to run
the reference's blocks as fibers in a few milliseconds."""
import math
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import util

GRADS = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dinvdepths", "dL_dmeans3D", "dL_dcov3D", "dL_dscales",
         "dL_drotations")
# the forward artefacts held bit for bit (all of them integers or fp32 written in the reference's order of operations)
FORWARD_EXACT = ("radii", "ranges", "point_list", "n_contrib", "final_T", "color", "invdepth")
# per-Gaussian state of the reference's GeometryState, compared where the Gaussian survived culling (the rest is never written)
GEOM_EXACT = ("xy", "depths", "conic_opacity", "cov3D", "tiles_touched")


def compiled_reference():
    """oracle.ref with its three libraries present, or a test FAILURE that says how to get them (never a skip)."""
    from oracle import ref, ref_build
    missing = [ref_build.lib_path(c) for c in ref.CHANNELS if not os.path.exists(ref_build.lib_path(c))]
    if missing:
        pytest.fail("the compiled reference rasterizer is missing (%s): run __graft_entry__.build() where the reference tree "
                    "is present -- oracle/ref_build.py compiles it into oracle/_ref/" % ", ".join(missing), pytrace=False)
    return ref


class RefCase:
    """One view: what oracle.forward / oracle.backward (and oracle.ref's) take."""

    def __init__(self, name, c, v=0, aa=False, smod=1.0, bg=None, use_inv=True, precomp=False, extreme=False, feat=None):
        self.name, self.v, self.aa, self.smod, self.extreme, self.precomp = name, v, aa, smod, extreme, precomp
        self.c, self.cam, self.scene_cam = c, c.ocams[v], c.cams[v]
        self.W, self.H = self.cam.W, self.cam.H
        self.means, self.opac, self.scales, self.quats = c.means, c.opac, c.scales, c.quats
        self.feat = c.feat if feat is None else feat
        self.P, self.C = self.feat.shape
        self.bg = bg
        self.dL_color = c.dL_color[v]
        self.dL_inv = c.dL_inv[v] if use_inv else None
        self.cov = None
        if precomp:
            self.cov = orc.forward(c.means, self.feat, c.opac, c.scales, c.quats, None, self.cam,
                                   scale_modifier=smod)["cov3D"].astype(np.float32)

    @property
    def args(self):
        if self.precomp:
            return (self.means, self.feat, self.opac, None, None, self.cov, self.cam)
        return (self.means, self.feat, self.opac, self.scales, self.quats, None, self.cam)

    def forward(self, mod):
        return mod.forward(*self.args, scale_modifier=self.smod, antialiasing=self.aa)

    def backward(self, mod, fwd, **kw):
        return mod.backward(fwd, *self.args, self.dL_color, self.dL_inv, bg=self.bg, scale_modifier=self.smod,
                            antialiasing=self.aa, **kw)


def _bg(C):
    return [0.3, 0.1, 0.7] + [0.05 * (k % 5) for k in range(C - 3)]


def _dense_tile_case():
    """P = 300 on 32 x 32: every Gaussian's rect covers the whole image, so each of the four tiles holds 300 entries --
    renderCUDA takes two rounds of 256 and the second is partial (44).  Opacity 0.012: alpha stays above 1/255 near the
    centres and T stays far above 1e-4 after 300 entries, so the second round really composites."""
    c = util.make_case(seed=11, W=32, H=32, n_views=1, scale_log=4.6)
    rng = np.random.default_rng(11)
    P, C = 300, c.C
    centre = c.means.mean(axis=0)
    c.means = (centre + rng.normal(0.0, 60.0, (P, 3))).astype(np.float32)
    c.scales = np.exp(rng.normal(4.6, 0.2, (P, 3))).astype(np.float32)
    q = rng.normal(0, 1, (P, 4))
    c.quats = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    c.opac = np.full((P, 1), 0.012, np.float32)
    c.feat = rng.random((P, C)).astype(np.float32)
    c.P = P
    return RefCase("tile-of-300", c)


def _culled_case():
    """One Gaussian behind the camera (p_view.z <= 0.2), one in front whose rect covers no tile (radii stays 0), one at the
    near plane's other side by a hair, the rest ordinary."""
    c = util.make_case(seed=12, W=96, H=64, n_views=1, scale_log=3.6)
    cam = c.ocams[0]
    V = cam.view.reshape(4, 4)             # row-major memory of the transposed matrix: p_view = p @ V[:3, :3] + V[3, :3]
    Rm, tr = V[:3, :3].astype(np.float64), V[3, :3].astype(np.float64)
    to_world = lambda pv: ((np.asarray(pv, np.float64) - tr) @ np.linalg.inv(Rm)).astype(np.float32)
    c.means = c.means.copy()
    c.scales = c.scales.copy()
    c.means[0] = to_world([0.0, 0.0, -500.0])          # behind
    c.means[1] = to_world([40000.0, 0.0, 2500.0])      # in front, far off the image: empty rect
    c.scales[1] = 1.0
    c.means[2] = to_world([0.0, 0.0, 0.19])            # just inside the near cut
    return RefCase("culled", c)


def hand_cases():
    """name -> builder.  The smallest cases at which each convention of the forward and each term of the backward can go wrong."""
    from tests.test_raster_gpu import CASES
    out = {}
    for kw in CASES:
        for aa in (False, True):
            out[f"seed{kw['seed']}-{'aa' if aa else 'plain'}"] = (
                lambda kw=kw, aa=aa: RefCase(f"seed{kw['seed']}", util.make_case(**kw), v=kw["seed"] % 2, aa=aa))
    out["70x36"] = lambda: RefCase("70x36", util.make_case(seed=21, W=70, H=36, scale_log=4.2, fxmul=0.8))
    out["tile-of-300"] = _dense_tile_case
    out["P=1"] = lambda: RefCase("P=1", _one_gaussian())
    out["culled"] = _culled_case
    out["cov3D_precomp"] = lambda: RefCase("cov3D_precomp", util.make_case(seed=23, W=80, H=64, scale_log=4.0), precomp=True)
    out["cov3D_precomp-aa"] = lambda: RefCase("cov3D_precomp-aa", util.make_case(seed=24, W=80, H=64, scale_log=3.4), precomp=True,
                                              aa=True, smod=1.25)
    out["scale_modifier"] = lambda: RefCase("scale_modifier", util.make_case(seed=25, W=80, H=64, scale_log=4.0), smod=0.7, aa=True)
    out["background"] = lambda: RefCase("background", util.make_case(seed=26, W=80, H=64, scale_log=4.0), bg=_bg(17))
    out["background-19"] = lambda: RefCase("background-19", util.make_case(seed=27, W=72, H=56, scale_log=3.6, dataset="panoptic"),
                                           bg=_bg(19), aa=True)
    out["no-invdepth-gradient"] = lambda: RefCase("no-invdepth", util.make_case(seed=28, W=80, H=64, scale_log=4.0), use_inv=False)
    out["op-15-translucent"] = lambda: RefCase("op-15", util.make_case(seed=29, W=90, H=50, scale_log=4.3, opac=0.3,
                                                                        dataset="occlusion-person", n_skeletons=2), bg=_bg(15))
    out["clamped-t"] = lambda: RefCase("clamped-t", util.make_case(seed=30, W=64, H=48, scale_log=5.0, fxmul=3.0), aa=True)
    return out


def _one_gaussian():
    c = util.make_case(seed=22, W=48, H=40, n_views=1, scale_log=4.4)
    k = 3
    for name in ("means", "scales", "quats", "opac", "feat"):
        setattr(c, name, getattr(c, name)[k:k + 1].copy())
    c.means[0] = np.asarray(util.make_case(seed=22, W=48, H=40, n_views=1).means.mean(axis=0), np.float32)   # mid-image
    c.P = 1
    return c


def random_case(seed, channels):
    """A seeded case of `channels` channels (17 / 19 / 15: the three rasterizer builds) for the GPU file: image <= 160 x 128,
    P <= 300, every switch drawn."""
    rng = np.random.default_rng(seed)
    dataset = {17: "h36m", 19: "panoptic", 15: "occlusion-person"}[channels]
    W, H = int(rng.integers(24, 161)), int(rng.integers(24, 129))
    nsk = int(rng.choice([1, 1, 2, 6, 15]))
    c = util.make_case(seed=seed, W=W, H=H, dataset=dataset, n_views=2, n_skeletons=nsk, scale_log=float(rng.uniform(2.6, 4.8)),
                       pitch=float(rng.uniform(30.0, 600.0)), onehot=bool(rng.integers(0, 2)),
                       opac=None if rng.integers(0, 2) else float(rng.choice([0.05, 0.3, 0.6, 1.0])),
                       fxmul=float(rng.uniform(0.6, 2.2)))
    assert c.P <= 300 and c.C == channels
    return RefCase(f"random {seed} C={channels} {W}x{H} P={c.P}", c, v=int(rng.integers(0, 2)), aa=bool(rng.integers(0, 2)),
                   smod=float(rng.choice([1.0, 1.0, 1.25, 0.7])), bg=_bg(channels) if rng.integers(0, 2) else None,
                   use_inv=bool(rng.integers(0, 3)), precomp=bool(rng.integers(0, 4) == 0))


def fuzz_cases(generator, seed):
    """One view of the scene that generator `generator` of tests/fuzz_cases.py draws for `seed`, or None when that scene has a
    channel count no rasterizer build has (the one-call generator's 33-71 channel cases)."""
    from tests import fuzz_cases as F
    if generator in ("binned", "extreme"):
        s = F.raster_scene(seed)
        assert s.extreme == (generator == "extreme")
        return RefCase(f"{generator} seed {seed} {s.W}x{s.H} P={s.c.P}", s.c, v=seed % s.nv, aa=s.aa, smod=s.smod,
                       bg=[0.3, 0.1, 0.7] + [0.0] * (s.c.C - 3) if s.use_bg else None, use_inv=s.use_inv, precomp=s.precomp,
                       extreme=s.extreme)
    if generator == "one-call":
        s = F.one_call_scene(seed)
        if s.feat.shape[1] != s.c.C:
            return None
        return RefCase(f"one-call seed {seed} {s.W}x{s.H} P={s.c.P}", s.c, v=seed % s.nv, aa=s.aa, bg=_bg(s.c.C) if s.use_bg else None,
                       use_inv=s.use_inv)
    if generator == "fused-loss":
        import torch
        s = F.fused_loss_scene(seed, "cpu")
        sc, gm, dataset, W, H, nv = s.sc, s.gm, s.dataset, s.W, s.H, s.nv
        P, C = sc.n_points, sc.n_joints
        rng = np.random.default_rng(seed)
        c = util.Case()
        with torch.no_grad():
            c.means, c.feat, c.opac, c.scales, c.quats = (
                np.ascontiguousarray(a.detach().numpy(), dtype=np.float32) for a in
                (gm._xyz, gm.get_features.reshape(P, C), gm.get_opacity, gm.get_scaling, gm.get_rotation))
        c.P, c.C, c.cams = P, C, sc.cameras
        c.ocams = [orc.Cam(W, H, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), cam.world_view_transform.numpy(),
                           cam.full_proj_transform.numpy()) for cam in sc.cameras]
        c.dL_color = rng.normal(0, 1, (nv, C, H, W)).astype(np.float32)
        c.dL_inv = rng.normal(0, 1, (nv, 1, H, W)).astype(np.float32)
        return RefCase(f"fused-loss seed {seed} {dataset} {W}x{H}", c, v=seed % nv)
    raise KeyError(generator)


def grad_ratios(rc, got, want, ratios=None):
    """Holds every gradient of `got` to `want` (the oracle's, with "bound" for an extreme case) and returns, per gradient,
    the largest observed / allowed error: ordinary cases at the project's standing tolerance (rtol 1e-3, atol 1e-5 x max),
    extreme ones at rtol 1e-3 + util.BOUND_KAPPA x 2^-24 x the oracle's sum of |terms| (dL_dconic and dL_dinvdepths, for
    which the oracle returns no such sum, stay at the standing tolerance)."""
    ratios = {} if ratios is None else ratios
    for k in GRADS:
        w, g = want.get(k), got.get(k)
        if w is None or (rc.precomp and k in ("dL_dscales", "dL_drotations")):
            continue
        assert g is not None, k
        g64, w64 = np.asarray(g, np.float64).reshape(np.shape(w)), np.asarray(w, np.float64)
        assert np.isfinite(g64).all(), f"{rc.name}: {k} has a non-finite entry"
        bound = want.get("bound", {}).get(k) if rc.extreme else None
        if bound is not None:
            b64 = np.asarray(bound, np.float64).reshape(w64.shape)
            tol = 1e-3 * np.abs(w64) + util.BOUND_KAPPA * util.EPS32 * b64
        else:
            tol = 1e-5 * (np.abs(w64).max() + 1e-30) + 1e-3 * np.abs(w64)
        err = np.abs(g64 - w64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / tol, 0.0)
        ratios[k] = max(ratios.get(k, 0.0), float(np.nan_to_num(r, nan=np.inf, posinf=np.inf).max()) if r.size else 0.0)
        if bound is not None:
            util.assert_close_bound(f"{rc.name}: {k}", g64, w64, b64, rtol=1e-3)
        else:
            util.assert_close(f"{rc.name}: {k}", g64, w64, rtol=1e-3, atol_scale=1e-5)
    return ratios
