"""Seeded scenes for the sparse fused-loss step (sks_geometry + sks_backward_fused_loss) at the smallest sizes that reach the
branches the bench scenes (P = C, one-hot features, the skeleton's own heat-maps in [0, 1]) never do: every channel-group
instantiation, the clamp on both sides, several Gaussians per channel and channels per Gaussian, signed features, a background,
all 64 lanes, rects of more than 16 tiles, culled and transparent Gaussians in the low indices, per-view sizes, signed heat-maps,
a view that sees nothing.  Host arrays only, drawn without a device (tests/test_fused_loss_cpu.py holds every case to what its row
claims, through the CPU reference alone).

draw(name) gives the suite's case; draw(name, seed) the same recipe at another seed (tools/fuzz_binned.py `hard`)."""
import math

import numpy as np

from oracle import oracle as orc
from tests import util


class FusedLossCase:
    """means (P,3), feat (P,C), opac (P,1), scales (P,3) / quats (P,4) or cov (P,6), cams / ocams per view, gt: list of (C,H_v,W_v)
    planes, bg (C floats or None), aa, smod; bounds: compare the gradients against the oracle's computed rounding bound
    (util.assert_close_bound) instead of a fraction of the tensor's largest entry; claims: what the CPU test must find in it;
    hm: None, or the inputs of generate_heatmaps for the planes-against-factors comparison (C joints)."""

    @property
    def params(self):
        return (self.means, self.feat, self.opac, self.scales, self.quats)

    @property
    def P(self):
        return self.means.shape[0]

    @property
    def C(self):
        return self.feat.shape[1]

    @property
    def V(self):
        return len(self.cams)

    @property
    def sizes(self):
        return [(o.W, o.H) for o in self.ocams]


def _planes(rng, C, sizes, density=0.3):
    """Random heat-maps: `density` of the pixels hold U(0, 1), the rest are exactly 0."""
    return [(rng.random((C, h, w)) * (rng.random((C, h, w)) < density)).astype(np.float32) for w, h in sizes]


def _base(name, seed, W, H, V, n_skeletons=1, pitch=700.0, scale_log=4.0, P=None, fxmul=1.0):
    c0 = util.make_case(seed=seed, W=W, H=H, n_views=V, n_skeletons=n_skeletons, pitch=pitch, scale_log=scale_log, fxmul=fxmul,
                        with_dL=False)
    c = FusedLossCase()
    P = c0.P if P is None else P
    c.name, c.seed, c.scene = name, seed, c0.scene
    c.means, c.feat, c.opac, c.scales, c.quats = (np.ascontiguousarray(a[:P]) for a in (c0.means, c0.feat, c0.opac, c0.scales, c0.quats))
    c.cov, c.cams, c.ocams = None, list(c0.cams), list(c0.ocams)
    c.bg, c.aa, c.smod, c.bounds, c.claims, c.hm = None, False, 1.0, False, set(), None
    c.rng = np.random.default_rng(seed + 7000)
    return c


def _features(c, C, lo, hi, density):
    """(P,C) features U(lo, hi) on `density` of the entries, 0 elsewhere; every Gaussian keeps at least one channel."""
    P = c.P
    f = c.rng.uniform(lo, hi, (P, C)) * (c.rng.random((P, C)) < density)
    keep = c.rng.integers(0, C, P)
    f[np.arange(P), keep] = np.where(f[np.arange(P), keep] == 0, c.rng.uniform(max(lo, 0.1), hi, P), f[np.arange(P), keep])
    c.feat = f.astype(np.float32)


def _heatmap_inputs(c):
    """What generate_heatmaps needs for C planes per view: channel j's joint is point j % P, its detection that point's plus a
    few pixels, isotropic-ish scales, identity rotations (the planes are then what the loop's heat-maps are: separable, in [0, 1])."""
    C, P, sc = c.C, c.P, c.scene
    idx = np.arange(C) % P
    c.hm = dict(means=np.ascontiguousarray(sc.pose_3d_gt[idx], dtype=np.float32),
                scaling=np.exp(c.rng.normal(4.0, 0.2, (C, 3))).astype(np.float32),
                rotation=np.tile(np.array([1.0, 0, 0, 0], np.float32), (C, 1)),
                p2d=(sc.poses_2d[:, idx] + c.rng.normal(0.0, 4.0, (c.V, C, 2))).astype(np.float32))


def _cg4(name, seed, C):
    c = _base(name, seed, 90, 70, 3, fxmul=1.0)
    _features(c, C, 0.0, 1.6, 0.5)
    c.gt = _planes(c.rng, C, c.sizes)
    _heatmap_inputs(c)
    c.claims = {"clamp"}
    return c


def _cg32(name, seed, C, n_skeletons):
    c = _base(name, seed, 131, 77, 2, n_skeletons=n_skeletons, pitch=250.0)
    _features(c, C, 0.0, 1.2, 0.6)
    c.gt = _planes(c.rng, C, c.sizes)
    _heatmap_inputs(c)
    return c


def _signed(name, seed, W=176, H=144, V=3):
    c = _base(name, seed, W, H, V, n_skeletons=3, pitch=300.0)
    _features(c, 17, 0.0, 1.0, 0.6)
    c.feat = np.where(c.feat != 0, c.feat * np.float32(2.4) - np.float32(0.8), 0).astype(np.float32)
    c.gt = _planes(c.rng, 17, c.sizes)
    c.claims = {"clamp", "signed"}
    return c


def _lanes64(name, seed):
    c = _base(name, seed, 176, 144, 8, n_skeletons=4, pitch=100.0, scale_log=4.4, P=64)
    c.gt = _planes(c.rng, 17, c.sizes)
    c.claims = {"clamp", "saturated"}
    return c


def _big(name, seed):
    c = _base(name, seed, 200, 160, 2, scale_log=5.2)
    c.gt = _planes(c.rng, 17, c.sizes)
    c.bounds = True
    c.claims = {"saturated", "big-rect"}
    return c


def _culled(name, seed):
    c = _signed(name, seed, 131, 77, 3)
    cam0 = c.cams[0]
    pos0 = -(cam0.R @ cam0.T)       # camera 0's centre (T = -R^T centre)
    target = np.array([0.0, 0.0, 900.0])
    c.means = c.means.copy()
    c.opac = c.opac.copy()
    c.means[0] += np.float32([0.0, 0.0, 60000.0])                       # far above every frustum: off screen in every view
    c.means[1] = (pos0 + 0.5 * (pos0 - target)).astype(np.float32)      # behind camera 0
    c.means[20] += np.float32([0.0, 0.0, -60000.0])
    c.opac[[5, 30]] = 0.0
    c.opac[[7, 33]] = 1.0 / 255.0
    c.bounds = True
    c.claims = {"signed", "culled"}
    return c


def _with_bg(c):
    c.bg = [0.3, 0.5, 0.2] + [0.0] * (c.C - 3)
    return c


def _precomp(name, seed):
    c = _signed(name, seed)
    c.cov = orc.forward(c.means, c.feat, c.opac, c.scales, c.quats, None, c.ocams[0])["cov3D"].astype(np.float32)
    c.scales = c.quats = None
    return c


def _smod(name, seed):
    c = _signed(name, seed)
    c.smod = 1.25
    return c


def _aa(name, seed):
    c = _signed(name, seed)
    c.aa = True
    return c


def _mixed(name, seed):
    """Widths W and W + 2 in one group (H36M's 1000 / 1002 sensors, quirk Q11)."""
    from skelsplat_amd.scene import Camera
    c = _signed(name, seed)
    for v in (1,):
        cam = c.cams[v]
        Wv = cam.image_width + 2
        K = cam.K.copy()
        K[0, 2] += 1.0
        c.cams[v] = cam2 = Camera(cam.uid, cam.R, cam.T, K, Wv, cam.image_height)
        c.ocams[v] = orc.Cam(Wv, cam2.image_height, math.tan(cam2.FoVx * 0.5), math.tan(cam2.FoVy * 0.5),
                             cam2.world_view_transform.numpy(), cam2.full_proj_transform.numpy())
    c.gt = _planes(c.rng, c.C, c.sizes)
    return c


def _signed_gt(c):
    """A tenth of the heat-map pixels negative, wherever they fall (on the splats and far from them)."""
    for v in range(c.V):
        neg = c.rng.random(c.gt[v].shape) < 0.1
        c.gt[v] = np.where(neg, -c.rng.random(c.gt[v].shape), c.gt[v]).astype(np.float32)
    c.claims = c.claims | {"signed-gt"}
    return c


def _empty(name, seed):
    c = _base(name, seed, 48, 48, 1)
    c.means = c.means + np.float32([0.0, 0.0, 60000.0])
    c.gt = [np.zeros((17, 48, 48), np.float32)]
    c.claims = {"empty"}
    return c


# name -> (seed of the suite's case, recipe)
CASES = {
    "cg4-c3": (11, lambda n, s: _cg4(n, s, 3)),
    "cg4-c4": (12, lambda n, s: _cg4(n, s, 4)),
    "cg32-p34c25": (13, lambda n, s: _cg32(n, s, 25, 2)),
    "cg32-p17c32": (14, lambda n, s: _cg32(n, s, 32, 1)),
    "signed": (15, _signed),
    "lanes64": (16, _lanes64),
    "big": (17, _big),
    "culled": (18, _culled),
    "bg-cg4": (19, lambda n, s: _with_bg(_cg4(n, s, 4))),
    "bg-signed": (20, lambda n, s: _with_bg(_signed(n, s))),
    "precomp": (21, _precomp),
    "smod": (22, _smod),
    "aa": (23, _aa),
    "mixed": (24, _mixed),
    "signed-gt-cg4": (25, lambda n, s: _signed_gt(_cg4(n, s, 4))),
    "signed-gt-signed": (26, lambda n, s: _signed_gt(_signed(n, s))),
    "empty": (27, _empty),
}
NAMES = tuple(CASES)


def draw(name, seed=None):
    s0, recipe = CASES[name]
    return recipe(name, s0 if seed is None else int(seed))


def draw_hard(seed):
    """Case `seed` of the open-ended sweep: the recipes in turn, each at its own seed."""
    return draw(NAMES[seed % len(NAMES)], seed)
