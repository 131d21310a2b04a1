"""Hand-placed rasterizer scenes at the limits of the image geometry, shared by tests/test_geometry_cpu.py (the oracle and the
library's own launch-regime query), tests/test_geometry_gpu.py (parity on the device) and tools/fuzz_binned.py (kind "geom").

The launch code switches on the image shape in about a dozen places (cover-row width and mode, 16-byte / pair-masked / 4-byte fill
stores, row-aligned or linear fill blocks, pixel index % W as a multiply-high, tile bands per scan block, the three compositing
backwards).  Each case here names the regime it is there for in `claims` = {field of _lib.launch_regime: value}; the tests assert
the claims against sks_launch_regime, so a retuned threshold makes a case fail instead of quietly missing its branch.  Shapes that
sit at a threshold are FOUND through the query (shapes()), not written down.

Scenes.  One near-orthographic camera per view: identity rotation, focal length F = 2**20 pixels, the Gaussians ~F in front of it,
so a world unit is a pixel and a Gaussian is placed by its target pixel; the views differ by a sub-pixel shift.  What every scene
holds as far as its shape allows, by role (Case.roles: role -> Gaussian indices):
  first   covers the first tile column and row;
  last    covers the last tile column and row (the ragged tile);
  anchor  sits ON a 32-tile-column seam of the cover words when the width has one (tile columns 31|32, 63|64, ...; with P = 5 the
          LAST seam, the one only this width reaches), covering the tiles on both sides, and is wide enough to cross more than
          8 tile columns (the solo band class) when the image has more than 10;
  pair    overlaps the anchor: a tile list of two or more;
  culled  lies behind the camera;
  seam    (P > 5) one more Gaussian on every further seam, up to a budget, always with the seams at which the cover row's fetch
          form changes (4 | 5 words, 8 | 9 words);
  fill    (P > 5) random clusters in the top and bottom rows of the image, every third one beside its predecessor, one of them far
          outside the image (visible to the frustum test, empty rect);
and, where the image is tall enough, bands that no rect crosses (Case.empty_bands)."""
import functools
import math

import numpy as np

from oracle import oracle as orc
from skelsplat_amd import _lib

F = float(2 ** 20)          # focal length in pixels and distance of the Gaussians: a world unit is a pixel
ZONE = 40                   # fill Gaussians live in the top and bottom ZONE rows
MAX_W, MAX_H = 65536, 1048560     # what check_common admits (include/skelsplat_hip.h)
SCAN_WIDE = 32768           # first width whose band is a whole block of the binned path's scan launch (k_bin_scan)
GATHER_ROW = 32768          # first tile row whose index needs bit 15 of a packed rect half (k_render_bwd_gather)


class Case:
    def __repr__(self):
        return f"<geometry case {self.name}>"


def _radius(sig):
    """Upper bound of the pixel radius preprocess gives a Gaussian whose larger image-plane sigma is `sig` (forward.cu:
    ceil(3 sqrt(lambda_max)), + 0.3 on the diagonal), + the views' shift and the perspective term."""
    return int(math.ceil(3.0 * math.sqrt(sig * sig + 0.3))) + 2


def seams_of(W):
    """Tile columns s with a cover-word seam between s - 1 and s."""
    gx = (W + 15) // 16
    return list(range(32, gx, 32))


def _pick_seams(seams, n):
    """Up to n seams: the last one first (only this width reaches it), the first, the two at which the row's fetch form changes
    (words 4 | 5: tile column 96; 8 | 9: 224), then evenly spread."""
    if n <= 0 or not seams:
        return []
    order = [seams[-1], seams[0]] + [s for s in (96, 224) if s in seams]
    step = max(1, len(seams) // max(1, n))
    order += seams[::step] + seams
    out = []
    for s in order:
        if s not in out:
            out.append(s)
    return out[:n]


def make(name, W, H, P, C, V=1, seed=0, dense=True, force_binned=False, extras=False, claims=None, flags=0):
    """extras: the backward gets a background and an inverse-depth gradient."""
    rng = np.random.default_rng(1000 + seed)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    c = Case()
    c.name, c.W, c.H, c.P, c.C, c.V, c.seed = name, W, H, P, C, V, seed
    c.dense, c.force_binned, c.extras, c.flags = dense, force_binned, extras, flags
    c.claims = dict(claims or {})
    c.gx, c.gy = gx, gy
    seams = seams_of(W)
    wide = gx > 10
    px, py, sig, culled = [], [], [], []
    roles = {}

    def add(role, x, y, s, cull=False):
        roles.setdefault(role, []).append(len(px))
        px.append(float(min(max(x, 0), W - 1)))
        py.append(float(min(max(y, 0), H - 1)))
        sig.append(float(s))
        culled.append(cull)

    ytop = min(7, H - 1)
    add("first", 2, 2, 1.3)
    add("last", W - 3, H - 3, 1.3)
    anchor_seam = _pick_seams(seams, 1)
    ax = 16 * anchor_seam[0] if anchor_seam else W // 2
    add("anchor", ax, ytop, 45.0 if wide else 2.0)      # (wide: > 8 tile columns even when the image's edge clips one side)
    add("pair", ax + 3, ytop + 2, 2.5)
    add("culled", W // 2, H // 2, 2.0, cull=True)
    c.seams = list(anchor_seam)
    if P > 5:
        more = [s for s in _pick_seams(seams, 1 + (P - 5) // 2) if s not in c.seams]
        for k, s in enumerate(more):
            add("seam", 16 * s, ytop if k % 2 == 0 else H - 1 - ytop, 2.0)
            c.seams.append(s)
        k = 0
        while len(px) < P:
            bottom = k % 2 == 1
            if k == 4:
                add("outside", W + 5000, ytop, 2.0)       # in front of the camera, rect clipped to nothing
                px[-1] = float(W + 5000)
            elif k % 3 == 2:
                add("fill", px[-1] + rng.uniform(-4, 4), py[-1] + rng.uniform(-4, 4), rng.uniform(1.0, 4.0))
            else:
                y = rng.uniform(0, min(H, ZONE))
                add("fill", rng.uniform(0, W), H - 1 - y if bottom else y, rng.uniform(1.0, 12.0) if k % 5 == 0 else rng.uniform(1.0, 5.0))
            k += 1
    assert len(px) == P, (len(px), P)
    c.roles = roles
    # bands that no rect can cross: a conservative reading of the placement (the CPU test holds it to the oracle's ranges)
    crossed = np.zeros(gy, bool)
    for i in range(P):
        if culled[i] or px[i] >= W:
            continue
        r = _radius(sig[i])
        crossed[max(0, int(py[i] - r) // 16):min(gy - 1, int(py[i] + r) // 16) + 1] = True
    c.empty_bands = bool((~crossed).any())
    # depth: distinct, in a random order, 16 apart (an fp32 ulp at 2**20 is 1/16)
    order = rng.permutation(P)
    Z = F + 16.0 * order
    Z = np.where(np.array(culled), -F, Z)
    means = np.stack([(np.array(px) - 0.5 * (W - 1)) * np.abs(Z) / F, (np.array(py) - 0.5 * (H - 1)) * np.abs(Z) / F, Z], axis=1)
    ratio = rng.uniform(0.4, 1.0, P)
    sg = np.array(sig)
    scales = np.stack([sg, sg * ratio, np.full(P, 0.5)], axis=1)
    ang = rng.uniform(0, math.pi, P)
    quats = np.stack([np.cos(0.5 * ang), np.zeros(P), np.zeros(P), np.sin(0.5 * ang)], axis=1)      # (w, x, y, z): a turn about the view axis
    c.means, c.scales, c.quats = (np.ascontiguousarray(a, np.float32) for a in (means, scales, quats))
    c.opac = rng.uniform(0.3, 0.95, (P, 1)).astype(np.float32)
    if dense:
        c.feat = rng.uniform(0.1, 1.0, (P, C)).astype(np.float32)
    else:
        c.feat = np.zeros((P, C), np.float32)
        c.feat[np.arange(P), np.arange(P) % C] = 1.0
    c.bg = rng.uniform(0.1, 0.9, C).astype(np.float32) if extras else None
    c.cams, c.ocams = cameras(W, H, V)
    return c


def cameras(W, H, V):
    """The V near-orthographic cameras of a W x H scene (identity rotation, focal length F, a sub-pixel shift per view), for the
    device and for the oracle."""
    from skelsplat_amd.scene import Camera
    K = np.array([[F, 0.0, 0.5 * W], [0.0, F, 0.5 * H], [0.0, 0.0, 1.0]])
    cams = [Camera(v, np.eye(3), np.array([0.25 * (v % 4), -0.25 * ((v // 4) % 4), 0.125 * (v % 3)]), K, W, H) for v in range(V)]
    ocams = [orc.Cam(W, H, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), cam.world_view_transform.numpy(),
                     cam.full_proj_transform.numpy()) for cam in cams]
    return cams, ocams


def host_bytes(c):
    return sum(a.nbytes for a in vars(c).values() if isinstance(a, np.ndarray)) + sum(o.view.nbytes + o.proj.nbytes for o in c.ocams)


def draw_dL(c):
    """Dense random upstream gradients (V,C,H,W), (V,1,H,W) or None: not kept in the case (the tall cases' are 134 MB)."""
    rng = np.random.default_rng(5000 + c.seed)
    dLc = rng.standard_normal((c.V, c.C, c.H, c.W), dtype=np.float32)
    dLi = rng.standard_normal((c.V, 1, c.H, c.W), dtype=np.float32) if c.extras else None
    return dLc, dLi


def oracle_forward(c, v):
    return orc.forward(c.means, c.feat, c.opac, c.scales, c.quats, None, c.ocams[v])


def oracle_backward(c, v, fwd, dLc, dLi, bounds=False):
    return orc.backward(fwd, c.means, c.feat, c.opac, c.scales, c.quats, None, c.ocams[v], dLc[v], None if dLi is None else dLi[v],
                        bg=c.bg, bounds=bounds)


def regime(c, aligned=True):
    return _lib.launch_regime(c.V, c.P, c.C, c.W, c.H, c.flags | (_lib.SKS_FORCE_BINNED if c.force_binned else 0), aligned)


def check_claims(c, aligned=True):
    r = regime(c, aligned)
    for k, want in c.claims.items():
        ok = want(r[k]) if callable(want) else r[k] == want
        assert ok, f"{c.name}: the launch regime has {k} = {r[k]}, not what the case is there for ({r})"
    return r


# ------------------------------------------------------------------------------------------------------------
# shapes: the smallest at each regime boundary, found through the query
# ------------------------------------------------------------------------------------------------------------
def _last(lo, hi, step, pred):
    """Largest x = lo + k step <= hi with pred(x), pred monotone (true, then false)."""
    a, b = 0, (hi - lo) // step
    assert pred(lo)
    while a < b:
        m = (a + b + 1) // 2
        if pred(lo + m * step):
            a = m
        else:
            b = m - 1
    return lo + a * step


def _q(P, C, W, H, flags=0):
    return _lib.launch_regime(1, P, C, W, H, flags)


@functools.lru_cache(maxsize=None)
def thresholds():
    t = {}
    t["cw4"] = _last(16, MAX_W, 16, lambda W: _q(5, 3, W, 17)["cw"] <= 4)             # widest image whose cover row is one 16-byte fetch
    t["cw8"] = _last(16, MAX_W, 16, lambda W: _q(5, 3, W, 17)["cw"] <= 8)             # ... two
    t["magic"] = _last(4, MAX_W, 4, lambda W: _q(5, 3, W, 16)["w_magic"] == 1) + 4     # first width with plain %
    t["per_plane"] = _last(16, MAX_H, 16, lambda H: _q(5, 3, 48, H)["cover"] == _lib.COVER_PER_PLANE)       # tallest 48-wide C = 3 image with per-plane rows
    t["per_view"] = _last(16, MAX_H, 16, lambda H: _q(5, 3, 48, H)["cover"] != _lib.COVER_NONE)             # ... with cover rows at all
    return t


def shapes():
    """[(group, W, H, claims)]; today's constants give the widths and heights in the comments."""
    t = thresholds()
    S, PP, PV, NONE = _lib.PATH_SMALL, _lib.COVER_PER_PLANE, _lib.COVER_PER_VIEW, _lib.COVER_NONE
    out = []
    for W, H in ((1, 1), (1, 17), (17, 1), (2, 2), (2, 34), (3, 5), (6, 16), (15, 15), (16, 16), (17, 17)):
        cl = {"ppt": 4 if (W % 4 == 0 or (W % 4 == 2 and H % 2 == 0)) else 1, "half": 1 if (W % 4 == 2 and H % 2 == 0) else 0,
              "gx": (W + 15) // 16}
        out.append(("tiny", W, H, cl))
    out += [("cw", t["cw4"], 17, {"cw": 4}),                                    # 1536
            ("cw", t["cw4"] + 16, 17, {"cw": 8}),                               # 1552
            ("cw", t["cw8"], 17, {"cw": 8}),                                    # 3584
            ("cw", t["cw8"] + 16, 17, {"cw": lambda v: v > 8, "rowmode": 0}),   # 3600: per-lane load, linear passes
            ("cw", 4096, 17, {"cw": lambda v: v > 8, "rowmode": 1})]            # per-lane load, row-aligned blocks
    m = t["magic"]                                                              # 16384
    out += [("nomagic", m - 4, 17, {"w_magic": 1, "ppt": 4}),
            ("nomagic", m, 16, {"w_magic": 0, "ppt": 4}),
            ("nomagic", m + 4, 18, {"w_magic": 0, "ppt": 4, "half": 0}),
            ("nomagic", m + 6, 18, {"w_magic": 0, "ppt": 4, "half": 1}),
            ("nomagic", m + 5, 17, {"w_magic": 0, "ppt": 1})]
    # (a band of SCAN_WIDE / 16 = 2048 tiles fills a scan block's 256 x 8 items on its own: the first width at which the launcher's
    # `gx >= SCAN_T * 8` holds.  The query cannot find it -- bands per block is 1 from 1025 tile columns on -- so it is written down)
    out += [("wide", SCAN_WIDE, 17, {"w_magic": 0, "gx": SCAN_WIDE // 16}),
            # (the widest image that is no power of two: ceil(2^32 / W) W - 2^32 is 0 for 16384, 32768 and 65536, so the multiply-high
            # those widths must not use would be exact there; here it is wrong at 24 of a band's 16-byte stores, in the last tile column)
            ("wide", MAX_W - 16, 16, {"w_magic": 0, "rowmode": 0}),
            ("wide", MAX_W, 16, {"w_magic": 0, "gx": 4096})]
    out += [("cover", 48, t["per_plane"], {"cover": PP}),                       # 6144
            ("cover", 48, t["per_plane"] + 16, {"cover": PV}),                  # 6160
            ("cover", 48, t["per_view"], {"cover": PV}),                        # 24576
            ("cover", 48, t["per_view"] + 16, {"cover": NONE})]                 # 24592
    out += [("tall", 16, 16 * GATHER_ROW + 16, {"gy": GATHER_ROW + 1, "cover": NONE}),      # 16 x 524304: a rect on tile row 32768
            ("tall", 4, MAX_H, {"gy": 65535, "cover": NONE})]
    return out


TALL_GATHER = f"tall-16x{16 * GATHER_ROW + 16}-P80"


@functools.lru_cache(maxsize=None)
def specs():
    """name -> keyword arguments of make(): every shape with P = 5, P = 80 (the gather backward) and forced onto the binned path,
    P = 260 for the two widest and the tallest, the last plane index, and the two shapes of the alignment test."""
    S, B = _lib.PATH_SMALL, _lib.PATH_BINNED
    out = {}
    k = 0

    def put(group, W, H, P, C, claims, V=1, force_binned=False, tag=None):
        nonlocal k
        name = f"{group}-{W}x{H}-{tag or ('P%d' % P)}"
        big = W * H > 1 << 20
        out[name] = dict(name=name, W=W, H=H, P=P, C=C, V=1 if big else V, seed=k, dense=k % 2 == 0, extras=(k // 2) % 2 == 0,
                         force_binned=force_binned, claims=claims)
        k += 1

    sh = shapes()
    for group, W, H, cl in sh:
        small = {k2: v for k2, v in cl.items()}
        binned = {k2: v for k2, v in cl.items() if k2 not in ("cover",)}
        put(group, W, H, 5, 3, dict(small, path=S, bwd=_lib.BWD_WAVE), V=2)
        put(group, W, H, 80, 3, dict(small, path=S, bwd=_lib.BWD_GATHER), V=2)
        bc = dict(binned, path=B, bwd=_lib.BWD_TILE, cover=_lib.COVER_PER_PLANE)
        if group == "wide":
            bc["bpc"] = 1
        put(group, W, H, 80, 3, bc, V=2, force_binned=True, tag="binned")
    big3 = [s for s in sh if s[0] == "wide" and s[1] in (SCAN_WIDE, MAX_W)] + [s for s in sh if s[0] == "tall"][-1:]
    for group, W, H, cl in big3:
        put(group, W, H, 260, 3, dict({k2: v for k2, v in cl.items() if k2 != "cover"}, path=B, bwd=_lib.BWD_TILE), tag="P260")
    put("plane", 20, 18, 5, 32, {"path": S, "cover": _lib.COVER_PER_PLANE}, V=64)
    put("plane", 20, 18, 5, 32, {"path": B}, V=64, force_binned=True, tag="binned")
    return out


def names():
    return list(specs())


def get(name):
    return make(**specs()[name])


# the alignment test's shapes: outputs 16 bytes past a 128-byte line through the raw C ABI
ALIGN_SHAPES = ((1000, 24), (64, 40))


def align_case(W, H, P, seed):
    return make(f"align-{W}x{H}-P{P}", W, H, P, 3, V=2, seed=seed, dense=seed % 2 == 0, claims={"lead": 31, "path": _lib.PATH_SMALL})


# ------------------------------------------------------------------------------------------------------------
# on the device (tests/test_geometry_gpu.py, tools/fuzz_binned.py)
# ------------------------------------------------------------------------------------------------------------
NAN = float("nan")
GRADS = (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
         ("rotations", "dL_drotations"), ("cov3D", "dL_dcov3D"), ("features", "dL_dcolors"))


class Run:
    """A case on the device with its upstream gradients and the oracle's forward and backward of every view."""

    def __init__(self, c, dev, fwd=None, bound=None):
        """fwd: the oracle's forward of every view where the caller has it already; bound: True = the gradients are held to the
        oracle's computed rounding bound (default: the two tallest images only)."""
        import torch
        from skelsplat_amd import rasterizer as R
        self.c = c
        self.regime = check_claims(c)
        self.dev = dev
        # pixel coordinates near 2**19 leave fp32 ~0.03 px: the oracle's computed rounding bound
        self.bound = c.H >= 1 << 19 if bound is None else bool(bound)
        t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
        self.views = R.ViewBatch.from_cameras([cam.to(dev) for cam in c.cams])
        self.args = (t(c.means), t(c.feat), t(c.opac), t(c.scales), t(c.quats), None)
        dLc, dLi = draw_dL(c)
        self.dLc, self.dLi, self.bg = t(dLc), t(dLi), t(c.bg)
        self.fwd = [oracle_forward(c, v) for v in range(c.V)] if fwd is None else fwd
        self.bwd = [oracle_backward(c, v, self.fwd[v], dLc, dLi, bounds=self.bound) for v in range(c.V)]

    def nan_workspace(self, **kw):
        """A Workspace whose forward outputs exist already and hold NaN."""
        import torch
        from skelsplat_amd import rasterizer as R
        c, ws = self.c, R.Workspace(**kw)
        ws.get(("fwd", "color"), (c.V, c.C, c.H, c.W), torch.float32, self.dev).fill_(NAN)
        ws.get(("fwd", "invdepth"), (c.V, 1, c.H, c.W), torch.float32, self.dev).fill_(NAN)
        return ws

    def forward(self, ws=None, **kw):
        from skelsplat_amd import rasterizer as R
        kw.setdefault("force_binned", self.c.force_binned)
        return R.forward_views(self.views, *self.args, workspace=ws, **kw)

    def backward(self, st, ws=None, **kw):
        from skelsplat_amd import rasterizer as R
        return R.backward_views(st, *self.args, self.dLc, self.dLi, bg=self.bg, workspace=ws, **kw)


def held_nan(ws, c, dev):
    import torch
    return (ws.get(("fwd", "color"), (c.V, c.C, c.H, c.W), torch.float32, dev), ws.get(("fwd", "invdepth"), (c.V, 1, c.H, c.W), torch.float32, dev))


def check_forward_bits(run, **kw):
    """kw: further switches of the forward (a bin_capacity, check_capacity)."""
    from skelsplat_amd import rasterizer as R
    c = run.c
    ws = run.nan_workspace()
    color, inv, radii, st, final_T, n_contrib = run.forward(ws, want_aux=True, **kw)
    assert color.data_ptr() == held_nan(ws, c, run.dev)[0].data_ptr(), "the forward did not render into the NaN-filled outputs"
    binned = run.regime["path"] == _lib.PATH_BINNED
    if binned:
        pl, rg, nr = R.export_lists(st)
    for v in range(c.V):
        o = run.fwd[v]
        assert np.array_equal(radii[v].cpu().numpy(), o["radii"]), f"view {v}: radii"
        for name, got, want in (("colour", color[v], o["color"]), ("inverse depth", inv[v], o["invdepth"]), ("final_T", final_T[v], o["final_T"]),
                                ("n_contrib", n_contrib[v], o["n_contrib"].astype(np.int32))):
            got = got.cpu().numpy()
            bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
            assert not bad.any(), (f"{c.name} view {v}: {name} differs from the oracle at {int(bad.sum())} of {bad.size} elements "
                                   f"({int(np.isnan(got).sum())} left NaN), first at {tuple(int(i) for i in np.argwhere(bad)[0])}")
        if binned:
            assert int(nr[v].item()) == o["R"]
            assert np.array_equal(rg[v].cpu().numpy().astype(np.uint32), o["ranges"]), f"view {v}: ranges"
            assert np.array_equal(pl[v, :o["R"]].cpu().numpy().astype(np.uint32), o["point_list"]), f"view {v}: point_list"


def check_gradients(run, stats=None, want_dfeatures=True):
    """stats: a dict that receives the largest bound excess per gradient (the cases held to the computed bound).
    want_dfeatures=False: the backward that skips the channels no Gaussian of a tile has a feature on; six gradients."""
    import torch
    from tests import util
    c = run.c
    _, _, _, st = run.forward()
    g = run.backward(st, want_dfeatures=want_dfeatures)
    torch.cuda.synchronize()
    failures = []
    for key, oname in GRADS:
        if g[key] is None and not want_dfeatures and key == "features":
            continue
        got = g[key].cpu().numpy()
        for v in range(c.V):
            want = run.bwd[v][oname]
            try:
                if run.bound:
                    ex = util.bound_excess(got[v], want, run.bwd[v]["bound"][oname])
                    if stats is not None:
                        stats[oname] = max(stats.get(oname, 0.0), ex)
                    print(f"{c.name} view {v} {oname}: excess {ex:.2f} x 2^-24 x sum|terms| (allowed {util.BOUND_KAPPA:g})")
                    util.assert_close_bound(f"{c.name} view {v} {oname}", got[v], want, run.bwd[v]["bound"][oname])
                else:
                    util.assert_close(f"{c.name} view {v} {oname}", got[v], want)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)
    vis = run.fwd[0]["radii"] > 0
    assert np.abs(run.bwd[0]["dL_dopacity"][vis]).max() > 0, "the case has no gradient to get wrong"




def fuzz_case(seed):
    """A shape drawn from the regime boundaries -- a threshold width or height, +- one tile, +- one pixel, W mod 4 in all four
    classes -- with one of the three (P, path) combinations, through the same builder."""
    rng = np.random.default_rng(77000 + seed)
    t = thresholds()
    kind = seed % 3
    if rng.uniform() < 0.7:      # a width boundary, two or three bands
        W0 = int(rng.choice([16, 32, 512, t["cw4"], t["cw8"], 4096, t["magic"], SCAN_WIDE, MAX_W]))
        W = W0 + int(rng.choice([-16, 0, 16])) + int(rng.choice([-1, 0, 0, 1, 2, 3]))
        H = int(rng.choice([15, 16, 17, 18, 33, 34]))
    else:                        # a height boundary, one to three tile columns
        H0 = int(rng.choice([t["per_plane"], t["per_view"], 16 * GATHER_ROW]))
        H = H0 + int(rng.choice([-16, 0, 16])) + int(rng.choice([-1, 0, 1, 2]))
        W = int(rng.choice([4, 6, 15, 16, 17, 33, 48]))
    W, H = min(max(W, 1), MAX_W), min(max(H, 1), MAX_H)
    P = (5, 80, 80)[kind]
    return make(f"fuzz{seed}-{W}x{H}-{('P5', 'P80', 'binned')[kind]}", W, H, P, 3, V=1 if W * H > 1 << 20 else 2, seed=seed,
                dense=seed % 2 == 0, extras=(seed // 2) % 2 == 0, force_binned=kind == 2)


def run_case(seed, dev):
    """tools/fuzz_binned.py `geom`, tests/test_fuzz_gpu.py: forward bit for bit, the seven gradients, the small path against the binned."""
    import torch
    c = fuzz_case(seed)
    run = Run(c, dev)
    check_forward_bits(run)
    check_gradients(run)
    color, inv, radii, _ = run.forward()
    if run.regime["path"] == _lib.PATH_SMALL:
        cb, ib, rb, _ = run.forward(force_binned=True)
        assert torch.equal(cb, color) and torch.equal(ib, inv) and torch.equal(rb, radii), f"{c.name}: the binned forward differs from the small path"
    vis = int((run.fwd[0]["radii"] > 0).sum())
    return {"visible": vis, "pixels": c.W * c.H, "grad": float(np.abs(run.bwd[0]["dL_dopacity"]).max())}
