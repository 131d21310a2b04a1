"""Rasterizer scenes whose TILE-LIST LENGTHS sit at the limits of the binned path, shared by tests/test_list_length_cpu.py (the
oracle, the compiled reference and the library's own list-regime query), tests/test_list_length_gpu.py (parity on the device) and
tools/fuzz_binned.py (kind "lists").

The binned path orders or walks a tile's list in six ways by its length (sks_binned.inc, sks_common.inc):
  1 .. ws entries            ranked by the forward's wavefront as it loads them (load_chunk, sort=true);
  ws+1 .. wk                 sort_list_wave: kn = 2 .. wk/64 registers per lane, the last chunk partial or whole;
  wk+1 .. lds                sort_long_tile: the scatter workgroup's bitonic network in LDS, N = the next power of two;
  more than lds              the same network on keys kept in global memory, in the still unused partial-sum rows;
  up to ll long tiles a band their columns are remembered by k_bin_band_scatter;
  more than ll               they are found again by a walk over all columns
(ws, wk, lds, ll = _lib.list_regime()'s wave_sort, wave_k, sort_lds, long_list).  No threshold is written down here: every P,
W and length derives from that query, so a retuned constant moves the cases, and every case carries `lists`, claims about its
lengths that are checked on the ORACLE alone (check_lists) before anything runs on a device -- a case that no longer reaches its
branch fails instead of quietly missing it.

Scenes.  The near-orthographic camera of tests/geometry_cases.py (focal length F = 2**20, a world unit is a pixel).  A Gaussian
whose centre lies inside a tile is in that tile's list, so a list length is set by construction:
  ladder   48 x 48 (3 x 3 tiles), every centre in the middle tile: its list is exactly P.  Small blobs (sigma 1.5 - 4 px) of low
           opacity, so that the tail of the list is really composited (n_contrib.max() > 0.75 P);
  depths   a ladder whose Gaussians share ONE camera-space z (the order is the index alone) or EIGHT (groups of indices in
           shuffled order): the (depth bits, index) tie-break of the three long-list sorters;
  saturate a ladder whose three nearest Gaussians are opaque, flat over the tile and centred in its upper (lower) 8 rows: every
           pixel of that half-tile stops inside the first chunk, the other half composites the whole list;
  wide     H = 16 (one band) of wk + 44 sheets (sigma_x 3000 px, sigma_y 1 - 3 px): every column's list is long.  16 ll pixels
           wide (ll long tiles: the last remembered column), 16 more (ll + 1: the walk), and one in which a third of the sheets
           is narrow, so that some columns fall to the forward's sorter and others stay above it;
  classes  one band with a tile of every length class (BIN_CLASSES: the lists by which the tiles are dispatched).
(`claims`, as in the geometry cases, stays what sks_launch_regime is asked: the binned path, the per-tile backward.)"""
import functools
import math

import numpy as np

from tests import geometry_cases as G
from skelsplat_amd import _lib

F = G.F
TILE = 16


class Case(G.Case):
    def __repr__(self):
        return f"<list-length case {self.name}>"


@functools.lru_cache(maxsize=None)
def regime():
    return _lib.list_regime()


def _finish(c, px, py, Z, scales, ang, opac, rng, dense):
    P, C, W, H = c.P, c.C, c.W, c.H
    means = np.stack([(px - 0.5 * (W - 1)) * Z / F, (py - 0.5 * (H - 1)) * Z / F, Z], axis=1)
    quats = np.stack([np.cos(0.5 * ang), np.zeros(P), np.zeros(P), np.sin(0.5 * ang)], axis=1)      # a turn about the view axis
    c.means, c.scales, c.quats = (np.ascontiguousarray(a, np.float32) for a in (means, scales, quats))
    c.opac = np.ascontiguousarray(opac, np.float32).reshape(P, 1)
    if dense:
        c.feat = rng.uniform(0.1, 1.0, (P, C)).astype(np.float32)
    else:
        c.feat = np.zeros((P, C), np.float32)
        c.feat[np.arange(P), rng.integers(0, C, P)] = 1.0
    if c.clamp:      # a share of the pixels outside [0, 1] on either side (a list this long averages its features: the channels
        # differ in their mean -- above 1, about 0, inside), so that the clamp's mask matters
        c.feat[:, 0::3] *= 3.0
        c.feat[:, 1::3] = (c.feat[:, 1::3] - 0.55) * 4.0
    c.bg = rng.uniform(0.1, 0.9, C).astype(np.float32) if c.extras else None
    c.cams, c.ocams = G.cameras(W, H, c.V)
    c.gx, c.gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    return c


def _new(name, W, H, P, C, V, seed, dense, extras, clamp, bound, lists):
    c = Case()
    c.name, c.W, c.H, c.P, c.C, c.V, c.seed = name, W, H, P, C, V, seed
    c.dense, c.extras, c.clamp, c.bound, c.flags = dense, extras, clamp, bound, 0
    c.force_binned = P <= _lib.SKS_SMALL_P
    c.claims = {"path": _lib.PATH_BINNED, "bwd": _lib.BWD_TILE}      # (of sks_launch_regime: G.check_claims)
    c.lists = dict(lists)
    return c


def ladder(name, P, C=17, V=1, seed=0, dense=True, extras=False, clamp=False, bound=False, depths=None, saturate=None):
    """depths: None = all distinct, in an order unrelated to the index; 1 / 8 = that many values.  saturate: "upper" / "lower"."""
    W = H = 3 * TILE
    lists = {"middle": P, "tail": 0.75}
    if depths:
        lists["depth_values"] = depths
    if saturate:
        lists["saturated"] = saturate
    c = _new(name, W, H, P, C, V, seed, dense, extras, clamp, bound, lists)
    rng = np.random.default_rng(9000 + seed)
    px, py = rng.uniform(TILE + 1.0, 2 * TILE - 1.0, P), rng.uniform(TILE + 1.0, 2 * TILE - 1.0, P)
    sg, ratio = rng.uniform(1.5, 4.0, P), rng.uniform(0.4, 1.0, P)
    scales = np.stack([sg, sg * ratio, np.full(P, 0.5)], axis=1)
    ang = rng.uniform(0, math.pi, P)
    # (opacities fall with the length of the list: a pixel's transmittance stays above the stop of 1e-4 to the list's end)
    opac = rng.uniform(0.006, max(0.009, 0.03 * min(1.0, 1000.0 / P)), P)
    if depths is None:      # 16 apart: an fp32 ulp at 2**20 is 1/16
        Z = F + 16.0 * (4 + rng.permutation(P))
    elif depths == 1:
        Z = np.full(P, F)
    else:
        Z = F + 16.0 * rng.integers(0, depths, P)
        Z[rng.permutation(P)[:depths]] = F + 16.0 * np.arange(depths)      # (every value is taken)
    if saturate:
        # alpha = 0.99 G stops a pixel after three such entries where G > 0.964: flat over the half-tile (16 x 8 pixels about the
        # centre: G > 0.97), and by then 0.67 .. 0.96 in the other half, whose pixels keep compositing
        k = np.sort(rng.permutation(P)[:3])
        px[k], py[k] = 1.5 * TILE - 0.5, (TILE + 3.5) if saturate == "upper" else (2 * TILE - 4.5)
        scales[k] = (80.0, 16.0, 0.5)
        ang[k] = 0.0
        opac[k] = 0.99
        Z[k] = F + 16.0 * np.arange(3)[rng.permutation(3)]
        c.opaque = k
    return _finish(c, px, py, Z, scales, ang, opac, rng, dense)


def wide(name, W, narrow=0.0, C=17, V=1, seed=0, dense=True, extras=False, clamp=False, bound=False, nlong=None):
    """nlong: the number of tile columns whose list is longer than wk -- a number, or "some" (at least one, and at least one
    column in ws+1 .. wk)."""
    r = regime()
    P = r["wave_k"] + 44
    c = _new(name, W, TILE, P, C, V, seed, dense, extras, clamp, bound, {"nlong": nlong, "tail": 0.75})
    rng = np.random.default_rng(9500 + seed)
    px, py = rng.uniform(0, W, P), rng.uniform(0.5, TILE - 0.5, P)
    sx = np.full(P, 3000.0)
    thin = rng.permutation(P)[:int(round(narrow * P))]
    sx[thin] = rng.uniform(150.0, 300.0, len(thin))      # (radius 450 .. 900 px, in the left half: the right columns lose them)
    px[thin] = rng.uniform(0, 0.5 * W, len(thin))
    scales = np.stack([sx, rng.uniform(1.0, 3.0, P), np.full(P, 0.5)], axis=1)
    ang = rng.uniform(-2e-4, 2e-4, P)
    opac = rng.uniform(0.01, 0.05, P)
    Z = F + 16.0 * (4 + rng.permutation(P))
    return _finish(c, px, py, Z, scales, ang, opac, rng, dense)


def classes(name, seed=0):
    """One band of as many tiles as there are tile classes; tile k holds 2**k entries (+ 1 from the second on: neither end of a
    class), each well inside it."""
    n = regime()["classes"]
    per = [(1 << k) + (1 if k else 0) for k in range(n)]
    P = sum(per)
    c = _new(name, TILE * n, TILE, P, 17, 1, seed, True, False, False, False, {"per_tile": per})
    rng = np.random.default_rng(9800 + seed)
    tile = rng.permutation(np.repeat(np.arange(n), per))
    px, py = TILE * tile + rng.uniform(6.0, 10.0, P), rng.uniform(6.0, 10.0, P)
    sg = rng.uniform(0.8, 1.2, P)      # (radius 4 at the most: no rect leaves its tile)
    scales = np.stack([sg, sg * rng.uniform(0.6, 1.0, P), np.full(P, 0.5)], axis=1)
    return _finish(c, px, py, F + 16.0 * (4 + rng.permutation(P)), scales, rng.uniform(0, math.pi, P), rng.uniform(0.01, 0.2, P), rng, True)


# ------------------------------------------------------------------------------------------------------------
# the set
# ------------------------------------------------------------------------------------------------------------
def ladder_lengths():
    """The ladder's P: both sides of every sorter's threshold, every register count of the wavefront's sorter with a whole and
    a partial last chunk, the LDS network at exact powers of two and one beyond, and one list far into global memory."""
    r = regime()
    ws, wk, lds = r["wave_sort"], r["wave_k"], r["sort_lds"]
    out = []
    for k in range(1, wk // 64):
        out += [64 * k, 64 * k + 1] if 64 * k >= ws else []
    out += [wk, wk + 1]
    n = 1
    while n <= wk:
        n *= 2
    while n < lds:
        out += [n, n + 1]
        n *= 2
    out += [lds, lds + 1, lds * 3 // 2 - 71]
    return sorted(set([ws, ws + 1] + out))


@functools.lru_cache(maxsize=None)
def specs():
    """name -> (builder, keyword arguments)."""
    r = regime()
    ws, wk, lds, ll = r["wave_sort"], r["wave_k"], r["sort_lds"], r["long_list"]
    out = {}
    k = 0

    def put(fn, name, **kw):
        nonlocal k
        kw.setdefault("seed", k)
        out[name] = (fn, dict(name=name, **kw))
        k += 1

    for P in ladder_lengths():
        put(ladder, f"ladder-{P}", P=P, dense=k % 2 == 0, extras=(k // 2) % 2 == 0)
    big = lds + 52
    for P in (wk - 56, 2 * wk + 88, big):
        put(ladder, f"depths1-{P}", P=P, depths=1)
        put(ladder, f"depths8-{P}", P=P, depths=8, dense=False)
    for P in (wk + 44, big):
        put(ladder, f"saturate-upper-{P}", P=P, saturate="upper", dense=P == big)
        put(ladder, f"saturate-lower-{P}", P=P, saturate="lower", dense=P != big, extras=True)
    put(wide, f"wide-{16 * ll}", W=16 * ll, nlong=ll)
    put(wide, f"wide-{16 * ll + 16}", W=16 * ll + 16, nlong=ll + 1, dense=False, extras=True)
    put(wide, f"wide-mixed-{8 * ll + 8}", W=8 * ll + 8, narrow=1.0 / 3.0, nlong="some")
    put(classes, "classes")
    put(ladder, f"onehot17-{big}", P=big, C=17, dense=False)
    put(ladder, f"dense17-{big}", P=big, C=17, dense=True)
    put(ladder, f"dense32-{big}", P=big, C=32, dense=True)
    put(ladder, f"extras-{big}", P=big, extras=True)
    put(ladder, f"nofeat-{big}", P=big, dense=False)       # (run without want_dfeatures: the backward that skips channels)
    return out


def BIG():
    """The length of the scene the switches are run on: 52 entries into the global-memory sort."""
    return regime()["sort_lds"] + 52


def NOFEAT():
    return f"nofeat-{BIG()}"


def LONGEST():
    return f"ladder-{ladder_lengths()[-1]}"


def names():
    return list(specs())


def get(name):
    fn, kw = specs()[name]
    return fn(**kw)


def clamp_cases():
    """The lds + 52 ladder and the narrowest wk + 44 band with features outside [0, 1] (three channels: the reference of the clamped
    backward is fp64 autograd over every Gaussian)."""
    r = regime()
    return {"clamp-ladder": lambda: ladder("clamp-ladder", P=r["sort_lds"] + 52, C=3, seed=70, clamp=True),
            "clamp-wide": lambda: wide("clamp-wide", W=16 * r["long_list"], C=3, seed=71, clamp=True, nlong=r["long_list"])}


def one_call_case():
    return ladder("one-call", P=BIG(), C=17, V=3, seed=72, extras=True)


# ------------------------------------------------------------------------------------------------------------
# the claims, on the oracle alone
# ------------------------------------------------------------------------------------------------------------
def lengths(o, c):
    rg = o["ranges"].reshape(c.gy, c.gx, 2).astype(np.int64)
    return rg[..., 1] - rg[..., 0]


def rows_of(n):
    """The rows of the sorter table a list of n entries belongs to."""
    r = regime()
    ws, wk, lds = r["wave_sort"], r["wave_k"], r["sort_lds"]
    if n <= 0:
        return set()
    if n <= ws:
        return {"load"}
    if n <= wk:
        return {"wave", f"wave-k{(n + 63) // 64}", "wave-whole" if n % 64 == 0 else "wave-partial"}
    N = 1 << (n - 1).bit_length()
    if n <= lds:
        return {"lds", "lds-pow2" if n == N else "lds-padded"}
    return {"global"}


def claimed_rows(c):
    """What a case's claims put it in (test_the_set_covers_every_regime): rows of the table, thresholds met exactly."""
    r = regime()
    out = set()
    if "middle" in c.lists:
        n = c.lists["middle"]
        out |= rows_of(n) | {f"len={n}"}
    if "nlong" in c.lists:
        n, ll = c.lists["nlong"], r["long_list"]
        out |= {"lds"}
        if n == "some":
            out |= {"remembered", "wave"}
        else:
            out |= {"remembered" if n <= ll else "walk", f"nlong={n}"}
    if "per_tile" in c.lists:
        out |= {f"class-{min(r['classes'] - 1, x.bit_length() - 1)}" for x in c.lists["per_tile"]}
    if "depth_values" in c.lists:
        out |= {f"ties-{x}" for x in rows_of(c.lists["middle"]) if x in ("wave", "lds", "global")}
    if "saturated" in c.lists:
        out |= {f"saturate-{c.lists['saturated']}-{x}" for x in rows_of(c.lists["middle"]) if x in ("wave", "lds", "global")}
    return out


def check_lists(c, o):
    """Asserts every claim of c.lists on the oracle's forward `o` of the first view; -> what the case reached."""
    r = regime()
    wk = r["wave_k"]
    n = lengths(o, c)
    nc = o["n_contrib"].astype(np.int64)
    got = {"longest": int(n.max()), "entries": int(o["R"]), "n_contrib": int(nc.max()), "nlong": int((n > wk).sum(axis=1).max()),
           "classes": sorted({min(r["classes"] - 1, int(x).bit_length() - 1) for x in n.ravel() if x > 0})}
    assert (o["radii"] > 0).all(), f"{c.name}: a Gaussian is culled"
    if "middle" in c.lists:
        assert c.gx == 3 and c.gy == 3 and n[1, 1] == c.lists["middle"] == c.P, f"{c.name}: the middle tile's list has {n[1, 1]} entries"
        mid = nc[TILE:2 * TILE, TILE:2 * TILE]
    else:
        mid = nc
    if "per_tile" in c.lists:
        assert c.gy == 1 and list(n[0]) == c.lists["per_tile"] and got["classes"] == list(range(r["classes"])), f"{c.name}: lists of {list(n[0])}"
    if "nlong" in c.lists:
        want = c.lists["nlong"]
        if want == "some":
            fwd = int(((n > r["wave_sort"]) & (n <= wk)).sum())
            assert 0 < got["nlong"] < c.gx and fwd > 0, f"{c.name}: {got['nlong']} columns above {wk}, {fwd} in the forward's sorter's range"
            got["forward_sorted"] = fwd
        else:
            assert c.gy == 1 and got["nlong"] == want, f"{c.name}: {got['nlong']} long columns, not {want}"
            assert (n == c.P).all(), f"{c.name}: not every column holds every sheet"
    if "depth_values" in c.lists:
        a, b = o["ranges"].reshape(c.gy, c.gx, 2)[1, 1]
        vals = np.unique(o["keys"][a:b] & np.uint64(0xffffffff))
        assert 1 <= len(vals) <= c.lists["depth_values"], f"{c.name}: {len(vals)} depth values in the middle tile"
        got["depth_values"] = len(vals)
    if "saturated" in c.lists:
        up = c.lists["saturated"] == "upper"
        half, other = (mid[:8], mid[8:]) if up else (mid[8:], mid[:8])
        assert 1 <= half.min() and half.max() <= 3, f"{c.name}: the saturated half-tile's n_contrib runs {half.min()} .. {half.max()}"
        a, b = o["ranges"].reshape(c.gy, c.gx, 2)[1, 1]
        assert set(o["point_list"][a:a + 3]) == set(c.opaque), f"{c.name}: the opaque three are not the nearest"
        mid = other
        got["saturated_pixels"] = int(half.size)
    if "tail" in c.lists:
        assert mid.max() > c.lists["tail"] * c.P, f"{c.name}: n_contrib reaches {mid.max()} of {c.P}: the tail is not composited"
    return got


# ------------------------------------------------------------------------------------------------------------
# on the device (tests/test_list_length_gpu.py, tools/fuzz_binned.py)
# ------------------------------------------------------------------------------------------------------------
class Run(G.Run):
    """G.Run of a list-length case; the case's claims are asserted on the oracle before the device is touched."""

    def __init__(self, c, dev):
        fwd = [G.oracle_forward(c, v) for v in range(c.V)]
        self.reached = check_lists(c, fwd[0])
        super().__init__(c, dev, fwd=fwd, bound=c.bound)


def clamped_autograd(c, v=0):
    """The gradients of sum(clip(colour, 0, 1) * dL) of view v by fp64 autograd over oracle/torch_ref.py (what the clamped backward
    is held to: the oracle's backward has no clamp): {the device's gradient name: array}, and the unclamped colour."""
    import torch
    from oracle import torch_ref
    dLc, dLi = G.draw_dL(c)
    tt = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tm, tf, to, ts, tq = tt(c.means), tt(c.feat), tt(c.opac), tt(c.scales), tt(c.quats)
    m2 = torch.zeros(c.P, 3, dtype=torch.float64, requires_grad=True)
    cam = c.cams[v]
    col, radii, inv = torch_ref.rasterize(tm, m2, tf, to, ts, tq, None, cam.world_view_transform.cpu(), cam.full_proj_transform.cpu(), c.W, c.H,
                                          math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                          bg=None if c.bg is None else torch.tensor(c.bg), dtype=torch.float64)
    loss = (col.clamp(0, 1) * torch.tensor(dLc[v], dtype=torch.float64)).sum()
    if dLi is not None:
        loss = loss + (inv * torch.tensor(dLi[v], dtype=torch.float64)).sum()
    loss.backward()
    grads = {"means3D": tm.grad, "means2D": m2.grad, "opacities": to.grad, "scales": ts.grad, "rotations": tq.grad, "features": tf.grad}
    return {k: g.numpy() for k, g in grads.items()}, col.detach().numpy()


def fuzz_case(seed):
    """A ladder whose length is drawn around a threshold (+- 1, +- 64), with every switch drawn too."""
    rng = np.random.default_rng(88000 + seed)
    r = regime()
    ws, wk, lds = r["wave_sort"], r["wave_k"], r["sort_lds"]
    base = int(rng.choice([ws, 2 * ws, wk, 512, 1024, lds]))
    P = max(2, base + int(rng.choice([-64, -1, 0, 1, 64])) + int(rng.choice([0, 0, 0, -1, 1])))
    depths = [None, None, 1, 8][int(rng.integers(0, 4))] if P >= 16 else None
    sat = [None, None, "upper", "lower"][int(rng.integers(0, 4))] if depths is None and P > 8 else None
    return ladder(f"fuzz{seed}-{P}", P=P, C=int(rng.choice([3, 17, 32])), V=int(rng.integers(1, 3)), seed=1000 + seed,
                  dense=bool(rng.integers(0, 2)), extras=bool(rng.integers(0, 2)), depths=depths, saturate=sat)


def run_case(seed, dev):
    """tools/fuzz_binned.py `lists`, tests/test_fuzz_gpu.py: forward bit for bit, the seven gradients."""
    c = fuzz_case(seed)
    run = Run(c, dev)
    G.check_forward_bits(run)
    G.check_gradients(run)
    return {"longest": run.reached["longest"], "n_contrib": run.reached["n_contrib"], "grad": float(np.abs(run.bwd[0]["dL_dopacity"]).max())}
