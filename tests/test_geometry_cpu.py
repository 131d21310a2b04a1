"""The geometry cases (tests/geometry_cases.py) are what they say, on the reference and the library's launch-regime query alone:
every case reaches the regime in its claim list (sks_launch_regime: host only, no GPU), and holds the visible count, the
overlapping pair, the culled Gaussian, the corner tiles, the seam tiles, the wide rect and the empty bands it promises -- read from
the oracle's ranges, point_list and radii of its first view."""
import numpy as np
import pytest

from tests import geometry_cases as G
from skelsplat_amd import _lib


def rects(o, c):
    """getRect (auxiliary.h) of every Gaussian from the oracle's pixel centres and radii: (P, 4) = x0, y0, x1, y1 in tiles."""
    xy, r = o["xy"].astype(np.float32), o["radii"].astype(np.float32)
    lo = lambda p, g: np.clip(((p - r) / np.float32(16)).astype(np.int64), 0, g)
    hi = lambda p, g: np.clip(((p + r + np.float32(15)) / np.float32(16)).astype(np.int64), 0, g)
    rc = np.stack([lo(xy[:, 0], c.gx), lo(xy[:, 1], c.gy), hi(xy[:, 0], c.gx), hi(xy[:, 1], c.gy)], axis=1)
    rc[o["radii"] <= 0] = 0
    return rc


def test_thresholds_are_found_not_written_down():
    """With today's constants the query gives the shapes of the pull request that added these cases; the assertion is on the
    REGIMES either side of each (a retune moves the shape, and the cases with it)."""
    t = G.thresholds()
    q = G._q
    assert q(5, 3, t["cw4"], 17)["cw"] <= 4 < q(5, 3, t["cw4"] + 16, 17)["cw"] <= 8
    assert q(5, 3, t["cw8"], 17)["cw"] <= 8 < q(5, 3, t["cw8"] + 16, 17)["cw"]
    assert q(5, 3, t["magic"] - 4, 16)["w_magic"] == 1 and q(5, 3, t["magic"], 16)["w_magic"] == 0
    assert q(5, 3, G.SCAN_WIDE, 17, _lib.SKS_FORCE_BINNED)["bpc"] == 1
    assert [q(5, 3, 48, t["per_plane"] + d)["cover"] for d in (0, 16)] == [_lib.COVER_PER_PLANE, _lib.COVER_PER_VIEW]
    assert [q(5, 3, 48, t["per_view"] + d)["cover"] for d in (0, 16)] == [_lib.COVER_PER_VIEW, _lib.COVER_NONE]
    # the cap of 32 passes per fill block (one skip bit per pass) binds on the widest images
    # (without it a band row is cut into ~8 fill blocks; with it into more)
    wide, mid = q(5, 3, G.MAX_W, 16, _lib.SKS_FILL_LINEAR), q(5, 3, t["magic"] - 1024, 16, _lib.SKS_FILL_LINEAR)
    assert wide["pb"] == 32 and wide["fsplit"] > 9 and mid["pb"] < 32 and mid["fsplit"] <= 9


def test_regime_query_refuses_what_the_entry_points_refuse():
    for W, H in ((G.MAX_W + 1, 16), (16, G.MAX_H + 1), (0, 16)):
        with pytest.raises(RuntimeError, match="out of range"):
            _lib.launch_regime(1, 5, 3, W, H)
        with pytest.raises(RuntimeError, match="out of range"):
            _lib.scratch_bytes(1, 5, 3, W, H)
    r = _lib.launch_regime(2, 5, 3, 1000, 24, 0, False)
    assert r["lead"] == 31 and _lib.launch_regime(2, 5, 3, 1000, 24)["lead"] == 0


def test_the_set_covers_every_regime():
    sp = G.specs()
    cs = {n: s["claims"] for n, s in sp.items()}
    small = [c for c in cs.values() if c.get("path") == _lib.PATH_SMALL]
    assert {c.get("cover") for c in small} >= {_lib.COVER_NONE, _lib.COVER_PER_VIEW, _lib.COVER_PER_PLANE}
    assert {c.get("bwd") for c in cs.values()} >= {_lib.BWD_WAVE, _lib.BWD_GATHER, _lib.BWD_TILE}
    assert any(c.get("bpc") == 1 for c in cs.values()) and any(c.get("half") == 1 and c.get("w_magic") == 0 for c in cs.values())
    assert any(c.get("ppt") == 1 and c.get("w_magic") == 0 for c in cs.values())
    assert sum(1 for s in sp.values() if s["dense"]) * 2 in range(len(sp) - 1, len(sp) + 2)
    assert G.TALL_GATHER in sp and sp[G.TALL_GATHER]["claims"]["bwd"] == _lib.BWD_GATHER


@pytest.mark.parametrize("name", G.names())
def test_case_is_what_it_says(name):
    c = G.get(name)
    r = G.check_claims(c)
    assert (r["gx"], r["gy"]) == (c.gx, c.gy)
    assert G.host_bytes(c) <= 64 << 20
    o = G.oracle_forward(c, 0)
    rc = rects(o, c)
    vis = o["radii"] > 0
    hidden = c.roles["culled"] + c.roles.get("outside", [])
    assert vis.sum() == c.P - len(hidden) and not vis[hidden].any(), (vis.sum(), c.P, hidden)
    ranges = o["ranges"].reshape(c.gy, c.gx, 2).astype(np.int64)
    n = ranges[..., 1] - ranges[..., 0]
    assert n[0, 0] > 0 and n[-1, -1] > 0, "first / last tile not covered"
    (a,), (p,) = c.roles["anchor"], c.roles["pair"]
    both = [(y, x) for y in range(rc[a, 1], rc[a, 3]) for x in range(rc[a, 0], rc[a, 2])
            if rc[p, 0] <= x < rc[p, 2] and rc[p, 1] <= y < rc[p, 3]]
    assert both, "the pair shares no tile"
    y, x = both[0]
    lst = o["point_list"][ranges[y, x, 0]:ranges[y, x, 1]]
    assert a in lst and p in lst and len(lst) >= 2
    for s in c.seams:
        assert ((n[:, s - 1] > 0) & (n[:, s] > 0)).any(), f"seam {s - 1}|{s} not covered on both sides"
    if G.seams_of(c.W):
        assert c.seams and c.seams[0] == G.seams_of(c.W)[-1]
        if c.P > 5:
            assert set(c.seams) >= {s for s in (96, 224) if s in G.seams_of(c.W)}
    if c.gx > 10:
        assert rc[a, 2] - rc[a, 0] > 8, "the anchor does not cross more than 8 tile columns"
    if c.empty_bands:
        assert (n.sum(axis=1) == 0).any(), "no band without a rect"
    assert c.empty_bands or c.gy < 20
    if c.name.startswith("tall-16x"):
        assert (rc[:, 3] >= G.GATHER_ROW).any() and c.gy > G.GATHER_ROW
        if c.P > 5:      # ... and not only the corner Gaussian: some with a neighbour in their list
            deep = np.nonzero(rc[:, 3] >= G.GATHER_ROW)[0]
            assert len(deep) >= 4 and (n[G.GATHER_ROW - 2:] >= 2).any()
