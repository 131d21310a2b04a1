"""The debug pictures on the device (skelsplat_amd/preview.py, csrc/sks_preview.hip): every picture is compared BIT FOR BIT with
the numpy restatement of the fixed sequence (tests/preview_ref.py), which tests/test_preview_cpu.py holds to the reference's own
pictures (tests/golden/reference_images.npz).  Each plane-path shape asserts, through sks_preview_launch, the load width, store
width and workgroup counts it was chosen for; the factor path is compared with the plane path over what sks_heatmaps writes; the
loops' pictures with those of a MultiViewLoop running each frame alone."""
import copy
import os

import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, io, preview
from tests import preview_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (W, H) -> (load bytes, store bytes, workgroups of pass A, of pass B); tests/test_preview_cpu.py holds the same table to the library
SHAPES = {(1, 1): (4, 1, 1, 1), (3, 5): (4, 1, 1, 1), (16, 4): (16, 16, 1, 1), (20, 3): (16, 1, 1, 1), (18, 7): (4, 1, 1, 1),
          (64, 48): (16, 16, 3, 1), (257, 1): (4, 1, 2, 2), (4, 257): (16, 1, 2, 5), (3, 171): (4, 1, 3, 3), (1024, 17): (16, 16, 17, 5)}


def _regime(W, H, aligned=True):
    r = _lib.preview_launch(W, H, aligned)
    return r["load_bytes"], r["store_bytes"], r["groups_sum"], r["groups_pack"]


def _check(planes, device, what=""):
    """channel_sum_u8 of host planes (V,C,H,W) equals the restatement: pictures and {lo, hi}."""
    want_q, want_mm = pr.preview_views(planes)
    got_q, got_mm = preview.channel_sum_u8(torch.from_numpy(planes).to(device), return_minmax=True)
    assert got_q.dtype == torch.uint8 and tuple(got_q.shape) == want_q.shape and got_mm.dtype == torch.float32
    got_q, got_mm = got_q.cpu().numpy(), got_mm.cpu().numpy()
    assert np.array_equal(got_mm, want_mm, equal_nan=True), (what, got_mm, want_mm)
    assert np.array_equal(got_q, want_q), (what, int((got_q != want_q).sum()))
    return got_q


def _random_planes(rng, V, C, H, W):
    """Blob-like planes (mostly small, some zero) with a different scale and offset per view."""
    p = np.maximum(rng.normal(0.0, 1.0, (V, C, H, W)), 0.0).astype(np.float32) ** 2
    return (p * np.arange(1, V + 1, dtype=np.float32)[:, None, None, None] + np.arange(V, dtype=np.float32)[:, None, None, None] * 0.5).astype(np.float32)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_images.npz"))


@pytest.mark.parametrize("shape", list(SHAPES), ids=[f"{w}x{h}" for w, h in SHAPES])
def test_plane_path_shapes(device, shape):
    """V = 3 views of different contents (a view that read another's partials would be caught), C = 17."""
    W, H = shape
    assert _regime(W, H) == SHAPES[shape]
    rng = np.random.default_rng(W * 1000 + H)
    planes = _random_planes(rng, 3, 17, H, W)
    if W * H == 1:
        planes[1] = -planes[1]      # (a one-pixel view is flat: an all-zero picture, whatever its value)
    q = _check(planes, device, shape)
    if W * H > 1:
        assert (q.reshape(3, -1).max(axis=1) == 255).all() and (q.reshape(3, -1).min(axis=1) == 0).all()
    single = preview.channel_sum_u8(torch.from_numpy(planes[2]).to(device))        # (C,H,W) -> (H,W)
    assert tuple(single.shape) == (H, W) and np.array_equal(single.cpu().numpy(), q[2])


@pytest.mark.parametrize("shape", [(257, 1), (4, 257), (3, 171), (64, 48), (1024, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_extrema_in_different_workgroups(device, shape):
    """Two or more workgroups per view (257 x 1 and 4 x 257 are the smallest such sizes with scalar and 16-byte loads; 3 x 171,
    64 x 48 and 1024 x 17 take an odd count): the minimum in the first workgroup's first lane and the maximum in the LAST pixel,
    which the last workgroup reads and whose partial the last lane of pass B's reduction holds -- and the other way round."""
    W, H = shape
    ld, st, ga, gb = _regime(W, H)
    assert ga >= 2
    unit = 4 if ld == 16 else 1
    last = (W * H - 1) // unit
    assert (last // 256) % ga == ga - 1 and 0 // 256 == 0       # the last pixel's unit belongs to the last workgroup
    rng = np.random.default_rng(7)
    planes = rng.uniform(1.0, 2.0, (2, 15, H, W)).astype(np.float32)
    flat = planes.reshape(2, 15, -1)
    flat[0, :, 0], flat[0, :, -1] = -3.0, 9.0
    flat[1, :, 0], flat[1, :, -1] = 11.0, -2.5
    q = _check(planes, device, shape).reshape(2, -1)
    assert q[0, 0] == 0 and q[0, -1] == 255 and q[1, 0] == 255 and q[1, -1] == 0
    assert ((q[:, 1:-1] > 0) & (q[:, 1:-1] < 255)).all()


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("C", [1, 15, 17, 19, _lib.SKS_MAX_CHANNELS])
def test_channel_counts_and_batches(device, C, V):
    """Every remainder of the channel loop's unroll by four, with 16-byte loads (64 x 48) and scalar loads (18 x 7)."""
    rng = np.random.default_rng(100 * C + V)
    for W, H in ((64, 48), (18, 7)):
        _check(rng.normal(0.0, 1.0, (V, C, H, W)).astype(np.float32), device, (C, V, W, H))


def test_more_channels_than_the_entry_takes_are_refused(device):
    with pytest.raises(ValueError, match="33 channels, at most 32"):
        preview.channel_sum_u8(torch.zeros((1, 33, 4, 4), device=device))
    lib = _lib.load()
    x = torch.zeros(64, device=device)
    assert lib.sks_preview_planes(1, 33, 1, 1, x.data_ptr(), x.data_ptr(), None, x.data_ptr(), None) == -1
    assert lib.sks_last_error().decode() == "preview_planes: C = 33 channels, at most 32 (SKS_MAX_CHANNELS)"


def test_the_references_hand_made_pictures(device, golden):
    """The 0 .. 255 ramp (any quotient one ulp low would show as k - 1), negative values, C = 15 / 17 / 19 / 1 at odd sizes: the
    device's bytes are the ones the reference's own save_heatmaps wrote."""
    for name in golden["hand_names"]:
        planes, png = golden[f"hand_{name}_planes"], golden[f"hand_{name}_png"]
        q = _check(planes[None], device, name)
        assert np.array_equal(q[0], png), name
    assert np.array_equal(golden["hand_ramp17_png"].reshape(-1), np.arange(256))


def test_the_references_loop_pictures_from_their_planes(device, golden):
    for name in ("heatmap", "render_1", "render"):
        q = _check(golden[name + "_planes"], device, name)
        assert np.array_equal(q, golden[name + "_png"]), name


@pytest.mark.parametrize("shape", [(64, 48), (18, 7), (257, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_undefined_views_are_all_zero_pictures(device, shape):
    """A flat view and views that hold a NaN, +inf or -inf: all-zero pictures, {lo, hi} reported as they are (NaN / inf), and the
    neighbour views untouched.  The bad pixel sits in the last workgroup's share."""
    W, H = shape
    rng = np.random.default_rng(5)
    good = _random_planes(rng, 6, 17, H, W)
    planes = good.copy()
    planes[1] = 0.125                                    # flat: every sum is 17 x 0.125
    for v, bad in ((2, np.nan), (3, np.inf), (4, -np.inf)):
        planes[v, 9].reshape(-1)[-1] = bad
    q = _check(planes, device, shape)
    assert not q[1:5].any()
    want = pr.preview_views(good)[0]
    assert np.array_equal(q[0], want[0]) and np.array_equal(q[5], want[5]) and q[0].max() == q[5].max() == 255
    mm = preview.channel_sum_u8(torch.from_numpy(planes).to(device), return_minmax=True)[1].cpu().numpy()
    assert mm[1, 0] == mm[1, 1] == np.float32(17 * 0.125) and np.isnan(mm[2]).all()
    assert mm[3, 1] == np.inf and np.isfinite(mm[3, 0]) and mm[4, 0] == -np.inf and np.isfinite(mm[4, 1])


@pytest.mark.parametrize("shape", [(64, 48), (16, 4), (20, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_unaligned_bases_fall_back(device, shape):
    """Planes and picture sliced by one element: sizes that take the 16-byte paths otherwise go through the scalar loads and the
    byte stores -- the same bytes -- and nothing outside the picture is written."""
    W, H = shape
    V, C, n = 2, 17, W * H
    assert _regime(W, H)[0] == 16 and _regime(W, H, aligned=False)[:2] == (4, 1)
    rng = np.random.default_rng(11)
    planes = _random_planes(rng, V, C, H, W)
    buf = torch.zeros(V * C * n + 1, device=device)
    buf[1:] = torch.from_numpy(planes).to(device).reshape(-1)
    src = buf[1:]
    outbuf = torch.full((V * n + 2,), 77, dtype=torch.uint8, device=device)
    out = outbuf[1:-1]
    assert src.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 1
    lib = _lib.load()
    scratch = torch.empty(lib.sks_preview_scratch_bytes(V, W, H), dtype=torch.uint8, device=device)
    mm = torch.empty((V, 2), device=device)
    for s, o in ((src, out), (src, None), (None, out)):       # both sliced; only the planes; only the picture
        aligned_in = torch.from_numpy(planes).to(device)
        aligned_out = torch.empty(V * n, dtype=torch.uint8, device=device)
        a, b = (s if s is not None else aligned_in), (o if o is not None else aligned_out)
        outbuf.fill_(77)
        rc = lib.sks_preview_planes(V, C, W, H, a.data_ptr(), scratch.data_ptr(), mm.data_ptr(), b.data_ptr(),
                                    torch.cuda.current_stream(device).cuda_stream)
        _lib.check(rc, "sks_preview_planes")
        want_q, want_mm = pr.preview_views(planes)
        assert np.array_equal(b.cpu().numpy().reshape(V, H, W), want_q)
        assert np.array_equal(mm.cpu().numpy(), want_mm)
        assert int(outbuf[0]) == 77 and int(outbuf[-1]) == 77


# ----------------------------------------------------------------------------------------------------------------------------
# the factor path
# ----------------------------------------------------------------------------------------------------------------------------
def _cameras(golden, device, widths=None, sizes=None):
    """The fixture's four cameras; `widths` / `sizes` [(W, H)]: the same cameras on other sensors, the principal point kept in the
    middle."""
    from skelsplat_amd.scene import Camera
    cams = []
    for i in range(4):
        W, H = (int(x) for x in golden["cam_WH"][i])
        K = golden["cam_K"][i].copy()
        w, h = sizes[i] if sizes is not None else (widths[i] if widths is not None else W, H)
        K[0, 2] += (w - W) / 2
        K[1, 2] += (h - H) / 2
        cams.append(Camera(i, golden["cam_R"][i], golden["cam_T"][i], K, w, h).to(device))
    return cams


def _detections(golden, sizes):
    """The fixture's detections moved with the principal points of _cameras(sizes=)."""
    p2d = golden["poses_2d"][..., :2].astype(np.float32).copy()
    for i, (w, h) in enumerate(sizes):
        W, H = (int(x) for x in golden["cam_WH"][i])
        p2d[i] += np.array([(w - W) / 2, (h - H) / 2], dtype=np.float32)
    return p2d


def _factors(golden, device, cams, p2d=None, drop_mask=None):
    """The heat-map factors of the fixture's scene at its initial Gaussians, by sks_heatmap_factors."""
    from skelsplat_amd.heatmaps import heatmap_factors
    from skelsplat_amd.sparse import HeatmapFactors
    from skelsplat_amd._base import ViewBatch
    t = lambda k: torch.from_numpy(golden[k]).to(device)
    views = ViewBatch.from_cameras(cams, allow_mixed=True)
    f = HeatmapFactors(4, 17, views.W, views.H, device)
    p2d = golden["poses_2d"][..., :2].astype(np.float32) if p2d is None else p2d
    heatmap_factors(t("render_1_xyz"), torch.exp(t("render_1_scaling")), t("render_1_rotation"), torch.from_numpy(p2d).to(device),
                    cams, views=views, out=f, drop_mask=drop_mask)
    return f, views


def _planes_of(f, v, w, h):
    """View v's (J,h,w) planes as sks_heatmaps writes them from its factors."""
    from skelsplat_amd.heatmaps import heatmap_planes
    return heatmap_planes(f.row[v:v + 1, :, :h].contiguous(), f.col[v:v + 1, :, :w].contiguous(), f.cmin[v:v + 1].contiguous(),
                          f.den[v:v + 1].contiguous())


def _assert_factor_path(f, views):
    got, mm = preview.heatmap_preview(f, views, return_minmax=True)
    assert tuple(got.shape) == (f.V, f.H, f.W) and got.dtype == torch.uint8
    for v, (w, h) in enumerate(views.sizes):
        planes = _planes_of(f, v, w, h)
        want, want_mm = preview.channel_sum_u8(planes, return_minmax=True)
        assert torch.equal(got[v, :h, :w], want[0]), v
        assert torch.equal(mm[v], want_mm[0]), v
        # ... which is the restatement of the factors' own float32 expression
        host = pr.heatmap_planes(*(a[v].cpu().numpy() for a in (f.row, f.col, f.cmin, f.den)), w=w, h=h)
        assert np.array_equal(planes[0].cpu().numpy(), host)
        assert np.array_equal(want[0].cpu().numpy(), pr.preview(host)[0])
        pad = got[v].clone()
        pad[:h, :w] = 0
        assert not pad.any(), v             # outside the view's own size: written 0
        assert torch.isfinite(mm[v]).all() and int(got[v].amax()) == 255, (v, mm[v])      # a picture, not the all-zero fall-back
    return got


def test_factor_path_equals_the_plane_path_and_the_reference(device, golden):
    """A 4-view scene: bit for bit the plane path over sks_heatmaps' planes, and the reference's heatmap_{i}.png."""
    f, views = _factors(golden, device, _cameras(golden, device))
    got = _assert_factor_path(f, views)
    assert np.array_equal(got.cpu().numpy(), golden["heatmap_png"])


def test_factor_path_with_a_dropped_plane_and_a_detection_outside(device, golden):
    drop = torch.zeros((4, 17), dtype=torch.bool)
    drop[1, 3] = drop[2, 0] = drop[2, 16] = True
    f, views = _factors(golden, device, _cameras(golden, device), drop_mask=drop)
    assert not f.row[1, 3].any() and float(f.den[1, 3]) == 1.0
    dropped = _assert_factor_path(f, views)
    full = _assert_factor_path(*_factors(golden, device, _cameras(golden, device)))
    assert not torch.equal(dropped[1], full[1]) and torch.equal(dropped[0], full[0])
    p2d = golden["poses_2d"][..., :2].astype(np.float32).copy()
    p2d[0, 5] = (-40.0, 20.0)            # left of the image
    p2d[3, 9] = (30.0, 48.0 + 25.0)      # below it
    p2d[2, 1] = (63.9, 0.2)              # on the border: a truncated response
    f, views = _factors(golden, device, _cameras(golden, device), p2d=p2d)
    _assert_factor_path(f, views)


def test_factor_path_with_per_view_sizes(device, golden):
    """66 x 48 beside 64 x 48 (H36M's sensor mix in small; widths only -- heights differ in the next test): strides of the largest
    view, min / max over a view's own pixels, zeros behind a narrower view's rows; 64 x 48 alone takes 16-byte stores, the 66-wide
    slab bytes."""
    cams = _cameras(golden, device, widths=[66, 64, 64, 66])
    f, views = _factors(golden, device, cams)
    assert views.mixed and (views.W, views.H) == (66, 48) and list(views.wh) == [66, 48, 64, 48, 64, 48, 66, 48]
    got = _assert_factor_path(f, views)
    assert got[1, :, 64:].eq(0).all() and got[2, :, 64:].eq(0).all()
    # without the sizes every view is taken as 66 wide: the pictures of the narrow views change (their columns 64, 65 count)
    f.col[1, :, 64:] = 1.0
    assert not torch.equal(preview.heatmap_preview(f)[1], got[1]) and torch.equal(preview.heatmap_preview(f, views)[1], got[1])
    with pytest.raises(ValueError, match="the views are 4 of 66 x 48, the factors 4 of 64 x 48"):
        preview.heatmap_preview(_factors(golden, device, _cameras(golden, device))[0], views)


@pytest.mark.parametrize("sizes", [[(64, 48), (64, 40), (64, 47), (60, 33)], [(32, 300), (32, 290), (32, 257), (24, 300)],
                                   [(32, 1002), (32, 1000), (32, 1002), (32, 999)]],
                         ids=["48-rows-bands-of-1", "300-rows-bands-of-2", "1002-rows-bands-of-4"])
def test_factor_path_with_per_view_heights(device, golden, sizes):
    """Views SHORTER than the stride H: pass A's row bands that lie wholly below a view see no pixel and hand pass B the identity
    {+inf, -inf}, which must leave the view's {lo, hi} alone; a band may also end inside the view's last rows; pass B writes 0
    below the view.  Bands of one row (H = 48: 64 x 40 leaves bands 40 .. 47 empty), of two (H = 300: 290 rows leave five empty,
    257 rows end in the middle of band 128) and of four (H = 1002 beside 1000 and 999: H36M's other axis).  Held to
    channel_sum_u8 over sks_heatmaps' planes of each view at its own size: picture, {lo, hi} and the zero padding."""
    H = max(h for _, h in sizes)
    band = -(-H // 256)
    assert band == {48: 1, 300: 2, 1002: 4}[H]
    assert any(-(-h // band) < -(-H // band) for _, h in sizes)        # some view leaves whole bands empty
    cams = _cameras(golden, device, sizes=sizes)
    f, views = _factors(golden, device, cams, p2d=_detections(golden, sizes))
    assert views.mixed and (views.W, views.H) == (max(w for w, _ in sizes), H) and views.sizes == sizes
    got = _assert_factor_path(f, views)
    for v, (w, h) in enumerate(sizes):
        assert not got[v, h:].any() and not got[v, :, w:].any()


def test_python_refusals_on_device_tensors(device, golden):
    """The dtype / shape / contiguity refusals behind the device check, on real device tensors."""
    x = torch.zeros((2, 17, 4, 6), device=device)
    with pytest.raises(ValueError, match="channel_sum_u8: `images` must be float32, got torch.float64"):
        preview.channel_sum_u8(x.double())
    for bad in (x[0, 0], x[None], x[:, :0]):
        with pytest.raises(ValueError, match=r"channel_sum_u8: `images` must be \(V,C,H,W\) or \(C,H,W\) and not empty"):
            preview.channel_sum_u8(bad)
    with pytest.raises(ValueError, match="channel_sum_u8: `images` must be contiguous"):
        preview.channel_sum_u8(x[:, :, :, ::2])
    with pytest.raises(ValueError, match=r"render_preview: `xyz` must be \(P,3\)"):
        preview.render_preview([], torch.zeros((2, 17, 3), device=device), None, None, None, None)
    f, views = _factors(golden, device, _cameras(golden, device))
    want = preview.heatmap_preview(f)
    for name, bad, text in (("row", f.row.double(), "`factors.row` must be float32, got torch.float64"),
                            ("col", f.col[:, :, ::2], r"`factors.col` must be a contiguous \(4, 17, 64\) tensor, got \(4, 17, 32\)"),
                            ("col", f.col.transpose(0, 1).contiguous().transpose(0, 1), r"`factors.col` must be a contiguous \(4, 17, 64\) tensor"),
                            ("cmin", f.cmin[:3], r"`factors.cmin` must be a contiguous \(4, 17\) tensor, got \(3, 17\)"),
                            ("den", f.den.cpu(), "`factors.den` must be a tensor on a ROCm device"),
                            ("row", f.row[:, :, :40], r"`factors.row` must be a contiguous \(4, 17, 48\) tensor")):
        g = copy.copy(f)
        setattr(g, name, bad)
        with pytest.raises(ValueError, match="heatmap_preview: " + text):
            preview.heatmap_preview(g)
    assert torch.equal(preview.heatmap_preview(f), want)


# ----------------------------------------------------------------------------------------------------------------------------
# renders
# ----------------------------------------------------------------------------------------------------------------------------
def _render_args(golden, device, name):
    t = lambda k: torch.from_numpy(golden[f"{name}_{k}"]).to(device)
    return (t("xyz"), torch.exp(t("scaling")), torch.nn.functional.normalize(t("rotation")), torch.sigmoid(t("opacity")),
            torch.from_numpy(golden["features"]).to(device))


@pytest.mark.parametrize("name", ["render_1", "render"])
def test_render_preview_equals_the_references_pictures(device, golden, name):
    """save_images' pictures from the parameters the reference held when it wrote them."""
    cams = _cameras(golden, device)
    got, mm = preview.render_preview(cams, *_render_args(golden, device, name), antialiasing=bool(golden["antialiasing"]),
                                     return_minmax=True)
    want = golden[name + "_png"]
    diff = int((got.cpu().numpy() != want).sum())
    print(f"{name}: {diff} of {want.size} bytes differ from the reference's file")
    assert diff == 0
    assert np.array_equal(mm.cpu().numpy(), pr.preview_views(golden[name + "_planes"])[1])


def test_render_preview_by_size_group(device, golden):
    """Views of two sizes: each size group rendered on its own, a narrower view in the leading part of its slab."""
    from skelsplat_amd._base import ViewBatch
    cams = _cameras(golden, device, widths=[66, 64, 64, 66])
    args = _render_args(golden, device, "render")
    got = preview.render_preview(cams, *args)
    assert tuple(got.shape) == (4, 48, 66)
    for ids in ([0, 3], [1, 2]):
        sub = preview.render_preview([cams[i] for i in ids], *args)
        w = sub.shape[2]
        for k, i in enumerate(ids):
            assert torch.equal(got[i, :, :w], sub[k]) and not got[i, :, w:].any()
    again = preview.render_preview(ViewBatch.from_cameras(cams, allow_mixed=True), *args)       # a ViewBatch is taken too
    assert torch.equal(again, got)


# ----------------------------------------------------------------------------------------------------------------------------
# loops
# ----------------------------------------------------------------------------------------------------------------------------
ITERS, ES_ITERS, ES_TOL = 24, 160, 3e-4         # tests/test_uncertainty_gpu.py's runs of tests/test_frames_es_gpu.py's scene
CHOSEN = [0, 3, 4]                              # frame 4 sits alone in the padded last batch of frames=2


def _alone(device, sc, model, pt, p2d_f, es, directory):
    """A MultiViewLoop running one frame alone (tests/test_frames_es_gpu.py's _reference) and the three pictures it saves."""
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.loop import FrameBatchLoop, MultiViewLoop, OptEarlyStopping
    one = FrameBatchLoop(model(device), sc.cameras, 1, dataset="h36m")
    one.new_scenes(pt[None], poses_2d=p2d_f[None])
    gm = model(device)
    stop = OptEarlyStopping(window_size=4, repeat_tolerance=ES_TOL) if es else "no_stopping"
    loop = MultiViewLoop(gm, sc.cameras, torch.zeros((4, 17, sc.H, sc.W), device=device), dataset="h36m", sparse=True,
                         early_stopping=stop)
    gm.reset_from_points(pt)
    for slots, vb, gt, stats, idx in loop.size_groups:
        generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(), torch.tensor(p2d_f[slots], device=device),
                          [sc.cameras[k] for k in slots], out=gt, views=vb, totals=stats.totals)
    loop.stats_all.totals.copy_(one.stats_all.totals)
    hm = loop.save_heatmaps(directory)
    first = loop.save_images(directory, name="render_1")
    loop.run(ES_ITERS if es else ITERS)
    last = loop.save_images(directory)
    return loop, (hm, first, last), gm._xyz.detach().clone()


@pytest.fixture(scope="module")
def sequence(device, tmp_path_factory):
    from tests.test_frames_es_gpu import _frames, _scene
    sc, model = _scene(device)
    pts, p2d = _frames(sc, 5)
    alone = {}
    for es in (False, True):
        for f in CHOSEN:
            d = str(tmp_path_factory.mktemp(f"alone_{int(es)}_{f}"))
            alone[es, f] = _alone(device, sc, model, pts[f], p2d[f], es, d) + (d,)
    return sc, model, pts, p2d, alone


def test_multi_view_loop_saves_the_references_files(device, sequence):
    """heatmaps/heatmap_{i}.png, images/render_1_{i}.png, images/render_{i}.png decode to the arrays the functions return; the
    heat-map picture is the plane path's, the renders are render_preview of the loop's parameters."""
    sc, model, pts, p2d, alone = sequence
    loop, (hm, first, last), xyz, d = alone[False, 3]
    for sub, name, pics in (("heatmaps", "heatmap", hm), ("images", "render_1", first), ("images", "render", last)):
        assert tuple(pics.shape) == (4, sc.H, sc.W) and pics.dtype == torch.uint8 and pics.is_cuda
        for i in range(4):
            assert np.array_equal(io.read_png_gray(os.path.join(d, sub, f"{name}_{i}.png")), pics[i].cpu().numpy())
    assert sorted(os.listdir(os.path.join(d, "images"))) == sorted([f"render_{i}.png" for i in range(4)] + [f"render_1_{i}.png" for i in range(4)])
    assert torch.equal(hm, preview.channel_sum_u8(loop.gt)) and np.array_equal(hm.cpu().numpy(), pr.preview_views(loop.gt.cpu().numpy())[0])
    gm = loop.gm
    want = preview.render_preview(sc.cameras, gm._xyz.detach(), gm.get_scaling.detach(), gm.get_rotation.detach(),
                                  gm.get_opacity.detach(), gm.get_features.detach().reshape(17, -1))
    assert torch.equal(last, want) and not torch.equal(first, last) and last.amax() == 255


@pytest.mark.parametrize("es", [False, True], ids=["no-stopping", "early-stopping"])
def test_frame_pipeline_pictures_the_chosen_frames(device, sequence, es, tmp_path):
    """5 frames, frames=2, streams=2: `images` holds what a MultiViewLoop running each chosen frame alone pictures; the joints are
    bit for bit those of a run with the pictures off; after set_debug_images(None) a sequence leaves `images` None."""
    from skelsplat_amd.loop import FramePipeline, OptEarlyStopping
    sc, model, pts, p2d, alone = sequence
    stop = (lambda: OptEarlyStopping(window_size=4, repeat_tolerance=ES_TOL)) if es else (lambda: "no_stopping")
    iters = ES_ITERS if es else ITERS
    run = lambda p: p.optimize_sequence(pts, p2d, iterations=iters, groups_per_graph=2, interleave=8)
    off = FramePipeline(model(device), sc.cameras, frames=2, streams=2, dataset="h36m", early_stopping=stop())
    want = run(off).clone()
    assert off.images is None and all(fb.images is None for fb in off.loops)
    pipe = FramePipeline(model(device), sc.cameras, frames=2, streams=2, dataset="h36m", early_stopping=stop())
    assert pipe.set_debug_images([4, 0, 3]) is pipe
    out = run(pipe)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    im = pipe.images
    assert isinstance(im, preview.SequenceImages) and im.frames == CHOSEN
    if es:
        stops = [int(s) for s in pipe.stopped_at.tolist()]
        assert any(s for s in stops) and any(s == 0 for s in stops), stops       # frames did stop, at their own iterations
    for k, f in enumerate(CHOSEN):
        loop, (hm, first, last), xyz, _ = alone[es, f]
        assert torch.equal(out[f], xyz), f
        assert torch.equal(im.heatmaps[k], hm), f
        assert torch.equal(im.render_first[k], first), f
        assert torch.equal(im.render_last[k], last), f
        assert im.heatmaps[k].amax() == 255 and not torch.equal(first, last)
    assert torch.isfinite(im.minmax).all() and (im.minmax[..., 0] == 0).all()
    dirs = im.save(str(tmp_path))
    assert [os.path.basename(d) for d in dirs] == ["frame_000000", "frame_000003", "frame_000004"]
    for k, d in enumerate(dirs):
        for sub, name, pics in (("heatmaps", "heatmap", im.heatmaps), ("images", "render_1", im.render_first),
                                ("images", "render", im.render_last)):
            for i in range(4):
                assert np.array_equal(io.read_png_gray(os.path.join(d, sub, f"{name}_{i}.png")), pics[k, i].cpu().numpy())
    # the same pipeline, pictures off again: the same joints from the graphs it captured, and nothing pictured
    assert pipe.set_debug_images(None) is pipe
    again = run(pipe)
    torch.cuda.synchronize()
    assert pipe.images is None and torch.equal(again, want)


def test_frame_batch_loop_pictures_planes_too(device, sequence):
    """FrameBatchLoop(factored=False) holds planes: the heat-map pictures come from the plane path and equal the factored loop's."""
    from skelsplat_amd.loop import FrameBatchLoop
    sc, model, pts, p2d, alone = sequence
    pics = {}
    for factored in (True, False):
        fb = FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m", factored=factored).set_debug_images([1, 2])
        fb.optimize_sequence(pts[:4], p2d[:4], iterations=8, groups_per_graph=1)
        pics[factored] = fb.images
    torch.cuda.synchronize()
    a, b = pics[True], pics[False]
    assert a.frames == b.frames == [1, 2]
    assert torch.equal(a.heatmaps, b.heatmaps) and torch.equal(a.render_first, b.render_first) and torch.equal(a.render_last, b.render_last)
    assert torch.equal(a.minmax, b.minmax)
    with pytest.raises(ValueError, match=r"frames \[7\] must be indices into the sequence's 4 frames"):
        FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m").set_debug_images([7]).optimize_sequence(pts[:4], p2d[:4], iterations=4)
