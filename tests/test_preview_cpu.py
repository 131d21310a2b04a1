"""The debug pictures (skelsplat_amd/preview.py, csrc/sks_preview.hip) without a device: the numpy restatement of the fixed
sequence (tests/preview_ref.py), which the GPU tests hold the kernels to bit for bit, reproduces every picture the reference's own
save_heatmaps / save_images wrote (tests/golden/reference_images.npz) exactly; the ABI tables are the header's prototypes; the C
entry points and the Python surface refuse what they must; the host-only launch answers are the ones the GPU tests' shapes were
chosen for; and the PNG writer round-trips."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, io, loop, preview
from tests import preview_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_images.npz")
PICTURES = ("heatmap", "render_1", "render")
# W, H -> (load bytes, store bytes, workgroups of pass A, of pass B) with aligned bases: the plane-path shapes of
# tests/test_preview_gpu.py (a unit of pass A is a float4 / a pixel, of pass B 16 pixels / a pixel; 256 units per workgroup)
LAUNCHES = {(1, 1): (4, 1, 1, 1), (3, 5): (4, 1, 1, 1), (16, 4): (16, 16, 1, 1), (20, 3): (16, 1, 1, 1), (18, 7): (4, 1, 1, 1),
            (64, 48): (16, 16, 3, 1), (257, 1): (4, 1, 2, 2), (4, 257): (16, 1, 2, 5), (3, 171): (4, 1, 3, 3),
            (1024, 17): (16, 16, 17, 5), (1000, 1000): (16, 1, 256, 256), (1920, 1080): (16, 16, 256, 256)}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_restatement_equals_the_reference_pictures(golden):
    """Every byte of every picture train.training() wrote with debug.save_images=True, from the tensor it was made of."""
    for name in PICTURES:
        planes, png = golden[name + "_planes"], golden[name + "_png"]
        assert planes.shape == (4, 17, 48, 64) and png.shape == (4, 48, 64) and png.dtype == np.uint8
        q, mm = pr.preview_views(planes)
        assert np.array_equal(q, png), (name, int((q != png).sum()))
        assert (png.reshape(4, -1).max(axis=1) == 255).all() and (png.reshape(4, -1).min(axis=1) == 0).all()
        assert np.array_equal(mm[:, 0], planes.sum(axis=1).reshape(4, -1).min(axis=1))
    # the two renders are different pictures: the optimiser stepped in between
    assert not np.array_equal(golden["render_1_png"], golden["render_png"])


def test_restatement_equals_the_reference_on_hand_made_tensors(golden):
    names = list(golden["hand_names"])
    assert names == ["blobs15", "dense19", "negative17", "ramp17", "single1"]
    for name in names:
        planes, png = golden[f"hand_{name}_planes"], golden[f"hand_{name}_png"]
        q, mm = pr.preview(planes)
        assert np.array_equal(q, png), (name, int((q != png).sum()))
    assert [golden[f"hand_{n}_planes"].shape[0] for n in names] == [15, 19, 17, 17, 1]
    # the ramp sums to 0 .. 255 exactly, and with a correctly rounded divide the reference's picture of it is the ramp itself:
    # (k / 255) * 255 >= k for every k, by at most a few ulp.  A quotient one ulp low would truncate to k - 1.
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal(pr.channel_sum(golden["hand_ramp17_planes"]).reshape(-1), k)
    assert np.array_equal(golden["hand_ramp17_png"].reshape(-1), np.arange(256))
    low = np.nextafter((k / np.float32(255)).astype(np.float32), np.float32(0)) * np.float32(255)
    assert (np.trunc(low) != k).sum() >= 16
    assert (golden["hand_negative17_planes"] < 0).mean() > 0.9


def test_restatement_is_the_documented_sequence():
    rng = np.random.default_rng(3)
    p = rng.normal(0, 1, (19, 6, 7)).astype(np.float32)
    s = p[0]
    for c in range(1, 19):
        s = np.float32(1) * (s + p[c])
    assert np.array_equal(pr.channel_sum(p), s)
    q, mm = pr.preview(p)
    assert mm[0] == s.min() and mm[1] == s.max() and q.min() == 0 and q.max() == 255
    # the undefined cases: all-zero pictures, lo / hi reported as they are
    flat = np.full((3, 4, 5), 0.25, dtype=np.float32)
    q, mm = pr.preview(flat)
    assert not q.any() and mm[0] == mm[1] == np.float32(0.75)
    for bad in (np.nan, np.inf, -np.inf):
        x = p.copy()
        x[4, 2, 3] = bad
        q, mm = pr.preview(x)
        assert not q.any(), bad
        assert np.isnan(mm).all() if np.isnan(bad) else (np.isinf(mm).sum() == 1 and bad in mm)
    # factors -> planes: the float32 expression of the header
    row, col = rng.uniform(0, 1, (17, 5)).astype(np.float32), rng.uniform(0, 1, (17, 9)).astype(np.float32)
    cmin, den = (row.min(axis=1) * col.min(axis=1)).astype(np.float32), rng.uniform(0.5, 2, 17).astype(np.float32)
    planes = pr.heatmap_planes(row, col, cmin, den, w=8, h=5)
    assert planes.shape == (17, 5, 8) and planes.dtype == np.float32 and (planes >= 0).all()
    assert planes[3, 2, 6] == (np.float32(row[3, 2] * col[3, 6]) - cmin[3]) / den[3]


def test_abi_tables_and_build():
    hdr = open(os.path.join(ROOT, "include", "skelsplat_hip.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert "csrc/sks_preview.hip; added to sks_version 14: the number did not move" in flat
    assert "every pixel whose t is NaN or outside [0, 255] is 0 by definition" in flat
    for i, name in enumerate(("SKS_PREVIEW_LOAD_BYTES", "SKS_PREVIEW_STORE_BYTES", "SKS_PREVIEW_GROUPS_SUM", "SKS_PREVIEW_GROUPS_PACK")):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == i
        assert _lib.PREVIEW_LAUNCH_FIELDS[i] == name[len("SKS_PREVIEW_"):].lower()
    assert int(re.search(r"#define\s+SKS_PREVIEW_LAUNCH_INTS\s+(\d+)", hdr).group(1)) == _lib.SKS_PREVIEW_LAUNCH_INTS == 4
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for symbol, restype in (("sks_preview_planes", "int"), ("sks_preview_factors", "int"), ("sks_preview_scratch_bytes", "size_t"),
                            ("sks_preview_launch", "int")):
        proto = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (restype, symbol), plain).group(1)
        kinds = []
        for param in proto.split(","):
            ctype, _ = re.fullmatch(r"\s*(.*?)(\w+)\s*", param, flags=re.S).groups()
            kinds.append(ctypes.c_void_p if "*" in ctype else scalars[ctype.strip()])
        assert _lib.SIGNATURES[symbol] == (scalars[restype], kinds), symbol
    from skelsplat_amd import build
    assert "sks_preview.hip" in build.SOURCES
    assert _lib.load().sks_version() == 14


def test_scratch_bytes_and_launch_forms():
    """Host only.  The launch forms are the regimes the GPU tests' shapes were chosen for."""
    lib = _lib.load()
    for (W, H), (ld, st, ga, gb) in LAUNCHES.items():
        got = _lib.preview_launch(W, H)
        assert got == dict(load_bytes=ld, store_bytes=st, groups_sum=ga, groups_pack=gb), (W, H, got)
        un = _lib.preview_launch(W, H, aligned=False)       # an unaligned base: scalar loads and byte stores, always
        n = W * H
        assert un == dict(load_bytes=4, store_bytes=1, groups_sum=min(256, -(-n // 256)), groups_pack=min(256, -(-n // 256)))
        for V in (1, 3, 4):
            assert lib.sks_preview_scratch_bytes(V, W, H) == (V * n * 4 + 15) // 16 * 16 + V * 256 * 2 * 4, (V, W, H)
    # 257 pixels are the fewest that take two workgroups; 4 x 257 the fewest with 16-byte loads
    assert _lib.preview_launch(256, 1)["groups_sum"] == 1 and _lib.preview_launch(4, 256)["groups_sum"] == 1
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 65536, 65536)):
        assert lib.sks_preview_scratch_bytes(*bad) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="a refusal that went missing would launch on made-up pointers")
def test_c_refusals():
    """Each refusal happens before any HIP call, with its exact text; every pointer is a placeholder nothing dereferences."""
    lib = _lib.load()
    x = 0x10000

    def refused(fn, args, code, text):
        assert fn(*args) == code, (fn.__name__, args)
        assert lib.sks_last_error().decode() == text

    ok = dict(V=4, C=17, W=64, H=48, planes=x, scratch=x, minmax=None, out=x, stream=None)
    call = lambda **change: tuple({**ok, **change}.values())
    pl = lib.sks_preview_planes
    for bad in (dict(V=0), dict(C=0), dict(W=-1), dict(H=0)):
        a = {**ok, **bad}
        refused(pl, call(**bad), -1,
                f"preview_planes: V = {a['V']}, C = {a['C']}, W = {a['W']}, H = {a['H']}; all must be at least 1")
    refused(pl, call(W=65536, H=32768), -1, "preview_planes: W x H = 65536 x 32768 pixels do not fit an int")
    big = 0x7fffffff
    refused(pl, call(V=big, C=big, W=46340, H=46340), -1,
            f"preview_planes: V x C x H x W = {big} x {big} x 46340 x 46340 floats do not fit a size_t")
    refused(pl, call(V=65536), -1, "preview_planes: V = 65536 views, at most 65535 per call")
    refused(pl, call(C=33), -1, "preview_planes: C = 33 channels, at most 32 (SKS_MAX_CHANNELS)")
    refused(pl, call(planes=None), -2, "preview_planes: missing planes")
    refused(pl, call(scratch=None), -2, "preview_planes: missing scratch (sks_preview_scratch_bytes)")
    refused(pl, call(out=None), -2, "preview_planes: missing out")
    refused(pl, call(scratch=x + 4), -2, "preview_planes: scratch must be 16-byte aligned")

    ok = dict(V=4, J=17, W=66, H=48, row=x, col=x, cmin=x, den=x, view_wh=None, scratch=x, minmax=None, out=x, stream=None)
    fa = lib.sks_preview_factors
    for bad in (dict(V=0), dict(J=-3), dict(W=0), dict(H=0)):
        a = {**ok, **bad}
        refused(fa, call(**bad), -1,
                f"preview_factors: V = {a['V']}, J = {a['J']}, W = {a['W']}, H = {a['H']}; all must be at least 1")
    refused(fa, call(W=65536, H=32768), -1, "preview_factors: W x H = 65536 x 32768 pixels do not fit an int")
    refused(fa, call(V=big, J=big, W=46340, H=46340), -1,
            f"preview_factors: V x J x H x W = {big} x {big} x 46340 x 46340 floats do not fit a size_t")
    refused(fa, call(V=65), -1, "preview_factors: V = 65 views, at most 64 (SKS_MAX_VIEWS)")
    for missing in ("row", "col", "cmin", "den"):
        refused(fa, call(**{missing: None}), -2, "preview_factors: missing factors (row, col, cmin, den)")
    refused(fa, call(scratch=None), -2, "preview_factors: missing scratch (sks_preview_scratch_bytes)")
    refused(fa, call(out=None), -2, "preview_factors: missing out")
    refused(fa, call(scratch=x + 8), -2, "preview_factors: scratch must be 16-byte aligned")
    wh = lambda *v: ctypes.cast((ctypes.c_int * 8)(*v), ctypes.c_void_p)
    refused(fa, call(view_wh=wh(66, 48, 64, 48, 67, 48, 64, 48)), -1,
            "preview_factors: view 2 is 67 x 48; every view's size must be within [1, 66] x [1, 48]")
    refused(fa, call(view_wh=wh(66, 48, 64, 49, 64, 48, 64, 48)), -1,
            "preview_factors: view 1 is 64 x 49; every view's size must be within [1, 66] x [1, 48]")
    refused(fa, call(view_wh=wh(66, 48, 64, 48, 64, 48, 0, 48)), -1,
            "preview_factors: view 3 is 0 x 48; every view's size must be within [1, 66] x [1, 48]")

    out = (ctypes.c_int * 4)()
    la = lib.sks_preview_launch
    refused(la, (64, 48, 1, None), -2, "preview_launch: missing out (SKS_PREVIEW_LAUNCH_INTS ints)")
    refused(la, (0, 48, 1, ctypes.cast(out, ctypes.c_void_p)), -1, "preview_launch: W = 0, H = 48; both must be at least 1")
    refused(la, (65536, 32768, 1, ctypes.cast(out, ctypes.c_void_p)), -1,
            "preview_launch: W x H = 65536 x 32768 pixels do not fit an int")


def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    for shape in ((1, 1), (48, 64), (7, 35), (250, 3)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / "sub" / f"p_{shape[0]}_{shape[1]}.png")
        io.write_png_gray(path, a)
        assert np.array_equal(io.read_png_gray(path), a)
    io.write_png_gray(str(tmp_path / "t.png"), torch.as_tensor(a))      # a host tensor is taken too
    assert np.array_equal(io.read_png_gray(str(tmp_path / "t.png")), a)
    for bad in (a.astype(np.int32), a[None], np.zeros((0, 4), dtype=np.uint8)):
        with pytest.raises(ValueError, match=r"write_png_gray: an \(H,W\) uint8 array"):
            io.write_png_gray(str(tmp_path / "bad.png"), bad)
    (tmp_path / "not.png").write_bytes(b"P5 1 1 255 \x00")
    with pytest.raises(ValueError, match="is not a PNG file"):
        io.read_png_gray(str(tmp_path / "not.png"))


def test_written_png_is_what_pil_reads(tmp_path, golden):
    Image = pytest.importorskip("PIL.Image")
    for k, a in enumerate((golden["heatmap_png"][0], golden["hand_ramp17_png"], np.arange(15, dtype=np.uint8).reshape(5, 3))):
        path = str(tmp_path / f"{k}.png")
        io.write_png_gray(path, a)
        im = Image.open(path)
        assert im.mode == "L" and im.size == (a.shape[1], a.shape[0]) and np.array_equal(np.asarray(im), a)


def test_save_previews_writes_the_reference_layout(tmp_path, golden):
    pics = golden["render_png"]
    paths = preview.save_previews(str(tmp_path / "images"), "render_1", pics)
    assert [os.path.relpath(p, tmp_path) for p in paths] == [os.path.join("images", f"render_1_{i}.png") for i in range(4)]
    for p, a in zip(paths, pics):
        assert np.array_equal(io.read_png_gray(p), a)
    paths = preview.save_previews(str(tmp_path / "m"), "heatmap", pics, sizes=[(64, 48), (60, 48), (64, 40), (1, 1)])
    assert [io.read_png_gray(p).shape for p in paths] == [(48, 64), (48, 60), (40, 64), (1, 1)]
    assert np.array_equal(io.read_png_gray(paths[1]), pics[1][:, :60])
    with pytest.raises(ValueError, match="save_previews"):
        preview.save_previews(str(tmp_path), "x", pics.astype(np.float32))


def test_python_refusals():
    """What is refused without a device; the dtype / shape / contiguity refusals behind the device check run on device tensors in
    tests/test_preview_gpu.py."""
    x = torch.zeros((2, 17, 4, 6))
    with pytest.raises(ValueError, match="channel_sum_u8: `images` must be a tensor on a ROCm device"):
        preview.channel_sum_u8(x)
    with pytest.raises(ValueError, match="channel_sum_u8: `images` must be a tensor on a ROCm device"):
        preview.channel_sum_u8(x.numpy())
    with pytest.raises(ValueError, match="render_preview: `xyz` must be a tensor on a ROCm device"):
        preview.render_preview([], torch.zeros((17, 3)), None, None, None, None)
    with pytest.raises(ValueError, match="heatmap_preview: `factors` must be a HeatmapFactors, got Tensor"):
        preview.heatmap_preview(x)
    f = types.SimpleNamespace(row=x, col=x, cmin=x, den=x, V=4, J=17, W=64, H=48)
    with pytest.raises(ValueError, match="heatmap_preview: `factors.row` must be a tensor on a ROCm device"):
        preview.heatmap_preview(f)
    with pytest.raises(ValueError, match="heatmap_preview: the factors are 0 views of 17 joints at 64 x 48; all must be at least 1"):
        preview.heatmap_preview(types.SimpleNamespace(row=x, col=x, cmin=x, den=x, V=0, J=17, W=64, H=48))


def test_sequence_images_frames_are_checked():
    with pytest.raises(ValueError, match=r"set_debug_images: frames \[5\] must be indices into the sequence's 5 frames"):
        preview.SequenceImages([5], 5, 4, 8, 8, "cpu")
    im = preview.SequenceImages([3, 0, 3], 5, 4, 8, 6, "cpu")
    assert im.frames == [0, 3] and im.heatmaps.shape == im.render_first.shape == im.render_last.shape == (2, 4, 6, 8)
    assert im.heatmaps.dtype == torch.uint8 and im.minmax.shape == (3, 2, 4, 2) and torch.isnan(im.minmax).all()
    assert im.chosen(0, 2) == [(0, 0)] and im.chosen(2, 2) == [(1, 1)] and im.chosen(4, 1) == []
    with pytest.raises(ValueError, match="3 scene names for 2 pictured frames"):
        im.save("unused", ["a", "b", "c"])


def test_loops_have_the_setter_and_keep_their_signatures():
    """The debug pictures are switched by a setter: the keyword lists tests/test_fuse_cpu.py pins end where they did."""
    for cls in (loop.FrameBatchLoop, loop.FramePipeline):
        assert list(inspect.signature(cls.set_debug_images).parameters) == ["self", "frames"]
        assert list(inspect.signature(cls.optimize_sequence).parameters)[-1] == "poses_3d"
    assert list(inspect.signature(loop.FrameBatchLoop.new_scenes).parameters) == \
        ["self", "points", "poses_2d", "heatmaps", "drop_masks", "rig_ids", "poses_3d"]
    assert list(inspect.signature(loop.MultiViewLoop.new_scene).parameters)[-1] == "poses_3d"
    assert list(inspect.signature(loop.MultiViewLoop.save_heatmaps).parameters) == ["self", "output_dir", "name"]
    assert list(inspect.signature(loop.MultiViewLoop.save_images).parameters) == ["self", "output_dir", "name"]
    assert inspect.signature(loop.MultiViewLoop.save_heatmaps).parameters["name"].default == "heatmap"
    assert inspect.signature(loop.MultiViewLoop.save_images).parameters["name"].default == "render"
    plain = types.SimpleNamespace(rigs=None)
    assert loop._debug_frames(plain, None) is None and loop._debug_frames(plain, [4, 0]) == (4, 0)
    for bad in ([], [-1], [0, -2]):
        with pytest.raises(ValueError, match="set_debug_images: frames"):
            loop._debug_frames(plain, bad)
    with pytest.raises(ValueError, match="set_debug_images: .* a rig bank"):
        loop._debug_frames(types.SimpleNamespace(rigs=object()), [0])
