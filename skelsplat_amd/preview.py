"""The reference's debug pictures on the device (csrc/sks_preview.hip): train.py:279-304 sums a view's channels, min-max
normalises and writes an 8-bit grey PNG -- of the pseudo-GT heat-maps (save_heatmaps), of the render after iteration 1 and of the
render at the end (save_images; configs/*.yaml `debug.save_images`).

channel_sum_u8    (V,C,H,W) float32 planes -> (V,H,W) uint8 pictures: two launches, the planes are read once;
heatmap_preview   the same picture of a sparse.HeatmapFactors, straight from the separable factors: no plane is ever written;
render_preview    save_images' render -- a dense forward of the given Gaussians over a black background, clamped to [0, 1] --
                  pictured; the planes are transient;
save_previews     (V,H,W) pictures -> {dir}/{name}_{i}.png, the reference's file names;
SequenceImages    what a FrameBatchLoop / FramePipeline pictures of the chosen frames of a sequence (set_debug_images).

Everything takes device tensors, enqueues on the current stream and never synchronises; every byte is reproducible.  The fixed
float32 sequence, and what a flat view or one with a NaN or inf gives (an all-zero picture: the reference is undefined there), are
in include/skelsplat_hip.h and DESIGN.md.  The files are written by io.write_png_gray; nothing here needs PIL."""
import os

import torch

from . import _lib


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _scratch(V, W, H, dev, what):
    n = _lib.load().sks_preview_scratch_bytes(V, W, H)
    if n == 0:
        raise ValueError(f"{what}: {V} views of {W} x {H} pixels are more than one call takes")
    return torch.empty(n, dtype=torch.uint8, device=dev)


def channel_sum_u8(images, return_minmax=False):
    """images (V,C,H,W) or (C,H,W) float32 on the device -> (V,H,W) / (H,W) uint8: per view the channels summed in ascending
    order, min-max normalised over the view and truncated to 8 bits (train.py:287-289).  `return_minmax=True`: also the (V,2) /
    (2,) float32 {min, max} of each view's sum.  A flat view and one that holds a NaN or an inf give an all-zero picture.  Runs on
    the current stream, never synchronises."""
    what = "channel_sum_u8"
    if not torch.is_tensor(images) or not images.is_cuda:
        raise ValueError(f"{what}: `images` must be a tensor on a ROCm device")
    if images.dtype != torch.float32:
        raise ValueError(f"{what}: `images` must be float32, got {images.dtype}")
    if images.dim() not in (3, 4) or images.numel() == 0:
        raise ValueError(f"{what}: `images` must be (V,C,H,W) or (C,H,W) and not empty, got {tuple(images.shape)}")
    single = images.dim() == 3
    x = images[None] if single else images
    if not x.is_contiguous():
        raise ValueError(f"{what}: `images` must be contiguous (strides {tuple(images.stride())} of shape {tuple(images.shape)})")
    V, C, H, W = x.shape
    if C > _lib.SKS_MAX_CHANNELS:
        raise ValueError(f"{what}: {C} channels, at most {_lib.SKS_MAX_CHANNELS} (SKS_MAX_CHANNELS)")
    dev = x.device
    out = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    mm = torch.empty((V, 2), dtype=torch.float32, device=dev) if return_minmax else None
    with torch.cuda.device(dev):
        scratch = _scratch(V, W, H, dev, what)
        rc = _lib.load().sks_preview_planes(V, C, W, H, x.data_ptr(), scratch.data_ptr(), None if mm is None else mm.data_ptr(),
                                            out.data_ptr(), _stream(dev))
    _lib.check(rc, "sks_preview_planes")
    if single:
        out, mm = out[0], None if mm is None else mm[0]
    return (out, mm) if return_minmax else out


def heatmap_preview(factors, views=None, return_minmax=False):
    """A sparse.HeatmapFactors (V views, J joints, strides W x H of the largest view) -> (V,H,W) uint8: bit for bit
    channel_sum_u8 of the planes sks_heatmaps would write from these factors, without writing them.  `views`: the ViewBatch the
    factors were made for, when its views differ in size (the host sizes `views.wh`): a view's picture is its leading
    (H_v, W_v) part, the rest of its (H,W) slab is 0.  Runs on the current stream, never synchronises."""
    what = "heatmap_preview"
    f = factors
    if not all(hasattr(f, a) for a in ("row", "col", "cmin", "den", "V", "J", "W", "H")):
        raise ValueError(f"{what}: `factors` must be a HeatmapFactors, got {type(factors).__name__}")
    V, J, W, H = (int(x) for x in (f.V, f.J, f.W, f.H))
    if min(V, J, W, H) < 1:
        raise ValueError(f"{what}: the factors are {V} views of {J} joints at {W} x {H}; all must be at least 1")
    for name, shape in (("row", (V, J, H)), ("col", (V, J, W)), ("cmin", (V, J)), ("den", (V, J))):
        t = getattr(f, name)
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: `factors.{name}` must be a tensor on a ROCm device")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: `factors.{name}` must be float32, got {t.dtype}")
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{what}: `factors.{name}` must be a contiguous {shape} tensor, got {tuple(t.shape)} with strides "
                             f"{tuple(t.stride())}")
        if t.device != f.row.device:
            raise ValueError(f"{what}: `factors.{name}` is on {t.device}, `factors.row` on {f.row.device}")
    wh = None
    if views is not None:
        if (views.V, views.W, views.H) != (f.V, f.W, f.H):
            raise ValueError(f"{what}: the views are {views.V} of {views.W} x {views.H}, the factors {f.V} of {f.W} x {f.H}")
        wh = views.wh
    dev = f.row.device
    out = torch.empty((f.V, f.H, f.W), dtype=torch.uint8, device=dev)
    mm = torch.empty((f.V, 2), dtype=torch.float32, device=dev) if return_minmax else None
    with torch.cuda.device(dev):
        scratch = _scratch(f.V, f.W, f.H, dev, what)
        rc = _lib.load().sks_preview_factors(f.V, f.J, f.W, f.H, f.row.data_ptr(), f.col.data_ptr(), f.cmin.data_ptr(),
                                             f.den.data_ptr(), wh, scratch.data_ptr(), None if mm is None else mm.data_ptr(),
                                             out.data_ptr(), _stream(dev))
    _lib.check(rc, "sks_preview_factors")
    return (out, mm) if return_minmax else out


def render_preview(cameras_or_views, xyz, scaling, rotation, opacity, features, scaling_modifier=1.0, antialiasing=False,
                   return_minmax=False):
    """save_images' picture (train.py:279-291) of the Gaussians xyz (P,3), scaling (P,3) and opacity (P,1) ACTIVATED, rotation
    (P,4), features (P,C) -- what rasterizer.forward_views takes -- in a list of cameras or a ViewBatch: a dense forward over a
    BLACK background, clamped to [0, 1], through a Workspace of its own (no loop's recorded plans, prefill state or captured
    graphs are touched), then channel_sum_u8.  Views of different sizes are rendered size group by size group; the result is
    (V,H,W) uint8 with H, W the largest view, a smaller view in the leading part of its slab and 0 behind it."""
    from ._base import ViewBatch
    from . import rasterizer as R
    what = "render_preview"
    if not torch.is_tensor(xyz) or not xyz.is_cuda:
        raise ValueError(f"{what}: `xyz` must be a tensor on a ROCm device")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] == 0:
        raise ValueError(f"{what}: `xyz` must be (P,3) -- one frame's Gaussians --, got {tuple(xyz.shape)}")
    dev = xyz.device
    if isinstance(cameras_or_views, ViewBatch):
        vb = cameras_or_views
    else:
        vb = ViewBatch.from_cameras([c.to(dev) for c in cameras_or_views], allow_mixed=True)
    groups = {}
    for v, sz in enumerate(vb.sizes):
        groups.setdefault(sz, []).append(v)
    out = mm = None
    if len(groups) > 1:
        out = torch.zeros((vb.V, vb.H, vb.W), dtype=torch.uint8, device=dev)
        mm = torch.empty((vb.V, 2), dtype=torch.float32, device=dev)
    ws = R.Workspace(prefill=0)
    args = (xyz.detach(), features.detach().reshape(xyz.shape[0], -1), opacity.detach(), scaling.detach(), rotation.detach(), None)
    for (w, h), ids in groups.items():
        if len(groups) == 1:
            sub = vb
        else:
            idx = torch.tensor(ids, dtype=torch.long, device=dev)
            sub = ViewBatch(vb.viewmatrix[idx], vb.projmatrix[idx], [vb.tanfovx[v] for v in ids], [vb.tanfovy[v] for v in ids], w, h)
        color = R.forward_views(sub, *args, scale_modifier=scaling_modifier, antialiasing=antialiasing, clamp01=True,
                                workspace=ws)[0]
        q, m = channel_sum_u8(color, return_minmax=True)
        if out is None:
            out, mm = q, m
        else:
            out[idx, :h, :w] = q
            mm[idx] = m
    return (out, mm) if return_minmax else out


def save_previews(directory, name, pictures, sizes=None):
    """(V,H,W) uint8 pictures -> {directory}/{name}_{i}.png for view i (train.py:291, 304), 8-bit grey.  `sizes`: per-view
    (W_v, H_v) when the views differ in size: the leading part of each slab is written.  Reads the pictures back (one copy, which
    waits for the stream they were made on).  Returns the paths."""
    from .io import write_png_gray
    host = pictures.detach().cpu().numpy() if torch.is_tensor(pictures) else pictures
    if host.ndim != 3 or host.dtype.name != "uint8":
        raise ValueError(f"save_previews: (V,H,W) uint8 pictures are needed, got {host.dtype} {host.shape}")
    paths = []
    for i, pic in enumerate(host):
        if sizes is not None:
            pic = pic[:sizes[i][1], :sizes[i][0]]
        paths.append(os.path.join(directory, f"{name}_{i}.png"))
        write_png_gray(paths[-1], pic)
    return paths


class SequenceImages:
    """What `optimize_sequence` of a FrameBatchLoop / FramePipeline pictures after set_debug_images(frames): for the K chosen
    frames of the sequence `heatmaps`, `render_first` (the render of the initial Gaussians: train.py:143-144) and `render_last`
    (the render at the end, or at the frame's stopping iteration: train.py:236-237), each (K,V,H,W) uint8 on the device, and
    `minmax` (3,K,V,2) float32, the {min, max} each picture was normalised with, in that order.  `frames` holds the K sequence
    indices, ascending.  Each batch's pictures are enqueued on the batch's own stream; nothing is read back before save().
    What a batch with a chosen frame pays: one heat-map picture of ALL its F x V views (two launches; the chosen frames' slabs are
    copied out), and per chosen frame two dense forwards of its V views, each in a fresh Workspace (V x C x H x W floats, freed
    after the call) with its two picture launches.  A batch without a chosen frame enqueues nothing."""

    def __init__(self, frames, N, V, W, H, device, sizes=None):
        chosen = sorted({int(f) for f in frames})
        if not chosen or chosen[0] < 0 or chosen[-1] >= N:
            raise ValueError(f"set_debug_images: frames {list(frames)!r} must be indices into the sequence's {N} frames")
        self.frames, self.V, self.W, self.H, self.sizes = chosen, int(V), int(W), int(H), sizes
        self._slot = {f: k for k, f in enumerate(chosen)}
        K = len(chosen)
        new = lambda: torch.zeros((K, V, H, W), dtype=torch.uint8, device=device)
        self.heatmaps, self.render_first, self.render_last = new(), new(), new()
        self.minmax = torch.full((3, K, V, 2), float("nan"), dtype=torch.float32, device=device)

    def chosen(self, b, n):
        """[(slot k, row i of the batch)] of the chosen frames among frames b .. b + n of the sequence."""
        return [(self._slot[f], f - b) for f in range(b, b + n) if f in self._slot]

    def _render(self, loop, i):
        # (the activations of scene/gaussian_model.py:39-47, as MultiViewLoop's dense step applies them)
        return render_preview(loop.frame_views(i), loop.xyz[i], torch.exp(loop.scaling[i]),
                              torch.nn.functional.normalize(loop.rotation[i]), torch.sigmoid(loop.opacity[i]), loop.features,
                              antialiasing=loop.antialiasing, return_minmax=True)

    def begin(self, loop, b, n):
        """Frames b .. b + n of the sequence are the first n frames of `loop`'s batch, just initialised (behind new_scenes, on the
        current stream): their heat-maps and first renders."""
        picked = self.chosen(b, n)
        if not picked:
            return
        hm, hmm = loop.heatmap_pictures()
        V = self.V
        for k, i in picked:
            self.heatmaps[k], self.minmax[0, k] = hm[i * V:(i + 1) * V], hmm[i * V:(i + 1) * V]
            self.render_first[k], self.minmax[1, k] = self._render(loop, i)

    def take(self, loop, b, n):
        """Frames b .. b + n of the sequence are the first n frames of `loop`'s batch, optimised (on the current stream, behind
        the copy of the joints): their last renders."""
        for k, i in self.chosen(b, n):
            self.render_last[k], self.minmax[2, k] = self._render(loop, i)

    def save(self, output_dir, scene_names=None):
        """The reference's layout (train.py:279-304): heatmaps/heatmap_{i}.png, images/render_1_{i}.png and images/render_{i}.png
        for view i.  One chosen frame goes straight under `output_dir`; several go under a sub-directory each, named by
        `scene_names` (one per chosen frame) or frame_{index}.  Returns the directories."""
        names = list(scene_names) if scene_names is not None else [f"frame_{f:06d}" for f in self.frames]
        if len(names) != len(self.frames):
            raise ValueError(f"SequenceImages.save: {len(names)} scene names for {len(self.frames)} pictured frames")
        dirs = []
        for k, name in enumerate(names):
            d = output_dir if len(names) == 1 and scene_names is None else os.path.join(output_dir, name)
            save_previews(os.path.join(d, "heatmaps"), "heatmap", self.heatmaps[k], self.sizes)
            save_previews(os.path.join(d, "images"), "render_1", self.render_first[k], self.sizes)
            save_previews(os.path.join(d, "images"), "render", self.render_last[k], self.sizes)
            dirs.append(d)
        return dirs
