"""What every part of the rasterizer's Python surface shares: argument checks, the scratch torch owns, the packed cameras of a call
(ViewBatch) and what a forward leaves for its backward (ForwardState)."""
import weakref

import torch

from . import _lib


# ------------------------------------------------------------------------------------------------------------
# scratch management (replaces resizeFunctional, DGR/rasterize_points.cu:27-33): torch owns every byte
# ------------------------------------------------------------------------------------------------------------
_accum_cache = {}
_VIEW_CACHE = {}     # ViewBatch.from_settings
_SCRATCH_BYTES = {}   # _scratch_bytes_cached
_BG_CACHE = {}        # _bg_channels


def _accum(device, stream, V, P, C):
    """Backward partial-sum scratch (uninitialised is fine): one buffer per (device, stream, shape)."""
    key = (device.index, stream, V, P, C)
    # While a hipGraph is being captured the current stream is torch's capture stream, the same handle for every capture --
    # and a handle that torch's pool of streams hands out again to eager code.  A cached buffer under that handle would be
    # baked into every graph captured with this shape, and graphs replayed side by side on different streams (FramePipeline)
    # would then share their partial sums.  So a capture never takes a buffer from the cache and never leaves one there: its
    # buffer comes from the graph's private pool, which keeps it alive for its own replays.
    capturing = torch.cuda.is_current_stream_capturing()
    buf = None if capturing else _accum_cache.get(key)
    if buf is None:
        _, _, nbytes = _lib.scratch_bytes(V, max(P, 1), C, 16, 16)
        buf = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
        if not capturing:
            _accum_cache[key] = buf
    return buf


def reset_scratch():
    """Drop cached accumulators (call after an aborted backward, e.g. an exception between kernels)."""
    _accum_cache.clear()


def _need_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"skelsplat_amd: `{name}` must live on a ROCm device (got {t.device}); "
                           "there is no CPU fallback")


def _f32c(t, name):
    if t is None or t.numel() == 0:
        return None
    _need_gpu(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"skelsplat_amd: `{name}` must be float32 (got {t.dtype})")
    return t.contiguous()


def _f32c_params(means3D, features, opacities, scales, rotations, cov3D_precomp):
    """The parameter tensors of a call as contiguous fp32 ROCm tensors (None = not provided)."""
    return (_f32c(means3D, "means3D"), _f32c(features, "features"), _f32c(opacities, "opacities"), _f32c(scales, "scales"),
            _f32c(rotations, "rotations"), _f32c(cov3D_precomp, "cov3D_precomp"))


def _grad_dict(new, V, P, C, has_scales, has_rotations, want_features):
    """The gradient dictionary of a backward: per-view (V,P,..) fp32 tensors from the allocator `new(name, *shape)`."""
    return dict(means3D=new("m3", V, P, 3), means2D=new("m2", V, P, 3), opacities=new("op", V, P, 1), cov3D=new("cov", V, P, 6),
                scales=new("sc", V, P, 3) if has_scales else None, rotations=new("rot", V, P, 4) if has_rotations else None,
                features=new("feat", V, P, C) if want_features else None)


def _fresh(fill, dev):      # _grad_dict's allocator of fresh tensors (fill: torch.empty / torch.zeros)
    return lambda name, *shape: fill(shape, dtype=torch.float32, device=dev)


class ViewBatch:
    """V cameras packed for one launch sequence.  The dense entry points (sks_forward / sks_backward write and read
    (V,C,H,W) tensors) need one image size; the sparse fused-loss path writes nothing dense and takes a batch whose
    views differ in size (`sizes`: per-view (W, H); H36M mixes 1000- and 1002-wide sensors, dataset_readers.py:68-80):
    then W, H are the largest and `wh` is the HOST array the C ABI's `view_wh` argument wants.
    `table`: None, or (a frame batch over a rigs.RigBank) the device-resident ViewTan table sks_rig_select fills together with
    the rows of `viewmatrix` / `projmatrix`: geometry_views, loop_fused_step, heatmap_factors and HeatmapFactors.totals then go
    through the library's *_dv entry points, which read the per-view scalars from it instead of from the host arrays."""

    def __init__(self, viewmatrices, projmatrices, tanfovx, tanfovy, W, H, sizes=None):
        import ctypes
        self.viewmatrix = _f32c(viewmatrices, "viewmatrix").reshape(-1, 16)
        self.projmatrix = _f32c(projmatrices, "projmatrix").reshape(-1, 16)
        self.V = self.viewmatrix.shape[0]
        if self.V > _lib.SKS_MAX_VIEWS:
            raise RuntimeError(f"at most {_lib.SKS_MAX_VIEWS} views per call")
        self.tanfovx = _lib.farray(tanfovx)
        self.tanfovy = _lib.farray(tanfovy)
        assert len(tanfovx) == self.V and len(tanfovy) == self.V
        self.W, self.H = int(W), int(H)
        self.sizes = [(self.W, self.H)] * self.V if sizes is None else [(int(w), int(h)) for w, h in sizes]
        assert len(self.sizes) == self.V
        self.mixed = any(sz != (self.W, self.H) for sz in self.sizes)
        self.wh = (ctypes.c_int * (2 * self.V))(*[x for sz in self.sizes for x in sz]) if self.mixed else None
        self.table = None

    @staticmethod
    def camera_rows(cams):
        """What a batch of these cameras holds, on the device the cameras live on (host cameras: host rows, rigs.RigBank builds
        its bank from them): viewmatrix, projmatrix (V,16), tanfovx, tanfovy (lists of V), sizes [(W_v, H_v)]."""
        import math
        sizes = [(int(c.image_width), int(c.image_height)) for c in cams]
        vm = torch.stack([c.world_view_transform.reshape(16) for c in cams])
        pm = torch.stack([c.full_proj_transform.reshape(16) for c in cams])
        return vm, pm, [math.tan(c.FoVx * 0.5) for c in cams], [math.tan(c.FoVy * 0.5) for c in cams], sizes

    @classmethod
    def from_cameras(cls, cams, allow_mixed=False):
        vm, pm, tanx, tany, sizes = cls.camera_rows(cams)
        W, H = max(s[0] for s in sizes), max(s[1] for s in sizes)
        if not allow_mixed and any(sz != (W, H) for sz in sizes):
            raise RuntimeError("all views of a batch must share the image size")
        return cls(vm, pm, tanx, tany, W, H, sizes)

    @classmethod
    def from_settings(cls, rs):
        """One view from a GaussianRasterizationSettings.  A training loop builds the settings of the same few cameras over
        and over (train.py:140 -> gaussian_renderer/__init__.py:46-60): the batch of a camera is kept while its two matrices
        are the same, unmodified tensors (the reference's are transposed views, scene/cameras.py:94-97: each rebuild would
        cost two small copy kernels and two ctypes arrays)."""
        vm, pm = rs.viewmatrix, rs.projmatrix
        key = (vm.data_ptr(), vm._version, pm.data_ptr(), pm._version, rs.tanfovx, rs.tanfovy, rs.image_width, rs.image_height)
        hit = _VIEW_CACHE.get(key)
        if hit is not None:
            vb, vm_ref, pm_ref = hit
            if vm_ref() is vm and pm_ref() is pm:
                return vb
        if len(_VIEW_CACHE) > 256:
            _VIEW_CACHE.clear()
        vb = cls(vm, pm, [rs.tanfovx], [rs.tanfovy], rs.image_width, rs.image_height)
        _VIEW_CACHE[key] = (vb, weakref.ref(vm), weakref.ref(pm))
        return vb


class ForwardState:
    """What backward needs (the reference keeps geomBuffer / binningBuffer / imgBuffer + num_rendered,
    DGR/diff_gaussian_rasterization_h36m/__init__.py:87-89)."""
    __slots__ = ("views", "P", "C", "flags", "scale_modifier", "geom", "binning", "bin_capacity", "radii",
                 "num_rendered_dev", "frames", "plan_key", "chunks")

    def __init__(self, views, P, C, flags, scale_modifier, radii, geom=None, binning=None, bin_capacity=0, num_rendered_dev=None,
                 frames=1):
        self.views, self.P, self.C, self.flags, self.scale_modifier = views, P, C, flags, float(scale_modifier)
        self.geom, self.binning, self.bin_capacity, self.radii, self.num_rendered_dev = geom, binning, bin_capacity, radii, num_rendered_dev
        self.frames = frames    # geometry_views(frames=F): F independent frames' Gaussians, stacked
        self.plan_key = None    # the autograd path: key of the forward's _Block in `plans`
        self.chunks = None      # more than SKS_MAX_CHANNELS channels: [(view, c0, c1, feature chunk, ForwardState of that call)]


def _scratch_bytes_cached(V, P, C, W, H, cap):
    key = (V, P, C, W, H, cap)
    r = _SCRATCH_BYTES.get(key)
    if r is None:
        r = _SCRATCH_BYTES[key] = _lib.scratch_bytes(V, P, C, W, H, cap)
    return r


def _bg_channels(bg, C, dev):
    """The background as C floats, or None when it is absent or all zero (the reference's default `[0, 0, 0]`,
    train.py:112-113): a zero background contributes nothing to the backward (backward.cu:612-615), and passing NULL
    selects the faster kernels.  The reference reads C floats from its 3-float bg tensor (backward.cu:613-614); pad
    with zeros instead.  One host read per (tensor, version), cached."""
    if bg is None or bg.numel() == 0:
        return None
    key = (id(bg), C, str(dev))
    hit = _BG_CACHE.get(key)
    if hit is not None:
        bg_ref, version, bgC = hit
        if bg_ref() is bg and version == bg._version:     # (else: another tensor at a recycled id, or modified in place since)
            return bgC
    if len(_BG_CACHE) > 64:
        _BG_CACHE.clear()
    bgC = None
    if bool((bg != 0).any()):
        bgC = torch.zeros(C, dtype=torch.float32, device=dev)
        k = min(C, bg.numel())
        bgC[:k] = bg.reshape(-1)[:k].to(device=dev, dtype=torch.float32)
    _BG_CACHE[key] = (weakref.ref(bg), bg._version, bgC)
    return bgC
