"""The sparse fused training step (sks_gt_tile_stats / sks_geometry / sks_backward_fused_loss / sks_loop_fused_step): the geometry
stage alone, and render + clamp + masked L2 + backward on the tiles the Gaussians cover -- no dense image is written."""
import math

import torch

from . import _lib
from ._base import ForwardState, ViewBatch, _accum, _bg_channels, _f32c, _f32c_params, _fresh, _grad_dict


class GtStats:
    """Per-scene statistics of the constant pseudo-GT heat-maps (V,C,H,W): what the masked-L2 loss sees wherever the
    render is zero (sum of gt^2 and count over the pixels with gt > 0: a negative entry is outside the mask).  `offsets`
    (HOST size_t array or None): views of different sizes -- `gt` is then a flat fp32 buffer and offsets[v] the start (in
    floats) of view v's (C,H_v,W_v) planes (HeatmapSet)."""
    __slots__ = ("gt", "tile_S", "tile_N", "totals", "offsets", "factors")

    def __init__(self):
        self.offsets = None
        self.factors = None      # HeatmapFactors: the heat-maps in separable form, no planes (then gt is None)

    @classmethod
    def _all_views(cls, V, device):
        """No per-tile arrays; a zeroed (V,2) `totals` table the caller has filled per scene."""
        st = cls()
        st.gt = st.tile_S = st.tile_N = None
        st.totals = torch.zeros((V, 2), dtype=torch.float64, device=device)
        return st

    @classmethod
    def of_set(cls, hset):
        """All views of a HeatmapSet, whatever their sizes, in one batch: its flat buffer and per-view offsets."""
        st = cls._all_views(len(hset.sizes), hset.flat.device)
        st.gt, st.offsets = hset.flat, hset.offsets
        return st

    @classmethod
    def of_factors(cls, factors):
        """The views of a HeatmapFactors: no planes at all."""
        st = cls._all_views(factors.V, factors.row.device)
        st.factors = factors
        return st


class HeatmapFactors:
    """The pseudo-GT heat-maps of V views in SEPARABLE form -- plane(v, j) = (row[v,j][:, None] * col[v,j][None, :] -
    cmin[v,j]) / den[v,j], what heatmaps.heatmap_factors computes -- for the sparse fused step, which evaluates the few
    thousand pixels it needs from the factors (bit for bit the value sks_heatmaps would have stored) instead of reading
    them back from (V,J,H,W) planes nobody else looks at: 68 MB per H36M view never written.  row (V,J,H), col (V,J,W) with
    H, W the LARGEST view (views of different sizes use the leading part of their rows), cmin / den (V,J).
    `totals()` fills a (V,2) fp64 table with each view's {sum gt^2, count gt > 0} (GtStats.totals)."""

    def __init__(self, V, J, W, H, device):
        import ctypes
        self.V, self.J, self.W, self.H = int(V), int(J), int(W), int(H)
        self.row = torch.zeros((V, J, H), dtype=torch.float32, device=device)
        self.col = torch.zeros((V, J, W), dtype=torch.float32, device=device)
        self.cmin = torch.zeros((V, J), dtype=torch.float32, device=device)
        self.den = torch.ones((V, J), dtype=torch.float32, device=device)
        self.ptrs = (ctypes.c_void_p * 4)(self.row.data_ptr(), self.col.data_ptr(), self.cmin.data_ptr(), self.den.data_ptr())

    def totals(self, views, out):
        lib = _lib.load()
        if tuple(out.shape) != (self.V, 2) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("HeatmapFactors.totals: `out` must be a contiguous fp64 (V,2) tensor")
        dev = self.row.device
        with torch.cuda.device(dev):
            if views.table is not None:
                rc = lib.sks_heatmap_totals_dv(self.V, self.J, self.W, self.H, self.row.data_ptr(), self.col.data_ptr(),
                                               self.cmin.data_ptr(), self.den.data_ptr(), views.table.data_ptr(), out.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream)
            else:
                rc = lib.sks_heatmap_totals(self.V, self.J, self.W, self.H, self.row.data_ptr(), self.col.data_ptr(),
                                            self.cmin.data_ptr(), self.den.data_ptr(), views.wh, out.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "sks_heatmap_totals")
        return out

    def planes(self, v, size=None):
        """View v's (J,H_v,W_v) planes as tensor ops (tests, debugging): the same fp32 expression, same order."""
        w, h = size or (self.W, self.H)
        return (self.row[v, :, :h, None] * self.col[v, :, None, :w] - self.cmin[v, :, None, None]) / self.den[v, :, None, None]


class HeatmapSet:
    """The heat-maps of V views whose image sizes may differ, in ONE flat buffer (so that a single launch can address
    all of them): `planes[v]` is view v's (C,H_v,W_v) tensor, a view into `flat`; views of equal size are adjacent, so
    `group(key)` is a (Vg,C,H,W) tensor for the dense entry points.  offsets: HOST size_t array for the C ABI."""

    def __init__(self, sizes, C, device):
        import ctypes
        self.sizes = [(int(w), int(h)) for w, h in sizes]
        self.C = int(C)
        order = {}
        for v, sz in enumerate(self.sizes):
            order.setdefault(sz, []).append(v)
        self.groups = order                         # (W,H) -> views, in first-appearance order of the sizes
        total = sum(self.C * w * h * len(vs) for (w, h), vs in order.items())
        self.flat = torch.empty(total, dtype=torch.float32, device=device)
        off = [0] * len(self.sizes)
        self._group_t = {}
        pos = 0
        for (w, h), vs in order.items():
            n = self.C * w * h
            self._group_t[(w, h)] = self.flat[pos:pos + n * len(vs)].view(len(vs), self.C, h, w)
            for i, v in enumerate(vs):
                off[v] = pos + i * n
            pos += n * len(vs)
        self.offsets_list = off
        self.offsets = (ctypes.c_size_t * len(off))(*off)
        self.planes = [self.flat[off[v]:off[v] + self.C * w * h].view(self.C, h, w) for v, (w, h) in enumerate(self.sizes)]

    def group(self, key):
        return self._group_t[key]

    @classmethod
    def adopt(cls, tensor):
        """A contiguous (V,C,H,W) tensor as a (single-size) set, without a copy."""
        import ctypes
        V, C, H, W = tensor.shape
        self = cls.__new__(cls)
        self.sizes, self.C = [(W, H)] * V, C
        self.groups = {(W, H): list(range(V))}
        self.flat = tensor.view(-1)
        self._group_t = {(W, H): tensor}
        n = C * H * W
        self.offsets_list = [v * n for v in range(V)]
        self.offsets = (ctypes.c_size_t * V)(*self.offsets_list)
        self.planes = [tensor[v] for v in range(V)]
        return self


def gt_tile_stats(gt, out=None, tiles=False):
    """Per-view heat-map totals (what the masked-L2 loss is for an all-zero render: {sum of gt^2 over gt > 0, count of gt > 0},
    planes of any sign); `tiles=True` also fills the per
    (view, tile, channel) arrays.  `out`: a GtStats of the same shape to refill in place (scene streaming keeps every
    pointer stable)."""
    gt = _f32c(gt, "gt")
    V, C, H, W = gt.shape
    NT = ((W + 15) // 16) * ((H + 15) // 16)
    dev = gt.device
    if out is not None:
        if out.totals.shape != (V, 2) or out.totals.device != dev or out.gt.shape != gt.shape or out.offsets is not None:
            raise ValueError("gt_tile_stats: `out` was made for another shape / device")
        st = out
    else:
        st = GtStats()
        st.tile_S = torch.empty((V, NT, C), dtype=torch.float32, device=dev) if tiles else None
        st.tile_N = torch.empty((V, NT, C), dtype=torch.float32, device=dev) if tiles else None
        st.totals = torch.empty((V, 2), dtype=torch.float64, device=dev)
    st.gt = gt
    with torch.cuda.device(dev):
        rc = _lib.load().sks_gt_tile_stats(V, C, W, H, gt.data_ptr(), _lib.ptr(st.tile_S), _lib.ptr(st.tile_N),
                                           st.totals.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "sks_gt_tile_stats")
    return st


def geometry_views(views: ViewBatch, means3D, C, opacities, scales, rotations, cov3D_precomp, scale_modifier=1.0,
                   antialiasing=False, raw_params=False, out=None, frames=1):
    """Geometry stage only (no image): returns a ForwardState usable by backward_fused_loss.  raw_params: the three
    tensors are the leaf parameters (_opacity, _scaling, _rotation); activations run in-kernel (SKS_RAW_PARAMS).
    frames > 1: `views` holds frames x Vf views (frame-major) and the parameter tensors are stacked (frames, P, ..):
    view f*Vf + j renders frame f's Gaussians (see sks_loop_fused_step)."""
    lib = _lib.load()
    means3D, _, opacities, scales, rotations, cov3D_precomp = _f32c_params(means3D, None, opacities, scales, rotations, cov3D_precomp)
    dev = means3D.device
    frames = int(frames)
    if frames < 1 or views.V % frames:
        raise ValueError(f"frames = {frames} must divide the number of views ({views.V})")
    if frames > 1 and (means3D.dim() != 3 or means3D.shape[0] != frames):
        raise ValueError(f"frames = {frames} needs parameters stacked (frames, P, ..); means3D is {tuple(means3D.shape)}")
    P = means3D.shape[-2]
    V, W, H = views.V, views.W, views.H
    flags = (_lib.SKS_ANTIALIASING if antialiasing else 0) | (_lib.SKS_RAW_PARAMS if raw_params else 0)
    gbytes, _, _ = _lib.scratch_bytes(V, max(P, 1), C, W, H, 0)
    if out is not None and out.P == P and out.C == C and out.views is views and out.flags == flags and out.frames == frames:
        radii, geom = out.radii, out.geom       # refill in place (persistent state of the fused loop step)
    else:
        radii = torch.empty((V, P), dtype=torch.int32, device=dev)
        geom = torch.empty(gbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        if views.table is not None:
            rc = lib.sks_geometry_dv(V, P, C, W, H, views.viewmatrix.data_ptr(), views.projmatrix.data_ptr(),
                                     views.table.data_ptr(), _lib.ptr(means3D), _lib.ptr(opacities), _lib.ptr(scales),
                                     _lib.ptr(rotations), _lib.ptr(cov3D_precomp), float(scale_modifier), flags,
                                     radii.data_ptr(), geom.data_ptr(), frames, torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(rc, "sks_geometry_dv")
            return ForwardState(views, P, C, flags, scale_modifier, radii, geom, frames=frames)
        rc = lib.sks_geometry(V, P, C, W, H, views.viewmatrix.data_ptr(), views.projmatrix.data_ptr(), views.tanfovx,
                              views.tanfovy, _lib.ptr(means3D), _lib.ptr(opacities), _lib.ptr(scales), _lib.ptr(rotations),
                              _lib.ptr(cov3D_precomp), float(scale_modifier), flags, radii.data_ptr(), geom.data_ptr(),
                              views.wh, frames, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "sks_geometry")
    return ForwardState(views, P, C, flags, scale_modifier, radii, geom, frames=frames)


def _check_heatmaps(views, C, stats):
    """The heat-maps must be what the views address: one (V,C,H,W) tensor, or (mixed sizes) a HeatmapSet's flat buffer,
    or (factored) a HeatmapFactors of the views' largest size."""
    if stats.factors is not None:
        f = stats.factors
        if (f.V, f.J, f.W, f.H) != (views.V, C, views.W, views.H):
            raise RuntimeError(f"heat-map factors {(f.V, f.J, f.W, f.H)} do not match the views {(views.V, C, views.W, views.H)}")
        return
    if views.mixed:
        if stats.offsets is None or len(stats.offsets) != views.V:
            raise RuntimeError("views of different sizes need heat-maps in one flat buffer with per-view offsets (HeatmapSet)")
        need = max(int(o) + C * w * h for o, (w, h) in zip(stats.offsets, views.sizes))
        if stats.gt.numel() < need:
            raise RuntimeError(f"heat-map buffer of {stats.gt.numel()} floats is too small for the views ({need})")
    elif stats.offsets is None and tuple(stats.gt.shape) != (views.V, C, views.H, views.W):
        raise RuntimeError(f"heat-maps {tuple(stats.gt.shape)} do not match the views {(views.V, C, views.H, views.W)}")


def loop_fused_step(st: ForwardState, stats: GtStats, features, packed, sums, slots, group_mask, last_view, xyz, scaling,
                    rotation, opacity, exp_avg, exp_avg_sq, counters, acc_steps, lr_sched, lrs, adam, lambda_consistency, limb,
                    es_state=None, es_window=0, es_tolerance=0.0, es_flags=None, view_weights=None):
    """sks_loop_fused_step: fused-loss compositing backward + (geometry backward, Adam step, geometry forward of the
    updated parameters) for one accumulation group; `st` must describe the current parameters and is left describing the
    updated ones.  lr_sched / lrs / adam / limb: ctypes arrays as for sks_loop_adam_step.  A state made with
    geometry_views(frames=F) steps F independent frames at once (stacked parameter / moment / slot / counter tensors).
    es_state: (F, 2 + 2 * es_window) int32 device tensor -> sks_loop_fused_step_es, the reference's opt_early_stopping per
    frame on the device (es_flags: (F,) pinned int32 host tensor that receives each frame's stopping iteration, or None).
    Views with a device `table` (a frame batch over a rig bank): `lr_sched` is the (frames,5) float64 DEVICE tensor of per-frame
    schedule rows and the step goes through sks_loop_fused_step_dv / _es_dv.
    view_weights: None, or (vw_mode 1 | 2, threshold, weights (F,Vf,P) float32 or None, similarity (F,P,Vf,Vf) float32 or None) ->
    sks_loop_fused_step_vw / _vw_dv: the views weighted by their agreement (include/skelsplat_hip.h "View agreement"), with or
    without the criterion."""
    lib = _lib.load()
    dev = xyz.device
    V, P, C = st.views.V, st.P, st.C
    W, H = st.views.W, st.views.H
    _check_heatmaps(st.views, C, stats)
    feat2 = _f32c(features, "features").reshape(P, -1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    accum = _accum(dev, stream, V, P, C)
    dv = st.views.table is not None
    if dv != torch.is_tensor(lr_sched):
        raise ValueError("lr_sched: a (frames,5) device tensor with views that carry a device table, the HOST array otherwise")
    if dv:
        if lr_sched.dtype != torch.float64 or tuple(lr_sched.shape) != (st.frames, 5) or not lr_sched.is_contiguous() \
                or lr_sched.device != dev:
            raise ValueError(f"lr_sched must be a contiguous float64 ({st.frames}, 5) tensor on {dev}")
        cams = (st.views.table.data_ptr(),)
        lr_sched = lr_sched.data_ptr()
    else:
        cams = (st.views.tanfovx, st.views.tanfovy)
    step, step_es = ((lib.sks_loop_fused_step_dv, lib.sks_loop_fused_step_es_dv) if dv
                     else (lib.sks_loop_fused_step, lib.sks_loop_fused_step_es))
    args = (V, P, C, W, H, st.views.viewmatrix.data_ptr(), st.views.projmatrix.data_ptr(), *cams,
            feat2.data_ptr(), st.scale_modifier, st.flags, st.radii.data_ptr(), st.geom.data_ptr(),
            _lib.ptr(stats.gt), stats.totals.data_ptr(), accum.data_ptr(), sums.data_ptr(), packed.data_ptr(),
            slots.data_ptr(), group_mask, last_view, xyz.data_ptr(), scaling.data_ptr(), rotation.data_ptr(),
            opacity.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), counters.data_ptr(), acc_steps, lr_sched, lrs,
            adam, float(lambda_consistency), limb, st.views.wh, stats.offsets, st.frames,
            None if stats.factors is None else stats.factors.ptrs)
    if es_state is None and view_weights is None:
        with torch.cuda.device(dev):
            rc = step(*args, stream)
        _lib.check(rc, "sks_loop_fused_step")
        return
    if es_state is None:
        es = (None, 0, 0.0, None)
    else:
        es = _es_args(st, dev, es_state, es_window, es_tolerance, es_flags)
    if view_weights is not None:
        mode, threshold, weights, similarity = view_weights
        Vf = V // st.frames
        for name, t, shape in (("weights", weights, (st.frames, Vf, P)), ("similarity", similarity, (st.frames, P, Vf, Vf))):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() != math.prod(shape)):
                raise ValueError(f"view_weights: {name} must be a contiguous float32 {shape} tensor on {dev}")
        with torch.cuda.device(dev):
            rc = (lib.sks_loop_fused_step_vw_dv if dv else lib.sks_loop_fused_step_vw)(
                *args, *es, int(mode), float(threshold), None if weights is None else weights.data_ptr(),
                None if similarity is None else similarity.data_ptr(), stream)
        _lib.check(rc, "sks_loop_fused_step_vw")
        return
    with torch.cuda.device(dev):
        rc = step_es(*args, *es, stream)
    _lib.check(rc, "sks_loop_fused_step_es")


def _es_args(st, dev, es_state, es_window, es_tolerance, es_flags):
    """The criterion's four arguments of the fused step's early-stopping forms, checked."""
    if es_state.dtype != torch.int32 or not es_state.is_contiguous() or es_state.device != dev \
            or tuple(es_state.shape) != (st.frames, 2 + 2 * int(es_window)):
        raise ValueError(f"es_state must be a contiguous int32 ({st.frames}, {2 + 2 * int(es_window)}) tensor on {dev}")
    if es_flags is not None and (es_flags.dtype != torch.int32 or es_flags.numel() != st.frames or es_flags.device.type != "cpu"):
        raise ValueError(f"es_flags must be a pinned int32 host tensor of {st.frames} ints")
    return (es_state.data_ptr(), int(es_window), float(es_tolerance), None if es_flags is None else es_flags.data_ptr())


def backward_fused_loss(st: ForwardState, stats: GtStats, means3D, features, opacities, scales, rotations, cov3D_precomp,
                        bg=None, packed_out=None, sums_out=None):
    """Render + clamp + masked-L2 + backward on the covered tiles only.  Returns (grads dict of (V,P,..) UNSCALED
    gradients, loss_sums (V,2) f64 = per-view {S, N}); the true gradient is grads / N_v, loss_v = S_v / N_v."""
    lib = _lib.load()
    means3D, features, opacities, scales, rotations, cov3D_precomp = _f32c_params(means3D, features, opacities, scales, rotations, cov3D_precomp)
    dev = means3D.device
    V, P, C, W, H = st.views.V, st.P, st.C, st.views.W, st.views.H
    _check_heatmaps(st.views, C, stats)
    feat2 = features.reshape(P, -1)
    bgC = _bg_channels(bg, C, dev)
    out = _grad_dict(_fresh(torch.empty, dev), V, P, C, scales is not None, rotations is not None, False)
    if sums_out is None:
        sums = torch.empty((V, 2), dtype=torch.float64, device=dev)
    else:
        sums = sums_out[:V]
        if sums.shape != (V, 2) or sums.dtype != torch.float64 or not sums.is_contiguous():
            raise ValueError("sums_out must be a contiguous fp64 tensor with at least V rows of 2")
    if packed_out is not None and (tuple(packed_out.shape) != (V, P, 11) or not packed_out.is_contiguous()):
        raise ValueError(f"packed_out must be a contiguous (V,P,11) = {(V, P, 11)} tensor")
    stream = torch.cuda.current_stream(dev).cuda_stream
    accum = _accum(dev, stream, V, P, C)
    with torch.cuda.device(dev):
        rc = lib.sks_backward_fused_loss(V, P, C, W, H, st.views.viewmatrix.data_ptr(), st.views.projmatrix.data_ptr(),
                                         st.views.tanfovx, st.views.tanfovy, _lib.ptr(bgC), _lib.ptr(means3D), _lib.ptr(feat2),
                                         _lib.ptr(opacities), _lib.ptr(scales), _lib.ptr(rotations), _lib.ptr(cov3D_precomp),
                                         st.scale_modifier, st.flags, st.radii.data_ptr(), st.geom.data_ptr(),
                                         _lib.ptr(stats.gt), _lib.ptr(stats.tile_S), _lib.ptr(stats.tile_N),
                                         stats.totals.data_ptr(), accum.data_ptr(), _lib.ptr(out["means3D"]),
                                         _lib.ptr(out["means2D"]), _lib.ptr(out["opacities"]), _lib.ptr(out["scales"]),
                                         _lib.ptr(out["rotations"]), _lib.ptr(out["cov3D"]), sums.data_ptr(),
                                         _lib.ptr(packed_out), st.views.wh, stats.offsets,
                                         None if stats.factors is None else stats.factors.ptrs, stream)
    _lib.check(rc, "sks_backward_fused_loss")
    return out, sums
