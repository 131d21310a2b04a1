"""Python surface of the rasterizer: the reference's GaussianRasterizationSettings / GaussianRasterizer API
(DGR/diff_gaussian_rasterization_h36m/__init__.py:21-207) on top of the C ABI in include/skelsplat_hip.h,
plus the batched multi-view entry points the MI355X loop uses.

"DGR/" = submodules/diff-gaussian-rasterization-h36m/ of the reference.
"""
from collections import namedtuple
from typing import NamedTuple, Optional

import operator
import os

import torch
import torch.nn as nn

from . import _arena, _lib
# (callers and tests reach all of this through this module, `R.geometry_views`, `R._FILL_TUNE`: the dictionaries are the same objects)
from ._arena import _BIN_CAP_HINT, _BIN_CAP_SEEN, _BIN_PROBE  # noqa: F401
from ._base import (ForwardState, ViewBatch, _accum, _bg_channels, _f32c, _f32c_params, _fresh, _grad_dict,  # noqa: F401
                    _need_gpu, _scratch_bytes_cached, reset_scratch)
from ._tuning import (PLAIN_STORES, TUNE_CANDIDATES, TUNE_CANDIDATES_FRESH, TUNE_CANDIDATES_WITH_PLAIN, TUNE_WARM,  # noqa: F401
                      _FILL_BITS, _FILL_TUNE, _FILL_TUNE_LOG, _MEASURING, _pick, _time_candidates, _tune_flag_bits, fill_tuning,
                      tune_name)
from .sparse import (GtStats, HeatmapFactors, HeatmapSet, backward_fused_loss, geometry_views, gt_tile_stats,  # noqa: F401
                     loop_fused_step)

_ENV_TUNE = int(os.environ.get("SKS_FWD_TUNE", "0"), 0)   # tuning experiments: extra forward flag bits (include/skelsplat_hip.h)
AUTOTUNE = os.environ.get("SKS_AUTOTUNE", "1") != "0"     # the autograd path and the loops measure a shape's fill configuration once


class GaussianRasterizationSettings(NamedTuple):
    """Same 13 fields, same order as DGR/diff_gaussian_rasterization_h36m/__init__.py:143-156."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    antialiasing: bool


class Workspace:
    """Reusable outputs and scratch of forward_views / backward_views.  A caller that runs the same shapes every step
    (a training loop: train.py:130-222 renders the same cameras 500 times per frame) passes the same Workspace to every
    call and the calls allocate nothing: a dozen caching-allocator round trips per step are ~20 us of host time next
    to ~78 us of kernels on the H36M step.  What the calls return are the workspace's tensors: the NEXT call of the same kind
    with the same shapes overwrites them (the reference's own outputs are fresh tensors per call; callers that keep results
    across calls simply do not pass a workspace).

    What is relied on instead of clearing.  Every element of the scratch, the gradients and the radii is written by every call that
    returns them.  The image (colour, inverse depth) of a recorded small-path forward whose set is at most 1 GiB lives in TWO sets
    that the forwards alternate between; every element of the set a forward returns is written either by that forward or, for
    its LAST planes, by the replayed backward_views in front of it, whose two latency-bound launches store zeros there while
    HBM would otherwise idle (sks_backward_prefill / sks_forward_prefilled, include/skelsplat_hip.h).  The invariant: `cur` is the
    set the last forward rendered; a replayed backward_views zeroes the other set's last planes and notes how many and on which
    stream; nothing else writes the other set; the next replayed forward_views on that stream renders into it with those planes
    taken as zero, the sets swap and the note is gone.  A forward without a valid note (the first, one on another stream, one
    after a call that took the validating path, under stream capture) renders into `cur` and fills everything, and
    forward_backward_views always does.  So the result tuples of successive forwards alternate between two (color, invdepth)
    pairs -- with the same radii and the same ForwardState object -- and a result stays valid until the next call of the same kind,
    as ever.  New with the second set: writing into a result that is already dead by that rule can corrupt a LATER image (the dead
    set may hold planes zeroed for the next forward).  The second set is allocated by the first backward that prefills
    (H36M: 2 x 288 MB); larger images (all 31 Panoptic views: 5.1 GB) and the binned path keep one set.  A call under stream
    capture neither prefills nor takes prefilled planes, and from then on the workspace stops for good: a graph replayed later
    renders into the pointers it captured, behind this object's back.

    prefill: None = the library's rule decides how many planes ride in the backward (sks_prefill_planes), 0 = off (one set,
    the behaviour before the second set existed), (n_wave, n_geom) = forced plane counts for the compositing / geometry
    backward's launch (tests and sweeps)."""

    def __init__(self, prefill=None):
        self._t = {}
        self._plans = {}     # "fwd" / "bwd" -> the last call's record (_FwdRecord / _BwdRecord)
        self._aux = {}
        self._pending_join = None     # device whose second stream still holds a forward_backward_views(join=False) backward
        if prefill is not None and prefill != 0:
            prefill = (int(prefill[0]), int(prefill[1]))
        self._prefill = prefill
        self._pf = None               # the two output sets of the recorded forward (_Prefill), or None: one set
        self._pf_off = prefill == 0   # no prefill (asked for, or a call was captured into a graph)

    def aux_stream(self, dev_index):
        """The second stream forward_backward_views runs the backward on (created on first use, one per device)."""
        st = self._aux.get(dev_index)
        if st is None:
            st = self._aux[dev_index] = torch.cuda.Stream(device=dev_index)
        return st

    def join(self, dev_index):
        """The current stream waits for everything enqueued on the second stream (forward_backward_views(join=False))."""
        torch.cuda.current_stream(dev_index).wait_stream(self.aux_stream(dev_index))
        self._pending_join = None

    def tune(self, step_fn, candidates=None, reps=8, rounds=3, confirm=True):
        """Picks how the forward's fill role writes for the step `step_fn` issues through THIS workspace's recorded forward, by
        timing it: 4 KB passes (or rows, on row-aligned widths) per fill block (bits 0..7 of a candidate -> bits 8..15 of the flags,
        0 = the library's default of two) and the KIND of store (candidate bit 8, PLAIN_STORES -> SKS_NO_NT_STORES).  Why per step
        and at run time: the fill role is bound by the life time of its ~36 000 blocks, and what shares the chip with them decides
        the best size -- two passes when the forward runs alone (sks_forward, then sks_backward), three for the H36M step through
        sks_forward_backward (the backward's wavefronts hold slots beside it), four for all 31 Panoptic views, five for four of
        them.  The store kind decides where the zeros go first: non-temporal stores stream past the 256 MB Infinity Cache to HBM;
        plain stores may stay in it, so a call that rewrites the SAME ~cache-sized output buffers step after step (a Workspace)
        hands them over at the cache's rate while the previous step's lines drain behind it (H36M, 288 MB per call) -- a gain of
        the STEP only where nothing else wants that bandwidth, and 40 % slower on Panoptic and the stress scene
        (NOTES_experiments.md).  The pick is the candidate with the lowest step time in its least disturbed round; the default
        stays unless another beats it by more than 2 % twice (_pick).  None of it moves a result bit (tests/test_raster_gpu.py).  `step_fn()` is called len(candidates) x rounds x (2 + reps)
        times (+ TUNE_WARM untimed calls in front, + up to 3 x 2 x (2 + reps) for the confirmation unless confirm=False: a caller
        whose step holds a collective wants every rank to issue the same number of steps) with device synchronisations in between
        (once, before a long loop); the candidates are interleaved round-robin.
        The pick also becomes the default of later Workspace recordings of the same shape.  Returns (best, {candidate: us})."""
        plan = self._plans.get("fwd")
        if plan is None or torch.cuda.is_current_stream_capturing():
            return None, {}
        candidates = TUNE_CANDIDATES if candidates is None else candidates
        args, dev_index = plan.args, plan.dev_index
        base = args[_F_FLAGS] & ~_FILL_BITS

        def set_bits(bits):
            args[_F_FLAGS] = base | bits
        times = _time_candidates(set_bits, step_fn, candidates, reps, rounds, dev_index)
        best, med = _pick(times, candidates, set_bits, step_fn, reps, dev_index, confirm)
        set_bits(_tune_flag_bits(best))
        key = (dev_index, *(args[_lib.FWD[n]] for n in ("V", "P", "C", "W", "H")), "workspace")
        _FILL_TUNE[key] = _tune_flag_bits(best)
        _FILL_TUNE_LOG[key] = {tune_name(c): round(v, 2) for c, v in med.items()}
        return best, med

    def settle(self):
        """A forward_backward_views(join=False) whose caller never joined: the next call through this workspace makes the join
        itself, before its geometry kernel overwrites what the backward on the second stream may still be reading."""
        if self._pending_join is not None:
            self.join(self._pending_join)

    def get(self, name, shape, dtype, device):
        key = (name, tuple(shape), dtype, device)
        t = self._t.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=device)
            self._t[key] = t
        return t


class _Prefill:
    """The two output sets of a Workspace's recorded forward (see Workspace).  sets[i] = (color, invdepth) (sets[1] None until the
    first prefilling backward), results[i] = what a forward that rendered set i returns, cur = the set the last forward rendered,
    note = None or (planes, stream): the other set's last `planes` planes are zero in `stream` order.  fargs = the live block of
    sks_forward_prefilled (the record's block with `prefilled_planes` in front of the stream; the flags word is copied from the
    record on every call, bench.py and Workspace.tune write it there), bargs = that of sks_backward_prefill for record `bplan`."""
    __slots__ = ("shape", "sets", "results", "cur", "note", "fargs", "bplan", "bargs", "rule")

    def __init__(self, shape, color, invdepth, radii, st, args):
        self.shape = shape      # (V, P, C, W, H)
        self.sets = [(color, invdepth), None]
        self.results = [(color, invdepth, radii, st), None]
        self.cur, self.note = 0, None
        self.fargs = list(args[:-1]) + [0, None]
        self.bplan = self.bargs = None
        self.rule = {}          # forward flags -> (planes_wave, planes_geom)


_PREFILL_MAX_SET_BYTES = 1 << 30


def _sig(t):
    """What identifies a tensor argument of a recorded call: None (not provided), (pointer, shape) of a contiguous fp32
    ROCm tensor, or False = "take the validating path" (anything else)."""
    if t is None or t.numel() == 0:     # (an empty tensor is the reference's "not provided": GaussianRasterizer hands torch.Tensor([]))
        return None
    if t.dtype is not torch.float32 or not t.is_cuda or not t.is_contiguous():
        return False
    return (t.data_ptr(), t.shape)


# The records of replayed calls.  Their field ORDER is part of the surface: bench.py writes the flags word of the live list between
# calls, `Workspace._plans["fwd"][2][_lib.FWD["flags"]]`.  key: _fwd_key / _bwd_key of the recorded call; keep: what the pointers in
# `args` belong to; args: the live argument block (_lib.FORWARD_PARAMS / BACKWARD_PARAMS) the next replay launches with; result: what
# every replay returns, (color, invdepth, radii, state) / the gradient dictionary; arena: None, or what a replay of a binned forward
# draws its ticket with, _arena.begin's (shape, capacity, mode) -- mode True when the record was made with check_capacity=True
# (replays check synchronously), "lazy" otherwise (a record made under "auto" replays lazily).
_FwdRecord = namedtuple("_FwdRecord", "key keep args dev_index result arena")      # Workspace._plans["fwd"]
_BwdRecord = namedtuple("_BwdRecord", "key keep args dev_index result")                # Workspace._plans["bwd"]
# An entry of the autograd path's `plans`: the validated block of a call whose tensors are fresh every call (a replay patches their
# pointers into a copy).  shape: (V, P, C, H, W, gbytes, flags) of a forward, (V, P, C, has_scales, has_rotations) of a backward.
_Block = namedtuple("_Block", "args dev_index dev shape")

# Slots of the recorded blocks that are addressed after the recording: the layouts live in _lib, by parameter name.
_F_V, _F_FLAGS, _F_COLOR, _F_INVDEPTH, _F_RADII, _F_GEOM, _F_NUM_RENDERED = (
    _lib.FWD[n] for n in ("V", "flags", "out_color", "out_invdepth", "radii", "geom", "num_rendered_dev"))
_B_RADII, _B_GEOM, _B_DL_COLOR, _B_DL_INVDEPTH = (_lib.BWD[n] for n in ("radii", "geom", "dL_dout_color", "dL_dout_invdepth"))
_B_DFEAT = _lib.BWD["dL_dfeatures"]
_GRAD_SLOTS = tuple((k, _lib.BWD[n]) for k, n in (      # gradient dictionary key -> sks_backward's slot
    ("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
    ("rotations", "dL_drotations"), ("cov3D", "dL_dcov3D"), ("features", "dL_dfeatures")))
_FB_STREAM, _FB_AUX_STREAM, _FB_FLAGS = (_lib.FWD_BWD[n] for n in ("stream", "aux_stream", "fb_flags"))
# sks_forward_backward's block as ONE gather (_lib.FWD_BWD_SOURCES) from forward block + backward block; slots no record has pick the
# forward's stream slot: like `stream` itself they are set per call
_FB_GATHER = operator.itemgetter(*(_lib.FWD["stream"] if src is None else src[1] + (len(_lib.FWD) if src[0] == "bwd" else 0)
                                   for src in _lib.FWD_BWD_SOURCES))


def _replay(fn, args, dev_index, stream_slot=-1):
    """Issue a recorded call on the CURRENT stream of the tensors' device (`stream` is the last parameter of sks_forward and
    sks_backward).  The host side of a step matters here: the H36M step is ~78 us of kernels, and building two ~30-argument ctypes
    calls from tensors (validation, data_ptr, current_stream, device guard) was ~60 us of Python per step -- host-bound on a slow
    box.  A recorded call is one tuple comparison and one ctypes call."""
    args[stream_slot] = torch._C._cuda_getCurrentRawStream(dev_index)
    if torch._C._cuda_getDevice() == dev_index:
        return fn(*args)
    with torch.cuda.device(dev_index):
        return fn(*args)


def forward_views(views: ViewBatch, means3D, features, opacities, scales, rotations, cov3D_precomp,
                  scale_modifier=1.0, antialiasing=False, clamp01=False, debug=False, force_binned=False,
                  bin_capacity=None, want_aux=False, tune_flags=0, check_capacity=True, workspace=None, plans=None):
    """Raw batched forward.  Returns (color (V,C,H,W), invdepth (V,1,H,W), radii (V,P) int32, state[, final_T, n_contrib]).
    `workspace`: a Workspace whose tensors receive the outputs (see there).  `check_capacity` (binned path, P > 256):
    True (the default) = read the pair count back every call (one host sync, like the reference: rasterizer_impl.cu:283-288) and
    redo the forward with a larger arena when it was too small -- never a wrong image; "lazy" = never synchronise, detect an
    overflowed arena at a LATER call of the shape, as soon as the GPU has been through the overflowed one (that call raises: the
    image before it missed entries; the arena has been grown for the calls after it); "auto" (what loops that own their error
    handling ask for: bench.py's stress step) = True for the first call of a shape, which also sizes the arena with 50 % headroom
    over that call's count, lazy afterwards; False = no check.
    `plans` (the autograd path, small path only): a dict that keeps the validated C-ABI argument block of a call; while the same
    parameter tensors and switches come back, a call allocates its four FRESH tensors (outputs + geometry scratch: they belong to
    the caller's autograd graph), patches their pointers into a copy of the block and launches -- no re-validation."""
    lib = _lib.load()
    key = None
    if features is not None and features.numel() and means3D is not None and means3D.dim() == 2 and means3D.shape[0] \
            and features.numel() // means3D.shape[0] > _lib.SKS_MAX_CHANNELS:
        return _forward_views_wide(views, means3D, features, opacities, scales, rotations, cov3D_precomp, scale_modifier, antialiasing,
                                   clamp01, debug, force_binned, bin_capacity, want_aux, tune_flags, check_capacity)
    if not want_aux and (workspace is not None or plans is not None):
        # the same call as a recorded one (same tensors, same switches)?  Then the validated argument list is replayed as is.
        key = _fwd_key(views, means3D, features, opacities, scales, rotations, cov3D_precomp, scale_modifier, antialiasing,
                       clamp01, debug, force_binned, bin_capacity, tune_flags, check_capacity)
    if key is not None and workspace is None:
        hit = plans.get(key)
        if hit is not None:
            args_t, dev_index, dev, (V, P, C, H, W, gbytes, flags) = hit
            color = torch.empty((V, C, H, W), dtype=torch.float32, device=dev)
            invdepth = torch.empty((V, 1, H, W), dtype=torch.float32, device=dev)
            radii = torch.empty((V, P), dtype=torch.int32, device=dev)
            geom = torch.empty((gbytes,), dtype=torch.uint8, device=dev)
            args = list(args_t)
            args[_F_COLOR], args[_F_INVDEPTH], args[_F_RADII], args[_F_GEOM] = color.data_ptr(), invdepth.data_ptr(), radii.data_ptr(), geom.data_ptr()
            _lib.check(_replay(lib.sks_forward, args, dev_index), "sks_forward")
            st = ForwardState(views, P, C, flags, scale_modifier, radii, geom)
            st.plan_key = key
            return color, invdepth, radii, st
    if workspace is not None:
        workspace.settle()
    if key is not None and workspace is not None:
        plan = workspace._plans.get("fwd")
        if plan is not None and plan.key == key:
            pf = workspace._pf
            if pf is not None:      # (small path, two output sets)
                rc = _forward_two_sets(lib, workspace, pf, plan)
                if rc != 0:
                    del workspace._plans["fwd"]
                    workspace._pf = None
                _lib.check(rc, "sks_forward")
                return pf.results[pf.cur]
            ticket = _replay_ticket(workspace, plan)
            rc = _replay(lib.sks_forward, plan.args, plan.dev_index)
            if rc != 0:
                del workspace._plans["fwd"]
            _lib.check(rc, "sks_forward")
            if ticket is None or (_arena.finish(ticket) or 0) <= ticket.cap:      # (a lazy ticket is looked at by a later call)
                return plan.result
            del workspace._plans["fwd"]      # the synchronous check: the arena overflowed, the validating path below grows it and redoes
    if workspace is not None and workspace._pf is not None:
        workspace._pf.note = None        # the validating path writes the first set whatever `cur` is: no promise about either survives
    if views.mixed:
        raise RuntimeError("the dense forward writes one (V,C,H,W) tensor: all views of the batch must share the image size")
    if means3D is None or means3D.dim() != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")  # DGR/rasterize_points.cu:58-60
    _need_gpu(means3D, "means3D")
    if means3D.shape[0] == 0:   # DGR/rasterize_points.cu:88: nothing is rasterised, the outputs stay zero
        dev, V, W, H = means3D.device, views.V, views.W, views.H
        C = int(features.shape[-1])
        st = ForwardState(views, 0, C, 0, scale_modifier, torch.zeros((V, 0), dtype=torch.int32, device=dev))
        out = (torch.zeros((V, C, H, W), device=dev), torch.zeros((V, 1, H, W), device=dev), st.radii, st)
        if want_aux:
            out += (torch.ones((V, H, W), device=dev), torch.zeros((V, H, W), dtype=torch.int32, device=dev))
        return out
    means3D, features, opacities, scales, rotations, cov3D_precomp = _f32c_params(means3D, features, opacities, scales, rotations, cov3D_precomp)
    dev = means3D.device
    P = means3D.shape[0]
    feat2 = features.reshape(P, -1)
    C = feat2.shape[1]
    V, W, H = views.V, views.W, views.H
    flags = (_lib.SKS_ANTIALIASING if antialiasing else 0) | (_lib.SKS_CLAMP01 if clamp01 else 0) | \
            (_lib.SKS_DEBUG_SYNC if debug else 0) | (_lib.SKS_FORCE_BINNED if force_binned else 0) | int(tune_flags) | _ENV_TUNE
    if plans is not None and workspace is None and AUTOTUNE and not flags & _FILL_BITS and not _MEASURING[0] and not force_binned \
            and (dev.index, V, P, C, W, H, "fresh") not in _FILL_TUNE:
        # the autograd path sees a shape for the first time: its fill configuration is measured once (tune_forward), on this call's
        # own tensors -- every later call of the shape, recorded or not, launches with the pick
        tune_forward(views, means3D, feat2, opacities, scales, rotations, cov3D_precomp, scale_modifier, antialiasing, clamp01,
                     tune_flags=tune_flags)
    if not flags & _FILL_BITS and not _MEASURING[0]:      # no explicit fill configuration: what tune_forward / Workspace.tune measured for this shape, if anything
        flags |= _FILL_TUNE.get((dev.index, V, P, C, W, H, "workspace" if workspace is not None else "fresh"), 0)
    binned = force_binned or P > _lib.SKS_SMALL_P
    # (the ticket of the arena's capacity check, _arena: a lazy one looks at earlier calls first and raises when one of them overflowed)
    ticket = _arena.begin((dev.index, V, P, C, W, H), bin_capacity, check_capacity, torch.cuda.is_current_stream_capturing()) if binned else None
    cap = ticket.cap if binned else int(bin_capacity or 0)
    gbytes, bbytes, _ = _scratch_bytes_cached(V, max(P, 1), C, W, H, cap)
    def new(name, shape, dtype):
        if workspace is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        return workspace.get(("fwd", name), shape, dtype, dev)

    color = new("color", (V, C, H, W), torch.float32)
    invdepth = new("invdepth", (V, 1, H, W), torch.float32)
    radii = new("radii", (V, P), torch.int32)
    geom = new("geom", (gbytes,), torch.uint8)
    binning = new("binning", (bbytes,), torch.uint8) if binned else None
    # (the pair counts, [0, V) written by k_bin_scan: in the ticket's host buffer, or in a device tensor)
    nrend = None if not binned else new("nrend", (V + 1,), torch.int32) if ticket.device else ticket.host
    final_T = torch.empty((V, H, W), dtype=torch.float32, device=dev) if want_aux else None
    n_contrib = torch.empty((V, H, W), dtype=torch.int32, device=dev) if want_aux else None
    args = [V, P, C, W, H, views.viewmatrix.data_ptr(), views.projmatrix.data_ptr(), views.tanfovx,
            views.tanfovy, _lib.ptr(means3D), _lib.ptr(feat2), _lib.ptr(opacities), _lib.ptr(scales),
            _lib.ptr(rotations), _lib.ptr(cov3D_precomp), float(scale_modifier), flags,
            color.data_ptr(), invdepth.data_ptr(), _lib.ptr(radii), geom.data_ptr(),
            _lib.ptr(binning), cap, _lib.ptr(nrend), _lib.ptr(final_T), _lib.ptr(n_contrib), None]
    _lib.check(_replay(lib.sks_forward, args, dev.index), "sks_forward")
    if binned:
        need = _arena.finish(ticket, nrend)      # (None: nobody has looked yet)
        if need is not None and need > cap:      # entries beyond the arena were dropped: redo with a larger one
            return forward_views(views, means3D, features, opacities, scales, rotations, cov3D_precomp, scale_modifier,
                                 antialiasing, clamp01, debug, force_binned, _arena.grown(need), want_aux, tune_flags,
                                 check_capacity, workspace)
    st = ForwardState(views, P, C, flags, scale_modifier, radii, geom, binning, cap, nrend)
    if want_aux:
        return color, invdepth, radii, st, final_T, n_contrib
    if key is None or not _recordable(key):
        return color, invdepth, radii, st
    if workspace is None:
        if not binned and P:
            if len(plans) > 64:
                plans.clear()
            # (the block keeps the parameter tensors' pointers: `keep` holds the tensors so that the pointers stay theirs)
            plans[key] = _Block(list(args), dev.index, dev, (V, P, C, H, W, gbytes, flags))
            plans[("keep", key)] = (views, means3D, feat2, opacities, scales, rotations, cov3D_precomp)
            st.plan_key = key
    elif not torch.cuda.is_current_stream_capturing():
        # (the tensors the pointers belong to stay alive in `keep`; the views object is held so that its id stays its own)
        keep = (means3D, feat2, opacities, scales, rotations, cov3D_precomp)
        # (the binning buffer needs no clearing between calls: every counter is written before it is read)
        arena = (ticket.key, cap, True if check_capacity is True else "lazy") if binned and check_capacity else None
        workspace._plans["fwd"] = _FwdRecord(key, (views, keep), args, dev.index, (color, invdepth, radii, st), arena)
        workspace._pf = None
        if not binned and P and not workspace._pf_off and _lib.HAS_PREFILL and 4 * (C + 1) * V * H * W <= _PREFILL_MAX_SET_BYTES:
            workspace._pf = _Prefill((V, P, C, W, H), color, invdepth, radii, st, args)
    else:      # (a captured call: the graph holds these pointers from now on)
        workspace._pf_off = True
    return color, invdepth, radii, st


def _forward_two_sets(lib, workspace, pf, plan):
    """A replayed small-path forward of a workspace with two output sets: into the other set with its noted planes taken as zero
    (sks_forward_prefilled; the sets swap), or into `cur` with everything filled (sks_forward).  The record's block keeps pointing
    at `cur`: forward_backward_views, Workspace.tune and bench.py read it."""
    note, pf.note = pf.note, None
    args = plan.args
    if note is not None:
        if workspace._pf_off or torch.cuda.is_current_stream_capturing():
            workspace._pf_off = True
        elif note[1] == torch._C._cuda_getCurrentRawStream(plan.dev_index):
            other = 1 - pf.cur
            color, invdepth = pf.sets[other]
            fargs = pf.fargs
            fargs[_F_FLAGS], fargs[_F_COLOR], fargs[_F_INVDEPTH], fargs[-2] = args[_F_FLAGS], color.data_ptr(), invdepth.data_ptr(), note[0]
            rc = _replay(lib.sks_forward_prefilled, fargs, plan.dev_index)
            if rc == 0:
                pf.cur = other
                args[_F_COLOR], args[_F_INVDEPTH] = fargs[_F_COLOR], fargs[_F_INVDEPTH]
            return rc
    elif not workspace._pf_off and torch.cuda.is_current_stream_capturing():
        workspace._pf_off = True
    return _replay(lib.sks_forward, args, plan.dev_index)


def _backward_prefill(lib, workspace, plan):
    """A replayed backward of the workspace's recorded small-path forward: sks_backward_prefill zeroing the last planes of the set
    the next forward renders into (and the note for that forward), or None where this call does not prefill."""
    pf = workspace._pf
    if pf is None or workspace._pf_off or plan.key[0] != id(pf.results[0][3]):
        return None
    if torch.cuda.is_current_stream_capturing():
        workspace._pf_off, pf.note = True, None
        return None
    fplan = workspace._plans.get("fwd")
    if fplan is None:
        return None
    fflags = fplan.args[_F_FLAGS]
    n = pf.rule.get(fflags)
    if n is None:
        V, P, C, W, H = pf.shape
        # (the counts are the FORWARD's: its live flags hold the store kind and the early region the rule leaves room for)
        n = pf.rule[fflags] = _lib.prefill_planes(V, P, C, W, H, fflags) if workspace._prefill is None else workspace._prefill
    if workspace._prefill is None and plan.args[_B_DFEAT] is not None:
        return None      # (the feature-gradient instantiations run 1-3 waves per SIMD: not what the rule's constants were measured on)
    if n[0] + n[1] == 0:
        return None
    if pf.sets[1] is None:      # the first prefilling backward allocates the second set
        color, invdepth, radii, st = pf.results[0]
        c2 = workspace.get(("fwd", "color2"), color.shape, color.dtype, color.device)
        i2 = workspace.get(("fwd", "invdepth2"), invdepth.shape, invdepth.dtype, invdepth.device)
        pf.sets[1], pf.results[1] = (c2, i2), (c2, i2, radii, st)
    if pf.bplan is not plan:
        pf.bplan, pf.bargs = plan, list(plan.args[:-1]) + [None, None, 0, 0, None]
    color, invdepth = pf.sets[1 - pf.cur]
    bargs = pf.bargs
    bargs[-5], bargs[-4], bargs[-3], bargs[-2] = color.data_ptr(), invdepth.data_ptr(), n[0], n[1]
    pf.note = None
    rc = _replay(lib.sks_backward_prefill, bargs, plan.dev_index)
    if rc == 0:
        pf.note = (n[0] + n[1], bargs[-1])
    return rc


def _replay_ticket(workspace, plan):
    """In front of a REPLAYED binned forward: its ticket (None: the arena is not checked), the call's pair counts patched into the
    record's block and state.  A lazy ticket looks at earlier calls first: when one of them overflowed the arena the record holds,
    the record is dropped -- the next call takes the validating path and allocates the grown one -- and the call raises."""
    if plan.arena is None:
        return None
    try:
        ticket = _arena.begin(*plan.arena, torch.cuda.is_current_stream_capturing())
    except RuntimeError:
        workspace._plans.pop("fwd", None)
        raise
    plan.args[_F_NUM_RENDERED] = _lib.ptr(ticket.host)
    plan.result[3].num_rendered_dev = ticket.host
    return ticket


def _forward_views_wide(views, means3D, features, opacities, scales, rotations, cov3D_precomp, scale_modifier, antialiasing, clamp01,
                        debug, force_binned, bin_capacity, want_aux, tune_flags, check_capacity):
    """Any number of channels ("any C via a generic path").  The kernels hold a pixel's channels in registers,
    SKS_MAX_CHANNELS at most; the channels of a Gaussian splat are independent given its alpha, so a wider feature row is rendered
    as ceil(C / 32) calls per view on 32-channel slices of the features, each writing its own planes: the same arithmetic per
    channel as one wide call would do (the oracle, which takes any C, is the judge: bit for bit).  The backward is linear in the
    channels (dL/dalpha is a sum over them): the slices' gradients add up.  A generic path, not a fast one: one launch sequence
    per (view, slice), outputs copied into place."""
    if want_aux:
        raise RuntimeError("final_T / n_contrib are not available beyond SKS_MAX_CHANNELS channels")
    if views.mixed:
        raise RuntimeError("the dense forward writes one (V,C,H,W) tensor: all views of the batch must share the image size")
    _need_gpu(means3D, "means3D")
    P = means3D.shape[0]
    feat2 = _f32c(features, "features").reshape(P, -1)
    C, V, W, H, dev = feat2.shape[1], views.V, views.W, views.H, means3D.device
    M = _lib.SKS_MAX_CHANNELS
    color = torch.empty((V, C, H, W), dtype=torch.float32, device=dev)
    invdepth = torch.empty((V, 1, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((V, P), dtype=torch.int32, device=dev)
    st = ForwardState(views, P, C, 0, scale_modifier, radii)
    st.chunks = []
    for v in range(V):
        one = ViewBatch(views.viewmatrix[v:v + 1], views.projmatrix[v:v + 1], [views.tanfovx[v]], [views.tanfovy[v]], W, H)
        for c0 in range(0, C, M):
            c1 = min(C, c0 + M)
            fc = feat2[:, c0:c1].contiguous()
            col, inv, rad, sub = forward_views(one, means3D, fc, opacities, scales, rotations, cov3D_precomp, scale_modifier,
                                               antialiasing, clamp01, debug, force_binned, bin_capacity, False, tune_flags, check_capacity)
            color[v, c0:c1].copy_(col[0])
            if c0 == 0:
                invdepth[v].copy_(inv[0])
                radii[v].copy_(rad[0])
            st.chunks.append((v, c0, c1, fc, sub))
    return color, invdepth, radii, st


def _backward_views_wide(st, means3D, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dinvdepth, bg, want_dfeatures,
                         tune_flags):
    dev, V, P, C = means3D.device, st.views.V, st.P, st.C
    dL_dcolor = _f32c(dL_dcolor, "dL_dout_color").reshape(V, C, st.views.H, st.views.W)
    dL_dinvdepth = _f32c(dL_dinvdepth, "dL_dout_invdepth")
    out = _grad_dict(_fresh(torch.zeros, dev), V, P, C, scales is not None and scales.numel(),
                     rotations is not None and rotations.numel(), want_dfeatures)
    bgC = _bg_channels(bg, C, dev)
    for v, c0, c1, fc, sub in st.chunks:
        g = backward_views(sub, means3D, fc, opacities, scales, rotations, cov3D_precomp, dL_dcolor[v:v + 1, c0:c1],
                           None if (dL_dinvdepth is None or c0) else dL_dinvdepth.reshape(V, 1, st.views.H, st.views.W)[v:v + 1],
                           None if bgC is None else bgC[c0:c1], want_dfeatures, tune_flags)
        for k in ("means3D", "means2D", "opacities", "cov3D", "scales", "rotations"):
            if out[k] is not None:
                out[k][v] += g[k][0]
        if want_dfeatures:
            out["features"][v, :, c0:c1] = g["features"][0]
    return out


def _fwd_key(views, means3D, features, opacities, scales, rotations, cov3D_precomp, scale_modifier, antialiasing, clamp01, debug,
             force_binned, bin_capacity, tune_flags, check_capacity):
    return (id(views), (_sig(means3D), _sig(features), _sig(opacities), _sig(scales), _sig(rotations), _sig(cov3D_precomp)),
            scale_modifier, antialiasing, clamp01, debug, force_binned, bin_capacity, tune_flags, check_capacity)


def _bwd_key(st, means3D, features, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dinvdepth, bg, want_dfeatures,
             tune_flags, want_mean, out_means3D, stream):
    return (id(st), (_sig(means3D), _sig(features), _sig(opacities), _sig(scales), _sig(rotations), _sig(cov3D_precomp),
                     _sig(dL_dcolor), _sig(dL_dinvdepth)), None if bg is None else (id(bg), bg._version), want_dfeatures, tune_flags,
            want_mean, None if out_means3D is None else out_means3D.data_ptr(), stream)   # (the partial-sum scratch is per stream)


def _recordable(key):
    """Every tensor of the call is one whose pointer a record may hold: a key's second element is the tuple of its tensors' _sig."""
    _owner, sigs, *_switches = key
    return all(sg is not False for sg in sigs)


def backward_views(st: ForwardState, means3D, features, opacities, scales, rotations, cov3D_precomp, dL_dcolor,
                   dL_dinvdepth=None, bg=None, want_dfeatures=False, tune_flags=0, workspace=None, want_mean=False,
                   out_means3D=None, plans=None):
    """Raw batched backward: per-view gradients, dict of (V,P,...) tensors (`workspace`: see Workspace).  `want_mean`: also
    "means3D_mean" (P,3), the mean of the joint gradients over the views (train.py:215-217), formed inside the library.
    `out_means3D`: a contiguous fp32 (V,P,3) tensor to receive "means3D" (a view-sharded caller passes the rows of its
    all_gather shard: no copy between the backward and the exchange)."""
    lib = _lib.load()
    key = pkey = None
    if st.chunks is not None:
        if want_mean or out_means3D is not None:
            raise RuntimeError("want_mean / out_means3D are not available beyond SKS_MAX_CHANNELS channels")
        return _backward_views_wide(st, means3D, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dinvdepth, bg,
                                    want_dfeatures, tune_flags)
    if plans is not None and workspace is None and st.plan_key is not None and out_means3D is None and not want_mean \
            and _sig(dL_dcolor) is not False and (dL_dinvdepth is None or _sig(dL_dinvdepth) is not False):
        # (the autograd path: same parameter tensors as the recorded forward, gradient tensors fresh every call)
        stream = torch._C._cuda_getCurrentRawStream(st.geom.device.index)
        pkey = ("bwd", st.plan_key, dL_dcolor.shape, dL_dinvdepth is None, None if bg is None else (id(bg), bg._version),
                want_dfeatures, tune_flags, stream)
        hit = plans.get(pkey)
        if hit is not None:
            args_t, dev_index, dev, shape = hit
            out = _grad_dict(_fresh(torch.empty, dev), *shape, want_dfeatures)
            args = list(args_t)
            args[_B_RADII], args[_B_GEOM], args[_B_DL_COLOR], args[_B_DL_INVDEPTH] = \
                st.radii.data_ptr(), st.geom.data_ptr(), dL_dcolor.data_ptr(), _lib.ptr(dL_dinvdepth)
            for k, i in _GRAD_SLOTS:
                g = out[k]
                args[i] = None if g is None else g.data_ptr()
            rc = _replay(lib.sks_backward, args, dev_index)
            if rc != 0:
                reset_scratch()
                plans.pop(pkey, None)
            _lib.check(rc, "sks_backward")
            return out
    if workspace is not None:
        workspace.settle()
    if workspace is not None and st.P:
        key = _bwd_key(st, means3D, features, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dinvdepth, bg,
                       want_dfeatures, tune_flags, want_mean, out_means3D, torch._C._cuda_getCurrentRawStream(st.geom.device.index))
        plan = workspace._plans.get("bwd")
        if plan is not None and plan.key == key:
            rc = _backward_prefill(lib, workspace, plan)
            if rc is None:
                rc = _replay(lib.sks_backward, plan.args, plan.dev_index)
            if rc != 0:
                reset_scratch()
                del workspace._plans["bwd"]
            _lib.check(rc, "sks_backward")
            return plan.result
    if st.P == 0:
        dev = means3D.device
        empty = _grad_dict(_fresh(torch.zeros, dev), st.views.V, 0, st.C, True, True, want_dfeatures)
        if want_mean:
            empty["means3D_mean"] = torch.zeros((0, 3), dtype=torch.float32, device=dev)
        return empty
    means3D, features, opacities, scales, rotations, cov3D_precomp = _f32c_params(means3D, features, opacities, scales, rotations, cov3D_precomp)
    dev = means3D.device
    V, P, C, W, H = st.views.V, st.P, st.C, st.views.W, st.views.H
    feat2 = features.reshape(P, -1)
    dL_dcolor, dL_dinvdepth = _f32c(dL_dcolor, "dL_dout_color"), _f32c(dL_dinvdepth, "dL_dout_invdepth")
    if dL_dcolor.numel() != V * C * H * W:
        raise RuntimeError("dL_dout_color has the wrong number of elements")
    bgC = _bg_channels(bg, C, dev)
    e = _fresh(torch.empty, dev) if workspace is None else lambda name, *s: workspace.get(("bwd", name), s, torch.float32, dev)
    out = _grad_dict(e, V, P, C, scales is not None, rotations is not None, want_dfeatures)
    if want_mean:
        out["means3D_mean"] = e("m3mean", P, 3)
    if out_means3D is not None:
        if tuple(out_means3D.shape) != (V, P, 3) or out_means3D.dtype != torch.float32 or not out_means3D.is_contiguous() \
                or out_means3D.device != dev:
            raise ValueError(f"out_means3D must be a contiguous fp32 (V,P,3) = {(V, P, 3)} tensor on {dev}")
        out["means3D"] = out_means3D
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    accum = _accum(dev, stream, V, P, C)
    args = [V, P, C, W, H, st.views.viewmatrix.data_ptr(), st.views.projmatrix.data_ptr(),
            st.views.tanfovx, st.views.tanfovy, _lib.ptr(bgC), _lib.ptr(means3D), _lib.ptr(feat2),
            _lib.ptr(opacities), _lib.ptr(scales), _lib.ptr(rotations), _lib.ptr(cov3D_precomp),
            st.scale_modifier, st.flags | int(tune_flags), _lib.ptr(st.radii), st.geom.data_ptr(), _lib.ptr(st.binning),
            st.bin_capacity, dL_dcolor.data_ptr(), _lib.ptr(dL_dinvdepth), accum.data_ptr(),
            _lib.ptr(out["means3D"]), _lib.ptr(out["means2D"]), _lib.ptr(out["opacities"]),
            _lib.ptr(out["scales"]), _lib.ptr(out["rotations"]), _lib.ptr(out["cov3D"]),
            _lib.ptr(out["features"]), _lib.ptr(out.get("means3D_mean")), None]
    rc = _replay(lib.sks_backward, args, dev.index)
    if rc != 0:
        reset_scratch()
    _lib.check(rc, "sks_backward")
    if key is not None and _recordable(key) and not torch.cuda.is_current_stream_capturing():
        keep = (st, means3D, feat2, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dinvdepth, bg, bgC, accum)
        workspace._plans["bwd"] = _BwdRecord(key, keep, args, dev.index, out)
    if pkey is not None and st.binning is None:
        plans[pkey] = _Block(list(args), dev.index, dev, (V, P, C, scales is not None, rotations is not None))
        plans[("keep", pkey)] = (bg, bgC, accum)
    return out


def forward_backward_views(views: ViewBatch, means3D, features, opacities, scales, rotations, cov3D_precomp, dL_dcolor,
                           dL_dinvdepth=None, bg=None, scale_modifier=1.0, antialiasing=False, clamp01=False, want_dfeatures=False,
                           tune_flags=0, workspace=None, want_mean=False, out_means3D=None, overlap=True, join=True,
                           force_binned=False, bin_capacity=None, check_capacity=True):
    """forward_views + backward_views of the same inputs as ONE C-ABI call (sks_forward_backward), for a caller whose upstream
    gradient `dL_dcolor` is complete when the call is made -- it does not depend on the image this call renders.  Returns
    (color, invdepth, radii, state, grads): the same tensors, bit for bit, the two calls return.  On the small path (P <= 256) the
    backward's launches go to the workspace's second stream, ordered behind the geometry kernel, and run BESIDE the dense
    forward (include/skelsplat_hip.h); everything is the caller's in current-stream order when the call returns.  Needs a
    Workspace: its first call of a shape IS the two separate calls (they validate, allocate and record their argument lists), the
    later ones replay both records through the combined entry point.  overlap=False: the combined entry point, one stream.
    join=False: the current stream is NOT made to wait for the backward; the caller enqueues what follows the gradients -- a
    view-sharded step's collective -- on `workspace.aux_stream(dev)` (under the forward, too) and then calls `workspace.join(dev)`.
    Whatever path the call takes, with join=False the gradients are ordered on the second stream when it returns, so the
    same caller code is right everywhere: where the halves run one after the other on the current stream (the first call of a
    shape, P == 0, debug, the binned path in one view group, overlap=False) the second stream is made to wait for it -- by the
    library (sks_forward_backward with SKS_FB_NO_JOIN) or, where no second stream reaches the library, here."""
    if workspace is None:
        raise ValueError("forward_backward_views needs a Workspace (outputs, scratch and the second stream live there)")
    lib = _lib.load()
    workspace.settle()
    fplan, bplan = workspace._plans.get("fwd"), workspace._plans.get("bwd")
    if fplan is not None and bplan is not None:
        dev_index = fplan.dev_index
        fkey = _fwd_key(views, means3D, features, opacities, scales, rotations, cov3D_precomp, scale_modifier, antialiasing, clamp01,
                        False, force_binned, bin_capacity, tune_flags, check_capacity)
        if fplan.key == fkey:
            _color, _invdepth, _radii, st = fplan.result
            bkey = _bwd_key(st, means3D, features, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dinvdepth, bg,
                            want_dfeatures, tune_flags, want_mean, out_means3D, torch._C._cuda_getCurrentRawStream(dev_index))
            if bplan.key == bkey:
                aux = workspace.aux_stream(dev_index) if (overlap or not join) else None
                # (a binned forward keeps its capacity check: the ticket is drawn in front of the call and handed back behind it -- on
                # the binned path the library runs the backward of a view group beside the forward of the next one, SKS_BIN_GROUPS)
                ticket = _replay_ticket(workspace, fplan)
                no_join = overlap and not join
                # (rebuilt from the LIVE blocks on every call: Workspace.tune and callers change the forward record's flags between calls)
                args = list(_FB_GATHER(fplan.args + bplan.args))
                args[_FB_AUX_STREAM], args[_FB_FLAGS] = aux.cuda_stream if overlap else None, _lib.SKS_FB_NO_JOIN if no_join else 0
                rc = _replay(lib.sks_forward_backward, args, dev_index, _FB_STREAM)
                if rc != 0:
                    reset_scratch()
                    workspace._plans.pop("fwd", None), workspace._plans.pop("bwd", None)
                _lib.check(rc, "sks_forward_backward")
                if no_join:
                    workspace._pending_join = dev_index     # (the caller's workspace.join(); settled by the next call otherwise)
                if not join and not overlap:     # (the gradients were produced on the current stream: aux must see them)
                    aux.wait_stream(torch.cuda.current_stream(dev_index))
                if ticket is None or (_arena.finish(ticket) or 0) <= ticket.cap:
                    # (two output sets: the record's block points at `cur`, the set this call rendered; the other set and a note
                    # about it are untouched)
                    pf = workspace._pf
                    return (fplan.result if pf is None else pf.results[pf.cur]) + (bplan.result,)
                del workspace._plans["fwd"]     # the arena overflowed (synchronous check): the two calls below grow it and redo the step
                workspace.settle()
    out = forward_views(views, means3D, features, opacities, scales, rotations, cov3D_precomp, scale_modifier, antialiasing, clamp01,
                        force_binned=force_binned, bin_capacity=bin_capacity, check_capacity=check_capacity,
                        tune_flags=tune_flags, workspace=workspace)
    g = backward_views(out[3], means3D, features, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dinvdepth, bg,
                       want_dfeatures, tune_flags, workspace, want_mean, out_means3D)
    if not join:
        workspace.aux_stream(means3D.device.index).wait_stream(torch.cuda.current_stream(means3D.device))
    return out + (g,)


def tune_forward(views, means3D, features, opacities, scales, rotations, cov3D_precomp, scale_modifier=1.0, antialiasing=False,
                 clamp01=False, tune_flags=0, reps=6, rounds=3, rotate=4):
    """The fill configuration for callers whose outputs are FRESH tensors every call (the autograd path: GaussianRasterizer,
    render_*; MultiViewLoop's dense step): times sks_forward of this very call over `rotate` output sets in turn (memory the
    kernel has not just written), non-temporal candidates only, and keeps the pick for the shape -- forward_views then uses it
    whenever a caller of that shape passes no fill bits of its own.  Small path only (the binned path's fill geometry has its own
    measured default).  ~100 forwards and a few device synchronisations, once per shape.  Returns the flag bits."""
    P = means3D.shape[0]
    dev = means3D.device
    feat2 = features.reshape(P, -1)
    C = feat2.shape[1]
    key = (dev.index, views.V, P, C, views.W, views.H, "fresh")
    if key in _FILL_TUNE:
        return _FILL_TUNE[key]
    if torch.cuda.is_current_stream_capturing():
        return 0
    _FILL_TUNE[key] = 0      # (the measuring calls below must not recurse into a measurement; shapes without one keep the default)
    if P == 0 or P > _lib.SKS_SMALL_P or C > _lib.SKS_MAX_CHANNELS:
        return 0
    wss = [Workspace() for _ in range(rotate)]
    state = {"bits": 0, "i": 0}

    def step():
        ws = wss[state["i"] % rotate]
        state["i"] += 1
        forward_views(views, means3D, feat2, opacities, scales, rotations, cov3D_precomp, scale_modifier, antialiasing, clamp01,
                      tune_flags=(int(tune_flags) & ~_FILL_BITS) | state["bits"], workspace=ws)

    def set_bits(bits):
        state["bits"] = bits
    _MEASURING[0] = True      # (candidate 0 means "no bits": the measuring calls must get exactly what they ask for)
    try:
        with torch.no_grad():
            times = _time_candidates(set_bits, step, TUNE_CANDIDATES_FRESH, reps, rounds, dev.index, warm=2 * rotate)
            best, med = _pick(times, TUNE_CANDIDATES_FRESH, set_bits, step, reps, dev.index)
    finally:
        _MEASURING[0] = False
    _FILL_TUNE[key] = _tune_flag_bits(best)
    _FILL_TUNE_LOG[key] = {tune_name(c): round(v, 2) for c, v in med.items()}
    return _FILL_TUNE[key]


def mean_views(grads, V, world=1, out=None):
    """Mean over the V views of (rows,P,3) joint gradients, summed in view order (train.py:215-217).  world > 1: `grads` is
    what all_gather_into_tensor left for a view-sharded group (world * ceil(V / world) rows, rank-major)."""
    vmax = (V + world - 1) // world
    P = grads.shape[1]
    if grads.dtype != torch.float32 or not grads.is_contiguous() or grads.shape[0] < (V if world == 1 else world * vmax) \
            or grads.shape[2] != 3:
        raise ValueError("mean_views: grads must be a contiguous fp32 (rows,P,3) tensor with a row for every view")
    _need_gpu(grads, "grads")
    if out is None:
        out = torch.empty((P, 3), dtype=torch.float32, device=grads.device)
    rc = _lib.load().sks_mean_views(V, P, grads.data_ptr(), world, out.data_ptr(),
                                    torch._C._cuda_getCurrentRawStream(grads.device.index))
    _lib.check(rc, "sks_mean_views")
    return out


def export_lists(st: ForwardState):
    """Parity/debug: (point_list (V,cap) int32, ranges (V,Tx*Ty,2) int32, num_rendered (V,) int32) of the binned path."""
    lib = _lib.load()
    if st.binning is None:
        raise RuntimeError("lists exist only on the binned path (force_binned=True)")
    dev = st.geom.device
    V, W, H = st.views.V, st.views.W, st.views.H
    NT = ((W + 15) // 16) * ((H + 15) // 16)
    pl = torch.empty((V, max(st.bin_capacity, 1)), dtype=torch.int32, device=dev)
    rg = torch.empty((V, NT, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sks_export_lists(V, W, H, st.binning.data_ptr(), st.bin_capacity, pl.data_ptr(), rg.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "sks_export_lists")
    # (a lazily checked call keeps its counts in a pinned host buffer, or nowhere: the ranges say the same -- a view's entries
    # end where its last non-empty tile's list ends)
    nr = rg[..., 1].amax(dim=1) if st.num_rendered_dev is None or not st.num_rendered_dev.is_cuda else st.num_rendered_dev[:V]
    return pl, rg, nr


# ------------------------------------------------------------------------------------------------------------
# autograd: single view (the reference's _RasterizeGaussians, __init__.py:44-141) and multi-view
# ------------------------------------------------------------------------------------------------------------
def _features_of(sh, colors_precomp, P):
    # the kernels read features straight from `sh` as flat (P, C) and need M == 1; colors_precomp is
    # ignored by the reference's kernels -- here it is used when no sh is given (the reference would dereference null).
    if sh is not None and sh.numel() > 0:
        if sh.dim() == 3 and sh.shape[1] != 1:
            raise RuntimeError(f"features must have exactly one SH coefficient (M == 1), got shape {tuple(sh.shape)}")
        return sh, "sh"
    if colors_precomp is not None and colors_precomp.numel() > 0:
        return colors_precomp, "colors"
    raise RuntimeError("no features: provide shs (P,1,C) or colors_precomp (P,C)")


_AUTOGRAD_PLANS = {}     # recorded C-ABI argument blocks of the autograd path (forward_views / backward_views `plans`)
if os.environ.get("SKS_AUTOGRAD_PLANS", "1") == "0":      # A/B runs: every call takes the validating path
    _AUTOGRAD_PLANS = None


class _RasterizeViews(torch.autograd.Function):
    """V views of the same Gaussians; outputs (V,C,H,W), (V,P), (V,1,H,W); gradients summed over views."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, views,
                scale_modifier, antialiasing, clamp01, debug, bg, single, raw=False):
        P = means3D.shape[0] if means3D.dim() == 2 else 0
        feats, src = _features_of(sh, colors_precomp, P)
        # raw: opacities / scales / rotations are the LEAF parameters; the kernels run sigmoid / exp / normalize themselves and
        # the backward returns the leaves' gradients (SKS_RAW_PARAMS | SKS_RAW_GRADS): no activation launches around the call
        tune = (_lib.SKS_RAW_PARAMS | _lib.SKS_RAW_GRADS) if raw else 0
        # check_capacity=True: like the reference, which reads the pair count back on every forward, the autograd path never
        # returns an image (and then gradients) with dropped entries -- a too-small arena is grown and the forward redone
        color, invdepth, radii, st = forward_views(views, means3D, feats, opacities, scales, rotations, cov3Ds_precomp,
                                                   scale_modifier, antialiasing, clamp01, debug, check_capacity=True,
                                                   tune_flags=tune, plans=_AUTOGRAD_PLANS)
        ctx.st, ctx.src, ctx.bg, ctx.single = st, src, bg, single
        ctx.save_for_backward(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)  # an unused inverse-depth output costs nothing in backward
        if single:
            return color[0], radii[0], invdepth[0]
        return color, radii, invdepth

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, grad_invdepth):
        means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp = ctx.saved_tensors
        st = ctx.st
        feats = sh if ctx.src == "sh" else colors_precomp
        if grad_color is None:
            V, C, H, W = st.views.V, st.C, st.views.H, st.views.W
            grad_color = torch.zeros((V, C, H, W), dtype=torch.float32, device=means3D.device)
        need_feat = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        g = backward_views(st, means3D, feats, opacities, scales, rotations, cov3Ds_precomp, grad_color, grad_invdepth,
                           ctx.bg, want_dfeatures=need_feat, plans=_AUTOGRAD_PLANS)
        red = (lambda t: None if t is None else t[0]) if st.views.V == 1 else (lambda t: None if t is None else t.sum(0))
        gf = red(g["features"])
        grad_sh = gf.reshape(sh.shape) if (gf is not None and ctx.src == "sh") else None
        grad_cp = gf.reshape(colors_precomp.shape) if (gf is not None and ctx.src == "colors") else None
        has_cov = cov3Ds_precomp is not None and cov3Ds_precomp.numel() > 0
        return (red(g["means3D"]), red(g["means2D"]), grad_sh, grad_cp, red(g["opacities"]).reshape(opacities.shape),
                red(g["scales"]), red(g["rotations"]), red(g["cov3D"]) if has_cov else None,
                None, None, None, None, None, None, None, None)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, clamp01=False, raw_params=False):
    """DGR/diff_gaussian_rasterization_h36m/__init__.py:21-42."""
    views = ViewBatch.from_settings(raster_settings)
    return _RasterizeViews.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                 views, raster_settings.scale_modifier, bool(raster_settings.antialiasing), clamp01,
                                 bool(raster_settings.debug), raster_settings.bg, True, bool(raw_params))


def rasterize_views(views: ViewBatch, means3D, means2D, sh, opacities, scales=None, rotations=None, cov3D_precomp=None,
                    colors_precomp=None, scale_modifier=1.0, antialiasing=False, clamp01=False, debug=False, bg=None):
    """Multi-view autograd entry point (no reference counterpart: the reference renders one view per call)."""
    emp = torch.empty(0)
    z = lambda t: emp if t is None else t
    return _RasterizeViews.apply(means3D, z(means2D), z(sh), z(colors_precomp), opacities, z(scales), z(rotations),
                                 z(cov3D_precomp), views, scale_modifier, antialiasing, clamp01, debug, bg, False)


class GaussianRasterizer(nn.Module):
    """DGR/diff_gaussian_rasterization_h36m/__init__.py:158-207.  `num_channels` pins C like the reference's
    compile-time NUM_CHANNELS (config.h:15); None accepts any C (beyond SKS_MAX_CHANNELS = 32 through the generic path of
    _forward_views_wide: 32-channel slices)."""
    num_channels: Optional[int] = None

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            rs = self.raster_settings
            _need_gpu(positions, "positions")
            pos = positions.contiguous().float()
            P = pos.shape[0]
            present = torch.zeros(P, dtype=torch.bool, device=pos.device)
            if P:
                with torch.cuda.device(pos.device):
                    rc = _lib.load().sks_mark_visible(P, pos.data_ptr(), _f32c(rs.viewmatrix, "viewmatrix").data_ptr(),
                                                      _f32c(rs.projmatrix, "projmatrix").data_ptr(), present.data_ptr(),
                                                      torch.cuda.current_stream(pos.device).cuda_stream)
                _lib.check(rc, "sks_mark_visible")
        return present

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, clamp01=False, raw_params=False):
        """The reference's signature plus two extensions: `clamp01` folds render_*'s clamp(0, 1) into the kernels;
        `raw_params`: `opacities`, `scales`, `rotations` are the model's LEAF parameters (_opacity logits, _scaling log-scales,
        raw _rotation, scene/gaussian_model.py:39-47) -- the activations and their Jacobians run inside the kernels."""
        raster_settings = self.raster_settings
        if raster_settings.prefiltered:
            # the reference's kernels TRAP the device when prefiltered is set and a point fails the frustum test
            # (auxiliary.h:166-174: printf + __trap()); render_* always passes False (gaussian_renderer/__init__.py:56)
            raise RuntimeError("raster_settings.prefiltered=True is refused: the reference aborts the device on the first "
                               "culled point in that mode (auxiliary.h:166-174); pass False (INTEGRATION.md)")
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        if shs is None:
            shs = torch.Tensor([])
        if colors_precomp is None:
            colors_precomp = torch.Tensor([])
        if scales is None:
            scales = torch.Tensor([])
        if rotations is None:
            rotations = torch.Tensor([])
        if cov3D_precomp is None:
            cov3D_precomp = torch.Tensor([])
        if self.num_channels is not None:
            f = shs if shs.numel() else colors_precomp
            if f.shape[-1] != self.num_channels:
                raise RuntimeError(f"this rasterizer package is fixed to NUM_CHANNELS={self.num_channels}, "
                                   f"got features with {f.shape[-1]} channels")
        if raw_params and (scales.numel() == 0 or rotations.numel() == 0):
            raise Exception('raw_params needs the scale/rotation pair (the leaves), not a precomputed 3D covariance')
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   raster_settings, clamp01=clamp01, raw_params=raw_params)


def make_package(num_channels):
    """Class pair for one of the reference's three packages (NUM_CHANNELS 17 / 19 / 15)."""
    cls = type(f"GaussianRasterizer{num_channels}", (GaussianRasterizer,), {"num_channels": num_channels})
    return GaussianRasterizationSettings, cls


def decode_geom(st: ForwardState):
    """Debug/parity view of the forward's per-(view, Gaussian) records: dict of conic_opacity (V,P,4),
    xy (V,P,2), depths (V,P), rect (V,P,4) [xmin,ymin,xmax,ymax in tiles]."""
    V, P = st.views.V, st.P
    n = V * P * 16
    seg = (n + 255) // 256 * 256
    g = st.geom
    co = g[0:n].view(torch.float32).reshape(V, P, 4)
    xyd = g[seg:seg + n].view(torch.float32).reshape(V, P, 4)
    rect = g[2 * seg:2 * seg + n].view(torch.int32).reshape(V, P, 4)
    return dict(conic_opacity=co, xy=xyd[..., :2], depths=xyd[..., 2], rect=rect)
