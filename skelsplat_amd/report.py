"""What the reference reports about a pose while and after it optimises it, on the device (csrc/sks_report.hip):

pose_errors        per-joint absolute and root-relative error against the ground truth and their means (train.py:184-213);
evaluate_sequence  absolute and root-relative MPJPE of a sequence, overall and per group of frames (eval.py:115-142);
align_poses, aligned_pose_errors, evaluate_sequence_aligned
                   the same after the best per-frame rigid / similarity / scale alignment of the prediction onto the ground
                   truth: PA-MPJPE and N-MPJPE, which the reference does not report (csrc/sks_align.hip);
LoopReport         the buffers a FrameBatchLoop reports into -- errors and losses at every optimiser step, the joints at
                   `save_iterations` (train.py:227-229) -- and the one small launch per group that fills them.

Everything takes device tensors, enqueues on the current stream and never synchronises; every result is bitwise reproducible.
The host-side counterparts behind a directory of .ply files are io.mpjpe / io.evaluate, and io.pa_mpjpe / io.n_mpjpe."""
import ctypes

import numpy as np
import torch

from . import _lib


def _poses(pred, gt, what):
    """`pred`, `gt` as contiguous (N,P,3) float32 tensors on one ROCm device (a single (P,3) pose gains the frame axis)."""
    for name, t in (("pred", pred), ("gt", gt)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: `{name}` must be a tensor on a ROCm device (the host-side counterpart is skelsplat_amd.io)")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: `{name}` must be float32, got {t.dtype}")
    if pred.shape != gt.shape or pred.dim() not in (2, 3) or pred.shape[-1] != 3 or pred.numel() == 0:
        raise ValueError(f"{what}: pred and gt must both be (N,P,3) or (P,3), got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.device != gt.device:
        raise ValueError(f"{what}: pred is on {pred.device}, gt on {gt.device}")
    single = pred.dim() == 2
    return (pred[None] if single else pred).contiguous(), (gt[None] if single else gt).contiguous(), single


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def pose_errors(pred, gt, per_joint=False):
    """pred, gt (N,P,3) float32 on the device -> mean (N,2): column 0 the mean over the joints of ||pred - gt||, column 1 of
    ||(pred - pred[0]) - (gt - gt[0])|| (train.py:198-204).  `per_joint=True`: returns (errors (N,P,2), mean).  A (P,3) pose
    gives results without the frame axis.  One launch, one wavefront per frame; a NaN joint poisons its own frame's means."""
    p, g, single = _poses(pred, gt, "pose_errors")
    N, P = p.shape[:2]
    dev = p.device
    mean = torch.empty((N, 2), dtype=torch.float32, device=dev)
    pj = torch.empty((N, P, 2), dtype=torch.float32, device=dev) if per_joint else None
    with torch.cuda.device(dev):
        rc = _lib.load().sks_pose_errors(N, P, p.data_ptr(), g.data_ptr(), None if pj is None else pj.data_ptr(), mean.data_ptr(),
                                         _stream(dev))
    _lib.check(rc, "sks_pose_errors")
    if single:
        mean, pj = mean[0], None if pj is None else pj[0]
    return (pj, mean) if per_joint else mean


def evaluate_sequence(pred, gt, groups=None, n_groups=None, abs_valid=None):
    """eval.py:115-142 on the device: pred, gt (N,P,3) float32 -> dict of float64 device tensors: `abs`, `rel` (0-d: absolute and
    root-relative MPJPE over all frames and joints), `abs_groups`, `rel_groups` ((n_groups,): the same per group; NaN for a group
    without frames).
    `groups` (N,) integer ids in [0, n_groups) -- H36M: the frame's activity -- on the host or the device; `n_groups` <= 64 is
    required with ids on the device (finding their maximum would wait for it).  `abs_valid` (N,) bool: frames with False are
    left out of the absolute figures only (H36M: S9's three broken sequences).  One launch; sums in float64 in a fixed order."""
    p, g, _ = _poses(pred, gt, "evaluate_sequence")
    N, P = p.shape[:2]
    dev = p.device
    ids, G = None, 0
    if groups is not None:
        if torch.is_tensor(groups) and groups.is_cuda:
            if n_groups is None:
                raise ValueError("evaluate_sequence: group ids on the device need n_groups (nothing here waits for the device)")
            if groups.is_floating_point():
                raise ValueError(f"evaluate_sequence: groups must be integers, got {groups.dtype}")
            ids = groups
        else:
            host = np.asarray(groups.cpu() if torch.is_tensor(groups) else groups)
            if host.dtype.kind not in "iu":
                raise ValueError(f"evaluate_sequence: groups must be integers, got {host.dtype}")
            if n_groups is None:
                n_groups = int(host.max()) + 1 if host.size else 0
            ids = torch.as_tensor(host.astype(np.int32))
        if tuple(ids.shape) != (N,):
            raise ValueError(f"evaluate_sequence: groups must be (N,) = ({N},), got {tuple(ids.shape)}")
        ids = ids.to(device=dev, dtype=torch.int32).contiguous()
        G = int(n_groups)
        if not 0 <= G <= _lib.SKS_EVAL_MAX_GROUPS:
            raise ValueError(f"evaluate_sequence: n_groups = {G}, at most {_lib.SKS_EVAL_MAX_GROUPS}")
        if G == 0:
            ids = None
    elif n_groups:
        raise ValueError("evaluate_sequence: n_groups without groups")
    valid = None
    if abs_valid is not None:
        valid = torch.as_tensor(abs_valid)
        if tuple(valid.shape) != (N,):
            raise ValueError(f"evaluate_sequence: abs_valid must be (N,) = ({N},), got {tuple(valid.shape)}")
        valid = valid.to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8)
    out = torch.empty((1 + G, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().sks_eval_sequence(N, P, p.data_ptr(), g.data_ptr(), None if ids is None else ids.data_ptr(), G,
                                           None if valid is None else valid.data_ptr(), out.data_ptr(), _stream(dev))
    _lib.check(rc, "sks_eval_sequence")
    return dict(abs=out[0, 0], rel=out[0, 1], abs_groups=out[1:, 0], rel_groups=out[1:, 1])


def _groups(what, groups, n_groups, N, dev):
    """Group ids as evaluate_sequence takes them -> ((N,) int32 device tensor or None, G)."""
    if groups is None:
        if n_groups:
            raise ValueError(f"{what}: n_groups without groups")
        return None, 0
    if torch.is_tensor(groups) and groups.is_cuda:
        if n_groups is None:
            raise ValueError(f"{what}: group ids on the device need n_groups (nothing here waits for the device)")
        if groups.is_floating_point():
            raise ValueError(f"{what}: groups must be integers, got {groups.dtype}")
        ids = groups
    else:
        host = np.asarray(groups.cpu() if torch.is_tensor(groups) else groups)
        if host.dtype.kind not in "iu":
            raise ValueError(f"{what}: groups must be integers, got {host.dtype}")
        if n_groups is None:
            n_groups = int(host.max()) + 1 if host.size else 0
        ids = torch.as_tensor(host.astype(np.int32))
    if tuple(ids.shape) != (N,):
        raise ValueError(f"{what}: groups must be (N,) = ({N},), got {tuple(ids.shape)}")
    G = int(n_groups)
    if not 0 <= G <= _lib.SKS_EVAL_MAX_GROUPS:
        raise ValueError(f"{what}: n_groups = {G}, at most {_lib.SKS_EVAL_MAX_GROUPS}")
    return (ids.to(device=dev, dtype=torch.int32).contiguous() if G else None), G


ALIGN_MODES = {"rigid": _lib.SKS_ALIGN_RIGID, "similarity": _lib.SKS_ALIGN_SIMILARITY, "scale": _lib.SKS_ALIGN_SCALE}


def _align_args(what, pred, gt, mode, valid):
    """The checks the three aligned entries share -> pred, gt (N,P,3), single, mode number, valid (N,P) uint8 or None."""
    if mode not in ALIGN_MODES:
        raise ValueError(f"{what}: mode = {mode!r}, one of {sorted(ALIGN_MODES)}")
    p, g, single = _poses(pred, gt, what)
    N, P = p.shape[:2]
    v = None
    if valid is not None:
        if not torch.is_tensor(valid) or not valid.is_cuda or valid.device != p.device:
            raise ValueError(f"{what}: `valid` must be a tensor on the poses' device, {p.device}")
        if valid.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"{what}: `valid` must be bool or uint8, got {valid.dtype}")
        if tuple(valid.shape) != ((P,) if single else (N, P)):
            raise ValueError(f"{what}: `valid` must be {'(P,)' if single else '(N,P)'} = {(P,) if single else (N, P)}, "
                             f"got {tuple(valid.shape)}")
        v = valid.reshape(N, P).contiguous()
        v = v.view(torch.uint8) if v.dtype == torch.bool else v
    return p, g, single, ALIGN_MODES[mode], v


def _align(p, g, v, mode, aligned=None, transform=None, per_joint=None, mean=None):
    ptr = lambda t: None if t is None else t.data_ptr()
    N, P = p.shape[:2]
    with torch.cuda.device(p.device):
        rc = _lib.load().sks_align_poses(N, P, p.data_ptr(), g.data_ptr(), ptr(v), mode, ptr(aligned), ptr(transform),
                                         ptr(per_joint), ptr(mean), _stream(p.device))
    _lib.check(rc, "sks_align_poses")


def align_poses(pred, gt, mode="similarity", valid=None, return_transform=False):
    """pred, gt (N,P,3) float32 on the device -> pred after the best per-frame alignment onto gt, (N,P,3) float32.
    `mode`: "rigid" (R, t), "similarity" (s, R, t: the alignment of PA-MPJPE) or "scale" (s alone, both poses relative to joint 0:
    N-MPJPE's).  R is always a proper rotation.  `valid` (N,P) bool or uint8 on the device: the joints the fit uses; every
    joint is transformed.  `return_transform=True`: also (scale (N,), rotation (N,3,3), translation (N,3)), float64 views of one
    (N,13) block, with aligned = scale * rotation @ pred + translation.  A frame without a valid joint keeps pred and the
    identity; a NaN in a valid joint (or, in "scale" mode, a masked joint 0) makes its own frame NaN.  A (P,3) pose gives results
    without the frame axis.  One launch, one wavefront per frame, float64 inside (include/skelsplat_hip.h)."""
    p, g, single, m, v = _align_args("align_poses", pred, gt, mode, valid)
    N = p.shape[0]
    aligned = torch.empty_like(p)
    tr = torch.empty((N, 13), dtype=torch.float64, device=p.device) if return_transform else None
    _align(p, g, v, m, aligned=aligned, transform=tr)
    if not return_transform:
        return aligned[0] if single else aligned
    s, R, t = tr[:, 0], tr[:, 1:10].view(N, 3, 3), tr[:, 10:13]
    return (aligned[0], (s[0], R[0], t[0])) if single else (aligned, (s, R, t))


def aligned_pose_errors(pred, gt, mode="similarity", valid=None, per_joint=False):
    """pred, gt (N,P,3) float32 on the device -> mean (N,) float32: the mean over the valid joints of ||gt - aligned||, aligned as
    align_poses gives it ("similarity": the frame's PA-MPJPE, "scale": its N-MPJPE, "rigid": the rigid-aligned error; NaN for a
    frame without a valid joint).  `per_joint=True`: returns (errors (N,P), mean), the errors of all joints, masked ones
    included.  A (P,3) pose gives results without the frame axis.  One launch."""
    p, g, single, m, v = _align_args("aligned_pose_errors", pred, gt, mode, valid)
    N, P = p.shape[:2]
    mean = torch.empty(N, dtype=torch.float32, device=p.device)
    pj = torch.empty((N, P), dtype=torch.float32, device=p.device) if per_joint else None
    _align(p, g, v, m, per_joint=pj, mean=mean)
    if single:
        mean, pj = mean[0], None if pj is None else pj[0]
    return (pj, mean) if per_joint else mean


def evaluate_sequence_aligned(pred, gt, groups=None, n_groups=None, valid=None):
    """pred, gt (N,P,3) float32 on the device -> dict of float64 device tensors: `pa_mpjpe`, `n_mpjpe` (0-d: the mean over all
    valid joints of all frames of aligned_pose_errors' per-joint errors in "similarity" and in "scale" mode), `pa_mpjpe_groups`,
    `n_mpjpe_groups` ((n_groups,): the same per group; NaN for a group without valid joints).  `groups`, `n_groups` as
    evaluate_sequence takes them; `valid` (N,P) as align_poses takes it.  Three launches; sums in float64 in a fixed order."""
    what = "evaluate_sequence_aligned"
    p, g, _, _, v = _align_args(what, pred, gt, "similarity", valid)
    N, P = p.shape[:2]
    dev = p.device
    ids, G = _groups(what, groups, n_groups, N, dev)
    lib = _lib.load()
    nbytes = lib.sks_eval_sequence_aligned_scratch_bytes(N, P)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((1 + G, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sks_eval_sequence_aligned(N, P, p.data_ptr(), g.data_ptr(), None if v is None else v.data_ptr(),
                                           None if ids is None else ids.data_ptr(), G, scratch.data_ptr(), nbytes, out.data_ptr(),
                                           _stream(dev))
    _lib.check(rc, what)
    return dict(pa_mpjpe=out[0, 0], n_mpjpe=out[0, 1], pa_mpjpe_groups=out[1:, 0], n_mpjpe_groups=out[1:, 1])


def check_report_args(report_steps, save_iterations):
    """FrameBatchLoop's `report_steps`, `save_iterations` -> (capacity, tuple of iterations); anything else is refused."""
    if isinstance(report_steps, bool) or not isinstance(report_steps, (int, np.integer)) or report_steps < 0:
        raise ValueError(f"report_steps = {report_steps!r}: the number of trace rows (initial row included), an integer >= 0")
    saves = tuple(save_iterations)
    if len(saves) > _lib.SKS_REPORT_MAX_SAVES:
        raise ValueError(f"save_iterations: {len(saves)} iterations, at most {_lib.SKS_REPORT_MAX_SAVES} (SKS_REPORT_MAX_SAVES)")
    for s in saves:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 0:
            raise ValueError(f"save_iterations = {save_iterations!r}: every entry is an iteration, an integer >= 0")
    return int(report_steps), tuple(int(s) for s in saves)


def loop_report(counters, es_state, es_window, xyz, gt, loss_sums, acc_steps, trace_err, trace_loss, final_err, save_iterations,
                snaps):
    """One sks_loop_report launch on the current stream (include/skelsplat_hip.h): tensors or None, shapes taken from `xyz`
    (F,P,3), `trace_err` (F,capacity,2) / `trace_loss` (F,capacity,V) and `loss_sums` (F*V,2)."""
    F, P = xyz.shape[:2]
    cap = trace_err.shape[1] if trace_err is not None else trace_loss.shape[1] if trace_loss is not None else 0
    V = trace_loss.shape[2] if trace_loss is not None else 1
    K = len(save_iterations)
    ptr = lambda t: None if t is None else t.data_ptr()
    dev = xyz.device
    with torch.cuda.device(dev):
        rc = _lib.load().sks_loop_report(F, V, P, ptr(counters), ptr(es_state), int(es_window), ptr(xyz), ptr(gt), ptr(loss_sums),
                                         int(acc_steps), cap, ptr(trace_err), ptr(trace_loss), ptr(final_err), K,
                                         ctypes.cast((ctypes.c_int * max(K, 1))(*save_iterations), ctypes.c_void_p), ptr(snaps),
                                         _stream(dev))
    _lib.check(rc, "sks_loop_report")


class LoopReport:
    """The report buffers of one FrameBatchLoop, allocated once (captured graphs keep their addresses), and its launch.
    `steps`: trace rows per frame, the initial row included (0: no traces, no errors); `save_iterations`: K <= 8 iterations.
      gt (F,P,3)             the batch's ground truth (NaN when the caller gave none: the errors are then NaN)
      trace_err (F,steps,2)  row n: mean absolute / root-relative error after n optimiser steps; NaN where the frame never got
      trace_loss (F,steps,V) row n >= 1: every view's loss in the group that led to step n (row 0 has no group: NaN)
      final_err (F,P,2)      per-joint errors of the current joints
      snaps (F,K,P,3)        slot k: the joints at the end of iteration save_iterations[k]; NaN where the frame never got"""

    def __init__(self, F, V, P, steps, save_iterations, device):
        self.steps, self.saves = check_report_args(steps, save_iterations)
        self.F, self.V, self.P, self.K = F, V, P, len(self.saves)
        new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=device)
        on = self.steps > 0
        self.gt = new(F, P, 3) if on else None
        self.trace_err = new(F, self.steps, 2) if on else None
        self.trace_loss = new(F, self.steps, V) if on else None
        self.final_err = new(F, P, 2) if on else None
        self.snaps = new(F, self.K, P, 3) if self.K else None

    def reset(self, gt):
        """The next batch: ground truth copied in place, traces and snapshots back to NaN."""
        for t in (self.trace_err, self.trace_loss, self.final_err, self.snaps):
            if t is not None:
                t.fill_(float("nan"))
        if self.gt is not None:
            if gt is None:
                self.gt.fill_(float("nan"))
            else:
                self.gt.copy_(gt)

    def launch(self, loop, losses=True):
        """Enqueue the report of `loop`'s frames as they stand (losses=False: no group has run yet)."""
        es = loop._es_state
        loop_report(loop.counters, es, 0 if es is None else loop._es[0], loop.xyz, self.gt,
                    loop._sums if losses and self.trace_loss is not None else None, loop.acc_steps, self.trace_err,
                    self.trace_loss if losses else None, self.final_err, self.saves, self.snaps)


class SequenceReport:
    """`optimize_sequence`'s report: the loop's arrays for all N frames of the sequence, filled batch by batch on the batch's own
    stream (like the joints).  trace_errors (N,steps,2), trace_losses (N,steps,V), final_errors (N,P,2), snapshots (N,K,P,3),
    steps (N,) int32; None for what the loop does not report."""

    def __init__(self, loop, N):
        rep, dev = loop._report, loop.device
        like = lambda t: None if t is None else torch.empty((N,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        self.trace_errors, self.trace_losses = like(rep.trace_err), like(rep.trace_loss)
        self.final_errors, self.snapshots = like(rep.final_err), like(rep.snaps)
        self.steps = torch.empty(N, dtype=torch.int32, device=dev)
        self.save_iterations = rep.saves

    def take(self, loop, b, n):
        """Frames b .. b + n of the sequence are the first n frames of `loop`'s batch."""
        rep = loop._report
        for dst, src in ((self.trace_errors, rep.trace_err), (self.trace_losses, rep.trace_loss),
                         (self.final_errors, rep.final_err), (self.snapshots, rep.snaps)):
            if dst is not None:
                dst[b:b + n] = src[:n]
        self.steps[b:b + n] = loop.counters[:n, 1]
