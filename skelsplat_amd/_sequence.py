"""One `optimize_sequence` call of a FrameBatchLoop / FramePipeline as a record (SequenceRun), and the checks of the per-sequence
settings.  Imports nothing from loop.py, which imports from here."""
import numpy as np

import torch


def _sequence_inputs(points, poses_2d):
    """optimize_sequence's (points or None, detections, N): tensors stay where they are, arrays become CPU tensors."""
    p2d = poses_2d if torch.is_tensor(poses_2d) else torch.as_tensor(np.asarray(poses_2d))
    if points is None:
        return None, p2d, p2d.shape[0]
    pts = points if torch.is_tensor(points) else torch.as_tensor(np.asarray(points))
    if p2d.shape[0] != pts.shape[0]:
        raise ValueError(f"{pts.shape[0]} frames of points, {p2d.shape[0]} of detections")
    return pts, p2d, pts.shape[0]


def _rejection(reject_px, min_inliers):
    """set_outlier_rejection's arguments -> None (off) or the checked (reject_px, min_inliers)."""
    if reject_px is None:
        return None
    from .triangulation import _checked_rejection
    return _checked_rejection(reject_px, min_inliers)


def _checked_reject(reject, points, poses_3d, who):
    """`reject`: a loop's set_outlier_rejection setting.  It acts on the triangulation of the initial joints alone: refused
    beside explicit points or poses_3d.  Returns (reject_px or None, min_inliers)."""
    if reject is None:
        return None, 3
    if points is not None:
        raise ValueError(f"{who}: outlier rejection (set_outlier_rejection) acts while the initial joints are triangulated "
                         "(points=None); explicit points are taken as they are -- switch it off with set_outlier_rejection(None)")
    if poses_3d is not None:
        raise ValueError(f"{who}: outlier rejection (set_outlier_rejection) belongs to the triangulation; fusing poses_3d is a "
                         "different estimator and takes every kept view -- switch it off with set_outlier_rejection(None)")
    return reject


def _refinement(max_iters, huber_px):
    """set_refinement's arguments -> None (off) or the checked (huber_px, max_iters)."""
    if max_iters is None:
        return None
    from .reprojection import _checked_refinement
    return _checked_refinement(huber_px, max_iters)


def _checked_refine(refine, points, poses_3d, who):
    """`refine`: a loop's set_refinement setting.  Like the rejection it belongs to the triangulation of the initial joints:
    refused beside explicit points or poses_3d.  Returns it."""
    if refine is None:
        return None
    if points is not None:
        raise ValueError(f"{who}: the refinement (set_refinement) follows the triangulation of the initial joints (points=None); "
                         "explicit points are taken as they are -- switch it off with set_refinement(None)")
    if poses_3d is not None:
        raise ValueError(f"{who}: the refinement (set_refinement) follows the triangulation; fusing poses_3d is a different "
                         "estimator -- switch it off with set_refinement(None)")
    return refine


def _sequence_reprojection(loop, N):
    """optimize_sequence's `reprojection`: None for a loop whose reprojection report is off (set_reprojection_report)."""
    if not getattr(loop, "_reproject", False):
        return None
    from .reprojection import SequenceReprojection
    return SequenceReprojection(N, loop.V, loop.P, loop.device)


def _smoothing(loop, half_window, degree, taper, use_covariance, cov_floor, groups):
    """set_smoothing's arguments -> None (off) or the checked settings as a dict of smoothing.smooth_sequence's keywords plus
    `use_covariance`; `groups` stays as given until a sequence's length is known (_sequence_smoothing)."""
    if half_window is None:
        return None
    from .smoothing import _settings
    h, d, floor, _ = _settings("set_smoothing", half_window, degree, taper, cov_floor)
    if use_covariance and not loop.keep_gaussians:
        raise ValueError("set_smoothing: use_covariance=True weights every frame by the covariance of its optimised Gaussians, which "
                         "this loop does not keep -- build it with FrameBatchLoop / FramePipeline(..., keep_gaussians=True), or "
                         "pass use_covariance=False for unit weights")
    return dict(half_window=h, degree=d, taper=taper, cov_floor=floor, use_covariance=bool(use_covariance), groups=groups)


def _sequence_smoothing(loop, N, who):
    """optimize_sequence's smoothing settings with `groups` as an (N,) int32 tensor on the loop's device (uploaded on the caller's
    stream); None for a loop whose smoothing is off (set_smoothing)."""
    s = getattr(loop, "_smooth", None)      # (a loop without the switch: off)
    if s is None:
        return None
    if s["use_covariance"] and not loop.keep_gaussians:
        raise ValueError(f"{who}: set_smoothing(use_covariance=True) needs the Gaussians this loop no longer keeps (keep_gaussians)")
    s = dict(s)
    g = s["groups"]
    if g is not None:
        g = g if torch.is_tensor(g) else torch.as_tensor(np.asarray(g))
        if g.dim() != 1 or g.shape[0] != N or g.is_floating_point() or g.dtype == torch.bool:
            raise ValueError(f"{who}: the groups given to set_smoothing must be ({N},) integers, one per frame of this sequence, "
                             f"got {tuple(g.shape)} {g.dtype}")
        s["groups"] = g.to(device=loop.device, dtype=torch.int32)
    return s


def _sequence_consensus(loop, reject, N):
    """optimize_sequence's (inliers (N,V,J) bool, n_consensus (N,J) int32) on the device, None without rejection."""
    if reject is None:
        return None
    return (torch.empty((N, loop.V, loop.P), dtype=torch.bool, device=loop.device),
            torch.empty((N, loop.P), dtype=torch.int32, device=loop.device))


def _sequence_predictions(points, poses_3d, N):
    """optimize_sequence's `poses_3d` -> None or the (N,V,J,3) predictions as a tensor where they are (arrays: on the host)."""
    if poses_3d is None:
        return None
    if points is not None:
        raise ValueError("optimize_sequence: poses_3d are fused into the initial joints when points is None; give one of the two")
    p3d = poses_3d if torch.is_tensor(poses_3d) else torch.as_tensor(np.asarray(poses_3d))
    if p3d.dim() != 4 or p3d.shape[0] != N or p3d.shape[-1] != 3:
        raise ValueError(f"poses_3d must be (N,V,J,3) with N = {N} frames like poses_2d, got {tuple(p3d.shape)}")
    return p3d


def _sequence_rig_ids(sel, rig_ids, N):
    """optimize_sequence's `rig_ids` -> None or an (N,) integer tensor on the device: host ids are validated against the bank
    and uploaded once per sequence; a device tensor is taken as it is (the gather kernel checks its bounds)."""
    if rig_ids is None:
        return None
    if sel is None:
        raise ValueError("rig_ids needs a rig bank: FrameBatchLoop / FramePipeline(gaussians, rigs=RigBank(rigs, device), ...)")
    if torch.is_tensor(rig_ids) and rig_ids.device.type != "cpu":
        if rig_ids.dim() != 1 or rig_ids.shape[0] != N or rig_ids.is_floating_point():
            raise ValueError(f"rig_ids must be ({N},) integers, got {tuple(rig_ids.shape)} {rig_ids.dtype}")
        return rig_ids
    from .rigs import validate_rig_ids
    return torch.as_tensor(validate_rig_ids(rig_ids, sel.bank.R, N), dtype=torch.int32).to(sel.ids.device)


def _checked_gt(loop, gt, n, what):
    """The ground truth handed to set_ground_truth -> the (n,P,3) float32 tensor on the loop's device that `what` (new_scenes: n = F
    frames; optimize_sequence: n = N frames) needs; None stays None; anything else is refused."""
    if gt is None:
        return None
    want = (n, loop.P, 3)
    if tuple(gt.shape) != want:
        raise ValueError(f"{what}: the ground truth given to set_ground_truth must be {want}, got {tuple(gt.shape)}")
    return gt


def _accept_gt(loop, gt):
    """set_ground_truth's argument: None, or a float32 (n,P,3) tensor on the loop's device, for a loop whose error reporting is on."""
    if gt is None:
        return None
    if loop._report is None or loop._report.steps == 0:
        raise ValueError("ground truth is given, but error reporting is off: the errors against it are trace rows, which need "
                         "FrameBatchLoop / FramePipeline(..., report_steps=rows) with rows > 0"
                         + (" (this loop has save_iterations only: snapshots need no ground truth)" if loop._report is not None else ""))
    dev = loop.xyz.device
    if (not torch.is_tensor(gt) or gt.dim() != 3 or tuple(gt.shape[1:]) != (loop.P, 3) or gt.dtype != torch.float32
            or gt.device != dev):
        got = f"{tuple(gt.shape)} {gt.dtype} on {gt.device}" if torch.is_tensor(gt) else type(gt).__name__
        raise ValueError(f"the ground truth must be a float32 tensor (frames,P,3) = (frames, {loop.P}, 3) on {dev}, got {got}")
    return gt


def _sequence_report(loop, N):
    """optimize_sequence's `report`: None for a loop that reports nothing."""
    if loop._report is None:
        return None
    from .report import SequenceReport
    return SequenceReport(loop, N)


def _sequence_gaussians(loop, out):
    """optimize_sequence's `gaussians` around the joints `out` it returns: None for a loop that does not keep them."""
    if not loop.keep_gaussians:
        return None
    from .uncertainty import SequenceGaussians
    return SequenceGaussians(out)


def _sequence_images(loop, N):
    """optimize_sequence's `images`: None for a loop whose debug pictures are off (set_debug_images)."""
    if loop._debug_frames is None:
        return None
    from .preview import SequenceImages
    va = loop.views_all
    return SequenceImages(loop._debug_frames, N, loop.V, va.W, va.H, loop.device, va.sizes[:loop.V] if va.mixed else None)


def _debug_frames(loop, frames):
    """set_debug_images' argument -> None (off) or a tuple of sequence indices >= 0."""
    if frames is None:
        return None
    if loop.rigs is not None:
        raise ValueError("set_debug_images: the debug pictures render a frame in its own cameras from HOST scalars; a loop over "
                         "a rig bank keeps them on the device (picture such a frame with preview.render_preview and its rig)")
    chosen = tuple(int(f) for f in frames)
    if not chosen or min(chosen) < 0:
        raise ValueError(f"set_debug_images: frames = {list(frames)!r} must be sequence indices >= 0, at least one (None: off)")
    return chosen


class SequenceRun:
    """One optimize_sequence call: N frames through batches of F.  The constructor checks the arguments against `loop`'s settings
    (a FrameBatchLoop; a pipeline gives its first) and allocates what the sequence fills, on the caller's stream; the drivers then
    call begin(loop, b) / take(loop, b) around the work of every batch b in starts(), on the stream of the loop that runs it.
      pts, p2d      (N,P,3) initial joints, or None: triangulated from the (N,V,J,2) detections `p2d`; tensors stay where they are
      p3d           None or the (N,V,J,3) predictions, fused into the initial joints instead of the triangulation (`pts` None)
      ids, gt       None or the (N,) rig ids as _sequence_rig_ids left them; None or the (N,P,3) ground truth (`gt_next`: what
                    set_ground_truth left) as _checked_gt left it
      out, initial  (N,P,3) optimised joints; the initial joints, None unless `return_initial`
      inliers, n_consensus, report, gaussians, images, reprojection   what optimize_sequence documents under these names, None where the loop
                    has the feature off;  stopped_at: None, or the (N,) int64 zeros of a pipeline with early stopping
      smoothing     None or set_smoothing's settings for this sequence; smoothed() makes the result once every batch is taken"""

    def __init__(self, loop, gt_next, points, poses_2d, poses_3d, rig_ids, return_initial, who="optimize_sequence"):
        self.pts, self.p2d, self.N = _sequence_inputs(points, poses_2d)
        self.p3d = _sequence_predictions(points, poses_3d, self.N)
        _checked_reject(loop._reject, points, poses_3d, who)
        _checked_refine(getattr(loop, "_refine", None), points, poses_3d, who)      # (a loop without the switch: off)
        self.ids = _sequence_rig_ids(loop._sel, rig_ids, self.N)    # (uploaded on the caller's stream)
        self.inliers, self.n_consensus = _sequence_consensus(loop, loop._reject, self.N) or (None, None)
        self.gt = _checked_gt(loop, gt_next, self.N, who)
        self.report = _sequence_report(loop, self.N)
        self.F, self.stopped_at = loop.F, None
        self.out = torch.empty((self.N, loop.P, 3), dtype=torch.float32, device=loop.device)
        self.initial = torch.empty_like(self.out) if return_initial else None
        self.gaussians = _sequence_gaussians(loop, self.out)
        self.images = _sequence_images(loop, self.N)
        self.reprojection = _sequence_reprojection(loop, self.N)
        self.smoothing = _sequence_smoothing(loop, self.N, who)

    def smoothed(self):
        """Behind the last take(), on the CALLER's stream once it waits for every batch: None with the smoothing off, else
        smoothing.smooth_sequence of `out` -- one launch, behind one joint_uncertainty launch when the covariances weight it.
        Reads `out` and the kept Gaussians, writes neither."""
        if self.smoothing is None:
            return None
        from .smoothing import smooth_sequence
        kw = dict(self.smoothing)
        cov6 = self.gaussians.uncertainty().cov6 if kw.pop("use_covariance") else None
        return smooth_sequence(self.out, cov6, **kw)

    def starts(self):
        return range(0, self.N, self.F)     # the first frame of every batch

    def rows(self, b):
        """The frames of batch b in the inputs: a slice (a full batch stays a view, no gather), or a short last batch filled up by
        repeating the sequence's final frame, rig included."""
        return slice(b, b + self.F) if b + self.F <= self.N else [min(b + i, self.N - 1) for i in range(self.F)]

    def begin(self, loop, b):
        """new_scenes of `loop` for batch b, then the batch's rows of what the initial joints decide, on the current stream."""
        rows, n = self.rows(b), min(self.F, self.N - b)
        of = lambda x: None if x is None else x[rows]
        if self.gt is not None:
            loop._gt_next = self.gt[rows]
        loop.new_scenes(of(self.pts), poses_2d=self.p2d[rows], rig_ids=of(self.ids), poses_3d=of(self.p3d))
        if self.initial is not None:
            self.initial[b:b + n] = loop.xyz[:n]
        if self.inliers is not None:
            self.inliers[b:b + n] = loop.inliers[:n]
            self.n_consensus[b:b + n] = loop.n_consensus[:n]
        if self.images is not None:
            self.images.begin(loop, b, n)       # (right behind new_scenes: the heat-maps and the first renders)
        if self.reprojection is not None:
            self.reprojection.begin(loop, b, n, self.p2d[rows])

    def take(self, loop, b):
        """Batch b is done on `loop`: its first n frames' results, on the current stream (the filler frames are dropped)."""
        n = min(self.F, self.N - b)
        self.out[b:b + n] = loop.xyz[:n]
        if self.stopped_at is not None:
            self.stopped_at[b:b + n] = loop._es_state[:n, 1]        # (0: the frame ran to the end)
        for kept in (self.gaussians, self.images, self.report, self.reprojection):
            if kept is not None:
                kept.take(loop, b, n)

    def result(self):
        return (self.out, self.initial) if self.initial is not None else self.out
