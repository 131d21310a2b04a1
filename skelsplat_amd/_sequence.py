"""What the loops share around a scene's start: where its initial joints come from (InitialJoints), the switches that decide it and
what a sequence keeps (JointSwitches, SequenceSwitches) with their checks, and one `optimize_sequence` call of a FrameBatchLoop /
FramePipeline as a record (SequenceRun).  Imports nothing from loop.py, which imports from here."""
import numpy as np

import torch

from . import initial_guess, reprojection, triangulation


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
    return triangulation._checked_rejection(reject_px, min_inliers)


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
    return reprojection._checked_refinement(huber_px, max_iters)


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


class InitialJoints:
    """Where the initial joints of a loop's next scene(s) come from: `check` refuses or returns a plan, nothing written yet;
    `write` then does the plan's launches.  Explicit `points` are taken as they are.  `points=None`: the joints are the DLT
    triangulation of `poses_2d` (triangulation.triangulate_sequence) -- behind outlier rejection and in front of the refinement
    (reprojection.refine_triangulation) where the loop has them switched on --, or, with `poses_3d`, the
    reprojection-error-weighted mean of the views' 3D predictions (initial_guess.fuse_predictions)."""

    @classmethod
    def check(cls, who, points, poses_2d, poses_3d, shape, reject, refine, proj, device):
        """`who`: the caller, for the refusal texts.  `shape` = (F, V, J): what the inputs must be -- `points` (F,J,3), `poses_2d`
        (F,V,J,>=2), `poses_3d` (F,V,J,3); F = None is the one-frame form, the same without the frame axis.  `reject`, `refine`: the
        loop's set_outlier_rejection / set_refinement settings; `proj`: its projection matrices, None for cameras without
        K / R / T.  The detections are only looked at when they decide the joints (`points=None`).  The plan holds `points`,
        `p2d`, `p3d` as tensors with the frame axis (F = 1 for the one-frame form), None for what does not enter."""
        F, V, J = shape
        one, ax = F is None, "" if F is None else "F,"
        lead = () if one else (F,)
        self = cls()
        self.one, self.proj, self.points, self.p2d, self.p3d = one, proj, None, None, None
        self.reject, self.refine = _checked_reject(reject, points, poses_3d, who), _checked_refine(refine, points, poses_3d, who)
        if points is not None:
            if poses_3d is not None:
                raise ValueError(f"{who}: poses_3d are fused into the initial joints when points is None; give one of the two")
            pts = points if torch.is_tensor(points) else torch.as_tensor(np.asarray(points))
            if tuple(pts.shape) != lead + (J, 3):
                raise ValueError(f"{who}: points must be ({ax}P,3) = {lead + (J, 3)}, got {tuple(pts.shape)}")
            self.points = pts[None] if one else pts
            return self
        if poses_2d is None:
            raise ValueError(f"{who}(points=None) triangulates the initial joints from poses_2d: give poses_2d "
                             "(ready heatmaps do not carry the detections)")
        if proj is None:
            raise ValueError(f"{who}(points=None): the cameras carry no K / R / T to build projection matrices from")
        p2d = torch.as_tensor(poses_2d, device=device)
        if p2d.dim() != len(lead) + 3 or tuple(p2d.shape[:-1]) != lead + (V, J) or p2d.shape[-1] < 2:
            raise ValueError(f"{who}: poses_2d must be ({ax}V,J,2) = {lead + (V, J, 2)}, got {tuple(p2d.shape)}")
        self.p2d = p2d[None] if one else p2d
        if poses_3d is not None:
            p3d = torch.as_tensor(poses_3d, device=device)
            if tuple(p3d.shape) != lead + (V, J, 3):
                raise ValueError(f"{who}: poses_3d must be ({ax}V,J,3) = {lead + (V, J, 3)}, got {tuple(p3d.shape)}")
            self.p3d = p3d[None] if one else p3d
        return self

    @property
    def estimated(self):
        """Do the detections decide the joints (`points=None`)?"""
        return self.points is None

    def write(self, keep, out, consensus=None):
        """The joints into `out` (F,J,3) float32, in place, on the current stream; returns `out`.  `keep`: None or (F,V,J) bool, the
        detections that enter (`valid`).  `consensus`: with rejection on, the (inliers (F,V,J) bool, n_consensus (F,J) int32)
        buffers its launch fills, and the refinement then minimises over those inliers instead of `keep`.  The one-frame form takes
        all of them without the frame axis."""
        given = out
        if self.one:
            lift = lambda t: None if t is None else t[None]
            keep, out, consensus = lift(keep), out[None], None if consensus is None else tuple(map(lift, consensus))
        if self.points is not None:
            out.copy_(self.points.to(device=out.device, dtype=out.dtype))
        elif self.p3d is not None:
            initial_guess.fuse_predictions(self.proj, self.p3d, self.p2d, valid=keep, out=out)
        else:
            reject_px, min_inliers = self.reject
            if reject_px is None:
                consensus = None
            triangulation.triangulate_sequence(self.proj, self.p2d, valid=keep, out=out, reject_px=reject_px,
                                               min_inliers=min_inliers, out_inliers=consensus)
            if self.refine is not None:      # one more launch in the same place, in place on the joints
                reprojection.refine_triangulation(self.proj, self.p2d, out, valid=keep if consensus is None else consensus[0],
                                                  huber_px=self.refine[0], max_iters=self.refine[1], out=out)
        return given


def _sequence_reprojection(loop, N):
    """optimize_sequence's `reprojection`: None for a loop whose reprojection report is off (set_reprojection_report)."""
    if not loop._reproject:
        return None
    return reprojection.SequenceReprojection(N, loop.V, loop.P, loop.device)


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
    s = loop._smooth
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


def _bone_constraint(loop, bones, use_covariance, cov_floor, symmetric, groups, max_sigma_mm, max_iters):
    """set_bone_constraint's arguments -> None (off) or the checked settings as a dict; `groups` stays as given until a
    sequence's length is known (_sequence_bones).  `pairs`: the (left, right) bone indices made equal, or None."""
    if bones is None:
        return None
    from . import skeleton
    from .scene import DATASETS
    who = "set_bone_constraint"
    d = DATASETS.get(loop.dataset)
    if isinstance(bones, str):
        if bones != "dataset" or d is None:
            raise ValueError(f"{who}: bones = {bones!r}: (B,2) integers, or 'dataset' for the tree of a loop built for one of "
                             f"{sorted(DATASETS)}")
        bones = d["bones"]
    bn = skeleton.checked_bones(bones, loop.P, who)
    floor, iters, _ = skeleton._projection_settings(cov_floor, max_iters, 0.0, who)
    if max_sigma_mm is not None:
        if not use_covariance:
            raise ValueError(f"{who}: max_sigma_mm gates a frame by the variance of its length, which needs use_covariance=True")
        max_sigma_mm = skeleton._max_sigma(max_sigma_mm, True, who)
    pairs = None
    if symmetric:
        if d is None:
            raise ValueError(f"{who}: symmetric=True pairs the arm and leg `limbs` of scene.DATASETS, which has no {loop.dataset!r}")
        try:
            l_arm, r_arm, l_leg, r_leg = skeleton.bone_index(bn, d["limbs"])
        except KeyError as e:
            raise ValueError(f"{who}: symmetric=True needs the dataset's limb {e.args[0]} among the bones") from None
        pairs = ((l_arm, r_arm), (l_leg, r_leg))
    if use_covariance and not loop.keep_gaussians and loop._smooth is None:
        raise ValueError(f"{who}: use_covariance=True takes every joint's covariance from the frame's optimised Gaussians, which "
                         "this loop does not keep -- build it with FrameBatchLoop / FramePipeline(..., keep_gaussians=True), or "
                         "pass use_covariance=False for the identity")
    return dict(bones=bn, use_covariance=bool(use_covariance), cov_floor=floor, pairs=pairs, groups=groups,
                max_sigma_mm=max_sigma_mm, max_iters=iters)


def _sequence_bones(loop, N, who):
    """optimize_sequence's bone-constraint settings with `groups` as an (N,) int32 tensor on the loop's device and `n_groups` from
    the HOST ids (a device tensor of ids: one number is read back on the caller's stream); None for a loop whose constraint is
    off (set_bone_constraint)."""
    s = getattr(loop, "_bones", None)       # (a loop from before the switch has none)
    if s is None:
        return None
    if s["use_covariance"] and not loop.keep_gaussians and loop._smooth is None:
        raise ValueError(f"{who}: set_bone_constraint(use_covariance=True) needs the Gaussians this loop does not keep "
                         "(keep_gaussians), or the smoothing's covariance (set_smoothing)")
    s = dict(s, n_groups=1)
    g = s["groups"]
    if g is not None:
        g = g if torch.is_tensor(g) else torch.as_tensor(np.asarray(g))
        if g.dim() != 1 or g.shape[0] != N or g.is_floating_point() or g.dtype == torch.bool:
            raise ValueError(f"{who}: the groups given to set_bone_constraint must be ({N},) integers, one per frame of this "
                             f"sequence, got {tuple(g.shape)} {g.dtype}")
        s["n_groups"] = int(g.max()) + 1
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


class JointSwitches:
    """The switches of the initial joints (InitialJoints), for MultiViewLoop, FrameBatchLoop and FramePipeline alike: each checks
    its arguments once and then sets the loops this object drives -- a loop itself, a pipeline's `loops` -- so a refused call
    changes none of them.  The settings live on the loops, as `_reject` and `_refine`.  Every switch returns the object it
    was called on."""

    def _driven(self):
        """The loops this object drives: a loop, itself (FramePipeline returns its `loops`)."""
        return (self,)

    def _set(self, name, value):
        for loop in self._driven():
            setattr(loop, name, value)
        return self

    def set_outlier_rejection(self, reject_px=None, min_inliers=3):
        """From now on new_scene / new_scenes / optimize_sequence with `points=None` (and without `poses_3d`) reject outlier
        detections while they triangulate the initial joints: exhaustive two-view consensus within `reject_px` pixels, at least
        `min_inliers` (2 .. 64) views for a consensus (triangulation.triangulate_sequence's `reject_px`, `min_inliers`: one more
        launch in the same place, the kept views still the ones it starts from).  The views each joint was solved from and the
        winners' counts are then kept on the device, in buffers allocated once: a loop's `inliers` and `n_consensus` per scene
        or batch, and per sequence `seq_inliers` (N,V,J) bool / `seq_n_consensus` (N,J) int32 of a FrameBatchLoop, `inliers` /
        `n_consensus` of a pipeline, each batch's rows copied on its own stream (None after a sequence without rejection).  The
        heat-maps are NOT changed: a rejected detection still draws its plane.  A caller who wants it dropped takes two steps,
        both on the device: `pts, inl, _ = triangulate_sequence(proj, p2d, reject_px=.., return_inliers=True)`, then
        `new_scenes(pts, p2d, drop_masks=~inl)`.  While it is on, explicit points or `poses_3d` are refused; `reject_px=None`
        switches it off."""
        return self._set("_reject", _rejection(reject_px, min_inliers))

    def set_refinement(self, max_iters=16, huber_px=None):
        """From now on new_scene / new_scenes / optimize_sequence with `points=None` (and without `poses_3d`) follow the
        triangulation of the initial joints by one launch that minimises their reprojection error from there
        (reprojection.refine_triangulation: at most `max_iters` (1 .. 16) damped Gauss-Newton trips per joint, plain squares or,
        with `huber_px`, the Huber cost), in place, on the same stream, in front of the heat-map factors that read the joints.
        It minimises over the kept views (`valid = ~drop_masks`), or, with outlier rejection on, over the consensus' `inliers`.
        While it is on, explicit points or `poses_3d` are refused; `max_iters=None` switches it off."""
        return self._set("_refine", _refinement(max_iters, huber_px))


class SequenceSwitches(JointSwitches):
    """JointSwitches plus what an `optimize_sequence` of a FrameBatchLoop or a FramePipeline keeps: the settings live on the loops
    as `_reproject`, `_smooth`, `_bones` and `_debug_frames`, the results arrive on the object that ran the sequence (SequenceRun.publish),
    a pipeline's batches each on their own stream."""

    def set_reprojection_report(self, on=True):
        """From now on every `optimize_sequence` measures the reprojection error of each batch's initial and final joints against
        the batch's detections (reprojection.reproject: one launch each, on the batch's own stream, nothing is read back) into
        `self.reprojection`, a reprojection.SequenceReprojection -- the ground-truth-free figure of the sequence; None after a
        sequence without it.  The optimiser's steps and captured graphs are untouched.  `False`: off again."""
        return self._set("_reproject", bool(on))

    def set_smoothing(self, half_window=None, degree=2, taper="tricube", use_covariance=True, cov_floor=0.0, groups=None):
        """From now on every `optimize_sequence` smooths the joints it returns over time once all batches are taken
        (smoothing.smooth_sequence: one launch on the caller's stream -- a pipeline's behind its wait for every batch's stream --,
        nothing is read back) into `self.smoothed`, a smoothing.Smoothed of joints, velocity, cov6 and n_used for all N frames;
        None after a sequence without it.
        `half_window` frames on each side (None: off again), `degree` 0 .. 2, `taper` "box" or "tricube".  `use_covariance`: every
        frame of a joint is weighted by the inverse of its optimised Gaussian's covariance -- one joint_uncertainty launch in
        front, on loops built with keep_gaussians=True (refused otherwise) --, with `cov_floor` mm^2 added to the diagonals;
        False: unit weights.  `groups` (N,) integers, host or device: a window never crosses from one recording into the next
        (checked against the next sequence's length).  A joint that ended NaN ("Unobserved joints") is filled from the frames
        around it.  The joints `optimize_sequence` returns, `gaussians`, `report` and every other output are untouched, as are the
        optimiser's steps and captured graphs.  What the covariance weights gain on real sequences depends on how well the
        optimised covariances are calibrated (uncertainty.calibration) and has not been measured."""
        return self._set("_smooth", _smoothing(self._driven()[0], half_window, degree, taper, use_covariance, cov_floor, groups))

    def set_bone_constraint(self, bones=None, use_covariance=True, cov_floor=0.0, symmetric=False, groups=None, max_sigma_mm=None,
                            max_iters=16):
        """From now on every `optimize_sequence` holds the sequence to constant limb lengths once all batches are taken: three
        launches on the caller's stream behind the smoothing, if that is on -- skeleton.bone_lengths (measure, then the medians
        per recording) and skeleton.project_to_lengths onto those medians --, nothing is read back.  The results arrive as
        `self.bone_lengths` (a skeleton.BoneLengths: length, mad, n_used per recording and bone, measured per frame; the lengths
        the frames were projected onto are `length`, made symmetric when asked) and `self.constrained` (a skeleton.Projected:
        joints, residual, n_trips, n_active); both None after a sequence without it.
        `bones` (B,2) host integers (parent, child), or "dataset" for scene.DATASETS[...]["bones"]; None: off again.  With the
        smoothing on, the SMOOTHED joints are constrained, under the fit's own cov6; otherwise the joints optimize_sequence
        returns, under the covariance of each frame's kept Gaussians (one joint_uncertainty launch in front; loops built with
        keep_gaussians=True, refused otherwise).  `use_covariance=False`: the identity, both ends of a wrong bone move alike.
        `cov_floor` mm^2 is added to the covariances' diagonals, `max_sigma_mm` leaves a frame out of a bone's median when the
        standard deviation of its length is larger, `symmetric=True` sets the dataset's left and right arm and leg `limbs` to
        their mean before projecting, `groups` (N,) integers, host or device, are the recordings (checked against the next
        sequence's length), `max_iters` 1 .. 16 trips per frame.  The joints `optimize_sequence` returns, `smoothed`, `gaussians`,
        `report` and every other output are untouched, as are the optimiser's steps and captured graphs.  The result is A pose on
        the lengths, reached by successive covariance-closest projections, not the closest one (skeleton.project_to_lengths);
        what it gains on real sequences has not been measured."""
        return self._set("_bones", _bone_constraint(self._driven()[0], bones, use_covariance, cov_floor, symmetric, groups,
                                                    max_sigma_mm, max_iters))

    def set_view_weighting(self, mode, threshold=0.5):
        """From now on the optimiser step of every frame weights each view's xyz gradient per joint by its agreement with the
        other views' (`mode` "scale" or "select" with the cosine `threshold`; None: the plain mean again) -- the loops'
        `view_weighting` keyword, set after construction.  Every `optimize_sequence` then keeps each frame's final weights in
        `view_weights` (N,V,P) (a FrameBatchLoop: `seq_view_weights`), each batch's rows copied on the batch's own stream; None
        after a sequence without it.  Captured graphs hold the step's entry point: they are dropped and captured again."""
        from . import _lib
        _lib.vw_mode(mode)
        for loop in self._driven():
            loop._set_view_weighting(mode, threshold)
        return self

    def set_debug_images(self, frames):
        """The reference's debug pictures (configs/*.yaml `debug.save_images`, train.py:113-114, 143-144, 236-237) for the frames
        with these sequence indices, from now on: every `optimize_sequence` fills `self.images` (a preview.SequenceImages) with
        each chosen frame's heat-map picture and the picture of its render before the first and after the last iteration, all
        on the device -- the heat-maps and the first render enqueued right behind the batch's new_scenes, the last render where
        the joints are copied, on the batch's own stream; nothing is read back until `images.save(dir)`.  The pictures stay
        outside the captured graphs and a group's launch sequence is the same with and without them.  With them on, a batch that
        holds a chosen frame enqueues one heat-map picture of all its views and two dense forwards per chosen frame (a debug
        path: preview.SequenceImages says what that is); other batches enqueue nothing more.  `None` switches them off: nothing
        is allocated or enqueued and `images` is None after the next sequence."""
        return self._set("_debug_frames", _debug_frames(self._driven()[0], frames))

    def set_ground_truth(self, gt):
        """The ground truth of the NEXT batch or sequence (loops with `report_steps`): (F,P,3) for `new_scenes`, (N,P,3) for
        `optimize_sequence`, float32 on the loops' device.  The next of those calls on this object takes it -- the errors it
        reports are against it -- and forgets it; None withdraws one that has not been taken."""
        self._gt_next = _accept_gt(self._driven()[0], gt)
        return self


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
      smoothing     None or set_smoothing's settings for this sequence; smoothed() makes the result once every batch is taken
      bones         None or set_bone_constraint's settings for this sequence; constrained(smoothed) makes the results behind it"""

    def __init__(self, loop, gt_next, points, poses_2d, poses_3d, rig_ids, return_initial, who="optimize_sequence"):
        self.pts, self.p2d, self.N = _sequence_inputs(points, poses_2d)
        self.p3d = _sequence_predictions(points, poses_3d, self.N)
        _checked_reject(loop._reject, points, poses_3d, who)
        _checked_refine(loop._refine, points, poses_3d, who)
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
        self.bones = _sequence_bones(loop, self.N, who)
        # view agreement on: every frame's final weights (N,V,P), each batch's rows copied on its own stream (take)
        self.view_weights = (torch.zeros((self.N, loop.V, loop.P), dtype=torch.float32, device=loop.device)
                             if getattr(loop, "_vw_mode", 0) else None)

    def publish(self, owner, consensus=("inliers", "n_consensus")):
        """The results this sequence fills, onto the object that runs it, under the names optimize_sequence documents; the
        consensus pair under the two names given (a FrameBatchLoop keeps `inliers` / `n_consensus` for its batch)."""
        for name, value in zip(consensus, (self.inliers, self.n_consensus)):
            setattr(owner, name, value)
        if hasattr(owner, "loops"):      # (a pipeline: a FrameBatchLoop's own `view_weights` is its batch's)
            owner.view_weights = self.view_weights
        else:
            owner.seq_view_weights = self.view_weights
        owner.report, owner.gaussians, owner.images, owner.reprojection = self.report, self.gaussians, self.images, self.reprojection

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

    def constrained(self, smoothed):
        """Behind smoothed(), on the caller's stream: (None, None) with the bone constraint off, else (skeleton.BoneLengths,
        skeleton.Projected) of the smoothed joints under the fit's cov6 when `smoothed` is given, of `out` under the kept
        Gaussians' covariance otherwise -- measure, lengths, project: three launches, behind one joint_uncertainty launch where
        the Gaussians' covariance enters.  Reads its inputs, writes none of them."""
        s = self.bones
        if s is None:
            return None, None
        from . import skeleton
        xyz = self.out if smoothed is None else smoothed.joints
        cov6 = None
        if s["use_covariance"]:
            cov6 = self.gaussians.uncertainty().cov6 if smoothed is None else smoothed.cov6
        lengths = skeleton.bone_lengths(xyz, s["bones"], cov6, groups=s["groups"], max_sigma_mm=s["max_sigma_mm"],
                                        n_groups=s["n_groups"])
        if s["pairs"] is not None:
            lengths = lengths._replace(length=skeleton.symmetrize(lengths.length, s["pairs"]))
        return lengths, skeleton.project_to_lengths(xyz, s["bones"], lengths.length, cov6, groups=s["groups"],
                                                    cov_floor=s["cov_floor"], max_iters=s["max_iters"])

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
        if self.view_weights is not None:
            self.view_weights[b:b + n] = loop.view_weights[:n]
        for kept in (self.gaussians, self.images, self.report, self.reprojection):
            if kept is not None:
                kept.take(loop, b, n)

    def result(self):
        return (self.out, self.initial) if self.initial is not None else self.out
