#!/usr/bin/env python3
"""A whole synthetic SEQUENCE through the hot path, the way the reference's train.py walks a dataset (one frame after the
other, train.py:74-99) -- but many frames per launch: noisy 2D detections of N frames -> DLT initial guesses -> 500
iterations of the multi-view loop for every frame (loop.FramePipeline) -> MPJPE per frame.
python examples/optimize_sequence.py [--frames 64] [--per-launch 16] [--streams 2] [--iters 500] [--init host|device|fuse] [--rigs R]
    [--report] [--uncertainty] [--reject-px PX] [--corrupt K] [--refine [--huber-px D]] [--images DIR [--image-frames 0,31,63]]
    [--smooth H [--smooth-degree D]] [--motion wobble|smooth|articulated] [--view-weights scale|select [--view-threshold T]]
    [--bones [--bones-symmetric]] [--people K [--assoc-px PX]]
--people K [--assoc-px PX]: K synthetic skeletons on a grid walk through the views; every view's detector returns them in a slot
order that is shuffled per frame.  The detections go to the device once and the front end runs there (skelsplat_amd/people.py):
associate (pairs within PX pixels of mean epipolar distance, default 15) -> triangulate -> track -> to_tracks -> the pipeline of
--init device over the K single-person sequences, smoothed per track through the `groups` to_tracks returns (--smooth H, default
2).  Printed: how many frames were associated and tracked correctly against the known permutation, and the MPJPE of every track.
The other switches do not apply.
--view-weights scale|select [--view-threshold T]: the optimiser step of every frame weights each view's joint gradient by its
agreement with the other views' (pipe.set_view_weighting; DESIGN.md "View agreement"; T: select's cosine threshold, default 0.5).
With --report: each view's mean final weight, and with --corrupt the mean weight of the corrupted (view, joint) detections
against the clean ones.
--rigs R: the frames cycle through R jittered ring rigs (SyntheticScene seeds 0 .. R-1), as a dataset whose scenes bring their own
cameras does; one rigs.RigBank holds them on the device and every batch names its frames' rigs (rig_ids).
--init host (default): the DLT runs on the host, frame by frame, and its points are uploaded; --init device: the detections
go to the device once and every batch is triangulated there (FramePipeline.optimize_sequence(None, ...)); --init fuse: the
reference's "metrabs" guess instead of the DLT -- synthetic monocular 3D predictions of every view (ground truth + 20-50 mm of
noise per view) go to the device once with the detections, and every batch starts from their reprojection-error-weighted mean
(initial_guess.fuse_predictions through optimize_sequence(None, ..., poses_3d=...)).  The timed region runs from the detections
(and predictions) to the joints every way.
--corrupt K: K random (view, joint) detections of every frame are moved by 80-300 px, as an occluded or mis-detected joint is.
--reject-px PX (with --init device): every batch's triangulation first rejects outlier detections by two-view consensus on the
device (pipe.set_outlier_rejection(PX), then optimize_sequence(None, ...)); the initial error is printed with and without the rejection, and how many
detections were rejected.  The heat-maps still draw every detection: the final error shows what the outliers left in them cost.
--refine [--huber-px D] (with --init device): every batch's triangulation is followed by the refinement that minimises the
reprojection error from there (pipe.set_refinement; plain squares, or the Huber cost at D pixels); the initial error is printed with
and without it.  With --reject-px it runs over the consensus' inliers.
--report: the synthetic ground truth goes to the device once and the loops report while they run (report_steps, save_iterations;
skelsplat_amd/report.py): the mean absolute / root-relative error over the sequence after 0, 1, 5, 25 and the last optimiser
step -- the reference's convergence curve (train.py:184-213) --, the error at the snapshot of the middle iteration, and
report.evaluate_sequence over four synthetic "activities" (eval.py:115-142).  Nothing is read back while the loops run.  Under
these lines, the figure that needs no ground truth: the mean reprojection error of the initial and of the optimised joints against the
detections, overall and per view (pipe.set_reprojection_report, skelsplat_amd/reprojection.py).
--uncertainty (with --report's ground truth): the loops keep every frame's optimised Gaussians (keep_gaussians=True) and the
covariances are read back as the pose's uncertainty on the device (skelsplat_amd/uncertainty.py): the share of ground-truth joints
inside the 1 / 2 / 3-sigma ellipsoid overall and per joint (utils/analize_error_confidence_correlation.py's percent_inside_sigmas
and .._per_joint) and the mean trace of the covariance.
--images DIR: the reference's debug pictures (configs/*.yaml `debug.save_images`, train.py:279-304) of the frames --image-frames
(default: the first, the middle and the last) -- heatmaps/heatmap_{view}.png, images/render_1_{view}.png, images/render_{view}.png,
one sub-directory per frame -- made on the device while the timed sequence runs (pipe.set_debug_images, skelsplat_amd/preview.py)
and written afterwards.  With --corrupt and --reject-px the misplaced blobs the rejection leaves in the heat-maps are there to see
in heatmap_*.png.  Not with --rigs > 1.
--smooth H [--smooth-degree D] (with --report's ground truth): the optimised joints are smoothed over time on the device once the
sequence is through (pipe.set_smoothing, skelsplat_amd/smoothing.py): a local polynomial fit of degree D (default 2) over H frames
on each side, tricube taper; with --uncertainty every frame of a joint is weighted by the inverse of its optimised Gaussian's
covariance, else by 1.  Printed: MPJPE, Accel and Accel error (smoothing.sequence_accel) of the raw and of the smoothed joints --
with --uncertainty for both weightings, next to the calibration table that says how far the covariances were from calibrated.
--motion smooth: the skeleton moves on low-frequency sinusoids per joint instead of the default `wobble`, whose ground truth jumps
independently by 5 mm per frame -- a signal no temporal filter can beat.  What the covariance weights gain on real sequences has not
been measured.
--motion articulated: ground truth that keeps its bone lengths -- forward kinematics over the dataset's skeleton tree
(scene.articulated_motion): every bone has the template's length and its direction turns on low-frequency sinusoids, the drift is
the other motions'.  `wobble` and `smooth` move every joint on its own, so THEIR ground truth has no constant lengths.
--bones [--bones-symmetric] (with --report's ground truth): the sequence is held to constant limb lengths on the device once it is
through (pipe.set_bone_constraint, skelsplat_amd/skeleton.py): the median length of every bone of the dataset's tree over the
sequence, then every frame projected onto those lengths -- under the covariance of its optimised Gaussians with --uncertainty,
else under the identity; after --smooth, the smoothed joints under the fit's covariance.  --bones-symmetric makes left and right
arms and legs equal first.  Printed: per bone the median and the MAD of the optimised sequence, the largest relative MAD before and
after the constraint, and MPJPE, PA-MPJPE and Accel of the constrained joints.  The constraint reaches A pose on the lengths by
successive covariance-closest projections, not the closest one; on `wobble` and `smooth` it holds the poses to lengths their ground
truth does not keep and must not be expected to help.  What it gains on real sequences has not been measured.
The curve falls from the reference's default start, --init fuse (21.7 -> 14.3 mm); from the DLT start (--init host / device) it
RISES from 13.4 to 14.3 mm in the first steps: on this synthetic sequence (3 px of detection noise, exact cameras) the DLT already
sits below the optimiser's fixed point, and the curve shows it."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from skelsplat_amd import io, triangulation
from skelsplat_amd.loop import FramePipeline
from skelsplat_amd.scene import GaussianModel, SyntheticScene, project_points


def people_main(args):
    """--people K: detections of K people in shuffled slots -> associate -> triangulate -> track -> to_tracks -> the pipeline."""
    from skelsplat_amd import people
    from skelsplat_amd.scene import articulated_motion
    dev = torch.device("cuda:0")
    K, N, V = args.people, args.frames, args.views
    sc = SyntheticScene(args.dataset, n_views=V, seed=0, device=dev)
    J = sc.n_joints
    rng = np.random.default_rng(1)
    side = int(np.ceil(np.sqrt(K)))
    off = np.array([[((k % side) - (side - 1) / 2) * 1200.0, ((k // side) - (side - 1) / 2) * 1200.0, 0.0] for k in range(K)])
    gt = np.stack([articulated_motion(args.dataset, N, seed=2 + k, drift=(4.0, 2.0, 0.0)) + off[k] for k in range(K)], axis=1)      # (N,K,J,3)
    det = np.zeros((N, V, K, J, 2), dtype=np.float32)
    perm = np.stack([[rng.permutation(K) for _ in range(V)] for _ in range(N)])       # perm[n, v, k]: the slot of person k
    for n in range(N):
        for v, cam in enumerate(sc.cameras):
            for k in range(K):
                det[n, v, perm[n, v, k]] = project_points(cam, gt[n, k]) + rng.normal(0, 3.0, (J, 2))
    gm = GaussianModel().create_from_points(gt[0, 0].astype(np.float32), sc.spatial_lr_scale, J, scene_type=args.dataset, device=dev)
    gm.training_setup()
    pipe = FramePipeline(gm, sc.cameras, frames=args.per_launch, streams=args.streams, dataset=args.dataset, accumulation_steps=V)
    det_dev = torch.as_tensor(det, device=dev)

    def run():
        a = people.associate(sc.cameras, det_dev, max_px=args.assoc_px, max_people=K)
        p2d = a.poses_2d.reshape(N * K, V, J, 2)
        joints = triangulation.triangulate_sequence(sc.cameras, p2d, valid=people.kept(p2d)).reshape(N, K, J, 3)
        t = people.track(joints, max_mm=300.0, max_gap=5, min_joints=5)
        tracks, groups = people.to_tracks(t.track_id, a.poses_2d, K)
        pipe.set_smoothing(2 if args.smooth is None else args.smooth, degree=args.smooth_degree, use_covariance=False, groups=groups)
        out = pipe.optimize_sequence(None, tracks.reshape(K * N, V, J, 2), iterations=args.iters)
        return a, t, out
    run()                                                             # captures the hipGraphs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a, t, out = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assign, tid = a.assign.cpu().numpy(), t.track_id.cpu().numpy()
    # person p is row k of frame n when the row holds p's slot in every view
    who = np.full((N, K), -1)
    for n in range(N):
        for k in range(K):
            hit = np.nonzero((perm[n].T == assign[n, k]).all(axis=1))[0]
            who[n, k] = hit[0] if len(hit) else -1
    associated = int(sum(sorted(who[n]) == list(range(K)) for n in range(N)))
    track_of = {int(who[0, k]): int(tid[0, k]) for k in range(K)}
    tracked = int(sum(all(who[n, k] >= 0 and tid[n, k] == track_of[int(who[n, k])] for k in range(K)) for n in range(N)))
    print(f"{args.dataset} V={V}: {K} people x {N} frames, slots shuffled per frame: {associated} / {N} frames associated correctly, "
          f"{tracked} / {N} tracked correctly ({int(t.n_tracks[0])} tracks, {int(t.n_dropped[0])} dropped, "
          f"{int(a.n_unassigned.sum())} detections unassigned); front end + {args.iters} iterations in {dt * 1e3:.1f} ms")
    pred = out.reshape(K, N, J, 3).cpu().numpy()
    smoothed = pipe.smoothed.joints.reshape(K, N, J, 3).cpu().numpy()
    for p in range(K):
        if p in track_of and 0 <= track_of[p] < K:
            e = np.mean([io.mpjpe(pred[track_of[p], n], gt[n, p]) for n in range(N)])
            es = np.mean([io.mpjpe(smoothed[track_of[p], n], gt[n, p]) for n in range(N)])
            print(f"  person {p} = track {track_of[p]}: mean MPJPE {e:.2f} mm, smoothed within the track {es:.2f} mm")
    return dict(associated=associated, tracked=tracked, frames=N, joints=out)


def main(argv=None):
    """Runs the example; with --report returns what the report lines were printed from (device tensors), else None."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="h36m")
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--per-launch", type=int, default=16)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--init", choices=("host", "device", "fuse"), default="host")
    ap.add_argument("--rigs", type=int, default=1)
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--uncertainty", action="store_true")
    ap.add_argument("--reject-px", type=float, default=None)
    ap.add_argument("--corrupt", type=int, default=0)
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--huber-px", type=float, default=None)
    ap.add_argument("--images", default=None, metavar="DIR")
    ap.add_argument("--image-frames", default=None, metavar="I,J,..")
    ap.add_argument("--smooth", type=int, default=None, metavar="H")
    ap.add_argument("--smooth-degree", type=int, default=2, metavar="D")
    ap.add_argument("--motion", choices=("wobble", "smooth", "articulated"), default="wobble")
    ap.add_argument("--bones", action="store_true")
    ap.add_argument("--bones-symmetric", action="store_true")
    ap.add_argument("--view-weights", choices=("scale", "select"), default=None)
    ap.add_argument("--view-threshold", type=float, default=None, metavar="T")
    ap.add_argument("--people", type=int, default=None, metavar="K")
    ap.add_argument("--assoc-px", type=float, default=15.0, metavar="PX")
    args = ap.parse_args(argv)
    if args.people is not None:
        if not 1 <= args.people <= 8:
            ap.error("--people K: 1 .. 8 people a frame")
        return people_main(args)
    dev = torch.device("cuda:0")
    sc = SyntheticScene(args.dataset, n_views=args.views, seed=0, device=dev)
    rigs = [sc.cameras] + [SyntheticScene(args.dataset, n_views=args.views, seed=r, device=dev).cameras for r in range(1, args.rigs)]
    rig_of = [f % args.rigs for f in range(args.frames)]
    rng = np.random.default_rng(1)
    # a moving skeleton: the template drifts and wobbles from frame to frame; detections carry 3 px of noise
    if args.motion == "wobble":
        gt = np.stack([sc.pose_3d_gt + np.array([8.0 * f, 3.0 * f, 0.0]) + rng.normal(0, 5.0, sc.pose_3d_gt.shape)
                       for f in range(args.frames)])
    elif args.motion == "articulated":      # the same drift; bones of constant length whose directions turn on sinusoids
        from skelsplat_amd.scene import articulated_motion
        gt = articulated_motion(args.dataset, args.frames, sc.pose_3d_gt)
    else:       # the same drift, and per joint and coordinate a sinusoid of 20-60 mm with a period of 25-100 frames
        mrng = np.random.default_rng(2)
        amp, period, phase = (mrng.uniform(lo, hi, sc.pose_3d_gt.shape) for lo, hi in ((20.0, 60.0), (25.0, 100.0), (0.0, 2.0 * np.pi)))
        gt = np.stack([sc.pose_3d_gt + np.array([8.0 * f, 3.0 * f, 0.0]) + amp * np.sin(2.0 * np.pi * f / period + phase)
                       for f in range(args.frames)])
    p2d = np.stack([np.stack([project_points(c, gt[f]) + rng.normal(0, 3.0, (sc.n_points, 2)) for c in rigs[rig_of[f]]])
                    for f in range(args.frames)]).astype(np.float32)
    corrupted = np.zeros((args.frames, args.views, sc.n_points), dtype=bool)
    for f in range(args.frames if args.corrupt else 0):
        for k in rng.choice(args.views * sc.n_points, size=args.corrupt, replace=False):
            r, th = rng.uniform(80.0, 300.0), rng.uniform(0.0, 2.0 * np.pi)
            p2d[f, k // sc.n_points, k % sc.n_points] += (r * np.cos(th), r * np.sin(th))
            corrupted[f, k // sc.n_points, k % sc.n_points] = True
    if args.view_threshold is not None and args.view_weights is None:
        ap.error("--view-threshold is the cosine threshold of --view-weights select")
    if args.uncertainty and not args.report:
        ap.error("--uncertainty measures against --report's ground truth: use the two together")
    if args.smooth is not None and not args.report:
        ap.error("--smooth prints its errors against --report's ground truth: use the two together")
    if args.bones and not args.report:
        ap.error("--bones prints its errors against --report's ground truth: use the two together")
    if args.bones_symmetric and not args.bones:
        ap.error("--bones-symmetric is an option of --bones")
    if args.reject_px is not None and args.init != "device":
        ap.error("--reject-px rejects while triangulating on the device: use it with --init device")
    if args.refine and args.init != "device":
        ap.error("--refine follows the triangulation on the device: use it with --init device")
    if args.huber_px is not None and not args.refine:
        ap.error("--huber-px is the cost of --refine")
    if args.images is not None and args.rigs > 1:
        ap.error("--images pictures frames seen by one rig: use it without --rigs")
    if args.image_frames is not None and args.images is None:
        ap.error("--image-frames chooses the frames of --images DIR")
    Pm = [triangulation.projection_matrices(rig) for rig in rigs]

    def host_init():
        return np.stack([triangulation.triangulate_poses(Pm[rig_of[f]], p2d[f])[:, :3] for f in range(args.frames)]).astype(np.float32)

    gm = GaussianModel().create_from_points(host_init()[0], sc.spatial_lr_scale, sc.n_joints, scene_type=args.dataset, device=dev)
    gm.training_setup()
    steps = -(-args.iters // args.views)        # optimiser steps of a frame: one per accumulation group
    rep = dict(report_steps=steps + 1, save_iterations=(0, args.iters // 2, args.iters)) if args.report else {}
    if args.uncertainty:
        rep["keep_gaussians"] = True
    if args.rigs > 1:
        from skelsplat_amd.rigs import RigBank
        pipe = FramePipeline(gm, rigs=RigBank(rigs, dev), frames=args.per_launch, streams=args.streams, dataset=args.dataset,
                             accumulation_steps=args.views, **rep)
        ids = dict(rig_ids=torch.tensor(rig_of, dtype=torch.int32, device=dev))
    else:
        pipe = FramePipeline(gm, sc.cameras, frames=args.per_launch, streams=args.streams, dataset=args.dataset,
                             accumulation_steps=args.views, **rep)
        ids = {}
    if args.init == "device":
        p2d_dev = torch.as_tensor(p2d, device=dev)
        pipe.set_outlier_rejection(args.reject_px)        # (None: off)
        pipe.set_refinement(16 if args.refine else None, huber_px=args.huber_px)
        run = lambda: pipe.optimize_sequence(None, p2d_dev, iterations=args.iters, return_initial=True, **ids)
    elif args.init == "fuse":
        sigma = np.linspace(20.0, 50.0, args.views)[:, None, None]
        p3d = np.stack([gt[f][None] + rng.normal(0, 1.0, (args.views,) + gt[f].shape) * sigma
                        for f in range(args.frames)]).astype(np.float32)
        p2d_dev, p3d_dev = torch.as_tensor(p2d, device=dev), torch.as_tensor(p3d, device=dev)
        run = lambda: pipe.optimize_sequence(None, p2d_dev, iterations=args.iters, return_initial=True, poses_3d=p3d_dev, **ids)
    else:
        def run():
            init = host_init()
            return pipe.optimize_sequence(init, p2d, iterations=args.iters, **ids), init
    if args.smooth is not None:
        pipe.set_smoothing(args.smooth, degree=args.smooth_degree, use_covariance=args.uncertainty)
    if args.bones:
        pipe.set_bone_constraint("dataset", use_covariance=args.uncertainty or args.smooth is not None,
                                 symmetric=args.bones_symmetric)
    if args.view_weights is not None:
        pipe.set_view_weighting(args.view_weights, 0.5 if args.view_threshold is None else args.view_threshold)
    if args.report:
        pipe.set_reprojection_report()
        gt_dev = torch.as_tensor(gt.astype(np.float32), device=dev)
        optimise = run

        def run():
            pipe.set_ground_truth(gt_dev)       # of the next sequence: its errors are reported against it
            return optimise()
    run()                                                             # captures the hipGraphs
    torch.cuda.synchronize()
    if args.images is not None:
        chosen = ([int(x) for x in args.image_frames.split(",")] if args.image_frames
                  else sorted({0, args.frames // 2, args.frames - 1}))
        pipe.set_debug_images(chosen)       # from the next sequence on; the graphs captured above are replayed as they are
    t0 = time.perf_counter()
    out, init = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pred = out.cpu().numpy()
    init = init.cpu().numpy() if torch.is_tensor(init) else init
    e0 = np.mean([io.mpjpe(init[f], gt[f]) for f in range(args.frames)])
    e1 = np.mean([io.mpjpe(pred[f], gt[f]) for f in range(args.frames)])
    print(f"{args.dataset} V={args.views} {sc.W}x{sc.H}: {args.frames} frames x {args.iters} iterations in {dt * 1e3:.1f} ms "
          f"({args.frames / dt:.0f} frames/s, {args.per_launch} frames per launch on {args.streams} streams, {args.rigs} rig(s)); "
          f"mean MPJPE {e0:.2f} mm ({'fused predictions on the device' if args.init == 'fuse' else f'DLT on the {args.init}'}) "
          f"-> {e1:.2f} mm")
    if args.images is not None:
        dirs = pipe.images.save(args.images, [f"frame_{f:06d}" for f in pipe.images.frames])
        print(f"debug pictures of frames {pipe.images.frames} (heat-maps, first and last render, {args.views} views each): "
              + ", ".join(dirs))
    if args.reject_px is not None:
        plain = host_init()
        ep = np.mean([io.mpjpe(plain[f], gt[f]) for f in range(args.frames)])
        rejected = int((~pipe.inliers).sum())
        fallbacks = int((pipe.n_consensus < 3).sum())
        print(f"initial joints, {args.corrupt} corrupted detections per frame: mean MPJPE {ep:.2f} mm from all views -> {e0:.2f} mm "
              f"with reject_px {args.reject_px:g} ({rejected} detections rejected, {fallbacks} joints without a consensus of 3)")
    if args.refine:
        det = torch.as_tensor(p2d, device=dev)
        Pd = torch.as_tensor(np.stack([Pm[r] for r in rig_of]), device=dev)
        valid = pipe.inliers if args.reject_px is not None else None
        dlt = triangulation.triangulate_sequence(Pd, det, valid=valid).cpu().numpy()
        ed = np.mean([io.mpjpe(dlt[f], gt[f]) for f in range(args.frames)])
        cost = "plain squares" if args.huber_px is None else f"Huber at {args.huber_px:g} px"
        print(f"initial joints: mean MPJPE {ed:.2f} mm from the DLT -> {e0:.2f} mm refined ({cost})")
    if args.report:
        from skelsplat_amd.report import evaluate_sequence, evaluate_sequence_aligned, pose_errors
        r = pipe.report
        curve = r.trace_errors.double().mean(dim=0).cpu().numpy()       # (steps + 1, 2): the sequence's mean after every step
        print("optimiser step   mean abs error   mean root-relative error  (mm, over the sequence)")
        for n in sorted({min(k, steps) for k in (0, 1, 5, 25, steps)}):
            print(f"{n:14d} {curve[n, 0]:16.3f} {curve[n, 1]:26.3f}")
        mid = pose_errors(r.snapshots[:, 1].contiguous(), gt_dev)
        print(f"snapshot of iteration {r.save_iterations[1]}: mean abs error {float(mid[:, 0].mean()):.3f} mm")
        acts = torch.arange(args.frames, device=dev, dtype=torch.int32) * 4 // args.frames       # four "activities" in a row
        valid = torch.ones(args.frames, dtype=torch.bool, device=dev)
        valid[::7] = False      # (stand-ins for the sequences the reference leaves out of the absolute figure)
        ev = evaluate_sequence(out, gt_dev, groups=acts, n_groups=4, abs_valid=valid)
        print(f"evaluate_sequence: abs MPJPE {float(ev['abs']):.3f} mm, rel {float(ev['rel']):.3f} mm; per activity abs "
              + " ".join(f"{x:.2f}" for x in ev["abs_groups"].tolist()) + " | rel "
              + " ".join(f"{x:.2f}" for x in ev["rel_groups"].tolist()))
        eva = evaluate_sequence_aligned(out, gt_dev, groups=acts, n_groups=4)      # one more call on what is on the device
        print(f"evaluate_sequence_aligned: PA-MPJPE {float(eva['pa_mpjpe']):.3f} mm, N-MPJPE {float(eva['n_mpjpe']):.3f} mm; "
              "per activity PA " + " ".join(f"{x:.2f}" for x in eva["pa_mpjpe_groups"].tolist()) + " | N "
              + " ".join(f"{x:.2f}" for x in eva["n_mpjpe_groups"].tolist()))
    if args.report:
        tables = pipe.reprojection.summary()        # two launches on what is on the device; read back here, to print
        for name, t in (("initial", tables["initial"][0].tolist()), ("optimised", tables["final"][0].tolist())):
            print(f"reprojection error of the {name} joints: mean {t[0]:.3f} px; per view "
                  + " ".join(f"{x:.3f}" for x in t[1:1 + args.views]))
    if args.report and args.view_weights is not None:
        w = pipe.view_weights.double()              # (frames, views, joints): every frame's weights at its last step
        print(f"view weights ({args.view_weights}), mean per view: " + " ".join(f"{x:.3f}" for x in w.mean(dim=(0, 2)).tolist()))
        if args.corrupt:
            bad = torch.as_tensor(corrupted[:, :, :sc.n_joints], device=dev)
            print(f"  mean weight of the {int(bad.sum())} corrupted (view, joint) detections {float(w[bad].mean()):.3f}, "
                  f"of the clean ones {float(w[~bad].mean()):.3f}")
    if args.smooth is not None:
        from skelsplat_amd.report import evaluate_sequence
        from skelsplat_amd.smoothing import sequence_accel, smooth_sequence
        rows = [("raw", out), ("smoothed, covariance weights" if args.uncertainty else "smoothed, unit weights", pipe.smoothed.joints)]
        if args.uncertainty:
            rows.append(("smoothed, unit weights", smooth_sequence(out, half_window=args.smooth, degree=args.smooth_degree).joints))
        print(f"temporal smoothing, {args.smooth} frames on each side, degree {args.smooth_degree}, tricube taper ({args.motion} motion):")
        for name, x in rows:
            acc = sequence_accel(x, gt_dev)
            print(f"  {name:30s} MPJPE {float(evaluate_sequence(x, gt_dev)['abs']):7.3f} mm   Accel {float(acc['accel']):7.3f}   "
                  f"Accel error {float(acc['accel_error']):7.3f}  (mm per frame^2)")
    if args.bones:
        from skelsplat_amd import skeleton
        from skelsplat_amd.report import evaluate_sequence, evaluate_sequence_aligned
        from skelsplat_amd.scene import DATASETS
        from skelsplat_amd.smoothing import sequence_accel
        bl, con = pipe.bone_lengths, pipe.constrained
        after = skeleton.bone_lengths(con.joints, DATASETS[args.dataset]["bones"])
        truth = skeleton.bone_lengths(gt_dev, DATASETS[args.dataset]["bones"])
        src = "smoothed" if args.smooth is not None else "optimised"
        print(f"constant limb lengths ({args.motion} motion), the {src} joints under "
              + ("their covariance" if args.uncertainty or args.smooth is not None else "the identity")
              + (", left and right limbs made equal" if args.bones_symmetric else "") + ":")
        print("  bone (parent, child)   median      MAD   frames   ground truth's median")
        for i, (p, c) in enumerate(DATASETS[args.dataset]["bones"]):
            print(f"  {p:6d} {c:6d} {float(bl.length[0, i]):14.2f} {float(bl.mad[0, i]):8.3f} {int(bl.n_used[0, i]):8d} "
                  f"{float(truth.length[0, i]):14.2f}")
        rel = lambda b: float((b.mad / b.length).max())
        print(f"  largest MAD / median over the bones: {rel(bl):.5f} before -> {rel(after):.2e} after the constraint "
              f"(ground truth: {rel(truth):.2e}); trips per frame: mean {float(con.n_trips.double().mean()):.2f}, "
              f"max {int(con.n_trips.max())}; frames with residual > 1e-3 mm: {int((~(con.residual <= 1e-3)).sum())}")
        base = pipe.smoothed.joints if args.smooth is not None else out
        for name, x in ((src, base), ("constrained", con.joints)):
            acc = sequence_accel(x, gt_dev)
            print(f"  {name:12s} MPJPE {float(evaluate_sequence(x, gt_dev)['abs']):7.3f} mm   PA-MPJPE "
                  f"{float(evaluate_sequence_aligned(x, gt_dev)['pa_mpjpe']):7.3f} mm   Accel {float(acc['accel']):7.3f}   "
                  f"Accel error {float(acc['accel_error']):7.3f}")
    if args.uncertainty:
        from skelsplat_amd.uncertainty import calibration
        unc = pipe.gaussians.uncertainty(gt_dev)
        cal = calibration(unc.d2, ks=(1, 2, 3))
        names = [f"joint {j}" for j in range(sc.n_joints)]
        print(f"uncertainty: mean trace of the covariance {float(unc.trace.double().mean()):.1f} mm^2, mean anisotropy "
              f"{float(unc.anisotropy.double().mean()):.2f}")
        print("ground truth inside   1 sigma   2 sigma   3 sigma")
        for name, row in [("all joints", cal["overall"].tolist())] + list(zip(names, cal["per_joint"].tolist())):
            print(f"{name:18s} " + " ".join(f"{100.0 * x:8.1f}%" for x in row))
    res = dict(joints=out, gt=gt_dev, activities=acts, aligned=eva) if args.report else None
    if args.smooth is not None:
        res["smoothed"] = pipe.smoothed
    if args.bones:
        res["bone_lengths"], res["constrained"] = pipe.bone_lengths, pipe.constrained
    return res


if __name__ == "__main__":
    main()
