#!/usr/bin/env python3
"""Initial joints fused from per-view 3D predictions (initial_guess.fuse_predictions): the vectorised host path + upload against
the kernel on the device, and what that does to a whole sequence through FramePipeline, predictions to joints.  At (N,V,J) =
(64,4,17), the H36M shape, and (64,31,19), every Panoptic view; three things interleaved, median of REPS repetitions:
  1. fuse_predictions on the device alone: an event pair around the call (which is as long as the host takes to issue it: the
     launch is shorter than its enqueue), its host side by perf_counter, and an event pair around a hipGraph of GRAPH_LAUNCHES
     launches divided by their number (the kernel itself plus the gap to the next node);
  2. the same inside a 64-frame FramePipeline sequence, predictions to joints: optimize_sequence(None, detections,
     poses_3d=predictions), both on the device, against the host path's guess uploaded and passed as `points`;
  3. the vectorised host path + upload of its (N,J,3) result, by perf_counter around a synchronised region: the baseline.
The reference's own way (its script's Python loop over frames x candidates x cameras x joints) is not timed here.
Usage: bench_fuse.py   (env: REPS, STREAMS, ITERS, SKIP_SEQUENCE=1)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd import triangulation
from skelsplat_amd.initial_guess import fuse_predictions
from skelsplat_amd.loop import FramePipeline
from skelsplat_amd.scene import SyntheticScene, GaussianModel

dev = torch.device("cuda", 0)
REPS = max(5, int(os.environ.get("REPS", "20")))
STREAMS = int(os.environ.get("STREAMS", "2"))
ITERS = int(os.environ.get("ITERS", "500"))
GRAPH_LAUNCHES = 50
N = 64


def inputs(sc, V, seed=1):
    """frame k: the scene's detections + a pixel of noise; view v's prediction: ground truth + 20-50 mm of noise; float32"""
    rng = np.random.default_rng(seed)
    base = np.asarray(sc.poses_2d, np.float32)
    p2d = np.stack([base + rng.normal(0, 1.0, base.shape) for k in range(N)]).astype(np.float32)
    gt = np.asarray(sc.pose_3d_gt, np.float64)
    sigma = np.linspace(20.0, 50.0, V)[:, None, None]
    p3d = np.stack([gt[None] + rng.normal(0, 1.0, (V,) + gt.shape) * sigma for k in range(N)]).astype(np.float32)
    return p2d, p3d


def stats(x):
    x = np.sort(np.asarray(x))
    return np.median(x), x[len(x) // 10], x[-1 - len(x) // 10]


for ds, V in (("h36m", 4), ("panoptic", 31)):
    sc = SyntheticScene(ds, n_views=V, seed=0, device=dev)
    J = sc.n_points
    Pm = triangulation.projection_matrices(sc.cameras)
    Pd = torch.as_tensor(Pm, device=dev)
    p2d, p3d = inputs(sc, V)
    p2d_dev, p3d_dev = torch.as_tensor(p2d, device=dev), torch.as_tensor(p3d, device=dev)
    out = torch.empty((N, J, 3), device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fuse_predictions(Pd, p3d_dev, p2d_dev, out=out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_LAUNCHES):
            fuse_predictions(Pd, p3d_dev, p2d_dev, out=out)
    graph.replay()
    ref = torch.as_tensor(fuse_predictions(Pm, p3d, p2d), device=dev)
    torch.cuda.synchronize()
    diff = float((out - ref).abs().max())

    seq = None
    if os.environ.get("SKIP_SEQUENCE") != "1":
        F = min(16, 64 // V)
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scene_type=ds, device=dev)
        gm.training_setup()
        pipe = FramePipeline(gm, sc.cameras, frames=F, streams=STREAMS, dataset=ds, accumulation_steps=V)
        via_device = lambda: pipe.optimize_sequence(None, p2d_dev, iterations=ITERS, poses_3d=p3d_dev)
        via_host = lambda: pipe.optimize_sequence(fuse_predictions(Pm, p3d, p2d), p2d_dev, iterations=ITERS)
        a, b = via_device().clone(), via_host().clone()           # the first pass captures the graphs
        torch.cuda.synchronize()
        seq = (F, float((a - b).abs().max()))
        print(f"{ds}: sequence warmed ({F} frames per launch)", flush=True)

    t_host, t_dev, t_call, t_graph, t_seq_dev, t_seq_host = [], [], [], [], [], []
    for _ in range(REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        up = torch.as_tensor(fuse_predictions(Pm, p3d, p2d)).to(dev)
        torch.cuda.synchronize(); t_host.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        e0.record()
        fuse_predictions(Pd, p3d_dev, p2d_dev, out=out)
        e1.record()
        t_call.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize(); t_dev.append(e0.elapsed_time(e1) * 1e3)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize(); t_graph.append(e0.elapsed_time(e1) * 1e3 / GRAPH_LAUNCHES)
        if seq is not None:
            for fn, ts in ((via_device, t_seq_dev), (via_host, t_seq_host)):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    h, d, c, g = stats(t_host), stats(t_dev), stats(t_call), stats(t_graph)
    print(f"{ds:8s} V={V:2d} J={J} N={N}, median [p10 .. p90] of {REPS} interleaved repetitions: host path + upload {h[0]:8.3f} ms "
          f"[{h[1]:.3f} .. {h[2]:.3f}]; device call (event pair) {d[0]:6.1f} us [{d[1]:.1f} .. {d[2]:.1f}], its host side "
          f"{c[0] * 1e3:.0f} us; per launch in a hipGraph of {GRAPH_LAUNCHES} {g[0]:6.2f} us [{g[1]:.2f} .. {g[2]:.2f}]; "
          f"max |device - host| {diff:.2e} mm (float32 joints)", flush=True)
    if seq is not None:
        sd, sh = stats(t_seq_dev), stats(t_seq_host)
        print(f"{ds:8s} predictions to joints, {N} frames, {STREAMS} streams x {seq[0]} frames, {ITERS} iterations: fused on the device "
              f"{sd[0]:8.3f} ms [{sd[1]:.3f} .. {sd[2]:.3f}] {N / sd[0] * 1e3:6.0f} frames/s; host path + upload "
              f"{sh[0]:8.3f} ms [{sh[1]:.3f} .. {sh[2]:.3f}] {N / sh[0] * 1e3:6.0f} frames/s; max |joints difference| {seq[1]:.2e} mm",
              flush=True)
