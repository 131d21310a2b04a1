#!/usr/bin/env python3
"""Initial joints by DLT: the host path (triangulation.triangulate_poses per frame in a Python loop + upload, what
examples/optimize_sequence.py --init host does) against the batched kernel (triangulation.triangulate_sequence on the device),
and what that does to a whole sequence through FramePipeline, detections to joints.
  1. H36M shape (4 views, 17 joints) and Panoptic shape (31 views, 19 joints), N = 64 and 1 024 frames: ms per batch -- the host
     path by perf_counter around a synchronised region, the device path by an event pair around the call (which is as long as
     the host takes to issue it: the launch is shorter than its enqueue) and by an event pair around a hipGraph of GRAPH_LAUNCHES
     launches, divided by their number (the kernel itself plus the gap to the next node); median of REPS interleaved repetitions.
     The kernel's own duration: rocprofv3 --kernel-trace --stats -- python tools/bench_triangulate.py with SKIP_SEQUENCE=1.
     The robust line: the same detections with outliers (per joint 0 .. (V - 2) // 2 views moved by 80 .. 300 px), reject_px =
     REJECT_PX: sks_triangulate_robust (consensus kernel + the plain kernel) the same three ways, against the plain call on the
     same detections in the same repetitions and against the vectorised host path (consensus_cpu + batched SVD) plus upload.
  2. 64 H36M frames @ 1000x1000, 500 iterations, no_stopping and opt_early_stopping at 1e-3 (tools/bench_frames_es.py's setting):
     host DLT + upload + optimize_sequence(init, detections) against optimize_sequence(None, detections on the device), interleaved;
     no_stopping also with reject_px, and new_scenes of one batch alone with and without it (what the consensus adds in
     front of a frame).
Usage: bench_triangulate.py   (env: REPS, FRAMES per batch, STREAMS, ITERS, REJECT_PX, SKIP_SEQUENCE=1)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd import triangulation
from skelsplat_amd.loop import FramePipeline, OptEarlyStopping
from skelsplat_amd.scene import SyntheticScene, GaussianModel

dev = torch.device("cuda", 0)
REPS = max(20, int(os.environ.get("REPS", "20")))
FRAMES = int(os.environ.get("FRAMES", "16"))
STREAMS = int(os.environ.get("STREAMS", "2"))
ITERS = int(os.environ.get("ITERS", "500"))
GRAPH_LAUNCHES = 50
REJECT_PX = float(os.environ.get("REJECT_PX", "20"))


def detections(sc, N, seed=1):
    """frame k: the scene's detections + (k % 8) x 0.5 px of noise, float32 (as tools/bench_frames_es.py)"""
    rng = np.random.default_rng(seed)
    base = np.asarray(sc.poses_2d, np.float32)
    return np.stack([base + rng.normal(0, 0.5 * (k % 8), base.shape) for k in range(N)]).astype(np.float32)


def with_outliers(p2d, seed=17):
    """per joint, k views drawn from 0 .. (V - 2) // 2 moved by 80 .. 300 px in a random direction"""
    rng = np.random.default_rng(seed)
    N, V, J = p2d.shape[:3]
    x = p2d.copy()
    k = rng.integers(0, (V - 2) // 2 + 1, (N, 1, J))
    bad = np.argsort(rng.random((N, V, J)), axis=1) < k
    r, th = rng.uniform(80.0, 300.0, (N, V, J)), rng.uniform(0.0, 2.0 * np.pi, (N, V, J))
    x += (bad * r)[..., None] * np.stack([np.cos(th), np.sin(th)], -1)
    return x.astype(np.float32), bad


def host_init(Pm, p2d):
    """today's way: one LAPACK batch per frame, then one upload"""
    init = np.stack([triangulation.triangulate_poses(Pm, p2d[f])[:, :3] for f in range(p2d.shape[0])]).astype(np.float32)
    return init


def stats(x):
    x = np.sort(np.asarray(x))
    return np.median(x), x[len(x) // 10], x[-1 - len(x) // 10]


print(f"-- DLT alone, median [p10 .. p90] of {REPS} interleaved repetitions")
for ds, V in (("h36m", 4), ("panoptic", 31)):
    sc = SyntheticScene(ds, n_views=V, seed=0, device=dev)
    Pm = triangulation.projection_matrices(sc.cameras)
    Pd = torch.as_tensor(Pm, device=dev)
    for N in (64, 1024):
        p2d = detections(sc, N)
        p2d_dev = torch.as_tensor(p2d, device=dev)
        out = torch.empty((N, sc.n_points, 3), device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            triangulation.triangulate_sequence(Pd, p2d_dev, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(GRAPH_LAUNCHES):
                triangulation.triangulate_sequence(Pd, p2d_dev, out=out)
        graph.replay()
        ref = torch.as_tensor(host_init(Pm, p2d), device=dev)
        torch.cuda.synchronize()
        diff = float((out - ref).abs().max())
        t_host, t_dev, t_call, t_graph = [], [], [], []
        for _ in range(REPS):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            up = torch.as_tensor(host_init(Pm, p2d)).to(dev)
            torch.cuda.synchronize(); t_host.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            e0.record()
            triangulation.triangulate_sequence(Pd, p2d_dev, out=out)
            e1.record()
            t_call.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize(); t_dev.append(e0.elapsed_time(e1) * 1e3)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize(); t_graph.append(e0.elapsed_time(e1) * 1e3 / GRAPH_LAUNCHES)
        h, d, c, g = stats(t_host), stats(t_dev), stats(t_call), stats(t_graph)
        print(f"{ds:8s} V={V:2d} J={sc.n_points} N={N:4d}: host DLT + upload {h[0]:8.3f} ms [{h[1]:.3f} .. {h[2]:.3f}]; "
              f"device call (event pair) {d[0]:6.1f} us [{d[1]:.1f} .. {d[2]:.1f}], its host side {c[0] * 1e3:.0f} us; "
              f"per launch in a hipGraph of {GRAPH_LAUNCHES} {g[0]:6.2f} us [{g[1]:.2f} .. {g[2]:.2f}]; "
              f"max |device - host| {diff:.2e} mm (float32 joints)")
        if N != 64:
            continue
        # ---- the robust call on detections with outliers, against the plain call on the same detections
        x_np, bad = with_outliers(p2d)
        x_dev = torch.as_tensor(x_np, device=dev)
        inl = torch.empty((N, V, sc.n_points), dtype=torch.bool, device=dev)
        n_cons = torch.empty((N, sc.n_points), dtype=torch.int32, device=dev)
        plain_fn = lambda: triangulation.triangulate_sequence(Pd, x_dev, out=out)
        robust_fn = lambda: triangulation.triangulate_sequence(Pd, x_dev, out=out, reject_px=REJECT_PX, out_inliers=(inl, n_cons))
        graphs = {}
        for name, fn in (("plain", plain_fn), ("robust", robust_fn)):
            for _ in range(3):
                fn()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(GRAPH_LAUNCHES):
                    fn()
            graphs[name].replay()
        torch.cuda.synchronize()
        found = int((inl.cpu().numpy() == ~bad).all(axis=1).sum())
        host = triangulation.triangulate_sequence(Pm, x_np, reject_px=REJECT_PX)
        diff = float((out.cpu() - torch.as_tensor(host)).abs().max())
        t = {k: [] for k in ("host", "plain", "robust", "plain graph", "robust graph")}
        for _ in range(REPS):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            up = torch.as_tensor(triangulation.triangulate_sequence(Pm, x_np, reject_px=REJECT_PX)).to(dev)
            torch.cuda.synchronize(); t["host"].append((time.perf_counter() - t0) * 1e3)
            for name, fn in (("plain", plain_fn), ("robust", robust_fn)):
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize(); t[name].append(e0.elapsed_time(e1) * 1e3)
                e0.record()
                graphs[name].replay()
                e1.record()
                torch.cuda.synchronize(); t[name + " graph"].append(e0.elapsed_time(e1) * 1e3 / GRAPH_LAUNCHES)
        m = {k: stats(v) for k, v in t.items()}
        print(f"{ds:8s} V={V:2d} J={sc.n_points} N={N:4d} robust, reject_px {REJECT_PX:g}: vectorised host path + upload "
              f"{m['host'][0]:8.3f} ms [{m['host'][1]:.3f} .. {m['host'][2]:.3f}]; device call (event pair) robust "
              f"{m['robust'][0]:6.1f} us [{m['robust'][1]:.1f} .. {m['robust'][2]:.1f}] / plain {m['plain'][0]:6.1f} us; per call "
              f"in a hipGraph of {GRAPH_LAUNCHES}: robust {m['robust graph'][0]:6.2f} us [{m['robust graph'][1]:.2f} .. "
              f"{m['robust graph'][2]:.2f}] / plain {m['plain graph'][0]:6.2f} us [{m['plain graph'][1]:.2f} .. "
              f"{m['plain graph'][2]:.2f}]; joints whose inliers are exactly the views left alone: {found} of {N * sc.n_points}; max |device - host| {diff:.2e} mm")

if os.environ.get("SKIP_SEQUENCE") == "1":
    sys.exit(0)

N = 64
sc = SyntheticScene("h36m", n_views=4, seed=0, device=dev)
Pm = triangulation.projection_matrices(sc.cameras)
p2d = detections(sc, N)
p2d_dev = torch.as_tensor(p2d, device=dev)


def model():
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, device=dev)
    gm.training_setup()
    return gm


print(f"-- detections to joints, {N} H36M frames, {STREAMS} streams x {FRAMES} frames, {ITERS} iterations, "
      f"median [p10 .. p90] of {REPS} interleaved repetitions")
for es in (None, 1e-3):
    pipe = FramePipeline(model(), sc.cameras, frames=FRAMES, streams=STREAMS, dataset="h36m",
                         early_stopping="no_stopping" if es is None else OptEarlyStopping(4, es))

    def via_host():
        return pipe.optimize_sequence(host_init(Pm, p2d), p2d, iterations=ITERS)

    def via_device():
        return pipe.optimize_sequence(None, p2d_dev, iterations=ITERS)

    def via_device_upload():          # detections still on the host: their upload is inside the timed region
        return pipe.optimize_sequence(None, torch.as_tensor(p2d).to(dev), iterations=ITERS)

    def via_device_robust():          # (detections without outliers: what the consensus costs, not what it saves)
        pipe.set_outlier_rejection(REJECT_PX)
        try:
            return pipe.optimize_sequence(None, p2d_dev, iterations=ITERS)
        finally:
            pipe.set_outlier_rejection(None)

    ways = (("host DLT + upload", via_host), ("device DLT", via_device), ("device DLT, detections uploaded", via_device_upload))
    if es is None:
        ways += ((f"device DLT, reject_px {REJECT_PX:g}", via_device_robust),)
    res = {}
    for name, fn in ways:             # the first pass captures the graphs
        res[name] = fn().clone()
    torch.cuda.synchronize()
    same = all(torch.equal(res[ways[0][0]], res[name]) for name, _ in ways[:3])
    rejected = int((~pipe.inliers).sum()) if es is None else 0      # (a view 20 px off its joint's best pair changes that joint)
    times = {name: [] for name, _ in ways}
    for _ in range(REPS):
        for name, fn in ways:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); times[name].append((time.perf_counter() - t0) * 1e3)
    tag = "no_stopping" if es is None else f"opt_early_stopping tol {es:g}"
    for name, _ in ways:
        m = stats(times[name])
        print(f"{tag:32s} {name:34s} {m[0]:8.3f} ms [{m[1]:.3f} .. {m[2]:.3f}]  {N / m[0] * 1e3:7.0f} frames/s")
    stops = "" if pipe.stopped_at is None else (lambda s: f"; stopping iterations min {s.min()} / median {int(np.median(s))} / "
                                                f"max {s.max()} (0: ran to the end)")(pipe.stopped_at.cpu().numpy())
    print(f"{tag:32s} joints identical across the three ways without rejection: {same}{stops}"
          + (f"; reject_px {REJECT_PX:g} rejected {rejected} of {pipe.inliers.numel()} detections" if es is None else ""))

# what the consensus adds to new_scenes, in front of the frames it starts
fb = pipe.loops[0]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t = {None: [], REJECT_PX: []}
for r in range(REPS + 2):
    for tau in t:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fb.set_outlier_rejection(tau).new_scenes(None, poses_2d=p2d_dev[:FRAMES])
        torch.cuda.synchronize()
        if r >= 2:
            t[tau].append((time.perf_counter() - t0) * 1e3)
a, b = stats(t[None]), stats(t[REJECT_PX])
print(f"new_scenes(None, detections) of {FRAMES} frames, synchronised: {a[0]:.3f} ms [{a[1]:.3f} .. {a[2]:.3f}] plain, "
      f"{b[0]:.3f} ms [{b[1]:.3f} .. {b[2]:.3f}] with reject_px {REJECT_PX:g}")
