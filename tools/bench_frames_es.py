#!/usr/bin/env python3
"""Frames per second of a sequence through FramePipeline (H36M, 4 views @ 1000x1000, up to 500 iterations per frame, heat-map
generation included) without and with per-frame early stopping (training.early_stopping = opt_early_stopping, window 4), and
where the frames stopped.  Frames differ in their noise, so that with a suitable tolerance they stop at spread-out iterations.
Usage: bench_frames_es.py [tolerance ...]   (env: N frames, FRAMES per batch, STREAMS, ITERS)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd.loop import FramePipeline, OptEarlyStopping
from skelsplat_amd.scene import SyntheticScene, GaussianModel

dev = torch.device("cuda", 0)
tols = [float(a) for a in sys.argv[1:]] or [3e-4]
N = int(os.environ.get("N", "64"))
FRAMES = int(os.environ.get("FRAMES", "16"))
STREAMS = int(os.environ.get("STREAMS", "2"))
ITERS = int(os.environ.get("ITERS", "500"))
sc = SyntheticScene("h36m", n_views=4, seed=0, device=dev)
rng = np.random.default_rng(1)
base3, base2 = np.asarray(sc.pose_3d_init, np.float32), np.asarray(sc.poses_2d, np.float32)
# frame k: noise grows with k % 8 (0 .. 35 mm, 0 .. 3.5 px): easy frames converge early, hard ones late or not at all
pts = np.stack([base3 + rng.normal(0, 5.0 * (k % 8), base3.shape) for k in range(N)]).astype(np.float32)
p2d = np.stack([base2 + rng.normal(0, 0.5 * (k % 8), base2.shape) for k in range(N)]).astype(np.float32)


def model():
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, device=dev)
    gm.training_setup()
    return gm


def measure(es):
    pipe = FramePipeline(model(), sc.cameras, frames=FRAMES, streams=STREAMS, dataset="h36m",
                         early_stopping="no_stopping" if es is None else OptEarlyStopping(4, es))
    best = None
    for rep in range(3):      # the first pass captures the graphs
        torch.cuda.synchronize(); t0 = time.perf_counter()
        pipe.optimize_sequence(pts, p2d, iterations=ITERS)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return N / best, pipe.stopped_at


fps0, _ = measure(None)
print(f"{N} frames, {STREAMS} streams x {FRAMES} frames, {ITERS} iterations: no_stopping {fps0:.0f} frames/s")
for tol in tols:
    fps, stops = measure(tol)
    s = stops.cpu().numpy()
    hit = s[s > 0]
    spread = (f"stopped {hit.size}/{N}, iterations min {hit.min()} / median {int(np.median(hit))} / max {hit.max()}"
              if hit.size else f"stopped 0/{N}")
    print(f"opt_early_stopping tol {tol:g}: {fps:.0f} frames/s (x{fps / fps0:.2f}); {spread}; "
          f"mean iterations per frame {np.where(s > 0, s, ITERS).mean():.0f}")
