#!/usr/bin/env python3
"""Aligned pose errors: report.aligned_pose_errors (one launch, "similarity" mode: a frame's PA-MPJPE) and
report.evaluate_sequence_aligned (three launches: a sequence's PA-MPJPE and N-MPJPE) against two ways of getting the same
numbers without the kernel:
  tensor ops   the same formula as batched tensor ops on the device -- centroids, einsum, torch.linalg.svd of the N 3x3
               cross-covariances, the reflection repair, the norms --, in float64 like the kernel; if this torch build cannot
               run torch.linalg.svd on the device the line says so and the column is left out;
  host         io.pa_mpjpe / io.n_mpjpe in numpy on the downloaded joints, the download included.
N = 64, 1 024 and 16 384 frames of P = 17 and 19 joints.  Per way: the median [p10 .. p90] of REPS repetitions, the ways
interleaved inside every repetition (so drift in clocks or load falls on all of them alike); the device ways by an event pair
around the call on a synchronised stream, the kernel way also per call inside a hipGraph of GRAPH_LAUNCHES calls (the kernels
plus the gap to the next node, without the host's enqueue time); the host way by perf_counter around a synchronised region.
Usage: bench_align.py   (env: REPS, HOST_REPS: the numpy way is slow at 16 384 frames and runs that many times)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd import io, report

dev = torch.device("cuda", 0)
REPS = max(20, int(os.environ.get("REPS", "20")))
HOST_REPS = max(3, int(os.environ.get("HOST_REPS", "3")))
GRAPH_LAUNCHES = 50


def poses(N, P, seed=1):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(-2000.0, 2000.0, (N, 1, 3)) + rng.uniform(-1000.0, 1000.0, (N, P, 3))
    return (gt + rng.normal(0.0, 40.0, gt.shape)).astype(np.float32), gt.astype(np.float32)


def pa_tensor_ops(pred, gt):
    """per-frame PA-MPJPE as batched tensor ops, float64 inside: (N,) float32"""
    x, y = pred.double(), gt.double()
    mx, my = x.mean(dim=1, keepdim=True), y.mean(dim=1, keepdim=True)
    x, y = x - mx, y - my
    H = torch.einsum("nia,nib->nab", x, y)
    U, S, Vh = torch.linalg.svd(H)
    V = Vh.transpose(1, 2)
    d = torch.ones_like(S)
    d[:, 2] = torch.sign(torch.linalg.det(V @ U.transpose(1, 2)))
    R = (V * d[:, None, :]) @ U.transpose(1, 2)
    s = (S * d).sum(dim=1) / (x * x).sum(dim=(1, 2))
    aligned = s[:, None, None] * (x @ R.transpose(1, 2)) + my
    return (y + my - aligned).norm(dim=2).mean(dim=1).float()


def n_tensor_ops(pred, gt):
    x, y = (pred - pred[:, :1]).double(), (gt - gt[:, :1]).double()
    s = (x * y).sum(dim=(1, 2)) / (x * x).sum(dim=(1, 2))
    return (y - s[:, None, None] * x).norm(dim=2)


def sequence_tensor_ops(pred, gt):
    return pa_tensor_ops(pred, gt).double().mean(), n_tensor_ops(pred, gt).mean()


def stats(x):
    x = np.sort(np.asarray(x))
    return np.median(x), x[len(x) // 10], x[-1 - len(x) // 10]


def fmt(m, unit="us"):
    return f"{m[0]:9.1f} {unit} [{m[1]:.1f} .. {m[2]:.1f}]"


svd_on_device = True
try:
    pa_tensor_ops(*(torch.as_tensor(a, device=dev) for a in poses(4, 17)))
    torch.cuda.synchronize()
except Exception as e:      # (a build without a device SVD raises here; nothing falls back silently)
    svd_on_device = False
    print(f"torch.linalg.svd cannot run on the device in this torch build ({type(e).__name__}: {e}): no tensor-op column")

print(f"-- aligned errors, median [p10 .. p90] of {REPS} interleaved repetitions (host way: {HOST_REPS})")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for P in (17, 19):
    for N in (64, 1024, 16384):
        pred_np, gt_np = poses(N, P)
        pred, gt = torch.as_tensor(pred_np, device=dev), torch.as_tensor(gt_np, device=dev)
        ways = {"aligned_pose_errors": lambda: report.aligned_pose_errors(pred, gt),
                "evaluate_sequence_aligned": lambda: report.evaluate_sequence_aligned(pred, gt)}
        if svd_on_device:
            ways["tensor ops, per frame"] = lambda: pa_tensor_ops(pred, gt)
            ways["tensor ops, sequence"] = lambda: sequence_tensor_ops(pred, gt)
        graphs = {}
        for name in ("aligned_pose_errors", "evaluate_sequence_aligned"):
            for _ in range(3):
                ways[name]()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(GRAPH_LAUNCHES):
                    ways[name]()
            graphs[name].replay()
        for fn in ways.values():
            fn()
        torch.cuda.synchronize()
        ev = report.evaluate_sequence_aligned(pred, gt)
        host = (io.pa_mpjpe(pred_np, gt_np), io.n_mpjpe(pred_np, gt_np))
        diff = max(abs(float(ev["pa_mpjpe"]) - host[0]), abs(float(ev["n_mpjpe"]) - host[1]))
        if svd_on_device:
            diff_t = float((pa_tensor_ops(pred, gt) - report.aligned_pose_errors(pred, gt)).abs().max())
        t = {name: [] for name in ways}
        t.update({name + ", in a graph": [] for name in graphs})
        t["host"] = []
        for r in range(REPS):
            for name, fn in ways.items():
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize(); t[name].append(e0.elapsed_time(e1) * 1e3)
            for name, graph in graphs.items():
                e0.record()
                graph.replay()
                e1.record()
                torch.cuda.synchronize(); t[name + ", in a graph"].append(e0.elapsed_time(e1) * 1e3 / GRAPH_LAUNCHES)
            if r < HOST_REPS:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                hp, hg = pred.cpu().numpy(), gt.cpu().numpy()
                io.pa_mpjpe(hp, hg), io.n_mpjpe(hp, hg)
                t["host"].append((time.perf_counter() - t0) * 1e3)
        m = {k: stats(v) for k, v in t.items()}
        print(f"P={P} N={N:5d}: aligned_pose_errors {fmt(m['aligned_pose_errors'])}, in a hipGraph of {GRAPH_LAUNCHES} "
              f"{fmt(m['aligned_pose_errors, in a graph'])}"
              + (f"; tensor ops {fmt(m['tensor ops, per frame'])} (max |difference| {diff_t:.2e} mm)" if svd_on_device else ""))
        print(f"P={P} N={N:5d}: evaluate_sequence_aligned {fmt(m['evaluate_sequence_aligned'])}, in a hipGraph "
              f"{fmt(m['evaluate_sequence_aligned, in a graph'])}"
              + (f"; tensor ops {fmt(m['tensor ops, sequence'])}" if svd_on_device else "")
              + f"; download + numpy {fmt(m['host'], 'ms')}; max |device - host| {diff:.2e} mm")
