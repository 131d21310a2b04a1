#!/usr/bin/env python3
"""The reprojection kernels: reprojection.reproject (one launch: uv, err, in_front and the three means) and
reprojection.refine_triangulation (one launch: damped Gauss-Newton from the DLT, plain squares) against the same formulas as
batched tensor ops on the device, in float64 like the kernels:
  reproject, tensor ops   einsum of the projection matrices with [X; 1], the division, the norm, nanmean over views / joints / both;
  refine, tensor ops      TRIPS undamped-but-for-lambda Gauss-Newton trips for every joint at once -- Jacobians, the 3 x 3 normal
                          equations by einsum, torch.linalg.solve, a masked accept --, TRIPS = the most trips the kernel's joints
                          took on the same data (so the tensor-op way does no more arithmetic than the kernel's slowest joint).
N = 64, 1 024 and 16 384 frames of 4 views x 17 joints and 31 views x 19 joints.  Per way: the median [p10 .. p90] of REPS
repetitions, the ways interleaved inside every repetition (so drift in clocks or load falls on all of them alike), each by an event
pair around the call on a synchronised stream; the kernel ways also per call inside a hipGraph of GRAPH_LAUNCHES calls (the
kernel plus the gap to the next node, without the host's enqueue time).
Usage: bench_reproject.py   (env: REPS)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd import reprojection, triangulation
from skelsplat_amd.scene import SyntheticScene, project_points

dev = torch.device("cuda", 0)
REPS = max(20, int(os.environ.get("REPS", "20")))
GRAPH_LAUNCHES = 50


def frames(dataset, V, N, seed=1):
    """P (V,3,4) float64, detections (N,V,J,2) float32 on the device: eight distinct frames with 3 px of noise, repeated with a
    pixel of noise each"""
    sc = SyntheticScene(dataset, n_views=V, seed=0, device="cpu")
    rng = np.random.default_rng(seed)
    gt = np.stack([sc.pose_3d_gt + np.array([8.0 * f, 3.0 * f, 0.0]) + rng.normal(0, 5.0, sc.pose_3d_gt.shape) for f in range(8)])
    base = np.stack([np.stack([project_points(c, gt[f]) + rng.normal(0, 3.0, (sc.n_points, 2)) for c in sc.cameras]) for f in range(8)])
    p2d = (base[np.arange(N) % 8] + rng.normal(0, 1.0, (N,) + base.shape[1:])).astype(np.float32)
    return torch.as_tensor(triangulation.projection_matrices(sc.cameras), device=dev), torch.as_tensor(p2d, device=dev)


def project_ops(P, X):
    u = torch.einsum("vrk,njk->nvjr", P[..., :3], X) + P[None, :, None, :, 3]
    return u[..., :2] / u[..., 2:3], u[..., 2]


def reproject_ops(P, X, det):
    uv, depth = project_ops(P, X.double())
    err = (uv - det.double()).norm(dim=-1)
    return uv, err, depth > 0, err.nanmean(dim=1), err.nanmean(dim=2), err.nanmean(dim=(1, 2))


def refine_ops(P, det, X0, trips):
    X, d = X0.double().clone(), det.double()
    lam = torch.full(X.shape[:2], 1e-3, dtype=torch.float64, device=dev)
    cost_of = lambda Y: ((project_ops(P, Y)[0] - d) ** 2).sum(dim=(1, 3))
    cost = cost_of(X)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    for _ in range(trips):
        uv, depth = project_ops(P, X)
        Jm = (P[None, :, None, :2, :3] - uv[..., None] * P[None, :, None, 2:3, :3]) / depth[..., None, None]      # (N,V,J,2,3)
        A = torch.einsum("nvjra,nvjrb->njab", Jm, Jm)
        g = torch.einsum("nvjra,nvjr->nja", Jm, uv - d)
        A = A + lam[..., None, None] * (A * eye)
        T = X + torch.linalg.solve(A, -g[..., None])[..., 0]
        tcost = cost_of(T)
        ok = tcost < cost
        X, cost = torch.where(ok[..., None], T, X), torch.where(ok, tcost, cost)
        lam = torch.where(ok, lam * 0.1, lam * 10.0)
    return X


def stats(x):
    x = np.sort(np.asarray(x))
    return np.median(x), x[len(x) // 10], x[-1 - len(x) // 10]


def fmt(m):
    return f"{m[0]:9.1f} us [{m[1]:.1f} .. {m[2]:.1f}]"


solve_on_device = True
try:
    Pw, dw = frames("h36m", 4, 4)
    refine_ops(Pw, dw, triangulation.triangulate_sequence(Pw, dw), 2)
    torch.cuda.synchronize()
except Exception as e:      # (a build without a device solver raises here; nothing falls back silently)
    solve_on_device = False
    print(f"torch.linalg.solve cannot run on the device in this torch build ({type(e).__name__}: {e}): no tensor-op refine column")

print(f"-- reprojection kernels, median [p10 .. p90] of {REPS} interleaved repetitions")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for dataset, V in (("h36m", 4), ("panoptic", 31)):
    for N in (64, 1024, 16384):
        P, det = frames(dataset, V, N)
        J = det.shape[2]
        X0 = triangulation.triangulate_sequence(P, det)
        refined, iters = reprojection.refine_triangulation(P, det, X0, return_iters=True)
        trips = int(iters.max())
        ways = {"reproject": lambda: reprojection.reproject(P, X0, det),
                "refine": lambda: reprojection.refine_triangulation(P, det, X0),
                "reproject, tensor ops": lambda: reproject_ops(P, X0, det)}
        if solve_on_device:
            ways["refine, tensor ops"] = lambda: refine_ops(P, det, X0, trips)
        graphs = {}
        for name in ("reproject", "refine"):
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
        diff_r = float((reproject_ops(P, X0, det)[1] - reprojection.reproject(P, X0, det).err).abs().max())
        diff_f = float((refine_ops(P, det, X0, trips) - refined.double()).norm(dim=-1).max()) if solve_on_device else float("nan")
        t = {name: [] for name in ways}
        t.update({name + ", in a graph": [] for name in graphs})
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
        m = {k: stats(v) for k, v in t.items()}
        print(f"V={V} J={J} N={N:5d}: reproject {fmt(m['reproject'])}, in a hipGraph of {GRAPH_LAUNCHES} {fmt(m['reproject, in a graph'])}; "
              f"tensor ops {fmt(m['reproject, tensor ops'])} (max |difference| {diff_r:.2e} px)")
        print(f"V={V} J={J} N={N:5d}: refine ({trips} trips at most, histogram {torch.bincount(iters.flatten()).tolist()}) {fmt(m['refine'])}, "
              f"in a hipGraph {fmt(m['refine, in a graph'])}"
              + (f"; tensor ops, {trips} trips {fmt(m['refine, tensor ops'])} (max distance {diff_f:.2e} mm)" if solve_on_device else ""))
