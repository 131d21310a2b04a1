#!/usr/bin/env python3
"""Constant limb lengths: the three launches of skeleton.bone_lengths + skeleton.project_to_lengths (measure, medians and MADs,
projection; covariances as the metric, and the identity) against
  tensor ops           the same definition as batched float64 tensor ops on the device: norms of the bones' differences,
                       torch.median (the lower median) over the frames twice, then per trip the directions, A Sigma A^T by
                       einsum, one torch.linalg.solve and the step, for the number of trips the slowest frame of the kernel took
                       (no per-frame exit: every frame takes every trip);
  download + host      the joints (and covariances) copied to the host and skeleton's float64 numpy functions (wall clock).
N = 64, 1 024 and 16 384 frames of J = 17 (H36M's tree) and 19 (Panoptic's) joints: template poses with 10 mm of noise drawn from
needle covariances of std ratio 3.  Per way: the median [p10 .. p90] of REPS repetitions, the device ways interleaved inside every
repetition (so drift in clocks or load falls on all of them alike), each by an event pair around the calls on a synchronised
stream; the kernels also per call inside a hipGraph of GRAPH_LAUNCHES calls (the three kernels plus the gaps to the next node,
without the host's enqueue time).
Usage: bench_bones.py   (env: REPS, HOST_REPS)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd import _lib, skeleton
from skelsplat_amd.scene import DATASETS, skeleton_template

dev = torch.device("cuda", 0)
REPS = max(20, int(os.environ.get("REPS", "20")))
HOST_REPS = max(3, int(os.environ.get("HOST_REPS", "3")))
GRAPH_LAUNCHES = 20
NOISE, RATIO = 10.0, 3.0


def sequence(N, dataset, seed=1):
    """xyz (N,J,3), cov6 (N,J,6) float32 on the device."""
    rng = np.random.default_rng(seed)
    t = skeleton_template(dataset)
    J = t.shape[0]
    v = rng.normal(size=(N, J, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    small = NOISE / RATIO
    C = small ** 2 * np.eye(3) + (NOISE ** 2 - small ** 2) * v[..., :, None] * v[..., None, :]
    x = t[None] + rng.uniform(-2000, 2000, (N, 1, 3)) + np.einsum("njab,njb->nja", np.linalg.cholesky(C), rng.normal(size=(N, J, 3)))
    cov6 = C[..., [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    return torch.as_tensor(x.astype(np.float32), device=dev), torch.as_tensor(cov6.astype(np.float32), device=dev)


def bones_ops(xyz, cov6, bones, trips):
    """(length (B,), mad (B,), joints (N,J,3) float64) by batched tensor ops; every frame of the inputs is finite."""
    N, J = xyz.shape[:2]
    p, c = bones[:, 0], bones[:, 1]
    B = p.shape[0]
    X = xyz.double()
    l = (X[:, c] - X[:, p]).norm(dim=-1).float()
    length = l.median(dim=0).values
    mad = (l - length).abs().median(dim=0).values
    Sig = (torch.eye(3, dtype=torch.float64, device=dev).expand(N, J, 3, 3) if cov6 is None
           else cov6.double()[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(N, J, 3, 3))
    inc = torch.zeros((B, J), dtype=torch.float64, device=dev)      # the incidence matrix: +1 at the child, -1 at the parent
    rows = torch.arange(B, device=dev)
    inc[rows, c], inc[rows, p] = 1.0, -1.0
    L = length.double()
    for _ in range(trips):
        d = X[:, c] - X[:, p]
        n = d.norm(dim=-1)
        u = d / n[..., None]
        A = inc[None, :, :, None] * u[:, :, None, :]                                  # (N,B,J,3)
        SA = torch.einsum("njrs,nbjs->nbjr", Sig, A)                                   # Sigma A^T, (N,B,J,3)
        S = torch.einsum("najr,nbjr->nab", A, SA)
        lam = torch.linalg.solve(S, (n - L)[..., None])[..., 0]
        X = X - torch.einsum("nb,nbjr->njr", lam, SA)
    return length, mad, X


def stats(x):
    x = np.sort(np.asarray(x))
    return np.median(x), x[len(x) // 10], x[-1 - len(x) // 10]


def fmt(m):
    return f"{m[0]:9.1f} us [{m[1]:.1f} .. {m[2]:.1f}]"


solve_on_device = True
try:
    xw, cw = sequence(32, "h36m")
    bones_ops(xw, cw, torch.as_tensor(DATASETS["h36m"]["bones"], device=dev), 2)
    torch.cuda.synchronize()
except Exception as e:      # (a build without a device solver raises here; nothing falls back silently)
    solve_on_device = False
    print(f"torch.linalg.solve cannot run on the device in this torch build ({type(e).__name__}: {e}): no tensor-op column")

print(f"-- constant limb lengths, {NOISE:g} mm of noise, needles of std ratio {RATIO:g}: median [p10 .. p90] of {REPS} interleaved "
      f"repetitions (host: {HOST_REPS}, wall clock)")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for dataset in ("h36m", "panoptic"):
    bones = DATASETS[dataset]["bones"]
    bones_dev = torch.as_tensor(bones, device=dev)
    for N in (64, 1024, 16384):
        xyz, cov6 = sequence(N, dataset)
        J, B = xyz.shape[1], len(bones)
        la = _lib.bones_launch(N, J, B, 1)
        for label, cov in (("covariances", cov6), ("identity", None)):
            def kernel():
                bl = skeleton.bone_lengths(xyz, bones)
                return bl, skeleton.project_to_lengths(xyz, bones, bl.length, cov)
            for _ in range(3):
                bl, got = kernel()
            torch.cuda.synchronize()
            trips = int(got.n_trips.max())
            unconverged = int((~(got.residual <= 1e-3)).sum())
            ways = {"kernels": kernel}
            if solve_on_device:
                ways["tensor ops"] = lambda: bones_ops(xyz, cov, bones_dev, trips)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(GRAPH_LAUNCHES):
                    kernel()
            graph.replay()
            for fn in ways.values():
                fn()
            torch.cuda.synchronize()
            diff = float("nan")
            if solve_on_device:
                ops = bones_ops(xyz, cov, bones_dev, trips)
                same_medians = bool((ops[0] == bl.length[0]).all() and (ops[1] == bl.mad[0]).all())
                diff = float((ops[2] - got.joints.double()).abs().max())
            t = {name: [] for name in ways}
            t["kernels, in a graph"] = []
            for r in range(REPS):
                for name, fn in ways.items():
                    torch.cuda.synchronize()
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize(); t[name].append(e0.elapsed_time(e1) * 1e3)
                e0.record()
                graph.replay()
                e1.record()
                torch.cuda.synchronize(); t["kernels, in a graph"].append(e0.elapsed_time(e1) * 1e3 / GRAPH_LAUNCHES)
            host = []
            for r in range(HOST_REPS if N <= 1024 else 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x_h, c_h = xyz.cpu().numpy(), None if cov is None else cov.cpu().numpy()
                h = skeleton.bone_lengths_host(x_h, bones)
                skeleton.project_host(x_h, bones, h.length, c_h)
                host.append((time.perf_counter() - t0) * 1e6)
            m = {k: stats(v) for k, v in t.items()}
            print(f"J={J} B={B} N={N:5d} {label:11s}: three launches {fmt(m['kernels'])}, in a hipGraph of {GRAPH_LAUNCHES} "
                  f"{fmt(m['kernels, in a graph'])} (at most {trips} trips, {unconverged} frames above 1e-3 mm; workgroups "
                  f"{la['measure_groups']} / {la['lengths_groups']} / {la['project_groups']}, projection {la['project_lds_bytes']} B LDS)"
                  + (f"; tensor ops {fmt(m['tensor ops'])} (medians and MADs equal: {same_medians}; max |difference| of the joints "
                     f"{diff:.2e} mm)" if solve_on_device else "")
                  + f"; download + host {np.median(host):.0f} us")
