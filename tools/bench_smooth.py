#!/usr/bin/env python3
"""The temporal fit: smoothing.smooth_sequence (one launch: joints, velocity, the fit's covariance, n_used) at half_window 8,
degree 2, tricube taper, with every tap's covariance as its weight and with unit weights, against
  tensor ops           the same normal equations as batched float64 tensor ops on the device: the frames unfolded into windows,
                       torch.linalg.inv of the covariances, the 9 x 9 normal matrices and right-hand sides by einsum about the
                       window's centre frame, one torch.linalg.solve for the coefficients and the inverse's position block;
  download + host      the joints (and covariances) copied to the host and smoothing.smooth_host, float64 numpy (wall clock).
N = 64, 1 024 and 16 384 frames of J = 17 and 19 joints.  Per way: the median [p10 .. p90] of REPS repetitions, the device ways
interleaved inside every repetition (so drift in clocks or load falls on all of them alike), each by an event pair around the
call on a synchronised stream; the kernel also per call inside a hipGraph of GRAPH_LAUNCHES calls (the kernel plus the gap to the
next node, without the host's enqueue time).  The counted traffic of a call is what it must read and write once: 12 (+ 24 with
covariances) bytes in and 12 + 12 + 24 + 4 bytes out per (frame, joint); the rate printed is that over the in-graph time.
Usage: bench_smooth.py   (env: REPS, HOST_REPS)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd import _lib, smoothing

dev = torch.device("cuda", 0)
REPS = max(20, int(os.environ.get("REPS", "20")))
HOST_REPS = max(3, int(os.environ.get("HOST_REPS", "3")))
GRAPH_LAUNCHES = 50
H, D = 8, 2


def sequence(N, J, seed=1):
    """xyz (N,J,3), cov6 (N,J,6) float32 on the device: slow sinusoids plus noise drawn from each tap's own covariance (largest
    eigenvalue 1 .. 1e3 mm^2, the others smaller by up to 1e2 and 1e4)."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(N, J, 3, 3)))[0]
    l1 = np.exp(rng.uniform(0, np.log(1e3), (N, J)))
    lam = np.stack([l1, l1 / np.exp(rng.uniform(0, np.log(1e2), (N, J))), l1 / np.exp(rng.uniform(0, np.log(1e4), (N, J)))], -1)
    C = np.einsum("njab,njb,njcb->njac", Q, lam, Q)
    f = np.arange(N)[:, None, None]
    x = rng.uniform(-3000, 3000, (1, J, 3)) + rng.uniform(20, 200, (1, J, 3)) * np.sin(rng.uniform(0.02, 0.15, (1, J, 3)) * f)
    x = x + np.einsum("njab,njb->nja", np.linalg.cholesky(C), rng.normal(size=x.shape))
    cov6 = C[..., [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    return torch.as_tensor(x.astype(np.float32), device=dev), torch.as_tensor(cov6.astype(np.float32), device=dev)


def smooth_ops(xyz, cov6):
    """(joints, velocity, cov (N,J,3,3)) in float64 by batched tensor ops; every frame of the inputs is finite."""
    N, J = xyz.shape[:2]
    K = 2 * H + 1
    t = torch.arange(-H, H + 1, dtype=torch.float64, device=dev)
    taper = (1 - (t.abs() / (H + 1)) ** 3) ** 3
    basis = torch.stack([t ** 0, t, t * t], dim=1)                                        # (K,3)
    pad = lambda a: torch.cat([a.new_zeros((H,) + a.shape[1:]), a, a.new_zeros((H,) + a.shape[1:])])
    inside = pad(torch.ones(N, dtype=torch.float64, device=dev)).unfold(0, K, 1)            # (N,K)
    X = xyz.double()
    win = pad(X).unfold(0, K, 1).permute(0, 3, 1, 2)                                       # (N,K,J,3)
    if cov6 is None:
        Lam = torch.eye(3, dtype=torch.float64, device=dev).expand(N, J, 3, 3)
    else:
        Lam = torch.linalg.inv(cov6.double()[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(N, J, 3, 3))
    LamW = pad(Lam).unfold(0, K, 1).permute(0, 4, 1, 2, 3)                                 # (N,K,J,3,3)
    w = inside * taper                                                                     # (N,K)
    A = torch.einsum("nk,ka,kb,nkjrc->njarbc", w, basis, basis, LamW).reshape(N, J, 9, 9)
    rhs = torch.einsum("nk,ka,nkjrc,nkjc->njar", w, basis, LamW, win - X[:, None]).reshape(N, J, 9)
    eye = torch.eye(9, dtype=torch.float64, device=dev)[:, :3].expand(N, J, 9, 3)
    sol = torch.linalg.solve(A, torch.cat([rhs[..., None], eye], dim=-1))
    return sol[..., 0:3, 0] + X, sol[..., 3:6, 0], sol[..., 0:3, 1:4]


def stats(x):
    x = np.sort(np.asarray(x))
    return np.median(x), x[len(x) // 10], x[-1 - len(x) // 10]


def fmt(m):
    return f"{m[0]:9.1f} us [{m[1]:.1f} .. {m[2]:.1f}]"


solve_on_device = True
try:
    xw, cw = sequence(32, 17)
    smooth_ops(xw, cw)
    torch.cuda.synchronize()
except Exception as e:      # (a build without a device solver raises here; nothing falls back silently)
    solve_on_device = False
    print(f"torch.linalg.solve / inv cannot run on the device in this torch build ({type(e).__name__}: {e}): no tensor-op column")

print(f"-- temporal fit, half_window {H}, degree {D}, tricube: median [p10 .. p90] of {REPS} interleaved repetitions "
      f"(host: {HOST_REPS}, wall clock)")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for J in (17, 19):
    for N in (64, 1024, 16384):
        xyz, cov6 = sequence(N, J)
        la = _lib.smooth_launch(N, J, H)
        for label, cov in (("covariances", cov6), ("unit weights", None)):
            kernel = lambda: smoothing.smooth_sequence(xyz, cov, half_window=H, degree=D)
            ways = {"kernel": kernel}
            if solve_on_device:
                ways["tensor ops"] = lambda: smooth_ops(xyz, cov)
            for _ in range(3):
                kernel()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(GRAPH_LAUNCHES):
                    kernel()
            graph.replay()
            for fn in ways.values():
                fn()
            torch.cuda.synchronize()
            got = kernel()
            diff = float("nan")
            if solve_on_device:
                ops = smooth_ops(xyz, cov)
                diff = float((ops[0] - got.joints.double()).abs().max())
            t = {name: [] for name in ways}
            t["kernel, in a graph"] = []
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
                torch.cuda.synchronize(); t["kernel, in a graph"].append(e0.elapsed_time(e1) * 1e3 / GRAPH_LAUNCHES)
            host = []
            for r in range(HOST_REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                smoothing.smooth_host(xyz.cpu().numpy(), None if cov is None else cov.cpu().numpy(), half_window=H, degree=D)
                host.append((time.perf_counter() - t0) * 1e6)
            m = {k: stats(v) for k, v in t.items()}
            traffic = N * J * (12 + (24 if cov is not None else 0) + 12 + 12 + 24 + 4)
            print(f"J={J} N={N:5d} {label:12s}: kernel {fmt(m['kernel'])}, in a hipGraph of {GRAPH_LAUNCHES} {fmt(m['kernel, in a graph'])} "
                  f"({traffic / m['kernel, in a graph'][0] * 1e-3:.2f} GB/s of {traffic} counted bytes; tile {la['tile']} frames, "
                  f"{la['groups']} workgroups, {la['lds_bytes']} B LDS)"
                  + (f"; tensor ops {fmt(m['tensor ops'])} (max |difference| {diff:.2e} mm)" if solve_on_device else "")
                  + f"; download + host {np.median(host):.0f} us")
