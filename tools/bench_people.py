#!/usr/bin/env python3
"""People: the two kernels of skelsplat_amd.people (sks_associate_people, one workgroup per frame; sks_track_people, one wavefront
per recording) against
  tensor ops           the pair-cost matrix ALONE -- no clustering, no people -- as batched float64 tensor ops on the device: the
                       fundamental matrices by the header's expansion, then per joint the two point-to-line distances of every pair
                       of detections in different views (frames in slices of at most 2^21 pairs, so the temporaries stay bounded);
  download + host      the detections copied to the host, people.associate_host + people.track_host (float64 numpy and a Python
                       walk per frame), and the assignment and the gathered detections copied back (wall clock; up to 1 024 frames of 5 views,
                       64 of 31).
N = 64, 1 024 and 16 384 frames of V x M x J = 5 x 4 x 19 and 31 x 4 x 19: three Panoptic templates 1 500 mm apart in four slots
shuffled per frame, 3 px of noise, ring cameras; the tracker on the triangulated people of the same frames, one recording.  Per way:
the median [p10 .. p90] of REPS repetitions, the device ways interleaved inside every repetition (so drift in clocks or load falls
on all of them alike), each by an event pair around the calls on a synchronised stream; the kernels also per call inside a hipGraph
of GRAPH_LAUNCHES calls (without the host's enqueue time).
Usage: bench_people.py   (env: REPS, HOST_REPS)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd import _lib, people
from skelsplat_amd.scene import DATASETS, project_points, ring_cameras, skeleton_template
from skelsplat_amd.triangulation import projection_matrices, triangulate_sequence

dev = torch.device("cuda", 0)
REPS = max(10, int(os.environ.get("REPS", "10")))
HOST_REPS = max(1, int(os.environ.get("HOST_REPS", "1")))
GRAPH_LAUNCHES = 5
PEOPLE, M, MAX_PX, BASE = 3, 4, 15.0, 64


def frames(V, seed=1):
    """P (V,3,4) float64 and BASE distinct frames of detections (BASE,V,M,J,2) float32, on the host."""
    d = DATASETS["panoptic"]
    rng = np.random.default_rng(seed)
    cams = ring_cameras(V, d["W"], d["H"], d["ring"], d["fx"], rng)
    tmpl = skeleton_template("panoptic")
    J = tmpl.shape[0]
    x = np.full((BASE, V, M, J, 2), np.nan, dtype=np.float32)
    for f in range(BASE):
        for v, cam in enumerate(cams):
            slots = rng.permutation(M)
            for k in range(PEOPLE):
                body = tmpl + np.array([(k - 1) * 1500.0 + 3.0 * f, 1.5 * f, 0.0])
                x[f, v, slots[k]] = project_points(cam, body) + rng.normal(0.0, 3.0, (J, 2))
    return projection_matrices(cams), x


def cost_matrix_ops(P, x, M):
    """c (N,n_pairs) float64 on the device: the header's pair cost of every a < b in different views (NaN joints left out)."""
    N, V, _, J = x.shape[:4]
    D = V * M
    idx = torch.arange(D, device=dev)
    ia, ib = torch.nonzero((idx[:, None] // M) < (idx[None, :] // M), as_tuple=True)
    rows = [[1, 2], [0, 2], [0, 1]]
    mins = []
    for i in range(3):
        a, b = P[:, rows[i][0]], P[:, rows[i][1]]
        mins.append(torch.stack([a[:, p] * b[:, q] - a[:, q] * b[:, p] for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))], dim=-1))
    m = torch.stack(mins, dim=1)                                                    # (V,3,6)
    A, B = m[:, None, None, :, :], m[None, :, :, None, :]
    det = ((((A[..., 0] * B[..., 5] - A[..., 1] * B[..., 4]) + A[..., 2] * B[..., 3]) + A[..., 3] * B[..., 2]) - A[..., 4] * B[..., 1]) + A[..., 5] * B[..., 0]
    sign = torch.tensor([[1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, 1.0]], dtype=torch.float64, device=dev)
    F = (det * sign)[ia // M, ib // M]                                              # (n_pairs,3,3)
    out = torch.empty((N, ia.numel()), dtype=torch.float64, device=dev)
    step = max(1, (1 << 21) // ia.numel())
    for lo in range(0, N, step):
        xs = x[lo:lo + step].reshape(-1, D, J, 2).double()
        total = torch.zeros((xs.shape[0], ia.numel()), dtype=torch.float64, device=dev)
        n = torch.zeros_like(total)
        for j in range(J):
            ax, ay, bx, by = xs[:, ia, j, 0], xs[:, ia, j, 1], xs[:, ib, j, 0], xs[:, ib, j, 1]
            l0, l1, l2 = ((F[:, k, 0] * ax + F[:, k, 1] * ay) + F[:, k, 2] for k in range(3))
            db = ((l0 * bx + l1 * by) + l2).abs() / (l0 * l0 + l1 * l1).sqrt()
            t0, t1, t2 = ((F[:, 0, k] * bx + F[:, 1, k] * by) + F[:, 2, k] for k in range(3))
            da = ((t0 * ax + t1 * ay) + t2).abs() / (t0 * t0 + t1 * t1).sqrt()
            dd = 0.5 * (db + da)
            ok = torch.isfinite(dd)
            total = torch.where(ok, total + dd, total)
            n = n + ok
        out[lo:lo + step] = total / n
    return out


def stats(x):
    x = np.sort(np.asarray(x))
    return np.median(x), x[len(x) // 10], x[-1 - len(x) // 10]


def fmt(m):
    return f"{m[0]:9.1f} us [{m[1]:.1f} .. {m[2]:.1f}]"


print(f"-- people: {PEOPLE} people in {M} slots a view, J = 19, max_px {MAX_PX:g}: median [p10 .. p90] of {REPS} interleaved repetitions "
      f"(host: {HOST_REPS}, wall clock)")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for V in (5, 31):
    P_h, base = frames(V)
    P = torch.as_tensor(P_h, device=dev)
    la = _lib.people_launch(V, M)
    J = base.shape[3]
    for N in (64, 1024, 16384):
        x = torch.as_tensor(base, device=dev).repeat(N // BASE, 1, 1, 1, 1).contiguous()
        assoc = lambda: people.associate(P, x, max_px=MAX_PX, max_people=M)
        a = assoc()
        p2d = a.poses_2d.reshape(N * M, V, J, 2)
        joints = triangulate_sequence(P, p2d, valid=people.kept(p2d)).reshape(N, M, J, 3).contiguous()
        del p2d
        track = lambda: people.track(joints, max_mm=300.0, max_gap=5, min_joints=5)
        t = track()
        torch.cuda.synchronize()
        found = f"{int((a.n_people == PEOPLE).sum())} / {N} frames with {PEOPLE} people, {int(t.n_tracks[0])} tracks"
        ways = {"associate": assoc, "track": track, "cost matrix, tensor ops": lambda: cost_matrix_ops(P, x, M)}
        graphs = {}
        for name in ("associate", "track"):
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(GRAPH_LAUNCHES):
                    ways[name]()
            graphs[name].replay()
        for fn in ways.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in list(ways) + [g + ", in a graph" for g in graphs]}
        for r in range(REPS):
            for name, fn in ways.items():
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize(); times[name].append(e0.elapsed_time(e1) * 1e3)
            for name, g in graphs.items():
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize(); times[name + ", in a graph"].append(e0.elapsed_time(e1) * 1e3 / GRAPH_LAUNCHES)
        host = {"associate": [], "track": []}
        for r in range(HOST_REPS if N * V <= 1024 * 5 else 0):       # (the Python walk: seconds per 1 000 frames of 31 views)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = people.associate_host(P_h, x.cpu().numpy(), None, MAX_PX, 3, 2, M)
            up = [torch.as_tensor(h.assign, device=dev), torch.as_tensor(h.poses_2d, device=dev)]
            torch.cuda.synchronize()
            host["associate"].append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            ht = people.track_host(joints.cpu().numpy(), None, 1, 300.0, 5, 5)
            up = torch.as_tensor(ht.track_id, device=dev)
            torch.cuda.synchronize()
            host["track"].append((time.perf_counter() - t0) * 1e6)
            same = bool((up == t.track_id).all()) and np.array_equal(h.assign, a.assign.cpu().numpy())
        m = {k: stats(v) for k, v in times.items()}
        print(f"V={V:2d} M={M} N={N:5d} ({found}; {la['assoc_lds_bytes']} B LDS a workgroup, list of {la['assoc_list_entries']}): "
              f"associate {fmt(m['associate'])}, in a hipGraph of {GRAPH_LAUNCHES} {fmt(m['associate, in a graph'])}; "
              f"track {fmt(m['track'])}, in a hipGraph {fmt(m['track, in a graph'])}; cost matrix alone by tensor ops "
              f"{fmt(m['cost matrix, tensor ops'])}"
              + (f"; download + host + upload: associate {np.median(host['associate']):.0f} us, track {np.median(host['track']):.0f} us "
                 f"(same assignment and ids: {same})" if host["associate"] else "; host path not run at this length"), flush=True)
        del x, joints, a, graphs
        torch.cuda.empty_cache()
