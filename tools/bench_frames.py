#!/usr/bin/env python3
"""Frames per second of the H36M training loop (4 views @ 1000x1000, 500 iterations per frame, heat-map generation
included) when F independent frames share the launches (loop.FrameBatchLoop), against one frame at a time
(loop.MultiViewLoop.new_scene + run, hipGraphs in both).  Usage: bench_frames.py [F ...]

bench_frames.py --rigs R [--reps N] [--frames F] [--streams S]: frames seen by different camera rigs (rigs.RigBank).  A
sequence of S x F x 4 frames through FramePipeline (S streams of F frames, graphs on), N interleaved repetitions of
  one_rig      FramePipeline(cameras=rig 0): the path that takes the per-view scalars by value;
  bank_equal   FramePipeline(rigs=bank), every frame on rig 0;
  bank_cycle   FramePipeline(rigs=bank), frame f on rig f % R;
  naive        what a caller had to do before: per batch, the cameras of the batch's rig rebuilt on the host (Camera objects, a
               new FrameBatchLoop with its ViewBatch) and the graphs captured again (one rig per batch: frames are taken rig by rig);
and the host cost of building one rig's Cameras alone.  Prints one line per case: median frames/s, min, max.

bench_frames.py --report [--reps N] [--frames F] [--streams S] [--parent DIR]: what reporting costs (FramePipeline(report_steps=,
save_iterations=), set_ground_truth(gt)): the H36M pipeline (S streams of F frames, graphs on, ITERS iterations) with reporting
  off          as it ran before: the launch sequence of a group is unchanged;
  on           errors and losses at every optimiser step, three snapshots: one more launch of F wavefronts per group;
  parent_off   (--parent DIR, a built checkout of the commit to compare with) that tree's pipeline, reporting unknown to it.
bench_frames.py --report --keep [...]: the same three-way comparison for FramePipeline(keep_gaussians=True) (case `keep`: every
frame's scaling / rotation / opacity copied next to its joints, three small device copies per batch) in place of `on`.
bench_frames.py --report --reproject [...]: the same for the two switches of skelsplat_amd/reprojection.py.  `off` (points given,
both switches off) is what `parent_off` is held against; the switches act on sequences that start from detections, so their cost is
read against `dlt` (optimize_sequence(None, detections on the device), both off): `refine` (set_refinement(16): one more launch
per batch behind the triangulation), `reproj` (set_reprojection_report(): two more launches per batch) and `both`.
Every tree is measured by a worker process of its own that stays warm; the driver asks them for one repetition of one case at a
time, round-robin, N times, so drift hits all cases alike.  Prints median, min and max per case and the ratios of the medians."""
import os, sys, time
ROOT = os.environ.get("SKS_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd.loop import MultiViewLoop, FrameBatchLoop
from skelsplat_amd.scene import SyntheticScene, GaussianModel

dev = torch.device("cuda", 0)


def bench_rigs(argv):
    import argparse, statistics
    from skelsplat_amd.loop import FramePipeline
    from skelsplat_amd.rigs import RigBank
    from skelsplat_amd.scene import Camera
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", type=int, required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--cases", default="one_rig,bank_equal,bank_cycle,naive")
    a = ap.parse_args(argv)
    iters = int(os.environ.get("ITERS", "500"))
    R_, F, S = a.rigs, a.frames, a.streams
    N = S * F * 4
    scenes = [SyntheticScene("h36m", n_views=4, seed=r, device=dev) for r in range(R_)]
    rigs = [sc.cameras for sc in scenes]
    bank = RigBank(rigs, dev)
    rng = np.random.default_rng(1)
    cyc = [f % R_ for f in range(N)]

    def frames_for(ids):
        return (np.stack([scenes[r].pose_3d_init + rng.normal(0, 10.0, (17, 3)) for r in ids]).astype(np.float32),
                np.stack([scenes[r].poses_2d + rng.normal(0, 2.0, (4, 17, 2)) for r in ids]).astype(np.float32))

    def model(r=0):
        gm = GaussianModel().create_from_points(scenes[r].pose_3d_init, scenes[r].spatial_lr_scale, 17, device=dev)
        gm.training_setup()
        return gm

    data = {"one_rig": frames_for([0] * N), "bank_equal": frames_for([0] * N), "bank_cycle": frames_for(cyc),
            "naive": frames_for(sorted(cyc))}
    pipes = {"one_rig": FramePipeline(model(), rigs[0], frames=F, streams=S, dataset="h36m"),
             "bank_equal": FramePipeline(model(), rigs=bank, frames=F, streams=S, dataset="h36m"),
             "bank_cycle": FramePipeline(model(), rigs=bank, frames=F, streams=S, dataset="h36m")}
    ids_dev = {"bank_equal": torch.zeros(N, dtype=torch.int32, device=dev), "bank_cycle": torch.tensor(cyc, dtype=torch.int32, device=dev)}

    def run_case(name):
        pts, p2d = data[name]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        if name == "naive":
            # one rig per batch: the rig's cameras are rebuilt from R / T / K, a loop is built around them, its graphs are captured
            order = sorted(cyc)
            for b in range(0, N, F):
                src = rigs[order[b]]
                cams = [Camera(c.uid, c.R, c.T, c.K, c.image_width, c.image_height, device=dev) for c in src]
                fb = FrameBatchLoop(model(order[b]), cams, F, dataset="h36m", use_graph=True)
                fb.new_scenes(pts[b:b + F], poses_2d=p2d[b:b + F])
                fb.run(iters)
        elif name == "one_rig":
            pipes[name].optimize_sequence(pts, p2d, iterations=iters)
        else:
            pipes[name].optimize_sequence(pts, p2d, iterations=iters, rig_ids=ids_dev[name])
        torch.cuda.synchronize()
        return N / (time.perf_counter() - t0)

    cases = [c for c in a.cases.split(",") if c]
    for c in cases:
        if c != "naive":
            run_case(c)         # warm-up: allocations, graph capture
    rates = {c: [] for c in cases}
    for rep in range(a.reps):   # interleaved: one repetition of every case after the other
        for c in cases:
            rates[c].append(run_case(c))
    for c in cases:
        v = rates[c]
        print(f"rigs={R_} {c:11s}: median {statistics.median(v):7.0f} frames/s  min {min(v):7.0f}  max {max(v):7.0f}  "
              f"({S} streams x {F} frames, {N} frames, {iters} iterations, {a.reps} interleaved repetitions)  all: "
              + " ".join(f"{x:.0f}" for x in v))
    t0 = time.perf_counter()
    for _ in range(20):
        [Camera(c.uid, c.R, c.T, c.K, c.image_width, c.image_height, device=dev) for c in rigs[0]]
    torch.cuda.synchronize()
    print(f"host: building one rig's 4 Cameras (uploads included) {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms, "
          f"{F} x 4 per batch of distinct rigs {(time.perf_counter() - t0) / 20 * F * 1e3:.2f} ms")


def report_worker(argv):
    """One tree's pipeline(s), warm; per line on stdin ("off" / "on" / "keep") one timed sequence, its frames/s on stdout."""
    import inspect
    from skelsplat_amd.loop import FramePipeline
    F, S = int(argv[0]), int(argv[1])
    keep = len(argv) > 2 and argv[2] == "keep"
    reproject = len(argv) > 2 and argv[2] == "reproject"
    iters = int(os.environ.get("ITERS", "500"))
    N = S * F * 4
    sc = SyntheticScene("h36m", n_views=4, seed=0, device=dev)
    rng = np.random.default_rng(1)
    pts = np.stack([sc.pose_3d_init + rng.normal(0, 10.0, (17, 3)) for _ in range(N)]).astype(np.float32)
    p2d = np.stack([sc.poses_2d + rng.normal(0, 2.0, (4, 17, 2)) for _ in range(N)]).astype(np.float32)
    gt = torch.as_tensor(np.asarray(sc.pose_3d_gt, np.float32), device=dev)[None].repeat(N, 1, 1).contiguous()

    def model():
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, 17, device=dev)
        gm.training_setup()
        return gm
    pipes = {"off": (FramePipeline(model(), sc.cameras, frames=F, streams=S, dataset="h36m"), None)}
    from_detections = set()
    if reproject:
        if hasattr(FramePipeline, "set_reprojection_report"):
            for name, refine, rep in (("dlt", None, False), ("refine", 16, False), ("reproj", None, True), ("both", 16, True)):
                pipe = FramePipeline(model(), sc.cameras, frames=F, streams=S, dataset="h36m")
                pipes[name] = (pipe.set_refinement(refine).set_reprojection_report(rep), None)
                from_detections.add(name)
    elif keep:
        if "keep_gaussians" in inspect.signature(FrameBatchLoop.__init__).parameters:
            pipes["keep"] = (FramePipeline(model(), sc.cameras, frames=F, streams=S, dataset="h36m", keep_gaussians=True), None)
    elif "report_steps" in inspect.signature(FrameBatchLoop.__init__).parameters:
        pipes["on"] = (FramePipeline(model(), sc.cameras, frames=F, streams=S, dataset="h36m", report_steps=iters // 4 + 1,
                                     save_iterations=(0, iters // 2, iters)), gt)
    p2d_dev = torch.as_tensor(p2d, device=dev)
    for name, (pipe, truth) in pipes.items():
        if truth is not None:
            pipe.set_ground_truth(truth)
        if name in from_detections:
            pipe.optimize_sequence(None, p2d_dev, iterations=iters)
        else:
            pipe.optimize_sequence(pts, p2d, iterations=iters)       # warm-up: allocations, graph capture
    torch.cuda.synchronize()
    print("ready " + ",".join(pipes), flush=True)
    for line in sys.stdin:
        pipe, truth = pipes[line.strip()]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        if truth is not None:
            pipe.set_ground_truth(truth)
        if line.strip() in from_detections:
            pipe.optimize_sequence(None, p2d_dev, iterations=iters)
        else:
            pipe.optimize_sequence(pts, p2d, iterations=iters)
        torch.cuda.synchronize()
        print(f"{N / (time.perf_counter() - t0):.1f}", flush=True)


def bench_report(argv):
    import argparse, statistics, subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--reproject", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps: at least 5 repetitions")

    def worker(root):
        env = dict(os.environ, SKS_BENCH_ROOT=os.path.abspath(root))
        w = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--report-worker", str(a.frames), str(a.streams),
                              "keep" if a.keep else "reproject" if a.reproject else "report"],
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=root)
        head = w.stdout.readline().split()
        if not head or head[0] != "ready":
            raise SystemExit(f"the worker of {root} did not start")
        return w, head[1].split(",")

    def ask(w, case):
        w.stdin.write(case + "\n"); w.stdin.flush()
        return float(w.stdout.readline())
    here, cases_here = worker(ROOT)
    cases = [(c, here) for c in cases_here]
    parent = None
    if a.parent:
        parent, _ = worker(a.parent)
        cases.append(("parent_off", parent))
    rates = {c: [] for c, _ in cases}
    for rep in range(a.reps):       # interleaved: one repetition of every case after the other
        for c, w in cases:
            rates[c].append(ask(w, "off" if c == "parent_off" else c))
    for w in (here, parent):
        if w is not None:
            w.stdin.close(); w.wait()
    N = a.frames * a.streams * 4
    med = {c: statistics.median(v) for c, v in rates.items()}
    for c, v in rates.items():
        print(f"report {c:10s}: median {med[c]:7.0f} frames/s  min {min(v):7.0f}  max {max(v):7.0f}  ({a.streams} streams x "
              f"{a.frames} frames, {N} frames, {os.environ.get('ITERS', '500')} iterations, {a.reps} interleaved repetitions)  all: "
              + " ".join(f"{x:.0f}" for x in v))
    for c in ("on", "keep"):
        if c in med:
            print(f"report {c} / off = {med[c] / med['off']:.4f}")
    for c in ("refine", "reproj", "both"):
        if c in med:
            print(f"report {c} / dlt = {med[c] / med['dlt']:.4f}")
    if "parent_off" in med:
        lo, hi = min(rates["parent_off"]), max(rates["parent_off"])
        print(f"report off / parent_off = {med['off'] / med['parent_off']:.4f}; median of off "
              f"{'inside' if lo <= med['off'] <= hi else 'OUTSIDE'} the parent's own range [{lo:.0f}, {hi:.0f}]")


if "--report-worker" in sys.argv:
    report_worker(sys.argv[sys.argv.index("--report-worker") + 1:])
    sys.exit(0)
if "--report" in sys.argv:
    bench_report(sys.argv[1:])
    sys.exit(0)
if "--rigs" in sys.argv:
    bench_rigs(sys.argv[1:])
    sys.exit(0)
Fs = [int(a) for a in sys.argv[1:]] or [1, 2, 4, 8, 16]
ITERS = int(os.environ.get("ITERS", "500"))
FACTORED = os.environ.get("FACTORED", "1") == "1"   # heat-maps as separable factors (no planes) or as planes
sc = SyntheticScene("h36m", n_views=4, seed=0, device=dev)
rng = np.random.default_rng(1)
base3, base2 = np.asarray(sc.pose_3d_init, np.float32), np.asarray(sc.poses_2d, np.float32)


def model():
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, device=dev)
    gm.training_setup()
    return gm


def frames(F):
    return (np.stack([base3 + rng.normal(0, 10.0, base3.shape) for _ in range(F)]).astype(np.float32),
            np.stack([base2 + rng.normal(0, 2.0, base2.shape) for _ in range(F)]).astype(np.float32))


# one frame at a time
base = None
if os.environ.get("ONLY_BATCH") != "1":
  gm = model()
  hm = torch.zeros((4, sc.n_joints, sc.H, sc.W), device=dev)
  one = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", sparse=True, use_graph=True)
  pts, p2d = frames(8)
  for rep in range(2):
      torch.cuda.synchronize(); t0 = time.perf_counter()
      for f in range(8):
          one.new_scene(pts[f], poses_2d=p2d[f])
          one.run(ITERS)
      torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 8
  print(f"one frame at a time: {dt*1e3:.3f} ms per frame, {1/dt:.0f} frames/s")
  base = dt
for F in Fs:
    fb = FrameBatchLoop(model(), sc.cameras, F, dataset="h36m", use_graph=True, factored=FACTORED)
    pts, p2d = frames(F)
    for rep in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fb.new_scenes(pts, poses_2d=p2d)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        fb.run(ITERS)
        torch.cuda.synchronize(); t2 = time.perf_counter()
    dt = (t2 - t0) / F
    print(f"F = {F:2d}: {(t2-t0)*1e3:.3f} ms per batch (heat-maps {(t1-t0)*1e3:.3f} ms, loop {(t2-t1)*1e3:.3f} ms = "
          f"{(t2-t1)*1e6/(ITERS/4):.1f} us per group), {1/dt:.0f} frames/s, x{(base or dt)/dt:.2f}")
    del fb
    torch.cuda.empty_cache()

# several batches on as many streams: one's single-workgroup tails run under the others' backward kernels
for spec in os.environ.get("STREAMS", "2x8,2x16,4x8,4x16").split(","):
    if not spec:
        continue
    ns, h = (int(x) for x in spec.split("x"))
    F = ns * h
    loops = [FrameBatchLoop(model(), sc.cameras, h, dataset="h36m", use_graph=True, factored=FACTORED) for _ in range(ns)]
    streams = [torch.cuda.Stream() for _ in range(ns)]
    pts, p2d = frames(F)
    for rep in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i, (fb, st) in enumerate(zip(loops, streams)):
            with torch.cuda.stream(st):
                fb.new_scenes(pts[i * h:(i + 1) * h], poses_2d=p2d[i * h:(i + 1) * h])
        for k in range(0, ITERS, 100):      # interleave the graph launches of the streams
            for fb, st in zip(loops, streams):
                with torch.cuda.stream(st):
                    fb.run(min(ITERS, k + 100))
        torch.cuda.synchronize(); t2 = time.perf_counter()
    dt = (t2 - t0) / F
    print(f"{ns} streams x {h:2d} frames: {(t2-t0)*1e3:.3f} ms per {F} frames, {1/dt:.0f} frames/s")
    del loops
    torch.cuda.empty_cache()
