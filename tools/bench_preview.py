#!/usr/bin/env python3
"""The debug pictures (skelsplat_amd.preview, sks_preview_planes / sks_preview_factors) against the reference's formulation as
plain tensor ops on the device (sum over channels, min, max, arithmetic, .to(uint8): train.py:287-289), at four H36M views
(4 x 17 x 1000 x 1000) and four Panoptic views (4 x 19 x 1080 x 1920):
  channel_sum_u8     from (V,C,H,W) planes; the algorithmic traffic is (4C + 4 + 4 + 1) bytes per pixel -- the planes read once,
                     the sum plane written and read back, the picture written;
  heatmap_preview    from the separable heat-map factors of a synthetic scene, against tensor ops that first materialise the planes
                     (HeatmapFactors.planes) -- what a caller without the kernel has to do.  No plane traffic at all: 9 bytes per
                     pixel, and the time is the arithmetic of the joints whose support a row crosses.
Timed by an event pair around each call (scratch and output allocation included: it is what a caller pays), the ways INTERLEAVED
repetition by repetition; median [p10 .. p90].
Usage: bench_preview.py   (env: REPS)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd import _lib
from skelsplat_amd._base import ViewBatch
from skelsplat_amd.heatmaps import heatmap_factors
from skelsplat_amd.preview import channel_sum_u8, heatmap_preview
from skelsplat_amd.scene import GaussianModel, SyntheticScene
from skelsplat_amd.sparse import HeatmapFactors

dev = torch.device("cuda", 0)
REPS = max(20, int(os.environ.get("REPS", "30")))


def tensor_ops(x):
    """train.py:287-289 per view, batched"""
    s = torch.sum(x, dim=1)
    lo, hi = s.amin(dim=(1, 2), keepdim=True), s.amax(dim=(1, 2), keepdim=True)
    return (((s - lo) / (hi - lo)) * 255).to(torch.uint8)


def stats(x):
    x = np.sort(np.asarray(x))
    return np.median(x), x[len(x) // 10], x[-1 - len(x) // 10]


def race(ways):
    for _ in range(3):
        for _, fn in ways:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in ways}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(REPS):
        for name, fn in ways:
            torch.cuda.synchronize()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: stats(t) for name, t in times.items()}


print(f"-- debug pictures, median [p10 .. p90] of {REPS} interleaved repetitions, event pair per call")
for dataset, V, C, H, W in (("h36m", 4, 17, 1000, 1000), ("panoptic", 4, 19, 1080, 1920)):
    launch = _lib.preview_launch(W, H)
    # blob-like planes: a render's statistics matter to neither way, the bytes do
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((V, C, H, W), device=dev, generator=g).pow_(8)
    with torch.no_grad():
        a, b = channel_sum_u8(x), tensor_ops(x)
        differ = int((a != b).sum())
        res = race((("channel_sum_u8", lambda: channel_sum_u8(x)), ("tensor ops", lambda: tensor_ops(x))))
    px = float(V * H * W)
    print(f"{V} x {C} x {H} x {W} planes ({launch['load_bytes']}-byte loads, {launch['store_bytes']}-byte stores, "
          f"{launch['groups_sum']} + {launch['groups_pack']} workgroups per view): {differ} of {int(px)} bytes differ between the ways")
    for name, (m, lo, hi) in res.items():
        print(f"    {name:16s} {m:9.1f} us [{lo:.1f} .. {hi:.1f}] = {(4 * C + 9) * px / m * 1e-6:5.2f} TB/s of (4C + 9) bytes per pixel")
    del x, a, b

    sc = SyntheticScene(dataset, n_views=V, seed=0, device=dev)
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scene_type=dataset, device=dev)
    views = ViewBatch.from_cameras(sc.cameras, allow_mixed=True)
    f = HeatmapFactors(V, sc.n_joints, views.W, views.H, dev)
    with torch.no_grad():
        heatmap_factors(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                        torch.as_tensor(np.asarray(sc.poses_2d, np.float32)[..., :2], device=dev), sc.cameras, views=views, out=f)

        def from_planes():
            return tensor_ops(torch.stack([f.planes(v) for v in range(V)]))

        a, b = heatmap_preview(f, views), from_planes()
        differ = int((a != b).sum())
        res = race((("heatmap_preview", lambda: heatmap_preview(f, views)), ("tensor ops", from_planes)))
    px = float(V * views.H * views.W)
    print(f"{V} x {sc.n_joints} factors of {views.H} x {views.W} ({dataset}): {differ} of {int(px)} bytes differ between the ways")
    for name, (m, lo, hi) in res.items():
        print(f"    {name:16s} {m:9.1f} us [{lo:.1f} .. {hi:.1f}] = {9 * px / m * 1e-6:5.2f} TB/s of 9 bytes per pixel")
    del f, a, b
    torch.cuda.empty_cache()
