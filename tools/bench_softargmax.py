#!/usr/bin/env python3
"""softargmax2d: the fused op (skelsplat_amd.keypoints, sks_softargmax_fwd / _bwd) against the reference's formulation as plain
tensor ops on the device (softmax, two index grids built by repeat, two weighted sums; autograd backward), forward and
forward + backward, at one H36M view (17 x 1000 x 1000) and one Panoptic view (19 x 1920 x 1080).
Timed by an event pair around each call (the calls are far longer than their enqueue), the ways INTERLEAVED repetition by
repetition; median [p10 .. p90].  Bandwidth is counted as 4 C H W bytes forward (one read) and 8 C H W backward (one read, one
write), so forward + backward moves 12 C H W.
Usage: bench_softargmax.py   (env: REPS)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from skelsplat_amd.keypoints import softargmax2d

dev = torch.device("cuda", 0)
REPS = max(20, int(os.environ.get("REPS", "30")))


def softargmax2d_tensor_ops(inp, beta=100):
    """utils/loss_utils.py:41-64 as tensor ops"""
    *lead, h, w = inp.shape
    p = torch.softmax(beta * inp.view(*lead, h * w), dim=-1)
    rows = torch.linspace(0, 1, steps=h, device=inp.device).view(-1, 1).repeat(1, w).view(1, h * w)
    cols = torch.linspace(0, 1, steps=w, device=inp.device).view(1, -1).repeat(h, 1).view(1, h * w)
    return torch.stack([torch.sum(p * cols, dim=-1) * (w - 1), torch.sum(p * rows, dim=-1) * (h - 1)], dim=-1)


def stats(x):
    x = np.sort(np.asarray(x))
    return np.median(x), x[len(x) // 10], x[-1 - len(x) // 10]


def heatmaps(C, H, W, peak):
    g = torch.Generator(device="cpu").manual_seed(0)
    cy, cx = torch.rand(C, generator=g) * (H - 1), torch.rand(C, generator=g) * (W - 1)
    r = torch.arange(H, dtype=torch.float64)[None, :, None] - cy.double()[:, None, None]
    c = torch.arange(W, dtype=torch.float64)[None, None, :] - cx.double()[:, None, None]
    return (peak * torch.exp(-(r * r + c * c) / (2 * 4.0 ** 2))).float().to(dev)


print(f"-- softargmax2d, median [p10 .. p90] of {REPS} interleaved repetitions, event pair per call")
for C, H, W in ((17, 1000, 1000), (19, 1080, 1920)):
    for peak in (1.0, 0.02):
        img = heatmaps(C, H, W, peak)
        cot = torch.randn((C, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        ways = (("fused", softargmax2d), ("tensor ops", softargmax2d_tensor_ops))

        def fwd(fn):
            with torch.no_grad():
                return fn(img)

        def fwd_bwd(fn):
            x = img.detach().requires_grad_(True)
            (fn(x) * cot).sum().backward()
            return x.grad

        out = {name: (fwd(fn), fwd_bwd(fn)) for name, fn in ways}      # warm-up; and the two ways agree
        for _ in range(2):
            for name, fn in ways:
                fwd(fn); fwd_bwd(fn)
        torch.cuda.synchronize()
        dxy = float((out["fused"][0] - out["tensor ops"][0]).abs().max())
        dg = float((out["fused"][1] - out["tensor ops"][1]).abs().max() / out["tensor ops"][1].abs().max())
        times = {(name, k): [] for name, _ in ways for k in ("fwd", "fwd+bwd")}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(REPS):
            for name, fn in ways:
                for k, run in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
                    torch.cuda.synchronize()
                    e0.record(); run(fn); e1.record()
                    torch.cuda.synchronize()
                    times[name, k].append(e0.elapsed_time(e1) * 1e3)
        nbytes = 4.0 * C * H * W
        print(f"{C} x {H} x {W}, peak {peak:g}: max |fused - tensor ops| {dxy:.2e} px, gradient {dg:.2e} of its largest entry")
        for name, _ in ways:
            f, fb = stats(times[name, "fwd"]), stats(times[name, "fwd+bwd"])
            b = fb[0] - f[0]
            print(f"    {name:10s} fwd {f[0]:8.1f} us [{f[1]:.1f} .. {f[2]:.1f}] = {nbytes / f[0] * 1e-6:5.2f} TB/s of 4CHW;  "
                  f"fwd+bwd {fb[0]:8.1f} us [{fb[1]:.1f} .. {fb[2]:.1f}];  bwd (difference) {b:8.1f} us = "
                  f"{2 * nbytes / max(b, 1e-9) * 1e-6:5.2f} TB/s of 8CHW")
