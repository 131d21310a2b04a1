"""Literal per-iteration restatement of the reference loop (train.py:130-222) on top of the PyTorch oracle
(oracle/torch_ref.py + autograd).  TEST INFRASTRUCTURE: the thing the HIP loop is compared against."""
import math

import torch

from oracle import torch_ref
from skelsplat_amd.loop import limb_3d_consistency_loss, l2_loss_gaussian
from skelsplat_amd.scene import DATASETS


def render_ref(cam, gm, W, H, keep=None):
    """gaussian_renderer.render_* (reference :28-138) with the oracle rasterizer; returns the clamped image.
    `keep`: the rows that are rendered (None: all) -- the rasterizer never sees the others."""
    P = gm._xyz.shape[0]
    rows = (lambda t: t) if keep is None else (lambda t: t[keep])
    color, radii, inv = torch_ref.rasterize(
        rows(gm.get_xyz), None, rows(gm.get_features.reshape(P, -1)), rows(gm.get_opacity), rows(gm.get_scaling),
        rows(gm.get_rotation), None,
        cam.world_view_transform, cam.full_proj_transform, W, H, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
    return color.clamp(0, 1)


def limb_loss_without(xyz, dataset, missing):
    """limb_3d_consistency_loss with the pairs (arms: the first two limbs, legs: the last two) that touch a joint of `missing`
    left out; the lengths of those pairs are never formed.  missing == set(): the function itself."""
    if not missing:
        return limb_3d_consistency_loss(xyz, dataset)
    limbs = DATASETS[dataset]["limbs"]
    total = xyz.new_zeros(())
    for a, b in ((limbs[0], limbs[1]), (limbs[2], limbs[3])):
        if not (set(a) | set(b)) & set(missing):
            total = total + torch.norm(torch.norm(xyz[a[0]] - xyz[a[1]], dim=-1) - torch.norm(xyz[b[0]] - xyz[b[1]], dim=-1))
    return total


def view_grads_ref(gm, cam, gt, W, H, dataset, lambda_consistency, missing=frozenset()):
    """One iteration's loss and autograd.grad wrt (xyz, _scaling, _rotation, _opacity) (train.py:140-161)."""
    keep = None
    if missing:
        keep = torch.tensor([p for p in range(gm._xyz.shape[0]) if p not in missing], dtype=torch.long)
    image = render_ref(cam, gm, W, H, keep)
    l2, _ = l2_loss_gaussian(image, gt)
    loss = l2 + limb_loss_without(gm.get_xyz, dataset, missing) * lambda_consistency
    params = [gm._xyz, gm._scaling, gm._rotation, gm._opacity]
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, params)]
    return loss.detach(), grads


def run_reference_loop(gm, cameras, heatmaps, W, H, dataset, iterations, accumulation_steps=4, lambda_consistency=1e-5,
                       on_step=None, early_stopping=None, missing=frozenset()):
    """`on_step(gm)`: called after every optimiser step.  `early_stopping`: a callable loss -> bool fed `loss.item()` of every
    iteration like train.py:155; when it fires the optimiser steps at once and the loop ends (train.py:182, 227-233) -- the
    stopping iteration is then left in `run_reference_loop.stopped_at` (None otherwise).  (This restatement is itself held to
    the reference's own train.training(), run in the build container: tests/golden/reference_loop.npz, tests/test_loop_golden.py.)
    `missing`: joints that are UNOBSERVED (DESIGN.md "Unobserved joints"; the reference has no such notion -- this is the
    library's own definition, restated): their Gaussians are left out of every render, a limb pair that touches one is left out
    of the loss, and their heat-map planes must be zero (asserted).  Their rows of `gm._xyz` may hold anything, NaN included:
    nothing reads them and their gradient is zero.  missing == set() is the loop as it always was, bit for bit."""
    V = len(cameras)
    missing = frozenset(int(p) for p in missing)
    for p in missing:
        assert all(float(torch.as_tensor(heatmaps[v][p]).abs().max()) == 0.0 for v in range(V)), f"joint {p}: a plane is not zero"
    accumulated = torch.zeros((V,) + tuple(gm._xyz.shape))
    cam_idx_counter = 0
    run_reference_loop.stopped_at = None
    for iteration in range(1, iterations + 1):
        gm.update_learning_rate(iteration)
        idx = cam_idx_counter % V
        cam_idx_counter += 1
        loss, (gx, gs, gr, go) = view_grads_ref(gm, cameras[idx], heatmaps[idx], W, H, dataset, lambda_consistency, missing)
        stop = early_stopping is not None and bool(early_stopping(loss.item()))
        accumulated[idx] = gx
        gm._scaling.grad, gm._rotation.grad, gm._opacity.grad = gs, gr, go
        if iteration % accumulation_steps == 0 or stop:
            gm._xyz.grad = accumulated.mean(dim=0)
            with torch.no_grad():
                gm.optimizer.step()
                gm.optimizer.zero_grad(set_to_none=True)
            if on_step is not None:
                on_step(gm)
        if stop:
            run_reference_loop.stopped_at = iteration
            break
    return gm._xyz.detach().clone()
