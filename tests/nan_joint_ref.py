"""TEST INFRASTRUCTURE -- the references the unobserved-joint tests compare with (DESIGN.md "Unobserved joints"), CPU only:

  raster_reference   the CPU oracle's forward and backward (with its rounding bounds) of a case's `cull` form -- the NaN rows at a
                     finite point behind every camera.  The oracle is never given a NaN.
  masked_literal_loop  tests/ref_loop.run_reference_loop with `missing=`: the reference's per-iteration loop with the unobserved
                     joint's Gaussian left out of the render, its planes zero and the limb pair it touches left out of the loss.
  masked_cons32      the limb term of the loss the criterion sees, float32(lambda x masked limb loss).
  zero_plane_factors what the heat-map factors of a plane without an impulse are.
"""
import copy
import functools

import numpy as np
import torch

from tests import geometry_cases as G, nan_joint_cases as NC, tail_ref


@functools.lru_cache(maxsize=None)
def raster_reference(name):
    """(case, oracle forwards per view, oracle backwards per view with bounds, dL_color, dL_invdepth) of the `cull` form;
    computed once and shared: nobody writes into it."""
    c = NC.get(name)
    fwd = [G.oracle_forward(c.cull, v) for v in range(c.V)]
    dLc, dLi = G.draw_dL(c.cull)
    bwd = [G.oracle_backward(c.cull, v, fwd[v], dLc, dLi, bounds=True) for v in range(c.V)]
    return c, fwd, bwd, dLc, dLi


def masked_cons32(xyz, lam, missing, limb=tail_ref.H36M_LIMB):
    """float32(float32(lambda) x limb loss without the pairs that touch `missing`), from the joints before the step."""
    x = torch.as_tensor(xyz).detach().cpu().double()
    return float(np.float32(np.float32(lam) * float(tail_ref.limb_loss(x, limb, missing))))


def masked_literal_loop(sc, model, points, heatmaps, iterations, missing, lambda_consistency=1e-5, early_stopping=None):
    """The literal loop on the CPU from `points` (P,3; the rows of `missing` may hold NaN) and `heatmaps` (V,J,H,W), the
    template's scaling / rotation / opacity.  Returns (final joints (P,3), mean distance the observed joints moved)."""
    from tests.ref_loop import run_reference_loop
    gm = model("cpu")
    pts = torch.as_tensor(np.asarray(points), dtype=torch.float32).cpu()
    with torch.no_grad():
        gm._xyz.copy_(pts)
    cams = [copy.copy(c).to("cpu") for c in sc.cameras]
    hm = torch.as_tensor(heatmaps).detach().cpu()
    out = run_reference_loop(gm, cams, hm, sc.W, sc.H, "h36m", iterations, lambda_consistency=lambda_consistency,
                             early_stopping=early_stopping, missing=missing)
    seen = [p for p in range(pts.shape[0]) if p not in set(missing)]
    moved = float((out[seen] - pts[seen]).norm(dim=1).mean())
    return out, moved


def zero_plane_factors(row, col, cmin, den, v, j):
    """Asserts that plane (v, j) of heat-map factors is the plane without an impulse: row, col, cmin exactly 0, den exactly
    float32(1e-8)."""
    r, c = row[v, j].cpu(), col[v, j].cpu()
    assert float(r.abs().max()) == 0.0 and float(c.abs().max()) == 0.0, (v, j, "row / col hold something")
    assert float(cmin[v, j]) == 0.0, (v, j, float(cmin[v, j]))
    assert np.float32(float(den[v, j])) == np.float32(1e-8), (v, j, float(den[v, j]))
