"""The CPU reference of the sparse fused-loss step (sks_geometry + sks_backward_fused_loss), one view at a time: oracle render ->
clamp(0, 1) -> masked L2 (utils/loss_utils.py:86-100 on the clamped render, train.py:150) -> oracle backward of 2 (render - gt) on
the mask, through the clamp's pass-through.  numpy + oracle.oracle only: no device.  Shared by tests/test_fullsize_gpu.py (the
bench scenes), tests/test_fused_loss_cpu.py and tests/test_fused_loss_gpu.py (the scenes of tests/fused_loss_cases.py)."""
import types

import numpy as np

from oracle import oracle as orc

# gradient dictionary key of backward_fused_loss -> the oracle's name
GRADS = (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
         ("rotations", "dL_drotations"), ("cov3D", "dL_dcov3D"))


def view_reference(params, ocam, gt, bg=None, antialiasing=False, scale_modifier=1.0, cov3D_precomp=None, bounds=False, fwd=None):
    """One view.  params: (means3D, features, opacities, scales, rotations) as numpy arrays (scales / rotations None with
    cov3D_precomp); gt: (C,H,W) fp32 planes of any sign; bg: up to C floats, left out of the forward and kept in the backward like
    the reference (quirk Q2); fwd: this view's orc.forward output when the caller has it already.
    -> namespace with fwd, render (clipped), mask, N (int), S (float64 sum of the squared float32 differences), dL and bwd (the
    oracle's gradients of the UNSCALED sum S, as the entry point returns them; bwd["bound"] with bounds=True)."""
    means, feat, opac, scales, quats = params
    o = fwd if fwd is not None else orc.forward(means, feat, opac, scales, quats, cov3D_precomp, ocam,
                                                scale_modifier=scale_modifier, antialiasing=antialiasing)
    gt = np.asarray(gt, dtype=np.float32)
    render = np.clip(o["color"], 0.0, 1.0)
    mask = (gt > 0) | (render > 0)
    diff = (render - gt).astype(np.float32)
    S = float((diff.astype(np.float64) ** 2)[mask].sum())
    N = int(mask.sum())
    dL = (2.0 * diff * mask * ((o["color"] >= 0) & (o["color"] <= 1))).astype(np.float32)   # clamp's pass-through
    b = orc.backward(o, means, feat, opac, scales, quats, cov3D_precomp, ocam, dL, None, bg=bg, scale_modifier=scale_modifier,
                     antialiasing=antialiasing, bounds=bounds)
    return types.SimpleNamespace(fwd=o, render=render, mask=mask, diff=diff, S=S, N=N, dL=dL, bwd=b)


def case_reference(case):
    """Every view of a tests/fused_loss_cases.py case -> list of view_reference results."""
    return [view_reference(case.params, case.ocams[v], case.gt[v], bg=case.bg, antialiasing=case.aa, scale_modifier=case.smod,
                           cov3D_precomp=case.cov, bounds=case.bounds) for v in range(case.V)]


_REFS = {}


def refs_of(name):
    """(the suite's case `name`, its per-view references), computed once per process and left unchanged."""
    from tests import fused_loss_cases
    if name not in _REFS:
        case = fused_loss_cases.draw(name)
        _REFS[name] = (case, case_reference(case))
    return _REFS[name]


def corrected_sum(ref, gt):
    """Sum of e^2 + gt^2 over the pixels the kernel corrects (render > 0): the size of the terms its fp32 partial sums carry."""
    gt = np.asarray(gt, dtype=np.float64)
    sel = ref.render > 0
    return float((ref.diff.astype(np.float64) ** 2 + gt * gt)[sel].sum())
