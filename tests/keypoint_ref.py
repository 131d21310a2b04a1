"""TEST INFRASTRUCTURE -- float64 restatement of the reference's `softargmax2d` and of its four keypoint criteria
(utils/loss_utils.py:41-64, 76-83, 131-150, 215-223), CPU only.  Nothing here loads the HIP library or imports
skelsplat_amd; tests/test_keypoints_cpu.py holds it to the reference's own fp32 results
(tests/golden/reference_keypoint.npz) and measures how far those lie from it.

The formulas are written from the definitions, not copied from the code under test: the softmax is normalised explicitly, and
the coordinates are the pixel indices themselves (the reference weights with linspace(0, 1, w) and multiplies by w - 1).
"""
import torch

# ---- measured: how far the reference's OWN fp32 CPU results lie from this restatement ------------------------------------
# tests/test_keypoints_cpu.py::test_restatement_agrees_with_the_reference_fixture computes these over the whole case set of
# tests/keypoint_cases.py (12 images) and pins them; MEASUREMENTS.md "softargmax2d" has the table.  Coordinates relative to
# W - 1 / H - 1, losses relative to the value (all four criteria, 'mean' / 'sum' / 'none').
# Both maxima come from `chunks_peak002` (251 x 263, peak 0.02): there the softmax is nearly uniform, the reference adds
# 66 013 products of ~1.5e-5 in fp32 and lands 6e-3 px off; a residual of 0.05 px (keypoint_cases.RESIDUALS) squared turns
# that into 19 % of an l2 'none' element.  Where the peak is near 1 the figures are 2e-7 and 1e-3.
REF_FP32_DEV_COORD = 2.36e-5    # measured 2.351e-5 of (W - 1), (H - 1)
REF_FP32_DEV_LOSS = 0.19        # measured 0.18998 of the value
# The device bar: 4 x the reference's own deviation, against the same restatement -- a different but fixed summation order and
# a different exp.  It never comes from the kernel's output.
DEVICE_FACTOR = 4.0


def softargmax2d(x, beta=100.0):
    """x (..., H, W) -> (..., 2) float64: [E col, E row] under softmax(beta x) over each plane."""
    x = x.to(torch.float64)
    H, W = x.shape[-2], x.shape[-1]
    z = beta * x.reshape(*x.shape[:-2], H * W)
    e = torch.exp(z - z.max(dim=-1, keepdim=True).values)
    p = e / e.sum(dim=-1, keepdim=True)
    k = torch.arange(H * W)
    col, row = (k % W).to(torch.float64), torch.div(k, W, rounding_mode="floor").to(torch.float64)
    return torch.stack([(p * col).sum(dim=-1), (p * row).sum(dim=-1)], dim=-1)


def criterion_xy(name, pred, gt_2d, delta=1.0):
    """The reference's reduction='none' form on float64 coordinates."""
    r = pred - gt_2d.to(torch.float64)
    if name == "l2":
        return r * r
    if name == "l2_sqrt":
        return (r * r).sum().sqrt()                      # ONE root over all joints and both coordinates
    if name == "huber":
        a = r.abs()
        return torch.where(a <= delta, a * a, (delta - a).abs() - 0.5 * delta)     # the reference's outer branch, as written
    if name == "cauchy":
        return torch.log1p(r * r)
    raise KeyError(name)


def reduce(loss, reduction):
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


def criterion(name, rendering, gt_2d, reduction="mean", delta=1.0, beta=100.0):
    return reduce(criterion_xy(name, softargmax2d(rendering, beta), gt_2d, delta), reduction)


CRITERIA = ("l2", "l2_sqrt", "huber", "cauchy")
