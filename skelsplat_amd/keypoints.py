"""The 2D keypoint read out of rendered heat-maps and the reference's keypoint-space criteria (C ABI: sks_softargmax_*).

utils/loss_utils.py:41-64 `softargmax2d` and the criteria built on it -- `l2`, `l2_sqrt`, `huber`, `cauchy` of
utils/__init__.py's `losses` -- compare the keypoint of every rendered channel with the detection `poses_2d[c, :, :2]`.
Only the image-sized work is HIP (one read of the image forward, one read and one write backward, csrc/sks_keypoint.hip);
the criterion on the (J, 2) coordinates is a handful of tensor ops on the device that autograd carries into `softargmax2d`.

The blends with a dense L1 image term (`l1_l2`, `l1_huber`, `l1_masked_l2`, `l1_masked_huber`) are NOT here: `losses`
holds the reference's keys for what exists and no others.
"""
import torch

from . import _lib
from .ops import _chk, l2_loss_gaussian


def _planes(x):
    if x.dim() < 2:
        raise RuntimeError(f"softargmax2d expects (..., H, W), got {tuple(x.shape)}")
    H, W = int(x.shape[-2]), int(x.shape[-1])
    n = H * W
    return (x.numel() // n if n else 0), H, W


def _fwd(x, beta):
    """x: contiguous fp32 (..., H, W) on the device -> xy (planes, 2), stats (planes, SKS_SOFTARGMAX_STATS).  No host synchronisation."""
    planes, H, W = _planes(x)
    dev = x.device
    lib = _lib.load()
    nbytes = int(lib.sks_softargmax_scratch_bytes(planes, W, H))      # (0 for sizes the call below rejects with their text)
    xy = torch.empty((planes, 2), dtype=torch.float32, device=dev)
    stats = torch.empty((planes, _lib.SKS_SOFTARGMAX_STATS), dtype=torch.float32, device=dev)
    scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sks_softargmax_fwd(planes, W, H, float(beta), x.data_ptr(), xy.data_ptr(), stats.data_ptr(), scratch.data_ptr(),
                                    nbytes, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "sks_softargmax_fwd")
    return xy, stats


def _bwd(x, stats, dL_dxy, beta):
    planes, H, W = _planes(x)
    dev = x.device
    g = dL_dxy.to(torch.float32).reshape(planes, 2).contiguous()
    dimg = torch.empty_like(x)
    with torch.cuda.device(dev):
        rc = _lib.load().sks_softargmax_bwd(planes, W, H, float(beta), x.data_ptr(), stats.data_ptr(), g.data_ptr(),
                                            dimg.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "sks_softargmax_bwd")
    return dimg


class _SoftArgmax2d(torch.autograd.Function):
    """Saves the image and six floats per plane {max, 1 / sum, E[col], E[row] as float pairs}, not a softmax."""

    @staticmethod
    def forward(ctx, inp, beta):
        x = _chk(inp, "inp")
        xy, stats = _fwd(x, beta)
        ctx.save_for_backward(x, stats)
        ctx.beta = beta
        return xy.view(*inp.shape[:-2], 2)

    @staticmethod
    def backward(ctx, g):
        x, stats = ctx.saved_tensors
        return _bwd(x, stats, g, ctx.beta), None


def softargmax2d(inp, beta=100.0):
    """utils/loss_utils.py:41-64: inp (..., H, W) float32 on the GPU -> (..., 2), the expectation of [column, row] in pixels
    under softmax(beta * inp) over each (H, W) plane.  Differentiable with respect to `inp`."""
    return _SoftArgmax2d.apply(inp, float(beta))


# ---- the criteria on the coordinates: the reference's arithmetic as written -------------------------------------------------
# pred, gt_2d: (..., J, 2); the reduction='none' forms.

def _l2_xy(pred, gt_2d, delta=None):
    return (pred - gt_2d) ** 2


def _huber_xy(pred, gt_2d, delta=1.0):
    error = torch.abs(pred - gt_2d)
    # (the outer branch is the reference's: |delta - error| - 0.5 delta, not delta (error - 0.5 delta))
    return torch.where(error <= delta, error ** 2, torch.abs(delta - error) - 0.5 * delta)


def _cauchy_xy(pred, gt_2d, delta=None):
    return torch.log(1 + ((pred - gt_2d) / 1.0) ** 2)


def _reduce(loss, reduction):
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss


def l2_loss(rendering, gt_heatmap, gt_2d, lambda_loss=1.0, reduction="mean"):
    """utils/loss_utils.py:76-83."""
    return _reduce(_l2_xy(softargmax2d(rendering), gt_2d), reduction)


def l2_loss_sqrt(rendering, gt_heatmap, gt_2d, lambda_loss=1.0, reduction="mean"):
    """utils/loss_utils.py:131-138: ONE square root over the sum of all joints and both coordinates -- a scalar under every
    `reduction` (its gradient is 0 / 0 where the keypoints sit exactly on the detections, as the reference's is)."""
    return _reduce(torch.sqrt(_l2_xy(softargmax2d(rendering), gt_2d).sum()), reduction)


def huber_loss(rendering, gt_heatmap, gt_2d, lambda_loss=1.0, delta=1.0, reduction="mean"):
    """utils/loss_utils.py:141-150."""
    return _reduce(_huber_xy(softargmax2d(rendering), gt_2d, delta), reduction)


def cauchy_loss(rendering, gt_heatmap, gt_2d, lambda_loss=1.0, reduction="mean"):
    """utils/loss_utils.py:215-223."""
    return _reduce(_cauchy_xy(softargmax2d(rendering), gt_2d), reduction)


# utils/__init__.py's `losses`, the keys that exist here
losses = {"l2": l2_loss, "l2_sqrt": l2_loss_sqrt, "huber": huber_loss, "cauchy": cauchy_loss, "l2_gaussian": l2_loss_gaussian}

_XY = {"l2": _l2_xy, "l2_sqrt": None, "huber": _huber_xy, "cauchy": _cauchy_xy}


def detections_by_size(cameras, gt_2d):
    """{(H, W): (Vg, J, 2)}: the detections of the cameras of each image size, in ascending view order -- the rows of the
    (Vg, C, H, W) batches MultiViewLoop hands to `loss_grad`, one batch per image size.  gt_2d: (V, J, 2) on the device."""
    rows = {}
    for v, cam in enumerate(cameras):
        rows.setdefault((int(cam.image_height), int(cam.image_width)), []).append(v)
    return {hw: gt_2d[torch.tensor(vs, dtype=torch.long, device=gt_2d.device)] for hw, vs in rows.items()}


def keypoint_loss_grad(name, gt_2d, beta=100.0, delta=1.0):
    """A `loss_grad` for MultiViewLoop: (render, gt) of a (Vg, C, H, W) batch -> (true gradient, per-view loss, ones).
    One softargmax forward over all Vg * C planes, the criterion `name` of every view with 'mean' reduction (what train.py:150
    computes per view), one backward pass over the image.  The heat-map `gt` is not read: these criteria compare keypoints.

    gt_2d: the detections of the batch's views, (Vg, J, 2) on the device.  MultiViewLoop calls `loss_grad` once per IMAGE SIZE with
    that size's views and nothing that names them, so for cameras of several sizes pass a dict {(H, W): (Vg, J, 2)} -- rows in
    ascending view order, `detections_by_size(cameras, poses_2d)` builds it -- and the callable picks its rows by the batch's
    (H, W).  A tensor serves every batch it is called with (one image size)."""
    if name not in _XY:
        raise KeyError(f"keypoint_loss_grad: `{name}` is not a keypoint criterion (have {sorted(_XY)})")
    crit = _XY[name]

    def loss_grad(render, gt=None):
        x = _chk(render, "render")
        if x.dim() != 4:
            raise RuntimeError(f"render must be (V, C, H, W), got {tuple(x.shape)}")
        g2d = gt_2d[(int(x.shape[2]), int(x.shape[3]))] if isinstance(gt_2d, dict) else gt_2d
        if tuple(g2d.shape) != (x.shape[0], x.shape[1], 2):
            raise RuntimeError(f"gt_2d {tuple(g2d.shape)} does not fit a render of {tuple(x.shape)}")
        xy, stats = _fwd(x, beta)
        with torch.enable_grad():       # (the loop calls this under no_grad; only these (Vg, J, 2) tensor ops are recorded)
            pred = xy.view(x.shape[0], x.shape[1], 2).requires_grad_(True)
            if crit is None:
                loss = torch.sqrt(_l2_xy(pred, g2d).sum(dim=(1, 2)))
            else:
                loss = crit(pred, g2d, delta).mean(dim=(1, 2))
            (g,) = torch.autograd.grad(loss.sum(), pred)
        loss = loss.detach()
        return _bwd(x, stats, g, beta), loss, torch.ones_like(loss)

    return loss_grad
