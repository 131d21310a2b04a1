"""Initial joints fused from the views' monocular 3D predictions (reference: compute_weighted_average_pose of
dataset_tools/h36m/compute_initial_guess.py:23-116 and dataset_tools/panoptic/compute_initial_guess_panoptic.py:23-117 -- what the
configs' `initial_guess: "metrabs"` / `"metrabs_occ_3"` start every frame from).

The reference walks frames x candidates x cameras x joints in Python; fuse_predictions does the frames of a whole sequence at
once: on a ROCm device by one launch of the library's kernel (sks_fuse_predictions), on the host by one vectorised float64
expression."""
import numpy as np
import torch

from . import _pose_args as _pa

_NORM_DTYPES = {torch.float64: torch.float64, torch.float32: torch.float32, np.float64: torch.float64, np.float32: torch.float32,
                np.dtype("float64"): torch.float64, np.dtype("float32"): torch.float32}


def _fuse_cpu(P, X, x, keep, norm):
    """P (V,3,4) or (N,V,3,4), X (N,V,J,3), x (N,V,J,2), all float64; keep (N,V,J) bool or None; norm: the dtype of the weight
    chain -> fused (N,J,3) float64, ebar (N,V,J) float64, n_used (N,J) int32."""
    N, V, J = X.shape[:3]
    Pc = (P if P.dim() == 4 else P[None])[:, None, :, None]             # (N|1, 1, Vc, 1, 3, 4)
    Xi = X[:, :, None, :, None, :]                                      # (N, Vi, 1, J, 1, 3)
    h = Pc[..., 0] * Xi[..., 0] + Pc[..., 1] * Xi[..., 1] + Pc[..., 2] * Xi[..., 2] + Pc[..., 3]      # (N,Vi,Vc,J,3)
    d = (h[..., :2] / h[..., 2:3] - x[:, None]).to(norm)                # the Panoptic script rounds u - x to float32 here
    e = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])       # (N,Vi,Vc,J)
    if keep is None:
        keep = torch.ones((N, V, J), dtype=torch.bool)
    e = torch.where(keep[:, None], e, torch.zeros((), dtype=norm))      # a left-out camera enters no mean ..
    n_used = keep.sum(dim=1)                                            # (N,J)
    ebar = e.sum(dim=2) / n_used[:, None].to(norm)                      # (N,Vi,J)
    w = torch.where(keep, 1 / ebar, torch.zeros((), dtype=norm))        # .. and a left-out candidate gets no weight
    w = (w / w.sum(dim=1, keepdim=True)).to(torch.float64)
    num = torch.where(keep[..., None], X * w[..., None], torch.zeros((), dtype=torch.float64)).sum(dim=1)
    fused = num / w.sum(dim=1)[..., None]
    nan = torch.full((), float("nan"), dtype=torch.float64)
    fused = torch.where((n_used > 0)[..., None], fused, nan)
    return fused, torch.where(keep, ebar.to(torch.float64), nan), n_used.to(torch.int32)


def fuse_predictions(proj_or_cameras, poses_3d, poses_2d, valid=None, norm_dtype=torch.float64, out=None,
                     return_errors=False, return_n_used=False):
    """The reprojection-error-weighted mean of the V views' 3D predictions for the N frames of a sequence at once.

    Per frame and joint, with candidate X_i = view i's prediction: e_ic = |pixel of P_c [X_i; 1] - x_c| (no test for points
    behind a camera), ebar_i = mean over c, w_i = (1 / ebar_i) / sum_k (1 / ebar_k), result = sum_i w_i X_i / sum_i w_i.
    `poses_3d`: (N,V,J,3) world coordinates, `poses_2d`: (N,V,J,>=2) pixel (x, y, ..) -- or (V,J,3) and (V,J,>=2), one frame,
    and then the results have no frame axis.  `proj_or_cameras`: (V,3,4) projection matrices, (N,V,3,4) for one rig per frame,
    or a list of V cameras (through projection_matrices).  `valid`: optional (N,V,J) bool, False = view v is out of that joint
    in both roles: its candidate gets no weight, its detection enters no ebar_i.  `norm_dtype`: torch.float64 -- everything
    float64, the H36M script -- or torch.float32 -- u - x rounded to float32, norm, mean, reciprocal and normalisation in
    float32, the average in float64, the Panoptic script.
    Returns the joints (N,J,3) float32 -- what the loops take as `points` --, written into `out` when given (a contiguous
    float32 or float64 tensor of that shape where the predictions live; float64 keeps the unrounded result).  With
    `return_errors=True` also ebar (N,V,J) float64 (NaN for a view left out), with `return_n_used=True` the (N,J) int32 count
    of kept views.  A joint with no kept view comes back NaN; with one it is that candidate.

    Predictions on a ROCm device: one launch of sks_fuse_predictions on the current stream (lane = candidate; float32 or
    float64 inputs are read as they are and widened exactly, nothing is copied to the host and nothing synchronises;
    detections and matrices given on the host are uploaded first).  A frame's result does not depend on N, on its place in
    the batch or on the stream.  Predictions on the host (arrays or CPU tensors): the same formula as one float64
    expression over all frames; arrays in, arrays out."""
    X, as_array = _pa.as_tensor(poses_3d)
    dev = X.device
    x = _pa.as_tensor(poses_2d)[0].to(dev)
    try:
        norm = _NORM_DTYPES[norm_dtype]
    except (KeyError, TypeError):
        raise ValueError(f"norm_dtype must be torch.float64 or torch.float32, got {norm_dtype!r}") from None
    P = _pa.projections(proj_or_cameras, dev)
    single = X.dim() == 3
    if single:
        X = X[None]
        x = x[None] if x.dim() == 3 else x
    if X.dim() != 4 or X.shape[-1] != 3:
        raise ValueError(f"poses_3d must be (N,V,J,3) or (V,J,3), got {tuple(poses_3d.shape)}")
    N, V, J = X.shape[:3]
    if x.dim() != 4 or tuple(x.shape[:3]) != (N, V, J) or x.shape[-1] < 2:
        raise ValueError(f"poses_2d must be (N,V,J,>=2) = {(N, V, J, 2)} like poses_3d, got {tuple(poses_2d.shape)}")
    if not (X.is_floating_point() and x.is_floating_point()):
        raise ValueError("poses_3d and poses_2d must be floating point")
    _pa.check_shapes(P, N, V, J)
    valid = _pa.check_valid(valid, single, dev, (N, V, J))
    if out is None:
        res = torch.empty((N, J, 3), dtype=torch.float32, device=dev)
    else:
        res = _pa.check_out(out, (N, J, 3), (torch.float32, torch.float64), dev, single)
    if dev.type == "cuda":
        from . import _lib
        Xd, xd, P = _pa.as_real(X), _pa.as_real(x[..., :2]), P.contiguous()
        errors = torch.empty((N, V, J), dtype=torch.float64, device=dev) if return_errors else None
        n_used = torch.empty((N, J), dtype=torch.int32, device=dev) if return_n_used else None
        with torch.cuda.device(dev):
            rc = _lib.load().sks_fuse_predictions(N, V, J, P.data_ptr(), _pa.rig_stride(P, V), *_pa.pointers(Xd), *_pa.pointers(xd),
                                                  _pa.byte_pointer(valid), int(norm == torch.float32), *_pa.pointers(res),
                                                  None if errors is None else errors.data_ptr(),
                                                  None if n_used is None else n_used.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "sks_fuse_predictions")
    else:
        fused, errors, n_used = _fuse_cpu(P, X.to(torch.float64), x[..., :2].to(torch.float64), valid, norm)
        res.copy_(fused)
    return _pa.results(res, out, single, as_array, [t for t, asked in ((errors, return_errors), (n_used, return_n_used)) if asked])
