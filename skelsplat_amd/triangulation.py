"""DLT / SVD linear triangulation (reference: triangulation.py:59-67, 111-150), batched over joints.

BASELINE config 1 ("plumbing, no GPU"): the reference solves one 2V x 4 homogeneous system per joint with
np.linalg.svd in a Python loop; here the J systems are one batched torch.linalg.svd (CPU or ROCm tensor).
triangulate_sequence does the frames of a whole sequence at once: on a ROCm device by one launch of the library's
batched DLT kernel (sks_triangulate), on the host by one batched SVD."""
import numpy as np
import torch


def projection_matrices(cameras):
    """P = K [R | t] per camera (triangulation.py:59-67 / 111-119); cameras carry R (camera-to-world), T, K."""
    out = []
    for c in cameras:
        RT = np.hstack((c.R.T, np.asarray(c.T).reshape(3, 1)))
        out.append(np.dot(c.K, RT))
    return np.stack(out, 0)


def triangulate_poses(P_list, poses_2d):
    """triangulation.py:122-150: P_list (V,3,4), poses_2d (V,J,>=2) -> (J,4) homogeneous points with X[3] == 1."""
    P = torch.as_tensor(np.asarray(P_list), dtype=torch.float64)
    x = torch.as_tensor(poses_2d, dtype=torch.float64)[..., :2].to(P.device)
    V, J = x.shape[0], x.shape[1]
    # rows (x * P[2] - P[0]) and (y * P[2] - P[1]) for every view, stacked view-major like the reference
    r0 = x[..., 0:1] * P[:, None, 2, :] - P[:, None, 0, :]          # (V,J,4)
    r1 = x[..., 1:2] * P[:, None, 2, :] - P[:, None, 1, :]
    A = torch.stack([r0, r1], dim=1).reshape(2 * V, J, 4).permute(1, 0, 2)   # (J, 2V, 4)
    _, _, Vt = torch.linalg.svd(A)
    X = Vt[:, -1, :]
    return (X / X[:, 3:4]).cpu().numpy()


def device_projection_matrices(cameras, device):
    """projection_matrices(cameras) as a contiguous float64 (V,3,4) tensor on `device`: what the loops keep for
    triangulate_sequence.  None when the cameras carry no intrinsics K (then initial joints have to be given)."""
    if not all(hasattr(c, "K") and hasattr(c, "R") and hasattr(c, "T") for c in cameras):
        return None
    return torch.as_tensor(projection_matrices(cameras), dtype=torch.float64).contiguous().to(device)


def _systems_cpu(P, x, valid):
    """The reference's systems for every (frame, joint): P (V,3,4) or (N,V,3,4), x (N,V,J,2), valid (N,V,J) bool or None
    -> A (N,J,2V,4) with the rows of left-out detections zero, n_used (N,J)."""
    N, V, J = x.shape[:3]
    r0 = x[..., 0:1] * P[..., None, 2, :] - P[..., None, 0, :]      # (N,V,J,4)
    r1 = x[..., 1:2] * P[..., None, 2, :] - P[..., None, 1, :]
    A = torch.stack([r0, r1], dim=2).permute(0, 3, 1, 2, 4)         # (N,J,V,2,4): view-major rows like the reference
    if valid is None:
        n_used = torch.full((N, J), V, dtype=torch.int32)
    else:
        keep = valid.permute(0, 2, 1)                                # (N,J,V)
        A = torch.where(keep[..., None, None], A, torch.zeros((), dtype=A.dtype))
        n_used = keep.sum(dim=2).to(torch.int32)
    return A.reshape(N, J, 2 * V, 4), n_used


def triangulate_sequence(proj_or_cameras, poses_2d, valid=None, out=None, homogeneous=False, return_n_used=False):
    """triangulate_poses for the N frames of a sequence at once (triangulation.py:122-150 per frame and joint).

    `poses_2d`: (N,V,J,>=2) pixel (x, y, ..) -- or (V,J,>=2), one frame, and then the results have no frame axis.
    `proj_or_cameras`: (V,3,4) projection matrices, (N,V,3,4) for one rig per frame, or a list of V cameras (through
    projection_matrices).  `valid`: optional (N,V,J) bool, False = leave this detection out of its joint's system.
    Returns the joints (N,J,3) float32 -- what the loops take as `points` -- or, with `homogeneous=True`, (N,J,4) float64 with
    w == 1 as the reference returns them; written into `out` when given (a contiguous tensor of that shape and dtype
    where the detections live).  With `return_n_used=True` also the (N,J) int32 count of detections that entered each
    joint's system.  A joint seen by fewer than two kept views has no solution: it comes back NaN.

    Detections on a ROCm device: one launch of sks_triangulate on the current stream (float64 one-sided Jacobi, lane =
    view; float32 or float64 detections are read as they are, nothing is copied to the host and nothing synchronises;
    projection matrices given on the host are uploaded first).  A frame's result does not depend on N, on its place in the
    batch or on the stream.  Detections on the host (arrays or CPU tensors): the batched float64 SVD of triangulate_poses
    over all frames, left-out rows zeroed; arrays in, arrays out."""
    as_array = not torch.is_tensor(poses_2d)
    x = torch.as_tensor(np.asarray(poses_2d)) if as_array else poses_2d
    dev = x.device
    if torch.is_tensor(proj_or_cameras):
        P = proj_or_cameras.to(device=dev, dtype=torch.float64)
    elif isinstance(proj_or_cameras, np.ndarray):
        P = torch.as_tensor(proj_or_cameras, dtype=torch.float64).to(dev)
    else:
        seq = list(proj_or_cameras)
        P = torch.as_tensor(np.asarray(seq) if seq and not hasattr(seq[0], "K") else projection_matrices(seq),
                            dtype=torch.float64).to(dev)
    single = x.dim() == 3
    if single:
        x = x[None]
        valid = None if valid is None else torch.as_tensor(valid)[None]
    if x.dim() != 4 or x.shape[-1] < 2:
        raise ValueError(f"poses_2d must be (N,V,J,>=2) or (V,J,>=2), got {tuple(poses_2d.shape)}")
    N, V, J = x.shape[:3]
    if N < 1 or J < 1:
        raise ValueError(f"poses_2d {tuple(x.shape)}: at least one frame and one joint")
    if not 1 <= V <= 64:
        raise ValueError(f"{V} views: a joint's system takes 1 .. 64 (SKS_MAX_VIEWS)")
    if tuple(P.shape) not in ((V, 3, 4), (N, V, 3, 4)):
        raise ValueError(f"projection matrices must be (V,3,4) = {(V, 3, 4)} or (N,V,3,4) = {(N, V, 3, 4)}, "
                         f"got {tuple(P.shape)}")
    if valid is not None:
        valid = torch.as_tensor(valid).to(device=dev, dtype=torch.bool)
        if tuple(valid.shape) != (N, V, J):
            raise ValueError(f"valid must be (N,V,J) = {(N, V, J)}, got {tuple(valid.shape)}")
    shape, dtype = ((N, J, 4), torch.float64) if homogeneous else ((N, J, 3), torch.float32)
    if out is not None:
        want = shape[1:] if single and out.dim() == 2 else shape
        if (not torch.is_tensor(out) or tuple(out.shape) != want or out.dtype != dtype or out.device != dev
                or not out.is_contiguous()):
            raise ValueError(f"`out` must be a contiguous {dtype} tensor of shape {want} on {dev}")
        res = out.view(shape)
    else:
        res = torch.empty(shape, dtype=dtype, device=dev)
    if dev.type == "cuda":
        from . import _lib
        xd = x[..., :2]
        xd = (xd if xd.dtype == torch.float64 else xd.to(torch.float32)).contiguous()
        P = P.contiguous()
        vd = None if valid is None else valid.contiguous().view(torch.uint8)
        n_used = torch.empty((N, J), dtype=torch.int32, device=dev) if return_n_used else None
        f64 = xd.dtype == torch.float64
        with torch.cuda.device(dev):
            rc = _lib.load().sks_triangulate(N, V, J, P.data_ptr(), V * 12 if P.dim() == 4 else 0,
                                             None if f64 else xd.data_ptr(), xd.data_ptr() if f64 else None,
                                             None if vd is None else vd.data_ptr(),
                                             None if homogeneous else res.data_ptr(), res.data_ptr() if homogeneous else None,
                                             None if n_used is None else n_used.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "sks_triangulate")
    else:
        A, n_used = _systems_cpu(P, x[..., :2].to(torch.float64), valid)
        X = torch.linalg.svd(A)[2][..., -1, :]
        X = X / X[..., 3:4]
        X = torch.where((n_used >= 2)[..., None], X, torch.full((), float("nan"), dtype=X.dtype))
        res.copy_(X if homogeneous else X[..., :3])
    ret = out if out is not None else (res[0] if single else res)
    if as_array and out is None:
        ret = ret.numpy()
    if not return_n_used:
        return ret
    n_used = n_used[0] if single else n_used
    return ret, (n_used.numpy() if as_array else n_used)
