"""DLT / SVD linear triangulation (reference: triangulation.py:59-67, 111-150), batched over joints.

BASELINE config 1 ("plumbing, no GPU"): the reference solves one 2V x 4 homogeneous system per joint with
np.linalg.svd in a Python loop; here the J systems are one batched torch.linalg.svd (CPU or ROCm tensor).
triangulate_sequence does the frames of a whole sequence at once: on a ROCm device by one launch of the library's
batched DLT kernel (sks_triangulate), on the host by one batched SVD.  With `reject_px` an exhaustive two-view consensus
picks the views that agree first (sks_triangulate_robust on the device, consensus_cpu on the host)."""
import itertools

import numpy as np
import torch

from . import _pose_args as _pa


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


def consensus_cpu(P, x, valid, reject_px, min_inliers):
    """The rule of sks_triangulate_robust on the host, float64, one batched SVD over every (frame, joint, pair): P (V,3,4) or
    (N,V,3,4), x (N,V,J,2), valid (N,V,J) bool or None -> inliers (N,V,J) bool, n_consensus (N,J) int32.  Per joint with
    three or more kept views every pair a < b of them is a hypothesis (the DLT of its four rows), a kept view is its inlier
    when the point lies in front of it and reprojects within `reject_px` of its detection, and the winner has the most
    inliers, then the smallest sum of their errors, then the lowest pair; its set is the answer when it holds at least
    `min_inliers` views, the kept views otherwise and for joints with fewer than three of them."""
    N, V, J = x.shape[:3]
    keep = torch.ones((N, V, J), dtype=torch.bool) if valid is None else valid
    inliers = keep.clone()
    n_kept = keep.sum(dim=1).to(torch.int32)
    n_cons = n_kept.clone()
    if V < 3:
        return inliers, n_cons
    pairs = list(itertools.combinations(range(V), 2))
    ia, ib = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    H = len(pairs)
    nan = torch.full((), float("nan"), dtype=torch.float64)
    step = max(1, (1 << 20) // (J * H * V))             # frames per slice: bounds the (n,J,H,V,3) reprojections
    for lo in range(0, N, step):
        sl = slice(lo, min(lo + step, N))
        Pn = P[sl] if P.dim() == 4 else P[None]             # (n or 1,V,3,4)
        xs, ks = x[sl], keep[sl].permute(0, 2, 1)           # (n,V,J,2), (n,J,V)
        r0 = xs[..., 0:1] * Pn[:, :, None, 2, :] - Pn[:, :, None, 0, :]      # (n,V,J,4)
        r1 = xs[..., 1:2] * Pn[:, :, None, 2, :] - Pn[:, :, None, 1, :]
        A = torch.stack([r0[:, ia], r1[:, ia], r0[:, ib], r1[:, ib]], dim=3).permute(0, 2, 1, 3, 4)      # (n,J,H,4,4)
        hyp = ks[..., ia] & ks[..., ib]                     # (n,J,H): both views kept
        finite = torch.isfinite(A).all(dim=(-1, -2))
        X = torch.linalg.svd(torch.where(finite[..., None, None], A, torch.zeros((), dtype=A.dtype)))[2][..., -1, :]
        X = torch.where(finite[..., None], X / X[..., 3:4], nan)             # a hypothesis on a NaN detection has no inliers
        u = torch.einsum("nvrk,njhk->njhvr", Pn.expand(xs.shape[0], V, 3, 4), X)      # (n,J,H,V,3)
        d = u[..., 2]
        det = xs.permute(0, 2, 1, 3)[:, :, None]            # (n,J,1,V,2)
        e = torch.hypot(u[..., 0] / d - det[..., 0], u[..., 1] / d - det[..., 1])
        inl = (d > 0) & (e <= reject_px) & ks[:, :, None, :] & hyp[..., None]          # (n,J,H,V)
        c = torch.where(hyp, inl.sum(dim=-1), torch.full((), -1, dtype=torch.int64))
        s = torch.where(inl, e, torch.zeros((), dtype=e.dtype)).sum(dim=-1)
        cmax = c.max(dim=-1, keepdim=True).values
        s = torch.where(c == cmax, s, torch.full((), float("inf"), dtype=s.dtype))
        first = (c == cmax) & (s == s.min(dim=-1, keepdim=True).values)
        win = torch.where(first, torch.arange(H), torch.full((), H)).min(dim=-1).values.clamp(max=H - 1)      # (n,J)
        wset = torch.gather(inl, 2, win[..., None, None].expand(-1, -1, 1, V))[:, :, 0]      # (n,J,V)
        wc = cmax[..., 0]
        tested = n_kept[sl] >= 3
        agreed = tested & (wc >= min_inliers)
        inliers[sl] = torch.where(agreed[:, None, :], wset.permute(0, 2, 1), keep[sl])
        n_cons[sl] = torch.where(tested, wc.to(torch.int32), n_kept[sl])
    return inliers, n_cons


def _checked_rejection(reject_px, min_inliers):
    reject_px = float(reject_px)
    if not (np.isfinite(reject_px) and reject_px > 0):
        raise ValueError(f"reject_px must be finite and > 0 pixels, got {reject_px}")
    if int(min_inliers) != min_inliers or not 2 <= int(min_inliers) <= 64:
        raise ValueError(f"min_inliers = {min_inliers}: a consensus takes 2 .. 64 views")
    return reject_px, int(min_inliers)


def triangulate_sequence(proj_or_cameras, poses_2d, valid=None, out=None, homogeneous=False, return_n_used=False,
                         reject_px=None, min_inliers=3, return_inliers=False, out_inliers=None):
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
    over all frames, left-out rows zeroed; arrays in, arrays out.

    `reject_px` (pixels, None = off: everything above, untouched): outlier rejection by exhaustive two-view consensus, the
    deterministic form of RANSAC, in front of the same DLT.  Per joint with three or more views kept by `valid`, every pair
    of them is a hypothesis (the DLT of the two), a kept view is its inlier when the point lies in front of it and
    reprojects within `reject_px` of its detection (a NaN or inf detection never is), and the winner has the most inliers,
    then the smallest sum of their errors, then the first pair.  With at least `min_inliers` (2 .. 64) views in the winner's
    set the joint is the DLT over that set, otherwise -- no consensus -- over all kept views as without rejection; joints
    with two kept views are their DLT, with fewer NaN.  One refit, no second inlier pass.  `return_inliers=True` appends
    `inliers` (N,V,J) bool, the views each joint was solved from, and `n_consensus` (N,J) int32, the winner's count
    (`n_consensus < min_inliers` marks a fallback; with fewer than three kept views it is their number), to the return
    value, after `n_used` when that is asked for too.  `out_inliers`: optional (inliers (N,V,J) bool or uint8, n_consensus
    (N,J) int32) contiguous tensors where the detections live, written in place (what the loops keep).  On a ROCm device:
    sks_triangulate_robust, two launches on the current stream -- the consensus kernel (lane = hypothesis), then the plain
    kernel with `valid = inliers`, so the joints are bit for bit triangulate_sequence(valid=inliers).  On the host:
    consensus_cpu, then the host path above."""
    robust = reject_px is not None
    if robust:
        reject_px, min_inliers = _checked_rejection(reject_px, min_inliers)
    elif return_inliers or out_inliers is not None:
        raise ValueError("return_inliers / out_inliers need reject_px: without rejection every kept view enters (inliers == valid)")
    x, as_array = _pa.as_tensor(poses_2d)
    dev = x.device
    P = _pa.projections(proj_or_cameras, dev)
    single = x.dim() == 3
    x = x[None] if single else x
    if x.dim() != 4 or x.shape[-1] < 2:
        raise ValueError(f"poses_2d must be (N,V,J,>=2) or (V,J,>=2), got {tuple(poses_2d.shape)}")
    N, V, J = x.shape[:3]
    _pa.check_shapes(P, N, V, J)
    valid = _pa.check_valid(valid, single, dev, (N, V, J))
    shape, dtype = ((N, J, 4), torch.float64) if homogeneous else ((N, J, 3), torch.float32)
    res = torch.empty(shape, dtype=dtype, device=dev) if out is None else _pa.check_out(out, shape, (dtype,), dev, single)
    inl = n_cons = None
    if robust and out_inliers is not None:
        inl = _pa.check_out(out_inliers[0], (N, V, J), (torch.bool, torch.uint8), dev, name="`out_inliers[0]`")
        n_cons = _pa.check_out(out_inliers[1], (N, J), (torch.int32,), dev, name="`out_inliers[1]`")
    elif robust:
        inl = torch.empty((N, V, J), dtype=torch.bool, device=dev)
        n_cons = torch.empty((N, J), dtype=torch.int32, device=dev)
    if dev.type == "cuda":
        from . import _lib
        xd, P = _pa.as_real(x[..., :2]), P.contiguous()
        n_used = torch.empty((N, J), dtype=torch.int32, device=dev) if return_n_used else None
        lib = _lib.load()
        det = (*_pa.pointers(xd), _pa.byte_pointer(valid))
        outs = (*_pa.pointers(res), None if n_used is None else n_used.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            if robust:
                rc = lib.sks_triangulate_robust(N, V, J, P.data_ptr(), _pa.rig_stride(P, V), *det, reject_px, min_inliers,
                                                inl.data_ptr(), n_cons.data_ptr(), *outs)
            else:
                rc = lib.sks_triangulate(N, V, J, P.data_ptr(), _pa.rig_stride(P, V), *det, *outs)
        _lib.check(rc, "sks_triangulate_robust" if robust else "sks_triangulate")
    else:
        x64 = x[..., :2].to(torch.float64)
        if robust:
            keep, n_c = consensus_cpu(P, x64, valid, reject_px, min_inliers)
            inl.copy_(keep)
            n_cons.copy_(n_c)
            valid = keep
        S, n_used = _systems_cpu(P, x64, valid)
        # (no consensus over a NaN detection: the joint is NaN as on the device, where LAPACK would refuse the batch)
        bad = ~torch.isfinite(S).all(dim=(-1, -2)) if robust else None
        if bad is not None and bool(bad.any()):
            S = torch.where(bad[..., None, None], torch.zeros((), dtype=S.dtype), S)
        X = torch.linalg.svd(S)[2][..., -1, :]
        X = X / X[..., 3:4]
        X = torch.where((n_used >= 2)[..., None], X, torch.full((), float("nan"), dtype=X.dtype))
        if bad is not None:
            X = torch.where(bad[..., None], torch.full((), float("nan"), dtype=X.dtype), X)
        res.copy_(X if homogeneous else X[..., :3])
    extras = [n_used] if return_n_used else []
    if return_inliers:
        extras += [inl if inl.dtype == torch.bool else inl.view(torch.bool), n_cons]
    return _pa.results(res, out, single, as_array, extras)
