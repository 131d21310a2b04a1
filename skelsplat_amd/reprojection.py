"""The reprojection error of a multi-view estimate -- the ground-truth-free figure: the distance in pixels between a joint
projected into a view and that view's detection (reference: compute_reprojection_error,
dataset_tools/h36m/compute_initial_guess.py:23-79) -- measured (reproject, evaluate_sequence_reprojection) and minimised from a
start (refine_triangulation: Hartley & Zisserman's "gold standard" triangulation next to triangulate_sequence's DLT).

Tensors on a ROCm device go through csrc/sks_reproject.hip (sks_reproject, sks_eval_reprojection, sks_triangulate_refine): one
launch each on the current stream, nothing is copied to the host and nothing synchronises.  Arrays and CPU tensors run the same
formulas on the host in float64 numpy, as triangulate_sequence does for its SVD; arrays in, arrays out."""
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import _pose_args as _pa
from ._pose_args import MAX_VIEWS, as_real as _as_real       # (names other modules and tests read from here)

REFINE_MAX_ITERS = 16               # SKS_REFINE_MAX_ITERS
# the constants of k_refine (csrc/sks_reproject.hip), which the host path shares
LAMBDA0, LAMBDA_DOWN, LAMBDA_UP, STOP_FRACTION = 1e-3, 0.1, 10.0, 1e-6
FIELDS = ("uv", "err", "in_front", "per_joint", "per_view", "per_frame", "n_used")


@dataclass
class Reprojection:
    """What reproject returns; a field that was not asked for is None.  uv (N,V,J,2), err (N,V,J), per_joint (N,J), per_view
    (N,V), per_frame (N) float64; in_front (N,V,J) bool; n_used (N,J) int32 (without the frame axis for one frame)."""
    uv: Optional[Any] = None
    err: Optional[Any] = None
    in_front: Optional[Any] = None
    per_joint: Optional[Any] = None
    per_view: Optional[Any] = None
    per_frame: Optional[Any] = None
    n_used: Optional[Any] = None


# ------------------------------------------------------------------------------------------------ the formulas on the host
def _project_np(P, X):
    """P (N or 1,V,3,4), X (N,J,3) float64 -> u0, u1, u2 (N,V,J): P_v [X; 1] added in column order 0..3."""
    Pb, Xb = P[:, :, None], X[:, None]
    row = lambda r: ((Pb[..., r, 0] * Xb[..., 0] + Pb[..., r, 1] * Xb[..., 1]) + Pb[..., r, 2] * Xb[..., 2]) + Pb[..., r, 3]
    return row(0), row(1), row(2)


def _ordered_mean(e, axis):
    """Mean of the non-NaN entries along `axis`, added in ascending index order (sks_reproject's order); (mean, count)."""
    e = np.moveaxis(e, axis, 0)
    s, c = np.zeros(e.shape[1:]), np.zeros(e.shape[1:], dtype=np.int64)
    for x in e:
        ok = ~np.isnan(x)
        s = np.where(ok, s + np.where(ok, x, 0.0), s)
        c = c + ok
    return s, c


def reproject_host(P, X, det, valid):
    """sks_reproject's formulas in float64 numpy: P (V,3,4) or (N,V,3,4), X (N,J,3), det (N,V,J,2) or None, valid (N,V,J) bool or
    None -> dict over FIELDS."""
    P = P[None] if P.ndim == 3 else P
    N, J = X.shape[:2]
    V = P.shape[1]
    with np.errstate(all="ignore"):
        u0, u1, u2 = _project_np(P, X)
        uv = np.stack([u0 / u2, u1 / u2], axis=-1)
        if det is None:
            err = np.full((N, V, J), np.nan)
        else:
            keep = np.isfinite(det).all(axis=-1) & ~np.isnan(X).any(axis=-1)[:, None, :]
            if valid is not None:
                keep &= valid
            dx, dy = uv[..., 0] - det[..., 0], uv[..., 1] - det[..., 1]
            err = np.where(keep, np.sqrt(dx * dx + dy * dy), np.nan)
        sj, cj = _ordered_mean(err, 1)              # (N,J): over the views
        sv, cv = _ordered_mean(err, 2)              # (N,V): over the joints
        S, C = np.zeros(N), np.zeros(N, dtype=np.int64)
        for v in range(V):
            S, C = S + sv[:, v], C + cv[:, v]
        return dict(uv=uv, err=err, in_front=u2 > 0, per_joint=sj / cj, per_view=sv / cv, per_frame=S / C,
                    n_used=cj.astype(np.int32))


def _rho(e, huber):
    return np.where(e <= huber, e * e, 2.0 * huber * e - huber * huber) if huber > 0 else e * e


def refine_host(P, det, valid, X0, huber, max_iters):
    """sks_triangulate_refine's formulas in float64 numpy, every joint at once (the sums over the views are numpy's, not the
    kernel's butterflies): P (V,3,4) or (N,V,3,4), det (N,V,J,2), valid (N,V,J) bool or None, X0 (N,J,3) -> X (N,J,3), cost
    (N,J,2), iters (N,J) int32."""
    P = P[None] if P.ndim == 3 else P
    Pb = P[:, None]                                                  # (N or 1,1,V,3,4)
    x, y = det[..., 0].transpose(0, 2, 1), det[..., 1].transpose(0, 2, 1)      # (N,J,V)
    use = np.isfinite(x) & np.isfinite(y)
    if valid is not None:
        use &= valid.transpose(0, 2, 1)

    def at(X):
        Xb = X[:, :, None]
        row = lambda r: ((Pb[..., r, 0] * Xb[..., 0] + Pb[..., r, 1] * Xb[..., 1]) + Pb[..., r, 2] * Xb[..., 2]) + Pb[..., r, 3]
        u2 = row(2)
        px, py = row(0) / u2, row(1) / u2
        dx, dy = px - x, py - y
        return px, py, u2, dx, dy, np.sqrt(dx * dx + dy * dy)

    vsum = lambda t: np.where(use, t, 0.0).sum(axis=-1)
    with np.errstate(all="ignore"):
        X = X0.astype(np.float64).copy()
        cur = at(X)
        cost = vsum(_rho(cur[5], huber))
        cost0 = cost.copy()
        active = (use.sum(axis=-1) >= 2) & np.isfinite(X).all(axis=-1) & ~(use & ~(cur[2] > 0)).any(axis=-1)
        lam = np.full(cost.shape, LAMBDA0)
        iters = np.zeros(cost.shape, dtype=np.int32)
        for _ in range(max_iters):
            if not active.any():
                break
            px, py, u2, dx, dy, e = cur
            w = np.where(e <= huber, 1.0, huber / e) if huber > 0 else np.ones_like(e)
            Jx = [(Pb[..., 0, k] - px * Pb[..., 2, k]) / u2 for k in range(3)]
            Jy = [(Pb[..., 1, k] - py * Pb[..., 2, k]) / u2 for k in range(3)]
            a = {(r, c): vsum(w * (Jx[r] * Jx[c] + Jy[r] * Jy[c])) for r in range(3) for c in range(r + 1)}
            g = [vsum(w * (Jx[r] * dx + Jy[r] * dy)) for r in range(3)]
            m00, m11, m22 = a[0, 0] + lam * a[0, 0], a[1, 1] + lam * a[1, 1], a[2, 2] + lam * a[2, 2]
            l00 = np.sqrt(m00)
            l10, l20 = a[1, 0] / l00, a[2, 0] / l00
            d1 = m11 - l10 * l10
            l11 = np.sqrt(d1)
            l21 = (a[2, 1] - l20 * l10) / l11
            d2 = (m22 - l20 * l20) - l21 * l21
            l22 = np.sqrt(d2)
            solved = (m00 > 0) & (d1 > 0) & (d2 > 0)
            y0 = -g[0] / l00
            y1 = (-g[1] - l10 * y0) / l11
            y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22
            e2 = y2 / l22
            e1 = (y1 - l21 * e2) / l11
            e0 = ((y0 - l10 * e1) - l20 * e2) / l00
            T = X + np.stack([e0, e1, e2], axis=-1)
            trial = at(T)
            tcost = vsum(np.where(trial[2] > 0, _rho(trial[5], huber), np.inf))
            accept = active & solved & (tcost < cost)
            stop = accept & (cost - tcost < STOP_FRACTION * cost)
            iters += active
            lam = np.where(accept, lam * LAMBDA_DOWN, np.where(active, lam * LAMBDA_UP, lam))
            X = np.where(accept[..., None], T, X)
            cur = tuple(np.where(accept[..., None], t, c) for t, c in zip(trial, cur))
            cost = np.where(accept, tcost, cost)
            active &= ~stop
    return X, np.stack([cost0, cost], axis=-1), iters


def eval_host(err, groups, n_groups):
    """sks_eval_reprojection's means in float64 numpy: err (N,V,J), groups (N) ints or None -> (1 + n_groups, 1 + V + J)."""
    N, V, J = err.shape
    out = np.full((1 + n_groups, 1 + V + J), np.nan)
    with np.errstate(all="ignore"):
        for r in range(1 + n_groups):
            e = err if r == 0 else err[groups == r - 1]
            ok = ~np.isnan(e)
            z = np.where(ok, e, 0.0)
            out[r, 0] = z.sum() / ok.sum()
            out[r, 1:1 + V] = z.sum(axis=(0, 2)) / ok.sum(axis=(0, 2))
            out[r, 1 + V:] = z.sum(axis=(0, 1)) / ok.sum(axis=(0, 1))
    return out


# ------------------------------------------------------------------------------------------------ the public functions
def _launch_reproject(P, X, det, valid, res):
    """One sks_reproject launch on the current stream: P (V,3,4) or (N,V,3,4) float64, X (N,J,3) and det (N,V,J,2) or None float32
    or float64, valid (N,V,J) bool or None, all contiguous on one ROCm device, into the contiguous tensors of `res` (a dict over
    some of FIELDS; in_front as uint8)."""
    from . import _lib
    dev, (N, J), V = X.device, X.shape[:2], P.shape[-3]
    with torch.cuda.device(dev):
        rc = _lib.load().sks_reproject(N, V, J, P.data_ptr(), _pa.rig_stride(P, V), *_pa.pointers(X), *_pa.pointers(det),
                                       _pa.byte_pointer(valid),
                                       *[res[k].data_ptr() if k in res else None for k in FIELDS],
                                       torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "sks_reproject")


def reproject(proj_or_cameras, xyz, poses_2d=None, valid=None, want=FIELDS):
    """Joints into every view, against the views' detections: a Reprojection record with the fields named in `want`.

    `xyz`: (N,J,3) joints -- or (J,3), one frame, and then no result has a frame axis; float32 or float64 are read as they are.
    `proj_or_cameras`: what triangulate_sequence accepts -- a list of V cameras, (V,3,4) projection matrices or (N,V,3,4), one rig
    per frame.  `poses_2d`: (N,V,J,>=2) detections, or None to project only (every err and mean is then NaN).  `valid`: optional
    (N,V,J) bool, False = leave the pair out.

    Float64 throughout: u = P_v [X; 1], uv = (u0 / u2, u1 / u2) with no test for points behind the camera (as the reference),
    in_front = u2 > 0, err = |uv - detection|.  A pair is left out -- err NaN, in no mean -- when valid is False, when its
    detection is not finite or when the joint is NaN.  per_joint: the mean over a joint's kept views (all kept: the reference's
    mean_l2) and n_used their number; per_view: over a view's kept joints; per_frame: over all kept pairs; NaN over nothing.

    Tensors on a ROCm device: one launch of sks_reproject on the current stream, nothing synchronises; a frame's numbers do not
    depend on N, on its place in the batch or on the stream.  Arrays or CPU tensors: the same formulas in numpy."""
    want = tuple(want)
    if not want or any(w not in FIELDS for w in want):
        raise ValueError(f"want: a non-empty selection of {FIELDS}, got {want}")
    X, as_array = _pa.as_tensor(xyz)
    dev = X.device
    single = X.dim() == 2
    X = X[None] if single else X
    if X.dim() != 3 or X.shape[-1] != 3:
        raise ValueError(f"xyz must be (N,J,3) or (J,3), got {tuple(X.shape)}")
    N, J = X.shape[:2]
    P = _pa.projections(proj_or_cameras, dev)
    det = None
    if poses_2d is not None:
        det = _pa.as_tensor(poses_2d)[0].to(dev)
        det = det[None] if single else det
        if det.dim() != 4 or det.shape[-1] < 2 or det.shape[0] != N or det.shape[2] != J:
            raise ValueError(f"poses_2d must be (N,V,J,>=2) with N = {N}, J = {J}, got {tuple(det.shape)}")
    V = det.shape[1] if det is not None else P.shape[-3] if P.dim() in (3, 4) else 0
    _pa.check_shapes(P, N, V, J)
    valid = _pa.check_valid(valid, single, dev, (N, V, J))
    if dev.type == "cuda":
        Xd = _as_real(X)
        dd = None if det is None else _as_real(det[..., :2])
        P = P.contiguous()
        kinds = dict(uv=((N, V, J, 2), torch.float64), err=((N, V, J), torch.float64), in_front=((N, V, J), torch.uint8),
                     per_joint=((N, J), torch.float64), per_view=((N, V), torch.float64), per_frame=((N,), torch.float64),
                     n_used=((N, J), torch.int32))
        res = {k: torch.empty(kinds[k][0], dtype=kinds[k][1], device=dev) for k in want}
        _launch_reproject(P, Xd, dd, valid, res)
        if "in_front" in res:
            res["in_front"] = res["in_front"].view(torch.bool)
    else:
        host = reproject_host(P.numpy(), X.numpy().astype(np.float64), None if det is None else det[..., :2].numpy().astype(np.float64),
                              None if valid is None else valid.numpy())
        res = {k: torch.as_tensor(host[k]) for k in want}
    return Reprojection(**{k: _pa.finish(t, single, as_array) for k, t in res.items()})


def _checked_refinement(huber_px, max_iters):
    huber = 0.0 if huber_px is None else float(huber_px)
    if not (np.isfinite(huber) and huber >= 0):
        raise ValueError(f"huber_px must be finite and >= 0 pixels (None or 0: plain squares), got {huber_px}")
    if int(max_iters) != max_iters or not 1 <= int(max_iters) <= REFINE_MAX_ITERS:
        raise ValueError(f"max_iters = {max_iters}: the refinement takes 1 .. {REFINE_MAX_ITERS} trips (SKS_REFINE_MAX_ITERS)")
    return huber, int(max_iters)


def refine_triangulation(proj_or_cameras, poses_2d, xyz0, valid=None, huber_px=None, max_iters=16, out=None, return_cost=False,
                         return_iters=False):
    """The joints that minimise the reprojection error, from the start `xyz0` (the DLT's, usually): per (frame, joint) the cost
    sum_v rho(e_v) over the kept views, e_v = reproject's err, rho(e) = e * e, or with `huber_px` = d the Huber cost e * e up to
    d and 2 d e - d * d beyond, by damped Gauss-Newton in float64 (the normal equations weighted by min(1, d / e_v), solved by
    Cholesky with lambda x diag added; lambda from 1e-3, x 0.1 when a trial is accepted, x 10 when it is not).  A trial is
    accepted only if its cost is strictly smaller and every kept view sees it in front.  A joint stops after an accepted trip
    that lowered the cost by less than 1e-6 of it, or after `max_iters` (1 .. 16) trips.  The cost never rises.  A joint with
    fewer than two kept views, with a start that is not finite or with a kept view behind which the start lies comes back
    unchanged.

    `poses_2d`, `proj_or_cameras`, `valid`: as triangulate_sequence takes them.  `xyz0`: (N,J,3) float32 or float64 (or (J,3) with
    (V,J,2) detections); the result has its dtype and shape, written into `out` when given -- which may be `xyz0` itself.
    `return_cost=True` appends cost (N,J,2) = {at the start, at the result}, `return_iters=True` iters (N,J) int32, the trips each
    joint took (0: unchanged).

    Tensors on a ROCm device: one launch of sks_triangulate_refine on the current stream (lane = view), nothing synchronises; a
    joint's result does not depend on N, on its place in the batch or on the stream.  Arrays or CPU tensors: the same formulas
    in numpy."""
    huber, max_iters = _checked_refinement(huber_px, max_iters)
    x, as_array = _pa.as_tensor(poses_2d)
    dev = x.device
    single = x.dim() == 3
    x = x[None] if single else x
    if x.dim() != 4 or x.shape[-1] < 2:
        raise ValueError(f"poses_2d must be (N,V,J,>=2) or (V,J,>=2), got {tuple(x.shape)}")
    N, V, J = x.shape[:3]
    P = _pa.projections(proj_or_cameras, dev)
    _pa.check_shapes(P, N, V, J)
    valid = _pa.check_valid(valid, single, dev, (N, V, J))
    X0 = _pa.as_tensor(xyz0)[0].to(dev)
    X0 = X0[None] if single and X0.dim() == 2 else X0
    if tuple(X0.shape) != (N, J, 3):
        raise ValueError(f"xyz0 must be (N,J,3) = {(N, J, 3)}, got {tuple(X0.shape)}")
    X0 = _as_real(X0)
    res = torch.empty_like(X0) if out is None else _pa.check_out(out, (N, J, 3), (X0.dtype,), dev, single)
    cost = torch.empty((N, J, 2), dtype=torch.float64, device=dev) if return_cost else None
    iters = torch.empty((N, J), dtype=torch.int32, device=dev) if return_iters else None
    if dev.type == "cuda":
        from . import _lib
        xd = _as_real(x[..., :2])
        P = P.contiguous()
        with torch.cuda.device(dev):
            rc = _lib.load().sks_triangulate_refine(N, V, J, P.data_ptr(), _pa.rig_stride(P, V), *_pa.pointers(xd),
                                                    _pa.byte_pointer(valid), *_pa.pointers(X0), huber, max_iters,
                                                    *_pa.pointers(res), None if cost is None else cost.data_ptr(),
                                                    None if iters is None else iters.data_ptr(),
                                                    torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "sks_triangulate_refine")
    else:
        Xn, cn, it = refine_host(P.numpy(), x[..., :2].numpy().astype(np.float64), None if valid is None else valid.numpy(),
                                 X0.numpy().astype(np.float64), huber, max_iters)
        # (an unchanged joint keeps its start's bits in the start's dtype: float32 -> float64 -> float32 is exact)
        res.copy_(torch.as_tensor(Xn).to(res.dtype))
        if cost is not None:
            cost.copy_(torch.as_tensor(cn))
        if iters is not None:
            iters.copy_(torch.as_tensor(it))
    return _pa.results(res, out, single, as_array, [t for t in (cost, iters) if t is not None])


def evaluate_sequence_reprojection(err, groups=None, n_groups=None):
    """The means of a sequence's reprojection errors `err` (N,V,J; NaN = left out, as reproject writes it), overall and per group
    (an activity, a camera rig): a float64 (1 + n_groups, 1 + V + J) table -- row 0 over all frames, row 1 + g over the frames with
    groups[i] == g; a row holds the overall mean, then the V per-view and the J per-joint means over the entries that are not
    NaN, NaN where there are none.  `groups`: optional (N) ints (ids outside 0 .. n_groups - 1 enter row 0 only); `n_groups`
    defaults to max(groups) + 1, which reads the ids back -- give it to stay on the device.  A tensor on a ROCm device: one launch
    of sks_eval_reprojection on the current stream; an array or a CPU tensor: numpy."""
    e, as_array = _pa.as_tensor(err)
    if e.dim() != 3 or e.shape[0] < 1 or e.shape[2] < 1 or not 1 <= e.shape[1] <= MAX_VIEWS:
        raise ValueError(f"err must be (N,V,J) with 1 .. {MAX_VIEWS} views, got {tuple(e.shape)}")
    N, V, J = e.shape
    dev = e.device
    if groups is None:
        if n_groups:
            raise ValueError(f"n_groups = {n_groups} without groups")
        n_groups, g = 0, None
    else:
        g = _pa.as_tensor(groups)[0].to(device=dev, dtype=torch.int32).contiguous()
        if tuple(g.shape) != (N,):
            raise ValueError(f"groups must be (N,) = {(N,)}, got {tuple(g.shape)}")
        if n_groups is None:
            n_groups = int(g.max()) + 1
    if not 0 <= n_groups <= 64:
        raise ValueError(f"n_groups = {n_groups}: 0 .. 64 (SKS_EVAL_MAX_GROUPS)")
    if dev.type == "cuda":
        from . import _lib
        e = e.to(torch.float64).contiguous()
        out = torch.empty((1 + n_groups, 1 + V + J), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.load().sks_eval_reprojection(N, V, J, e.data_ptr(), None if g is None else g.data_ptr(), n_groups,
                                                   out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "sks_eval_reprojection")
    else:
        out = torch.as_tensor(eval_host(e.numpy().astype(np.float64), None if g is None else g.numpy(), n_groups))
    return out.numpy() if as_array else out


class SequenceReprojection:
    """The reprojection errors of one optimize_sequence call (FrameBatchLoop / FramePipeline after set_reprojection_report), all on
    the device, in the manner of report.SequenceReport: every batch's rows are written by one sks_reproject launch behind its
    new_scenes (the initial joints) and one behind its last step (the final joints), on the batch's own stream, against the
    batch's detections; nothing is read back.
      initial_err, final_err   (N,V,J) float64 pixels, NaN where a detection is not finite or a joint is NaN
      final_uv                 (N,V,J,2) the final joints in every view
      per_joint, per_frame     (N,J), (N) means of final_err over a joint's views / over all of a frame's pairs
    Final once the stream(s) of the sequence have been waited for, as the joints optimize_sequence returns."""

    def __init__(self, N, V, J, device):
        new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=device)
        self.initial_err, self.final_err, self.final_uv = new(N, V, J), new(N, V, J), new(N, V, J, 2)
        self.per_joint, self.per_frame = new(N, J), new(N)
        self._det = {}          # batch start -> its detections on the device, from begin to take

    def _rows(self, loop, n):
        P = loop._proj
        return (P[:n] if P.dim() == 4 else P).contiguous(), loop.xyz[:n]

    def begin(self, loop, b, n, poses_2d):
        """Batch b (n frames) has its initial joints in loop.xyz: their errors, on the current stream."""
        det = _as_real(poses_2d[:n].to(loop.device)[..., :2])
        self._det[b] = det
        P, X = self._rows(loop, n)
        _launch_reproject(P, X, det, None, dict(err=self.initial_err[b:b + n]))

    def take(self, loop, b, n):
        """Batch b is done: the errors of its final joints, on the current stream."""
        det = self._det.pop(b)
        P, X = self._rows(loop, n)
        _launch_reproject(P, X, det, None, dict(uv=self.final_uv[b:b + n], err=self.final_err[b:b + n],
                                                per_joint=self.per_joint[b:b + n], per_frame=self.per_frame[b:b + n]))

    def summary(self, groups=None, n_groups=None):
        """{"initial", "final"}: evaluate_sequence_reprojection's (1 + n_groups, 1 + V + J) table of each -- the overall mean, the
        per-view and the per-joint means, for all frames and per group -- by one sks_eval_reprojection launch each on the current
        stream."""
        return {name: evaluate_sequence_reprojection(err, groups, n_groups)
                for name, err in (("initial", self.initial_err), ("final", self.final_err))}
