"""Covariance-weighted temporal smoothing of a sequence of poses (csrc/sks_smooth.hip), and the smoothness figures that go with it.

smooth_sequence   per (frame, joint) a local polynomial fit over the frames around it, every tap weighted by the inverse of its own
                  3x3 covariance (uncertainty.joint_uncertainty's cov6, e.g. pipe.gaussians.uncertainty().cov6): the smoothed
                  joints, their velocity, the fit's own covariance and the number of taps used.  Joints that are NaN (DESIGN.md
                  "Unobserved joints") or masked out are filled from the frames around them.
smooth_host       the same fit in float64 numpy, for arrays and CPU tensors.
sequence_accel    "Accel" and "Accel error" of the video-pose literature, overall, per joint and per group.

The fit is defined once, in include/skelsplat_hip.h above sks_smooth_sequence, with the order of every sum; the kernel and
smooth_host both follow it.  Tensors on a ROCm device: one launch on the current stream, nothing is read back.  What the
covariance weights gain on real sequences depends on how well the optimised covariances are calibrated (uncertainty.calibration
measures that); that gain has not been measured on real data."""
import collections

import numpy as np
import torch

from . import _lib

Smoothed = collections.namedtuple("Smoothed", "joints velocity cov6 n_used")
TAPERS = {"box": _lib.SKS_SMOOTH_BOX, "tricube": _lib.SKS_SMOOTH_TRICUBE}
WANT = ("joints", "velocity", "cov6", "n_used")
_SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))       # entry (r, c) of xx, xy, xz, yy, yz, zz


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _settings(what, half_window, degree, taper, cov_floor, want=WANT):
    h, d, floor = int(half_window), int(degree), float(cov_floor)
    if not 1 <= h <= _lib.SKS_SMOOTH_MAX_HALF_WINDOW:
        raise ValueError(f"{what}: half_window = {half_window}, 1 .. {_lib.SKS_SMOOTH_MAX_HALF_WINDOW} frames on each side")
    if not 0 <= d <= 2:
        raise ValueError(f"{what}: degree = {degree}, 0 .. 2")
    if taper not in TAPERS:
        raise ValueError(f"{what}: taper = {taper!r}, one of {sorted(TAPERS)}")
    if not (floor >= 0.0) or floor == float("inf"):
        raise ValueError(f"{what}: cov_floor = {cov_floor!r} must be finite and >= 0 (mm^2)")
    want = tuple(want)
    if "joints" not in want or any(w not in WANT for w in want):
        raise ValueError(f"{what}: want = {want!r}: 'joints' and any of {WANT[1:]}")
    return h, d, floor, want


def _device_block(t, name, shape, dtype, what, dev):
    """`t` as a contiguous tensor of `shape` on `dev`: floats must be float32 already, masks and ids are converted."""
    if not torch.is_tensor(t) or t.device != dev:
        raise ValueError(f"{what}: `{name}` must be a tensor on {dev} like the joints")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: `{name}` must be {tuple(shape)}, got {tuple(t.shape)}")
    if dtype == torch.float32 and t.dtype != torch.float32:
        raise ValueError(f"{what}: `{name}` must be float32, got {t.dtype}")
    if dtype == torch.int32 and (t.is_floating_point() or t.dtype == torch.bool):
        raise ValueError(f"{what}: `{name}` must hold integers, got {t.dtype}")
    return t.to(dtype).contiguous()


def _joints(xyz, what):
    if not torch.is_tensor(xyz) or not xyz.is_cuda:
        raise ValueError(f"{what}: `xyz` must be a tensor on a ROCm device")
    if xyz.dtype != torch.float32:
        raise ValueError(f"{what}: `xyz` must be float32, got {xyz.dtype}")
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or xyz.numel() == 0:
        raise ValueError(f"{what}: `xyz` must be (N,J,3), got {tuple(xyz.shape)}")
    if xyz.shape[1] > _lib.SKS_SMOOTH_MAX_JOINTS and what == "smooth_sequence":
        raise ValueError(f"{what}: {xyz.shape[1]} joints, at most {_lib.SKS_SMOOTH_MAX_JOINTS} (SKS_SMOOTH_MAX_JOINTS)")
    return xyz.contiguous()


def smooth_sequence(xyz, cov6=None, weights=None, valid=None, groups=None, half_window=8, degree=2, taper="tricube",
                    cov_floor=0.0, want=WANT):
    """xyz (N,J,3) float32 -> Smoothed(joints (N,J,3), velocity (N,J,3) mm per frame, cov6 (N,J,6), n_used (N,J) int32); the
    outputs not named in `want` are None.  Optional, all on the joints' device: cov6 (N,J,6) float32, every tap's covariance
    (xx, xy, xz, yy, yz, zz: joint_uncertainty's), whose inverse weights the tap; weights (N,J) float32; valid (N,J) bool, the
    taps to keep; groups (N,) integers: a window never crosses from one recording into the next.  half_window 1 .. 32 frames on
    each side, degree 0 .. 2, taper "box" or "tricube", cov_floor >= 0 mm^2 added to the covariances' diagonals.
    A tap that is NaN, masked out, of weight <= 0 or whose covariance is not positive definite is left out; a target with no tap
    left is NaN with n_used 0, and one whose own row is missing is filled from its neighbours (the definition:
    include/skelsplat_hip.h).  Device tensors: one launch (sks_smooth_sequence) on the current stream, nothing read back.
    Arrays and CPU tensors: smooth_host, float64 numpy, the same named tuple of arrays."""
    what = "smooth_sequence"
    if not (torch.is_tensor(xyz) and xyz.is_cuda):
        np_of = lambda a: None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))
        return smooth_host(np_of(xyz), np_of(cov6), np_of(weights), np_of(valid), np_of(groups), half_window, degree, taper,
                           cov_floor, want)
    h, d, floor, want = _settings(what, half_window, degree, taper, cov_floor, want)
    x = _joints(xyz, what)
    N, J = x.shape[:2]
    dev = x.device
    opt = lambda t, name, shape, dtype: None if t is None else _device_block(t, name, shape, dtype, what, dev)
    c = opt(cov6, "cov6", (N, J, 6), torch.float32)
    w = opt(weights, "weights", (N, J), torch.float32)
    v = opt(valid, "valid", (N, J), torch.bool)
    g = opt(groups, "groups", (N,), torch.int32)
    new = lambda name, tail, dtype: torch.empty((N, J) + tail, dtype=dtype, device=dev) if name in want else None
    out = Smoothed(new("joints", (3,), torch.float32), new("velocity", (3,), torch.float32), new("cov6", (6,), torch.float32),
                   new("n_used", (), torch.int32))
    p = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = _lib.load().sks_smooth_sequence(N, J, x.data_ptr(), p(c), p(w), None if v is None else v.view(torch.uint8).data_ptr(),
                                             p(g), h, d, TAPERS[taper], floor, out.joints.data_ptr(), p(out.velocity), p(out.cov6),
                                             p(out.n_used), _stream(dev))
    _lib.check(rc, "sks_smooth_sequence")
    return out


def _ldl3(xx, xy, xz, yy, yz, zz):
    d0 = xx
    l10 = xy / d0
    l20 = xz / d0
    d1 = yy - l10 * xy
    e = yz - l20 * xy
    z1 = zz - l20 * xz
    l21 = e / d1
    d2 = z1 - l21 * e
    return d0, d1, d2, l10, l20, l21


def _inverse3(d0, d1, d2, l10, l20, l21):
    """(L D L^T)^-1 as (..,6): the header's formula."""
    i0, i1, i2 = 1.0 / d0, 1.0 / d1, 1.0 / d2
    m = l21 * l10 - l20
    return np.stack([(i0 + (l10 * l10) * i1) + (m * m) * i2, -(l10 * i1) - (m * l21) * i2, m * i2,
                     i1 + (l21 * l21) * i2, -(l21 * i2), i2], axis=-1)


def _solve(Mo, R, de):
    """The normal equations of effective degree `de` for a batch of targets: Mo (2d+1,K,6), R (d+1,K,3) -> c0 (K,3), c1 (K,3),
    cov6 (K,6); unknowns ordered c_de .. c_0, LDL^T in the header's loop order."""
    K, m = Mo.shape[1], 3 * (de + 1)
    B = np.zeros((m, m, K))
    y = np.zeros((m, K))
    for a in range(de + 1):
        for r in range(3):
            y[3 * a + r] = R[de - a][:, r]
            for b in range(a + 1):
                for c in range(3):
                    if 3 * b + c <= 3 * a + r:
                        B[3 * a + r, 3 * b + c] = Mo[(de - a) + (de - b)][:, _SYM[r][c]]
    for j in range(m):
        col = {i: B[i, j] / B[j, j] for i in range(j + 1, m)}
        for i in range(j + 1, m):
            for c in range(j + 1, i + 1):
                B[i, c] = B[i, c] - col[i] * B[c, j]
        for i in range(j + 1, m):
            B[i, j] = col[i]
            y[i] = y[i] - col[i] * y[j]
    for j in range(m):
        y[j] = y[j] / B[j, j]
    for j in range(m - 1, 0, -1):
        for i in range(j):
            y[i] = y[i] - B[j, i] * y[j]
    c0 = np.stack([y[m - 3], y[m - 2], y[m - 1]], axis=-1)
    c1 = np.stack([y[m - 6], y[m - 5], y[m - 4]], axis=-1) if de >= 1 else np.zeros((K, 3))
    cov = _inverse3(B[m - 3, m - 3], B[m - 2, m - 2], B[m - 1, m - 1], B[m - 2, m - 3], B[m - 1, m - 3], B[m - 1, m - 2])
    return c0, c1, cov


def smooth_host(xyz, cov6=None, weights=None, valid=None, groups=None, half_window=8, degree=2, taper="tricube", cov_floor=0.0,
                want=WANT):
    """smooth_sequence's fit in float64 numpy, vectorised over the (N,J) targets and stepping through the tap offsets
    t = -h .. h, which is every target's ascending tap order.  Arrays in (xyz and cov6 are taken as float32, what the kernel
    reads), Smoothed of arrays out: float32 joints, velocity and cov6, int32 n_used."""
    what = "smooth_host"
    h, d, floor, want = _settings(what, half_window, degree, taper, cov_floor, want)
    X = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    if X.ndim != 3 or X.shape[-1] != 3 or X.size == 0:
        raise ValueError(f"{what}: `xyz` must be (N,J,3), got {X.shape}")
    N, J = X.shape[:2]

    def given(a, name, shape, dtype):
        a = np.asarray(a)
        if a.shape != shape:
            raise ValueError(f"{what}: `{name}` must be {shape}, got {a.shape}")
        return a.astype(dtype)

    usable = np.isfinite(X).all(-1)
    W = np.ones((N, J))
    if valid is not None:
        usable &= given(valid, "valid", (N, J), bool)
    if weights is not None:
        W = given(weights, "weights", (N, J), np.float32).astype(np.float64)
        usable &= np.isfinite(W) & (W > 0)
    gid = np.zeros(N, dtype=np.int64) if groups is None else given(groups, "groups", (N,), np.int64)
    Lam = np.zeros((N, J, 6))
    Lam[..., [0, 3, 5]] = 1.0
    with np.errstate(all="ignore"):
        if cov6 is not None:
            C = given(cov6, "cov6", (N, J, 6), np.float32).astype(np.float64)
            f = _ldl3(C[..., 0] + floor, C[..., 1], C[..., 2], C[..., 3] + floor, C[..., 4], C[..., 5] + floor)
            usable &= np.all([np.isfinite(p) & (p > 0) for p in f[:3]], axis=0)
            Lam = _inverse3(*f)
        Mo = np.zeros((2 * d + 1, N, J, 6))
        R = np.zeros((d + 1, N, J, 3))
        x0 = np.zeros((N, J, 3))
        n = np.zeros((N, J), dtype=np.int32)
        frames = np.arange(N)
        for t in range(-h, h + 1):
            k = frames + t
            kc = np.clip(k, 0, N - 1)
            use = (((k >= 0) & (k < N) & (gid[kc] == gid))[:, None] & usable[kc])
            xk = X[kc]
            x0 = np.where((use & (n == 0))[..., None], xk, x0)
            n = n + use
            tap = 1.0
            if taper == "tricube":
                u = abs(float(t)) / float(h + 1)
                q = 1.0 - (u * u) * u
                tap = (q * q) * q
            wl = (W[kc] * tap)[..., None] * Lam[kc]
            dx = xk - x0
            v = np.stack([(wl[..., s[0]] * dx[..., 0] + wl[..., s[1]] * dx[..., 1]) + wl[..., s[2]] * dx[..., 2] for s in _SYM], axis=-1)
            t1 = float(t)
            tp = (1.0, t1, t1 * t1, (t1 * t1) * t1, (t1 * t1) * (t1 * t1))
            for p in range(2 * d + 1):
                Mo[p] = np.where(use[..., None], Mo[p] + tp[p] * wl, Mo[p])
            for a in range(d + 1):
                R[a] = np.where(use[..., None], R[a] + tp[a] * v, R[a])
        joints = np.full((N, J, 3), np.nan)
        vel = np.full((N, J, 3), np.nan)
        cov = np.full((N, J, 6), np.nan)
        deff = np.minimum(d, n - 1)
        for de in range(d + 1):
            at = (n > 0) & (deff == de)
            if at.any():
                c0, c1, cv = _solve(Mo[:, at], R[:, at], de)
                joints[at], vel[at], cov[at] = c0 + x0[at], c1, cv
        f32 = lambda name, a: a.astype(np.float32) if name in want else None
        return Smoothed(f32("joints", joints), f32("velocity", vel), f32("cov6", cov), n if "n_used" in want else None)


def accel_host(xyz, gt=None, groups=None, n_groups=0):
    """sks_eval_accel's table in float64 numpy: (1 + n_groups, 2, 1 + J); [.,0,.] the mean norm of x[f-1] - 2 x[f] + x[f+1],
    [.,1,.] the mean norm of its difference from the ground truth's (NaN without gt); column 0 all joints, 1 + j joint j; row 0
    all frames, 1 + g group g.  An entry needs its three positions finite and its three frames in one group."""
    X = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    N, J = X.shape[:2]
    G = int(n_groups)
    out = np.full((1 + G, 2, 1 + J), np.nan)
    if N < 3:
        return out
    gid = np.zeros(N, dtype=np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    with np.errstate(all="ignore"):
        second = lambda A: (A[:-2] - 2.0 * A[1:-1]) + A[2:]
        a = second(X)
        norm = lambda A: np.sqrt((A[..., 0] * A[..., 0] + A[..., 1] * A[..., 1]) + A[..., 2] * A[..., 2])
        figures = [norm(a)]
        if gt is not None:
            ag = second(np.asarray(gt, dtype=np.float32).astype(np.float64))
            figures.append(np.where(np.isfinite(norm(ag)), norm(a - ag), np.nan))
        fenced = (gid[:-2] == gid[1:-1]) & (gid[2:] == gid[1:-1])
        for row in range(1 + G):
            keep = fenced if row == 0 else fenced & (gid[1:-1] == row - 1)
            for k, fig in enumerate(figures):
                e = np.where(keep[:, None] & np.isfinite(figures[0]) & np.isfinite(fig), fig, np.nan)
                cnt = np.isfinite(e).sum(0)
                out[row, k, 1:] = np.nansum(e, 0) / cnt
                out[row, k, 0] = np.nansum(e) / cnt.sum()
    return out


def sequence_accel(xyz, gt=None, groups=None, n_groups=None):
    """"Accel" (the mean norm of the joints' second difference x[f-1] - 2 x[f] + x[f+1], mm per frame^2) and, with `gt`, "Accel
    error" (the mean norm of its difference from the ground truth's) of xyz (N,J,3) float32 -> dict of float64 figures:
      accel, accel_error                  overall (0-d);
      accel_joints, accel_error_joints    (J,) per joint;
      accel_groups, accel_error_groups    (n_groups,) per group, with `groups` (N,) integers and n_groups (at most 64);
      table                               (1 + n_groups, 2, 1 + J): everything, per group and joint (sks_eval_accel's layout).
    An entry needs its three positions (and the ground truth's, for the error) finite and its three frames in the same group
    (`groups` fence the frames even with n_groups left out); a figure over nothing is NaN, and the error figures are NaN without
    `gt`.  Device tensors: one launch (sks_eval_accel) on the current stream, device tensors out; arrays and CPU tensors:
    accel_host."""
    what = "sequence_accel"
    G = 0 if n_groups is None else int(n_groups)
    if not 0 <= G <= _lib.SKS_EVAL_MAX_GROUPS:
        raise ValueError(f"{what}: n_groups = {n_groups}, 0 .. {_lib.SKS_EVAL_MAX_GROUPS} (SKS_EVAL_MAX_GROUPS)")
    if G > 0 and groups is None:
        raise ValueError(f"{what}: n_groups = {G} without groups")
    if torch.is_tensor(xyz) and xyz.is_cuda:
        x = _joints(xyz, what)
        N, J = x.shape[:2]
        dev = x.device
        y = None if gt is None else _device_block(gt, "gt", (N, J, 3), torch.float32, what, dev)
        g = None if groups is None else _device_block(groups, "groups", (N,), torch.int32, what, dev)
        table = torch.empty((1 + G, 2, 1 + J), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.load().sks_eval_accel(N, J, x.data_ptr(), None if y is None else y.data_ptr(),
                                            None if g is None else g.data_ptr(), G, table.data_ptr(), _stream(dev))
        _lib.check(rc, "sks_eval_accel")
    else:
        np_of = lambda a: None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))
        X = np_of(xyz)
        if X.ndim != 3 or X.shape[-1] != 3 or X.size == 0:
            raise ValueError(f"{what}: `xyz` must be (N,J,3), got {X.shape}")
        for name, a, shape in (("gt", np_of(gt), X.shape), ("groups", np_of(groups), X.shape[:1])):
            if a is not None and a.shape != shape:
                raise ValueError(f"{what}: `{name}` must be {shape}, got {a.shape}")
        table = accel_host(X, np_of(gt), np_of(groups), G)
    return dict(accel=table[0, 0, 0], accel_joints=table[0, 0, 1:], accel_groups=table[1:, 0, 0],
                accel_error=table[0, 1, 0], accel_error_joints=table[0, 1, 1:], accel_error_groups=table[1:, 1, 0], table=table)
