"""Constant limb lengths over a sequence of poses (csrc/sks_bones.hip): the subject of one recording is a skeleton whose bones
have one length in every frame.

bone_lengths        every bone's length in every frame, and per recording (`groups`) the lower median of those lengths, their
                    median absolute deviation and the number of frames used -- the MAD relative to the median is a figure of a
                    sequence that needs no ground truth, next to the reprojection error.
symmetrize          left/right pairs of bones set to their common mean.
project_to_lengths  every frame moved onto given lengths, each joint's 3x3 covariance (uncertainty.joint_uncertainty's cov6, or
                    smoothing's) deciding which end of a wrong bone moves and in which direction.
*_host              the same in float64 numpy, for arrays and CPU tensors.

The three definitions stand once, in include/skelsplat_hip.h above sks_bone_measure, with the order of every sum; the kernels and
the host functions both follow them.  What the fit is: a pose that meets the lengths, reached by successive Sigma-closest
projections onto the linearised constraints -- NOT the Sigma-closest feasible pose, and without a covariance of its own (DESIGN.md
"Constant limb lengths").  Tensors on a ROCm device: one launch per step on the current stream, nothing is read back.  `bones` are
HOST integers (a list, an array or a CPU tensor of (parent, child) pairs, e.g. scene.DATASETS[name]["bones"]): the forest check
and the kernels' argument block need them there.  What the constraint gains on real sequences has not been measured."""
import collections

import numpy as np
import torch

from . import _lib
from .smoothing import _device_block, _stream

BoneLengths = collections.namedtuple("BoneLengths", "length mad n_used measured")
Projected = collections.namedtuple("Projected", "joints residual n_trips n_active")
_SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))       # entry (r, c) of xx, xy, xz, yy, yz, zz


def checked_bones(bones, J, what="bones"):
    """`bones` -> a contiguous (B,2) int32 array of (parent, child) pairs over joints 0 .. J-1 that form a forest, or ValueError:
    the check sks_bone_measure / sks_bone_project make on the host, with the same union-find over the bones in index order."""
    if torch.is_tensor(bones):
        if bones.is_floating_point() or bones.dtype == torch.bool:
            raise ValueError(f"{what}: `bones` must hold integers, got {bones.dtype}")
        bones = bones.detach().cpu().numpy()
    b = np.asarray(bones)
    if b.ndim != 2 or b.shape[1] != 2 or b.shape[0] < 1 or b.dtype.kind not in "iu":
        raise ValueError(f"{what}: `bones` must be (B,2) integers (parent, child), B >= 1, got {b.shape} {b.dtype}")
    if not 2 <= J <= _lib.SKS_BONES_MAX_JOINTS:
        raise ValueError(f"{what}: {J} joints, 2 .. {_lib.SKS_BONES_MAX_JOINTS} (SKS_BONES_MAX_JOINTS)")
    if b.shape[0] > _lib.SKS_BONES_MAX_JOINTS - 1:
        raise ValueError(f"{what}: {b.shape[0]} bones, at most {_lib.SKS_BONES_MAX_JOINTS - 1}")
    if b.min() < 0 or b.max() >= J:
        raise ValueError(f"{what}: `bones` names a joint outside 0 .. {J - 1}")
    root = list(range(J))

    def find(j):
        while root[j] != j:
            j = root[j]
        return j
    for i, (p, c) in enumerate(b.tolist()):
        rp, rc = find(p), find(c)
        if rp == rc:
            raise ValueError(f"{what}: bone {i} = ({p}, {c}) closes a cycle: the bones must form a forest")
        root[rc] = rp
    return np.ascontiguousarray(b, dtype=np.int32)


def _joints(xyz, what):
    if xyz.dtype != torch.float32:
        raise ValueError(f"{what}: `xyz` must be float32, got {xyz.dtype}")
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or xyz.numel() == 0:
        raise ValueError(f"{what}: `xyz` must be (N,J,3), got {tuple(xyz.shape)}")
    return xyz.contiguous()


def _np_of(a):
    return None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))


def _on_device(*tensors):
    return any(torch.is_tensor(t) and t.is_cuda for t in tensors)


def _n_groups(groups, n_groups, what):
    """The number of recordings: `n_groups` as given, 1 without groups, else the largest id + 1 (a device tensor: ONE number is
    read back, which waits for the stream -- pass n_groups to avoid it)."""
    if n_groups is None:
        if groups is None:
            return 1
        g = groups if torch.is_tensor(groups) else np.asarray(groups)
        n_groups = int(g.max()) + 1
    G = int(n_groups)
    if not 1 <= G <= _lib.SKS_BONES_MAX_GROUPS:
        raise ValueError(f"{what}: {n_groups} groups, 1 .. {_lib.SKS_BONES_MAX_GROUPS} (SKS_BONES_MAX_GROUPS)")
    if groups is None and G != 1:
        raise ValueError(f"{what}: n_groups = {G} without groups")
    return G


def _max_sigma(max_sigma_mm, cov6, what):
    if max_sigma_mm is None:
        return None
    if cov6 is None:
        raise ValueError(f"{what}: max_sigma_mm gates a frame by the variance of its length, which needs cov6")
    s = float(max_sigma_mm)
    if not (s >= 0.0) or s == float("inf"):
        raise ValueError(f"{what}: max_sigma_mm = {max_sigma_mm!r} must be finite and >= 0")
    return s


def _projection_settings(cov_floor, max_iters, tol_mm, what):
    floor, it, tol = float(cov_floor), int(max_iters), float(tol_mm)
    if not (floor >= 0.0) or floor == float("inf"):
        raise ValueError(f"{what}: cov_floor = {cov_floor!r} must be finite and >= 0 (mm^2)")
    if not 1 <= it <= _lib.SKS_BONES_MAX_ITERS:
        raise ValueError(f"{what}: max_iters = {max_iters}, 1 .. {_lib.SKS_BONES_MAX_ITERS} (SKS_BONES_MAX_ITERS)")
    if not (tol >= 0.0) or tol == float("inf"):
        raise ValueError(f"{what}: tol_mm = {tol_mm!r} must be finite and >= 0")
    return floor, it, tol


def bone_lengths(xyz, bones, cov6=None, valid=None, groups=None, max_sigma_mm=None, n_groups=None):
    """xyz (N,J,3) float32, bones (B,2) host integers -> BoneLengths(length (G,B) float32: per recording the lower median of every
    bone's length over the frames; mad (G,B) float32: the lower median of |l - length|; n_used (G,B) int32: the frames that
    entered; measured (N,B) float32: every frame's lengths, NaN where an end is NaN, masked out by valid (N,J) bool or, with
    cov6 (N,J,6) float32 and max_sigma_mm, where the standard deviation of the length along the bone exceeds max_sigma_mm).
    groups (N,) integers in 0 .. G-1: the recording of every frame (None: one); G = n_groups or, when that is None, the largest id
    + 1, read back from a device tensor.  A recording without a usable frame has NaN, NaN, 0.  Medians are selected, not
    averaged: each is one of the measures, exactly.  Device tensors: two launches (sks_bone_measure, sks_bone_lengths) on the
    current stream; arrays and CPU tensors: bone_lengths_host, the same named tuple of arrays."""
    what = "bone_lengths"
    if not _on_device(xyz):
        return bone_lengths_host(_np_of(xyz), bones, _np_of(cov6), _np_of(valid), _np_of(groups), max_sigma_mm, n_groups)
    x = _joints(xyz, what)
    N, J = x.shape[:2]
    bn = checked_bones(bones, J, what)
    B = bn.shape[0]
    sigma = _max_sigma(max_sigma_mm, cov6, what)
    G = _n_groups(groups, n_groups, what)
    dev = x.device
    opt = lambda t, name, shape, dtype: None if t is None else _device_block(t, name, shape, dtype, what, dev)
    c = opt(cov6, "cov6", (N, J, 6), torch.float32) if sigma is not None else None
    v = opt(valid, "valid", (N, J), torch.bool)
    g = opt(groups, "groups", (N,), torch.int32)
    out = BoneLengths(torch.empty((G, B), dtype=torch.float32, device=dev), torch.empty((G, B), dtype=torch.float32, device=dev),
                      torch.empty((G, B), dtype=torch.int32, device=dev), torch.empty((N, B), dtype=torch.float32, device=dev))
    p = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        lib, st = _lib.load(), _stream(dev)
        rc = lib.sks_bone_measure(N, J, B, bn.ctypes.data, x.data_ptr(), p(c), None if v is None else v.view(torch.uint8).data_ptr(),
                                  0.0 if sigma is None else sigma, out.measured.data_ptr(), st)
        _lib.check(rc, "sks_bone_measure")
        rc = lib.sks_bone_lengths(N, B, out.measured.data_ptr(), p(g), G, out.length.data_ptr(), out.mad.data_ptr(),
                                  out.n_used.data_ptr(), st)
        _lib.check(rc, "sks_bone_lengths")
    return out


def symmetrize(lengths, pairs):
    """lengths (G,B) (or (B,)) with both bones of every (left, right) pair of bone indices set to the float32 mean of the two;
    a new tensor or array, plain indexing where `lengths` lives."""
    pairs = [(int(a), int(b)) for a, b in pairs]
    out = lengths.clone() if torch.is_tensor(lengths) else np.array(lengths, dtype=np.float32)
    for a, b in pairs:
        mean = (out[..., a] + out[..., b]) * 0.5
        out[..., a] = mean
        out[..., b] = mean
    return out


def bone_index(bones, pairs):
    """The indices in `bones` of the bones (parent, child) named by `pairs` of joints, e.g. a dataset's `limbs`."""
    where = {tuple(b): i for i, b in enumerate(np.asarray(bones).tolist())}
    return [where[(int(p), int(c))] for p, c in pairs]


def project_to_lengths(xyz, bones, lengths, cov6=None, valid=None, groups=None, cov_floor=0.0, max_iters=16, tol_mm=1e-3):
    """xyz (N,J,3) float32, bones (B,2) host integers, lengths (G,B) (or (B,)) float32 -> Projected(joints (N,J,3) float32: every
    frame moved until each of its bones has the length of the frame's recording; residual (N,) float32: the largest |length -
    target| left, mm; n_trips (N,) int32: the projections taken, at most max_iters (1 .. 16); n_active (N,) int32: the bones
    that were constrained).  A trip is x <- x - Sigma A^T (A Sigma A^T)^-1 (n(x) - L) with Sigma the joints' covariances
    cov6 (N,J,6) float32 plus cov_floor mm^2 on the diagonals (None: the identity, both ends of a wrong bone move alike), and a
    frame stops when residual <= tol_mm; one that still has residual > tol_mm did not converge.  A bone is left out of a frame
    (inactive) when an end is NaN or masked out by valid (N,J) bool, its target is NaN or <= 0, its ends coincide or an end's
    covariance is not finite and positive definite; a joint that only inactive bones touch comes back with every bit of its
    input, NaN included, and a frame without an active bone is a copy with residual NaN.  groups (N,) integers: the row of
    `lengths` of every frame.  This reaches A pose on the lengths by successive Sigma-closest projections, not the Sigma-closest
    one (the definition: include/skelsplat_hip.h).  Device tensors: one launch (sks_bone_project, one wavefront per frame) on the
    current stream; arrays and CPU tensors: project_host."""
    what = "project_to_lengths"
    if not _on_device(xyz):
        return project_host(_np_of(xyz), bones, _np_of(lengths), _np_of(cov6), _np_of(valid), _np_of(groups), cov_floor, max_iters,
                            tol_mm)
    floor, iters, tol = _projection_settings(cov_floor, max_iters, tol_mm, what)
    x = _joints(xyz, what)
    N, J = x.shape[:2]
    bn = checked_bones(bones, J, what)
    B = bn.shape[0]
    dev = x.device
    if not torch.is_tensor(lengths) or lengths.device != dev or lengths.dtype != torch.float32:
        raise ValueError(f"{what}: `lengths` must be a float32 tensor on {dev} like the joints")
    L = lengths[None] if lengths.dim() == 1 else lengths
    if L.dim() != 2 or L.shape[1] != B or not 1 <= L.shape[0] <= _lib.SKS_BONES_MAX_GROUPS:
        raise ValueError(f"{what}: `lengths` must be (G,{B}) with G 1 .. {_lib.SKS_BONES_MAX_GROUPS}, got {tuple(lengths.shape)}")
    G = L.shape[0]
    if groups is None and G != 1:
        raise ValueError(f"{what}: {G} rows of lengths without groups")
    L = L.contiguous()
    opt = lambda t, name, shape, dtype: None if t is None else _device_block(t, name, shape, dtype, what, dev)
    c = opt(cov6, "cov6", (N, J, 6), torch.float32)
    v = opt(valid, "valid", (N, J), torch.bool)
    g = opt(groups, "groups", (N,), torch.int32)
    out = Projected(torch.empty_like(x), torch.empty((N,), dtype=torch.float32, device=dev),
                    torch.empty((N,), dtype=torch.int32, device=dev), torch.empty((N,), dtype=torch.int32, device=dev))
    p = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = _lib.load().sks_bone_project(N, J, B, bn.ctypes.data, x.data_ptr(), p(c), None if v is None else v.view(torch.uint8).data_ptr(),
                                          p(g), G, L.data_ptr(), floor, iters, tol, out.joints.data_ptr(), out.residual.data_ptr(),
                                          out.n_trips.data_ptr(), out.n_active.data_ptr(), _stream(dev))
    _lib.check(rc, "sks_bone_project")
    return out


# ------------------------------------------------------------------------------------------------ float64 numpy, vectorised over frames
def _quad(a, S, b):
    """a^T S b for batches: a, b (K,3), S (K,6); the header's order."""
    w = [(S[:, s[0]] * b[:, 0] + S[:, s[1]] * b[:, 1]) + S[:, s[2]] * b[:, 2] for s in _SYM]
    return (a[:, 0] * w[0] + a[:, 1] * w[1]) + a[:, 2] * w[2]


def _host_inputs(xyz, bones, cov6, valid, groups, what):
    X32 = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32))
    if X32.ndim != 3 or X32.shape[-1] != 3 or X32.size == 0:
        raise ValueError(f"{what}: `xyz` must be (N,J,3), got {X32.shape}")
    N, J = X32.shape[:2]
    bn = checked_bones(bones, J, what)

    def given(a, name, shape, dtype):
        a = np.asarray(a)
        if a.shape != shape:
            raise ValueError(f"{what}: `{name}` must be {shape}, got {a.shape}")
        return a.astype(dtype)
    C = None if cov6 is None else given(cov6, "cov6", (N, J, 6), np.float32).astype(np.float64)
    usable = np.isfinite(X32).all(-1)
    if valid is not None:
        usable &= given(valid, "valid", (N, J), bool)
    gid = np.zeros(N, dtype=np.int64) if groups is None else given(groups, "groups", (N,), np.int64)
    return X32, bn, C, usable, gid


def measure_host(xyz, bones, cov6=None, valid=None, max_sigma_mm=None):
    """sks_bone_measure in float64 numpy: (N,B) float32."""
    what = "measure_host"
    sigma = _max_sigma(max_sigma_mm, cov6, what)
    X32, bn, C, usable, _ = _host_inputs(xyz, bones, cov6, valid, None, what)
    X = X32.astype(np.float64)
    p, c = bn[:, 0], bn[:, 1]
    with np.errstate(all="ignore"):
        d = X[:, c] - X[:, p]
        n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        keep = usable[:, p] & usable[:, c]
        if sigma is not None:
            u = (d / n[..., None]).reshape(-1, 3)
            S = (C[:, p] + C[:, c]).reshape(-1, 6)
            keep &= (_quad(u, S, u) <= sigma * sigma).reshape(n.shape)
        return np.where(keep, n, np.nan).astype(np.float32)


def lengths_host(measured, groups=None, n_groups=None):
    """sks_bone_lengths in numpy: (length (G,B) float32, mad (G,B) float32, n_used (G,B) int32); a sort and an index."""
    M = np.asarray(measured, dtype=np.float32)
    N, B = M.shape
    G = _n_groups(groups, n_groups, "lengths_host")
    gid = np.zeros(N, dtype=np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    length, mad = np.full((G, B), np.nan, dtype=np.float32), np.full((G, B), np.nan, dtype=np.float32)
    n_used = np.zeros((G, B), dtype=np.int32)
    usable = np.isfinite(M) & ~np.signbit(M)
    for g in range(G):
        for b in range(B):
            l = M[(gid == g) & usable[:, b], b]
            if l.size:
                k = (l.size - 1) // 2
                length[g, b] = np.sort(l)[k]
                mad[g, b] = np.sort(np.abs(l - length[g, b]))[k]           # (float32 - float32, as the kernel's keys)
                n_used[g, b] = l.size
    return length, mad, n_used


def bone_lengths_host(xyz, bones, cov6=None, valid=None, groups=None, max_sigma_mm=None, n_groups=None):
    """bone_lengths in numpy: BoneLengths of arrays."""
    measured = measure_host(xyz, bones, cov6, valid, max_sigma_mm)
    if groups is not None and np.asarray(groups).shape != measured.shape[:1]:
        raise ValueError(f"bone_lengths_host: `groups` must be {measured.shape[:1]}, got {np.asarray(groups).shape}")
    return BoneLengths(*lengths_host(measured, groups, n_groups), measured)


def project_host(xyz, bones, lengths, cov6=None, valid=None, groups=None, cov_floor=0.0, max_iters=16, tol_mm=1e-3):
    """sks_bone_project in float64 numpy, every operation of the header's trip on all the frames still running at once (the
    frames are independent, so a frame's bits are the kernel's): Projected of arrays."""
    what = "project_host"
    floor, iters, tol = _projection_settings(cov_floor, max_iters, tol_mm, what)
    X32, bn, C, fit, gid = _host_inputs(xyz, bones, cov6, valid, groups, what)
    N, J = X32.shape[:2]
    B = bn.shape[0]
    p, c = bn[:, 0], bn[:, 1]
    Lt = np.asarray(lengths, dtype=np.float32)
    Lt = Lt[None] if Lt.ndim == 1 else Lt
    if Lt.ndim != 2 or Lt.shape[1] != B or not 1 <= Lt.shape[0] <= _lib.SKS_BONES_MAX_GROUPS:
        raise ValueError(f"{what}: `lengths` must be (G,{B}) with G 1 .. {_lib.SKS_BONES_MAX_GROUPS}, got {Lt.shape}")
    G = Lt.shape[0]
    if groups is None and G != 1:
        raise ValueError(f"{what}: {G} rows of lengths without groups")
    with np.errstate(all="ignore"):
        Sig = np.zeros((N, J, 6))
        Sig[..., [0, 3, 5]] = 1.0
        if C is not None:
            Sig = C.copy()
            Sig[..., [0, 3, 5]] += floor
            d0 = Sig[..., 0]
            l10 = Sig[..., 1] / d0
            l20 = Sig[..., 2] / d0
            d1 = Sig[..., 3] - l10 * Sig[..., 1]
            e = Sig[..., 4] - l20 * Sig[..., 1]
            z1 = Sig[..., 5] - l20 * Sig[..., 2]
            l21 = e / d1
            d2 = z1 - l21 * e
            fit = fit & np.isfinite(Sig).all(-1) & np.all([np.isfinite(q) & (q > 0) for q in (d0, d1, d2)], axis=0)
        inrange = (gid >= 0) & (gid < G)
        L = Lt[np.clip(gid, 0, G - 1)].astype(np.float64)
        active = inrange[:, None] & fit[:, p] & fit[:, c] & np.isfinite(L) & (L > 0)
        X = X32.astype(np.float64)
        moved = np.zeros((N, J), dtype=bool)
        res = np.full(N, np.nan)
        trips, n_active = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
        idx = np.arange(N)
        for it in range(iters + 1):
            if idx.size == 0:
                break
            x, act = X[idx], active[idx]
            d = x[:, c] - x[:, p]
            n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
            act = act & (n != 0)
            active[idx] = act
            u = d / n[..., None]
            r = np.where(act, n - L[idx], 0.0)
            rho = np.where(act, np.where(np.isfinite(r), np.abs(r), np.inf), 0.0).max(1)
            n_active[idx] = act.sum(1)
            some = n_active[idx] > 0
            res[idx[some]] = rho[some]
            go = some & ~(rho <= tol) & (it < iters)
            idx, x, act, u, r = idx[go], x[go], act[go], u[go], r[go]
            K = idx.size
            if K == 0:
                break
            S = np.zeros((B, B, K))
            lam = [r[:, b].copy() for b in range(B)]
            for a in range(B):
                for b in range(a + 1):
                    s = np.zeros(K)
                    if p[a] == p[b]:
                        s = s + _quad(u[:, a], Sig[idx, p[a]], u[:, b])
                    if p[a] == c[b]:
                        s = s - _quad(u[:, a], Sig[idx, p[a]], u[:, b])
                    if c[a] == p[b]:
                        s = s - _quad(u[:, a], Sig[idx, c[a]], u[:, b])
                    if c[a] == c[b]:
                        s = s + _quad(u[:, a], Sig[idx, c[a]], u[:, b])
                    S[a, b] = np.where(act[:, a] & act[:, b], s, 1.0 if a == b else 0.0)
            ok = np.ones(K, dtype=bool)
            for j in range(B):
                dj = S[j, j]
                ok &= np.isfinite(dj) & (dj > 0)
                col = {i: S[i, j] / dj for i in range(j + 1, B)}
                for i in range(j + 1, B):
                    for cc in range(j + 1, i + 1):
                        S[i, cc] = S[i, cc] - col[i] * S[cc, j]
                for i in range(j + 1, B):
                    S[i, j] = col[i]
                    lam[i] = lam[i] - col[i] * lam[j]
            for j in range(B):
                lam[j] = lam[j] / S[j, j]
            for j in range(B - 1, 0, -1):
                for i in range(j):
                    lam[i] = lam[i] - S[j, i] * lam[j]
            for j in range(J):
                g = np.zeros((K, 3))
                touched = np.zeros(K, dtype=bool)
                for b in range(B):
                    if c[b] == j:
                        g = np.where(act[:, b, None], g + lam[b][:, None] * u[:, b], g)
                        touched |= act[:, b]
                    if p[b] == j:
                        g = np.where(act[:, b, None], g - lam[b][:, None] * u[:, b], g)
                        touched |= act[:, b]
                touched &= ok
                Sj = Sig[idx, j]
                step = np.stack([(Sj[:, s[0]] * g[:, 0] + Sj[:, s[1]] * g[:, 1]) + Sj[:, s[2]] * g[:, 2] for s in _SYM], axis=-1)
                x[:, j] = np.where(touched[:, None], x[:, j] - step, x[:, j])
                moved[idx, j] |= touched
            X[idx] = x
            trips[idx[ok]] += 1
            idx = idx[ok]                                   # (a frame with a bad pivot ends at the x it had)
        joints = np.where(moved[..., None], X.astype(np.float32), X32)
        return Projected(joints, res.astype(np.float32), trips, n_active)
