"""Several people in front of the sequence pipeline: which detections of a frame's views show the same person (associate), which
person of a frame is which person of the frame before (track), and the tracked detections as one single-person sequence per
track (to_tracks) -- what triangulate_sequence, FramePipeline.optimize_sequence(None, ..), set_smoothing and set_bone_constraint
take, the last two with the `groups` to_tracks returns.

The two rules stand in include/skelsplat_hip.h ("People"), with the order of every operation.  Tensors on a ROCm device: one launch
each of the library's kernels (sks_associate_people, sks_track_people) on the current stream, nothing is copied to the host and
nothing synchronises.  Arrays or CPU tensors: the same rules in float64 numpy (associate_host, track_host), op for op, so the two
paths agree bit for bit; arrays in, arrays out."""
import collections

import numpy as np
import torch

from . import _pose_args as _pa

MAX_DETS, MAX_SLOTS, MAX_PEOPLE, MAX_GROUPS, MAX_JOINTS = 128, 16, 8, 65535, 32     # SKS_PEOPLE_*, SKS_MAX_CHANNELS

Association = collections.namedtuple("Association", "assign n_people n_overflow n_unassigned cost poses_2d")
Tracks = collections.namedtuple("Tracks", "track_id n_tracks n_dropped")


def _checked_association(V, M, J, K, max_px, min_joints, min_views):
    if not 1 <= M <= MAX_SLOTS:
        raise ValueError(f"M = {M} candidates a view: 1 .. {MAX_SLOTS} (SKS_PEOPLE_MAX_SLOTS)")
    if V * M > MAX_DETS:
        raise ValueError(f"V * M = {V * M} detections a frame: at most {MAX_DETS} (SKS_PEOPLE_MAX_DETS)")
    if not 1 <= J <= MAX_JOINTS:
        raise ValueError(f"J = {J} joints: 1 .. {MAX_JOINTS} (SKS_MAX_CHANNELS)")
    if int(K) != K or not 1 <= K <= MAX_PEOPLE:
        raise ValueError(f"max_people = {K}: 1 .. {MAX_PEOPLE} (SKS_PEOPLE_MAX)")
    max_px = float(max_px)
    if not (np.isfinite(max_px) and max_px >= 0):
        raise ValueError(f"max_px must be finite and >= 0 pixels, got {max_px}")
    if int(min_joints) != min_joints or not 1 <= min_joints <= J:
        raise ValueError(f"min_joints = {min_joints}: 1 .. J = {J}")
    if int(min_views) != min_views or not 2 <= min_views <= _pa.MAX_VIEWS:
        raise ValueError(f"min_views = {min_views}: 2 .. {_pa.MAX_VIEWS} (a person is seen by two views at least)")
    return int(K), max_px, int(min_joints), int(min_views)


# ------------------------------------------------------------------------------------------------------------ association, host
def _minors(P):
    """(.., V, 3, 4) -> (.., V, 3, 6): per dropped row i the 2x2 minors of the two other rows, columns 01 02 03 12 13 23."""
    out = np.empty(P.shape[:-2] + (3, 6))
    for i, (r0, r1) in enumerate(((1, 2), (0, 2), (0, 1))):
        a, b = P[..., r0, :], P[..., r1, :]
        for e, (p, q) in enumerate(((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))):
            out[..., i, e] = a[..., p] * b[..., q] - a[..., q] * b[..., p]
    return out


def fundamental_matrices(P):
    """The header's F for every ordered pair of views: P (.., V, 3, 4) float64 -> (.., V, V, 3, 3), [.., va, vb] maps a pixel of va
    to its line in vb (the rule reads the entries va < vb only)."""
    m = _minors(np.asarray(P, dtype=np.float64))
    A, B = m[..., :, None, None, :, :], m[..., None, :, :, None, :]         # [.., va, vb, j, i, minor]
    det = ((((A[..., 0] * B[..., 5] - A[..., 1] * B[..., 4]) + A[..., 2] * B[..., 3]) + A[..., 3] * B[..., 2])
           - A[..., 4] * B[..., 1]) + A[..., 5] * B[..., 0]
    sign = np.array([[1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, 1.0]])
    return det * sign


def pair_costs_host(P, x, valid, min_joints):
    """The header's pair cost for every a < b in different views of every frame: P (V,3,4) or (N,V,3,4), x (N,V,M,J,2) float64,
    valid (N,V,M,J) bool or None -> (ia, ib, c (N,n_pairs) float64, measured (N,n_pairs) bool).  The joints are added one after the
    other, the pairs and the frames side by side."""
    N, V, M, J = x.shape[:4]
    D = V * M
    ia, ib = np.nonzero(np.arange(D)[:, None] // M < np.arange(D)[None, :] // M)       # ascending (a, b)
    F = fundamental_matrices(P)[..., ia // M, ib // M, :, :]                              # (n_pairs,3,3) or (N,n_pairs,3,3)
    xs = x.reshape(N, D, J, 2)
    keep = np.ones((N, D, J), dtype=bool) if valid is None else valid.reshape(N, D, J)
    total, n = np.zeros((N, len(ia))), np.zeros((N, len(ia)), dtype=np.int64)
    with np.errstate(all="ignore"):
        for j in range(J):
            ax, ay, bx, by = xs[:, ia, j, 0], xs[:, ia, j, 1], xs[:, ib, j, 0], xs[:, ib, j, 1]
            ok = keep[:, ia, j] & keep[:, ib, j] & np.isfinite(ax) & np.isfinite(ay) & np.isfinite(bx) & np.isfinite(by)
            l0, l1, l2 = ((F[..., k, 0] * ax + F[..., k, 1] * ay) + F[..., k, 2] for k in range(3))
            db = np.abs((l0 * bx + l1 * by) + l2) / np.sqrt(l0 * l0 + l1 * l1)
            t0, t1, t2 = ((F[..., 0, k] * bx + F[..., 1, k] * by) + F[..., 2, k] for k in range(3))
            da = np.abs((t0 * ax + t1 * ay) + t2) / np.sqrt(t0 * t0 + t1 * t1)
            d = 0.5 * (db + da)
            ok &= np.isfinite(d)
            total = np.where(ok, total + d, total)
            n += ok
        c = total / n
    return ia, ib, c, n >= min_joints


def _bits(mask):
    return [i for i in range(mask.bit_length()) if (mask >> i) & 1]


def associate_host(P, x, valid, max_px, min_joints, min_views, K):
    """sks_associate_people's rule on the host: P (V,3,4) or (N,V,3,4) float64, x (N,V,M,J,2), valid (N,V,M,J) bool or None ->
    Association of arrays (poses_2d in x's dtype)."""
    N, V, M, J = x.shape[:4]
    D = V * M
    x64 = x.astype(np.float64)
    ia, ib, c, measured = pair_costs_host(P, x64, valid, min_joints)
    edge = measured & (c <= max_px)
    veto = measured & ~edge
    keep = np.ones((N, V, M, J), dtype=bool) if valid is None else valid
    live = (keep & np.isfinite(x64).all(axis=-1)).any(axis=-1).reshape(N, D)
    assign = np.full((N, K, V), -1, dtype=np.int32)
    n_people, n_overflow, n_unassigned = (np.zeros(N, dtype=np.int32) for _ in range(3))
    cost = np.full((N, K), np.nan)
    gathered = np.full((N, K, V, J, 2), np.nan, dtype=x.dtype)
    for f in range(N):
        vetoes = [0] * D
        for a, b in zip(ia[veto[f]], ib[veto[f]]):
            vetoes[a] |= 1 << int(b)
            vetoes[b] |= 1 << int(a)
        e = np.nonzero(edge[f])[0]
        e = e[np.lexsort((ib[e], ia[e], c[f, e]))]
        label, members, views = list(range(D)), [1 << i for i in range(D)], [1 << (i // M) for i in range(D)]
        for a, b in zip(ia[e], ib[e]):
            la, lb = label[a], label[b]
            if la == lb or views[la] & views[lb]:
                continue
            if any(vetoes[i] & members[lb] for i in _bits(members[la])):
                continue
            keep_l, drop_l = min(la, lb), max(la, lb)
            for i in _bits(members[drop_l]):
                label[i] = keep_l
            members[keep_l] |= members[drop_l]
            views[keep_l] |= views[drop_l]
        roots = [i for i in range(D) if label[i] == i and bin(members[i]).count("1") >= min_views]
        roots.sort(key=lambda i: (-bin(members[i]).count("1"), i))
        n_people[f], n_overflow[f] = min(len(roots), K), max(0, len(roots) - K)
        written = 0
        edge_cost = {(int(a), int(b)): c[f, i] for i, (a, b) in enumerate(zip(ia, ib)) if edge[f, i]}
        for k, root in enumerate(roots[:K]):
            mem = _bits(members[root])
            written |= members[root]
            total, n = 0.0, 0
            for a in mem:                               # ascending (a, b)
                assign[f, k, a // M] = a % M
                for b in mem:
                    if (a, b) in edge_cost:
                        total, n = total + edge_cost[(a, b)], n + 1
            cost[f, k] = total / n if n else np.nan
            for a in mem:
                v, m = divmod(a, M)
                gathered[f, k, v] = np.where(keep[f, v, m][:, None], x[f, v, m], np.nan)
        n_unassigned[f] = sum(1 for i in range(D) if live[f, i] and not (written >> i) & 1)
    return Association(assign, n_people, n_overflow, n_unassigned, cost, gathered)


def associate(proj_or_cameras, detections, valid=None, max_px=15.0, min_joints=3, min_views=2, max_people=8, out=None):
    """Which detections of a frame's views show the same person (include/skelsplat_hip.h, sks_associate_people).

    `detections`: (N,V,M,J,>=2) pixel (x, y, ..) of up to M candidate skeletons per view in arbitrary slot order -- or (V,M,J,>=2),
    one frame, and then the results have no frame axis.  `proj_or_cameras`: what triangulate_sequence takes ((V,3,4), (N,V,3,4) for
    one rig per frame, or V cameras).  `valid`: optional (N,V,M,J) bool, False = this joint of this candidate was not detected.
    Two detections of different views cost the mean symmetric epipolar distance of their common joints (at least `min_joints`);
    pairs within `max_px` pixels are merged in ascending cost, never two detections of one view and never across a measured pair
    above `max_px`; clusters seen by at least `min_views` views are the frame's people, largest first, `max_people` (K <= 8) written.
    Returns Association(assign (N,K,V) int32 -- the slot of person k in view v or -1 --, n_people, n_overflow, n_unassigned (N) int32,
    cost (N,K) float64 -- a person's mean edge cost, NaN for an empty slot --, poses_2d (N,K,V,J,2) in the detections' type: the
    detections in person order, NaN where a person has none or the joint is not kept; poses_2d.reshape(N * K, V, J, 2) is what
    triangulate_sequence and optimize_sequence(None, ..) take, and kept(poses_2d) the `valid` that goes with it).  `out`: an
    Association of contiguous tensors of these shapes where the detections live, written in place.  On a ROCm device: one launch
    on the current stream, nothing synchronises; a frame's result does not depend on N, on its place in the batch or on the
    stream.  On the host: associate_host."""
    x, as_array = _pa.as_tensor(detections)
    dev = x.device
    P = _pa.projections(proj_or_cameras, dev)
    single = x.dim() == 4
    x = x[None] if single else x
    if x.dim() != 5 or x.shape[-1] < 2:
        raise ValueError(f"detections must be (N,V,M,J,>=2) or (V,M,J,>=2), got {tuple(detections.shape)}")
    N, V, M, J = x.shape[:4]
    _pa.check_shapes(P, N, V, J)
    K, max_px, min_joints, min_views = _checked_association(V, M, J, max_people, max_px, min_joints, min_views)
    valid = _pa.check_valid(valid, single, dev, (N, V, M, J))
    xd = _pa.as_real(x[..., :2])
    shapes = (((N, K, V), torch.int32), ((N,), torch.int32), ((N,), torch.int32), ((N,), torch.int32), ((N, K), torch.float64),
              ((N, K, V, J, 2), xd.dtype))
    if out is None:
        res = Association(*(torch.empty(s, dtype=d, device=dev) for s, d in shapes))
    else:
        res = Association(*(_pa.check_out(o, s, (d,), dev, single, name=f"`out.{n}`")
                            for o, (s, d), n in zip(out, shapes, Association._fields)))
    if dev.type == "cuda":
        from . import _lib
        P = P.contiguous()
        with torch.cuda.device(dev):
            rc = _lib.load().sks_associate_people(
                N, V, M, J, K, P.data_ptr(), _pa.rig_stride(P, V), *_pa.pointers(xd), _pa.byte_pointer(valid), max_px, min_joints,
                min_views, res.assign.data_ptr(), res.n_people.data_ptr(), res.n_overflow.data_ptr(), res.n_unassigned.data_ptr(),
                res.cost.data_ptr(), *_pa.pointers(res.poses_2d), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "sks_associate_people")
    else:
        got = associate_host(P.numpy(), xd.numpy(), None if valid is None else valid.numpy(), max_px, min_joints, min_views, K)
        for t, a in zip(res, got):
            t.copy_(torch.as_tensor(a))
    if out is not None:
        return out
    return Association(*(_pa.finish(t, single, as_array) for t in res))


# ------------------------------------------------------------------------------------------------------------ tracking
def _n_groups(groups, n_groups, N):
    if groups is None:
        if n_groups not in (None, 1):
            raise ValueError(f"n_groups = {n_groups} without groups")
        return None, 1
    g = _pa.as_tensor(groups)[0]
    if g.dim() != 1 or g.shape[0] != N or g.dtype.is_floating_point:
        raise ValueError(f"groups must be (N,) = ({N},) integers, got {tuple(g.shape)} {g.dtype}")
    if n_groups is None:
        n_groups = int(g.max()) + 1          # (a device tensor: ONE number is read back -- pass n_groups to avoid it)
    if not 1 <= int(n_groups) <= MAX_GROUPS:
        raise ValueError(f"{n_groups} recordings: 1 .. {MAX_GROUPS} (SKS_PEOPLE_MAX_GROUPS)")
    return g, int(n_groups)


def track_host(joints, groups, n_groups, max_mm, max_gap, min_joints):
    """sks_track_people's rule on the host: joints (N,K,J,3) float32, groups (N,) ints or None -> Tracks of arrays."""
    N, K, J = joints.shape[:3]
    x = joints.astype(np.float64)
    fin = np.isfinite(x).all(axis=-1)                               # (N,K,J)
    track_id = np.full((N, K), -1, dtype=np.int32)
    n_tracks, n_dropped = np.zeros(n_groups, dtype=np.int32), np.zeros(n_groups, dtype=np.int32)
    S = MAX_PEOPLE
    for g in range(n_groups):
        alive, age, ids = [False] * S, [0] * S, [-1] * S
        pose, pose_fin = np.zeros((S, J, 3)), np.zeros((S, J), dtype=bool)
        frames = range(N) if groups is None else np.nonzero(groups == g)[0]
        for f in frames:
            present = fin[f].sum(axis=-1) >= min_joints
            total, n = np.zeros((S, K)), np.zeros((S, K), dtype=np.int64)
            with np.errstate(all="ignore"):
                for j in range(J):
                    both = pose_fin[:, None, j] & fin[f, None, :, j]
                    d = x[f, None, :, j] - pose[:, None, j]
                    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
                    total = np.where(both, total + dist, total)
                    n += both
                c = total / n
            ok = np.asarray(alive)[:, None] & present[None, :] & (n >= min_joints) & (c <= max_mm)
            matched_s, matched_k = {}, {}
            for s, k in sorted(zip(*np.nonzero(ok)), key=lambda sk: (c[sk], sk[0], sk[1])):
                if s not in matched_s and k not in matched_k:
                    matched_s[s], matched_k[k] = k, s
            for s in range(S):
                if not alive[s]:
                    continue
                if s in matched_s:
                    age[s] = 0
                    pose[s], pose_fin[s] = x[f, matched_s[s]], fin[f, matched_s[s]]
                    track_id[f, matched_s[s]] = ids[s]
                else:
                    age[s] += 1
                    alive[s] = age[s] <= max_gap
            for k in range(K):
                if not present[k] or k in matched_k:
                    continue
                free = [s for s in range(S) if not alive[s]]
                if not free:
                    n_dropped[g] += 1
                    continue
                s = free[0]
                alive[s], age[s], ids[s] = True, 0, int(n_tracks[g])
                pose[s], pose_fin[s] = x[f, k], fin[f, k]
                track_id[f, k] = ids[s]
                n_tracks[g] += 1
    return Tracks(track_id, n_tracks, n_dropped)


def track(joints, groups=None, max_mm=300.0, max_gap=5, min_joints=3, n_groups=None):
    """Which person of a frame is which person of the frame before (include/skelsplat_hip.h, sks_track_people).

    `joints`: (N,K,J,3) float32, the triangulated people of every frame in any order, an absent person all NaN (what
    triangulate_sequence makes of associate's poses_2d, reshaped to (N,K,J,3)).  `groups`: optional (N,) integers, the recording of
    every frame: each is tracked on its own, its frames in ascending order, ids from 0 (`n_groups`: their number; None reads the
    largest id back when groups live on the device).  A person is present with `min_joints` finite joints; it continues the alive
    track whose last matched pose lies nearest in mean joint distance, within `max_mm`, greedily in ascending (distance, slot,
    person); a track unmatched for more than `max_gap` frames ends; at most 8 tracks are alive at a time.  Returns
    Tracks(track_id (N,K) int32, -1 = absent or dropped; n_tracks, n_dropped (n_groups,) int32).  On a ROCm device: a memset and
    one launch on the current stream, one wavefront per recording; on the host: track_host."""
    x, as_array = _pa.as_tensor(joints)
    if x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"joints must be (N,K,J,3), got {tuple(x.shape)}")
    N, K, J = x.shape[:3]
    if N < 1 or not 1 <= K <= MAX_PEOPLE or not 1 <= J <= MAX_JOINTS:
        raise ValueError(f"joints (N,K,J,3) = {tuple(x.shape)}: N >= 1, K 1 .. {MAX_PEOPLE} (SKS_PEOPLE_MAX), J 1 .. {MAX_JOINTS}")
    max_mm = float(max_mm)
    if not (np.isfinite(max_mm) and max_mm >= 0):
        raise ValueError(f"max_mm must be finite and >= 0, got {max_mm}")
    if int(max_gap) != max_gap or not 0 <= max_gap <= 1 << 26:
        raise ValueError(f"max_gap = {max_gap} frames: 0 .. 2^26")
    if int(min_joints) != min_joints or not 1 <= min_joints <= J:
        raise ValueError(f"min_joints = {min_joints}: 1 .. J = {J}")
    dev = x.device
    g, G = _n_groups(groups, n_groups, N)
    x = x.to(torch.float32).contiguous()
    if dev.type == "cuda":
        from . import _lib
        g = None if g is None else g.to(device=dev, dtype=torch.int32).contiguous()
        res = Tracks(torch.empty((N, K), dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.int32, device=dev),
                     torch.empty(G, dtype=torch.int32, device=dev))
        with torch.cuda.device(dev):
            rc = _lib.load().sks_track_people(N, K, J, x.data_ptr(), None if g is None else g.data_ptr(), G, max_mm, int(max_gap),
                                              int(min_joints), res.track_id.data_ptr(), res.n_tracks.data_ptr(),
                                              res.n_dropped.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "sks_track_people")
        return res
    got = track_host(x.numpy(), None if g is None else g.cpu().numpy(), G, max_mm, int(max_gap), int(min_joints))
    return got if as_array else Tracks(*(torch.as_tensor(a) for a in got))


def kept(poses_2d):
    """The `valid` of gathered detections: (..,V,J,2) -> (..,V,J) bool, True where both coordinates are finite.  The pose entry points
    read a NaN detection as "this joint is unobserved in this frame"; with this mask they solve the joint from the views that do
    have it (triangulate_sequence(.., valid=kept(p2d))).  A tensor op where the detections live: nothing is read back."""
    t, as_array = _pa.as_tensor(poses_2d)
    ok = torch.isfinite(t[..., :2]).all(dim=-1)
    return ok.numpy() if as_array else ok


def to_tracks(track_id, poses_2d, max_tracks, groups=None, n_groups=None):
    """The tracked detections as one single-person sequence per track: track_id (N,K) from track, poses_2d (N,K,V,J,2) from
    associate -> (tracks (max_tracks,N,V,J,2), groups (max_tracks * N,) int32).  tracks[t, n] holds the detections of the person
    with id t in frame n and NaN where that track has none (an unobserved frame for everything downstream); a person whose id is
    -1 or >= max_tracks goes nowhere.  tracks.reshape(max_tracks * N, V, J, 2) is what triangulate_sequence and
    optimize_sequence(None, ..) take, and the returned vector is the `groups` of those frames for set_smoothing and
    set_bone_constraint: t without `groups`, t * n_groups + groups[n] with them (ids restart in every recording), so no window and
    no median mixes two people or two recordings.  Tensor indexing where the inputs live: nothing is read back, nothing
    synchronises.  Arrays in, arrays out."""
    tid, as_array = _pa.as_tensor(track_id)
    p2d = _pa.as_tensor(poses_2d)[0]
    if p2d.dim() != 5 or tid.dim() != 2 or tuple(p2d.shape[:2]) != tuple(tid.shape):
        raise ValueError(f"track_id must be (N,K) and poses_2d (N,K,V,J,2), got {tuple(tid.shape)} and {tuple(p2d.shape)}")
    if int(max_tracks) != max_tracks or max_tracks < 1:
        raise ValueError(f"max_tracks = {max_tracks}: at least 1")
    T, dev = int(max_tracks), p2d.device
    N = tid.shape[0]
    t = tid.to(device=dev, dtype=torch.long)
    t = torch.where((t >= 0) & (t < T), t, torch.full((), T, dtype=torch.long, device=dev))      # row T: nowhere
    out = torch.full((T + 1, N) + tuple(p2d.shape[2:]), float("nan"), dtype=p2d.dtype, device=dev)
    out[t, torch.arange(N, device=dev)[:, None]] = p2d
    ids = torch.arange(T, device=dev, dtype=torch.int32)[:, None]
    if groups is None:
        if n_groups not in (None, 1):
            raise ValueError(f"n_groups = {n_groups} without groups")
        gid = ids.expand(T, N)
    else:
        if n_groups is None:
            raise ValueError("to_tracks with groups needs n_groups, the number of recordings (it reads nothing back)")
        g = _pa.as_tensor(groups)[0].to(device=dev, dtype=torch.int32)
        if tuple(g.shape) != (N,):
            raise ValueError(f"groups must be (N,) = ({N},), got {tuple(g.shape)}")
        gid = ids * int(n_groups) + g[None, :]
    tracks, gid = out[:T], gid.reshape(-1).contiguous()
    return (tracks.numpy(), gid.numpy()) if as_array else (tracks, gid)
