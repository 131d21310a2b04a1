"""TEST INFRASTRUCTURE -- the two rules of include/skelsplat_hip.h "People" restated op by op in float64 numpy, one frame and one
recording at a time with plain Python containers (sets and lists where the kernel and the host path keep bit masks), and an
independent reference for the pair costs.

associate_frame / associate: the fundamental matrices by the header's expansion, the pair costs with the joints added one after
the other (the pairs side by side), the edges in ascending (cost, a, b), the constrained complete-link walk, the people.  It also
counts the branches the walk took, so a test can assert that its case reaches the branch it is there for:
    view_refused   merges refused because the two clusters share a view
    veto_refused   merges refused because a pair across the two clusters is a veto
    same_cluster   edges between two members of one cluster
    unmeasured     pairs of different views with fewer than min_joints common joints
    index_ties     neighbours in the sorted edge list with equal cost, ordered by (a, b) alone
`link="single"` drops the veto test (single-link under the view rule): what the rule is NOT.
track: the tracker, one recording after the other.
reference_costs: F = [e_b]x P_b pinv(P_a) with numpy's pseudo-inverse and the point-to-line distances in plain vectorised numpy: no
minors, no fixed order -- what the restatement's costs are held to within a measured bound."""
import numpy as np

S = 8       # SKS_PEOPLE_MAX: people written a frame, track slots of a recording


def minors(P):
    """(3,4) -> [i] = the six 2x2 minors of the two rows other than i, columns 01 02 03 12 13 23."""
    out = []
    for i in range(3):
        r0, r1 = [P[r] for r in range(3) if r != i]
        out.append([r0[p] * r1[q] - r0[q] * r1[p] for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))])
    return out


def fundamental(Pa, Pb):
    """The header's F of views a < b: float64 (3,3), x_b^T F x_a = 0."""
    ma, mb = minors(np.asarray(Pa, np.float64)), minors(np.asarray(Pb, np.float64))
    F = np.empty((3, 3))
    for j in range(3):
        for i in range(3):
            A, B = ma[i], mb[j]
            det = ((((A[0] * B[5] - A[1] * B[4]) + A[2] * B[3]) + A[3] * B[2]) - A[4] * B[1]) + A[5] * B[0]
            F[j, i] = det if (i + j) % 2 == 0 else -det
    return F


def pair_costs(P, x, keep, min_joints):
    """One frame: P (V,3,4), x (V,M,J,2) float64, keep (V,M,J) bool -> {(a, b): cost} over the MEASURED pairs a < b of different
    views, and the number of unmeasured ones."""
    V, M, J = x.shape[:3]
    D = V * M
    xs, ks = x.reshape(D, J, 2), keep.reshape(D, J)
    Fs = {(va, vb): fundamental(P[va], P[vb]) for va in range(V) for vb in range(va + 1, V)}
    pairs = [(a, b) for a in range(D) for b in range(D) if a // M < b // M]
    if not pairs:
        return {}, 0
    ia, ib = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    F = np.stack([Fs[(a // M, b // M)] for a, b in pairs])                  # (n,3,3)
    total, n = np.zeros(len(pairs)), np.zeros(len(pairs), dtype=np.int64)
    with np.errstate(all="ignore"):
        for j in range(J):                                                  # sequential over the joints
            ax, ay, bx, by = xs[ia, j, 0], xs[ia, j, 1], xs[ib, j, 0], xs[ib, j, 1]
            ok = ks[ia, j] & ks[ib, j] & np.isfinite(ax) & np.isfinite(ay) & np.isfinite(bx) & np.isfinite(by)
            l0 = (F[:, 0, 0] * ax + F[:, 0, 1] * ay) + F[:, 0, 2]
            l1 = (F[:, 1, 0] * ax + F[:, 1, 1] * ay) + F[:, 1, 2]
            l2 = (F[:, 2, 0] * ax + F[:, 2, 1] * ay) + F[:, 2, 2]
            db = np.abs((l0 * bx + l1 * by) + l2) / np.sqrt(l0 * l0 + l1 * l1)
            t0 = (F[:, 0, 0] * bx + F[:, 1, 0] * by) + F[:, 2, 0]
            t1 = (F[:, 0, 1] * bx + F[:, 1, 1] * by) + F[:, 2, 1]
            t2 = (F[:, 0, 2] * bx + F[:, 1, 2] * by) + F[:, 2, 2]
            da = np.abs((t0 * ax + t1 * ay) + t2) / np.sqrt(t0 * t0 + t1 * t1)
            d = 0.5 * (db + da)
            ok = ok & np.isfinite(d)
            total[ok] = total[ok] + d[ok]
            n[ok] += 1
        c = total / n
    measured = n >= min_joints
    return {p: float(c[i]) for i, p in enumerate(pairs) if measured[i]}, int((~measured).sum())


def associate_frame(P, x, keep, max_px, min_joints, min_views, K, link="complete"):
    """One frame of sks_associate_people -> dict(assign (K,V), n_people, n_overflow, n_unassigned, cost (K), poses_2d (K,V,J,2),
    counters, costs = {(a, b): c} of the measured pairs, clusters = the people's member lists, all of them)."""
    V, M, J = x.shape[:3]
    D = V * M
    x64 = x.astype(np.float64)
    costs, unmeasured = pair_costs(P, x64, keep, min_joints)
    edges = sorted((c, a, b) for (a, b), c in costs.items() if c <= max_px)
    vetoes = {p for p, c in costs.items() if not c <= max_px}
    counters = dict(view_refused=0, veto_refused=0, same_cluster=0, unmeasured=unmeasured,
                    index_ties=sum(1 for e, g in zip(edges, edges[1:]) if e[0] == g[0]))
    cluster = {i: [i] for i in range(D)}            # label (the lowest member) -> members
    label = list(range(D))
    for c, a, b in edges:
        la, lb = label[a], label[b]
        if la == lb:
            counters["same_cluster"] += 1
            continue
        if {i // M for i in cluster[la]} & {i // M for i in cluster[lb]}:
            counters["view_refused"] += 1
            continue
        if link == "complete" and any((min(i, o), max(i, o)) in vetoes for i in cluster[la] for o in cluster[lb]):
            counters["veto_refused"] += 1
            continue
        keep_l, drop_l = min(la, lb), max(la, lb)
        for i in cluster[drop_l]:
            label[i] = keep_l
        cluster[keep_l] = sorted(cluster[keep_l] + cluster.pop(drop_l))
    people = sorted((m for m in cluster.values() if len(m) >= min_views), key=lambda m: (-len(m), m[0]))
    assign = np.full((K, V), -1, dtype=np.int32)
    cost = np.full(K, np.nan)
    gathered = np.full((K, V, J, 2), np.nan, dtype=x.dtype)
    written = set()
    for k, mem in enumerate(people[:K]):
        written |= set(mem)
        total, n = 0.0, 0
        for a in mem:
            v, m = divmod(a, M)
            assign[k, v] = m
            for j in range(J):
                if keep[v, m, j]:
                    gathered[k, v, j] = x[v, m, j]
            for b in mem:
                if a < b and (a, b) in costs and costs[(a, b)] <= max_px:
                    total, n = total + costs[(a, b)], n + 1
        if n:
            cost[k] = total / n
    live = (keep & np.isfinite(x64).all(axis=-1)).any(axis=-1).reshape(D)
    return dict(assign=assign, n_people=min(len(people), K), n_overflow=max(0, len(people) - K),
                n_unassigned=sum(1 for i in range(D) if live[i] and i not in written), cost=cost, poses_2d=gathered,
                counters=counters, costs=costs, clusters=people)


def associate(P, x, valid, max_px, min_joints=3, min_views=2, K=8, link="complete"):
    """N frames: P (V,3,4) or (N,V,3,4), x (N,V,M,J,2) float32 / float64, valid (N,V,M,J) bool or None -> dict of stacked arrays
    (assign int32, the three counts int32, cost float64, poses_2d in x's dtype) and `frames`, the per-frame records."""
    P = np.asarray(P, np.float64)
    N = x.shape[0]
    keep = np.ones(x.shape[:4], dtype=bool) if valid is None else np.asarray(valid, bool)
    frames = [associate_frame(P[f] if P.ndim == 4 else P, x[f], keep[f], max_px, min_joints, min_views, K, link) for f in range(N)]
    out = {k: np.stack([fr[k] for fr in frames]) for k in ("assign", "cost", "poses_2d")}
    for k in ("n_people", "n_overflow", "n_unassigned"):
        out[k] = np.array([fr[k] for fr in frames], dtype=np.int32)
    out["frames"] = frames
    out["counters"] = {k: sum(fr["counters"][k] for fr in frames) for k in frames[0]["counters"]}
    return out


def track(joints, groups, n_groups, max_mm, max_gap, min_joints):
    """sks_track_people: joints (N,K,J,3) float32, groups (N,) ints or None -> dict(track_id (N,K), n_tracks, n_dropped (G),
    counters: ties = candidate pairs of one frame with equal cost, freed = slots freed by age, reused = tracks opened in a slot
    that held another track before)."""
    N, K, J = joints.shape[:3]
    x = joints.astype(np.float64)
    track_id = np.full((N, K), -1, dtype=np.int32)
    n_tracks, n_dropped = np.zeros(n_groups, dtype=np.int32), np.zeros(n_groups, dtype=np.int32)
    counters = dict(ties=0, freed=0, reused=0)
    for g in range(n_groups):
        slots = [None] * S                          # dict(id, age, pose) or None
        used = [False] * S
        for f in range(N):
            if (0 if groups is None else int(groups[f])) != g:
                continue
            fin = np.isfinite(x[f]).all(axis=-1)    # (K,J)
            present = [int(fin[k].sum()) >= min_joints for k in range(K)]
            cands = []
            for s in range(S):
                if slots[s] is None:
                    continue
                q = slots[s]["pose"]
                qfin = np.isfinite(q).all(axis=-1)
                for k in range(K):
                    if not present[k]:
                        continue
                    total, n = 0.0, 0
                    for j in range(J):
                        if fin[k, j] and qfin[j]:
                            d = x[f, k, j] - q[j]
                            total, n = total + float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])), n + 1
                    if n >= min_joints and total / n <= max_mm:
                        cands.append((total / n, s, k))
            cands.sort()
            counters["ties"] += sum(1 for a, b in zip(cands, cands[1:]) if a[0] == b[0])
            got_s, got_k = {}, {}
            for c, s, k in cands:
                if s not in got_s and k not in got_k:
                    got_s[s], got_k[k] = k, s
            for s in range(S):
                if slots[s] is None:
                    continue
                if s in got_s:
                    slots[s].update(age=0, pose=x[f, got_s[s]].copy())
                    track_id[f, got_s[s]] = slots[s]["id"]
                else:
                    slots[s]["age"] += 1
                    if slots[s]["age"] > max_gap:
                        slots[s] = None
                        counters["freed"] += 1
            for k in range(K):
                if not present[k] or k in got_k:
                    continue
                free = [s for s in range(S) if slots[s] is None]
                if not free:
                    n_dropped[g] += 1
                    continue
                s = free[0]
                counters["reused"] += int(used[s])
                used[s] = True
                slots[s] = dict(id=int(n_tracks[g]), age=0, pose=x[f, k].copy())
                track_id[f, k] = n_tracks[g]
                n_tracks[g] += 1
    return dict(track_id=track_id, n_tracks=n_tracks, n_dropped=n_dropped, counters=counters)


# ------------------------------------------------------------------------------------------------ the independent reference
def reference_fundamental(Pa, Pb):
    """F = [e_b]x P_b pinv(P_a), e_b = P_b C_a with C_a the null vector of P_a (Hartley & Zisserman 9.1)."""
    Pa, Pb = np.asarray(Pa, np.float64), np.asarray(Pb, np.float64)
    C = np.linalg.svd(Pa)[2][-1]
    e = Pb @ C
    ex = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
    return ex @ Pb @ np.linalg.pinv(Pa)


def reference_costs(P, x, keep, min_joints):
    """pair_costs by the independent route: {(a, b): cost} over the measured pairs of one frame."""
    V, M, J = x.shape[:3]
    D = V * M
    xs = np.concatenate([x.reshape(D, J, 2).astype(np.float64), np.ones((D, J, 1))], axis=-1)
    ks = keep.reshape(D, J) & np.isfinite(xs).all(axis=-1)
    out = {}
    for va in range(V):
        for vb in range(va + 1, V):
            F = reference_fundamental(P[va], P[vb])
            for a in range(va * M, va * M + M):
                for b in range(vb * M, vb * M + M):
                    ok = ks[a] & ks[b]
                    if ok.sum() < min_joints:
                        continue
                    lb, la = xs[a, ok] @ F.T, xs[b, ok] @ F
                    db = np.abs((lb * xs[b, ok]).sum(-1)) / np.hypot(lb[:, 0], lb[:, 1])
                    da = np.abs((la * xs[a, ok]).sum(-1)) / np.hypot(la[:, 0], la[:, 1])
                    out[(a, b)] = float(np.mean(0.5 * (db + da)))
    return out
