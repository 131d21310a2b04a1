"""float64 numpy references for csrc/sks_report.hip, the rounding allowances its float results are held to, and the snapshot
rule of sks_loop_report as a pure function next to a literal host model of the control flow it stands for (train.py:130-233).
No torch, no device."""
import numpy as np

U32 = 2.0 ** -24        # unit roundoff of float32 (round to nearest)
U64 = 2.0 ** -53


def pose_errors_ref(pred, gt):
    """pred, gt (N,P,3) -> per_joint (N,P,2), mean (N,2) in float64: ||pred - gt|| and ||(pred - pred[0]) - (gt - gt[0])||
    (train.py:198-204), mean over the joints."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    e_abs = np.linalg.norm(pred - gt, axis=-1)
    e_rel = np.linalg.norm((pred - pred[:, 0:1]) - (gt - gt[:, 0:1]), axis=-1)
    pj = np.stack([e_abs, e_rel], axis=-1)
    return pj, pj.mean(axis=1)


def per_joint_allowance(pred, gt):
    """What the kernel's float arithmetic may differ by from pose_errors_ref on the same float32 inputs, per joint and column,
    from its order of operations.  Each float subtraction is off by at most U32 x |result| <= U32 x (|a| + |b|); column 1 chains
    two levels of them, and the first level's errors pass through the second.  In the norm sqrt((x^2 + y^2) + z^2) every term goes
    through at most three roundings (its square, two additions); the correctly rounded square root halves that and adds its
    own: 2.5 units of the norm, of which the formula allows 4.
        allowance = U32 x (4 ||d|| + sum of |operands of every subtraction|)"""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    pj, _ = pose_errors_ref(pred, gt)
    terms_abs = (np.abs(pred) + np.abs(gt)).sum(axis=-1)
    a, b = pred - pred[:, 0:1], gt - gt[:, 0:1]
    terms_rel = (np.abs(pred) + np.abs(pred[:, 0:1]) + np.abs(gt) + np.abs(gt[:, 0:1]) + np.abs(a) + np.abs(b)).sum(axis=-1)
    return U32 * (4.0 * pj + np.stack([terms_abs, terms_rel], axis=-1))


def mean_allowance(per_joint):
    """The kernel's float mean over P joints against the float64 mean OF THE SAME float32 per-joint values: P - 1 additions in
    some fixed order, one conversion of P, one division -- at most (P + 2) units of the mean (all terms are >= 0)."""
    per_joint = np.asarray(per_joint, np.float64)
    P = per_joint.shape[1]
    return (P + 2) * U32 * per_joint.mean(axis=1)


def eval_sequence_ref(pred, gt, groups=None, n_groups=0, abs_valid=None):
    """eval.py:123-142 in float64: (1 + n_groups, 2) = {absolute, root-relative} MPJPE, row 0 over all frames, row 1 + g over
    the frames of group g; frames with abs_valid False are left out of column 0 only; a row without frames is NaN."""
    pj, _ = pose_errors_ref(pred, gt)
    N = pj.shape[0]
    valid = np.ones(N, bool) if abs_valid is None else np.asarray(abs_valid, bool)
    out = np.full((1 + n_groups, 2), np.nan)
    for r in range(1 + n_groups):
        sel = np.ones(N, bool) if r == 0 else np.asarray(groups) == r - 1
        if (sel & valid).any():
            out[r, 0] = pj[sel & valid, :, 0].mean()
        if sel.any():
            out[r, 1] = pj[sel, :, 1].mean()
    return out


def loss_row_ref(S, N):
    """The loss early_stop_decide forms from a view's sums: (float)(S / max(N, 1)) with S, N float64."""
    S, N = np.asarray(S, np.float64), np.asarray(N, np.float64)
    return (S / np.maximum(N, 1.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the snapshot rule
def snapshot_action(s, acc_steps, n, stop):
    """What one sks_loop_report launch does to the slot of save iteration `s` for a frame that has made `n` optimiser steps and
    stopped at iteration `stop` (0: running): "write" the current joints, "clear" the slot back to NaN, or None (leave it)."""
    if stop == 0:
        return "write" if s // acc_steps == n else None
    if s == stop:
        return "write"
    return "clear" if s > stop else None


def device_snapshots(saves, acc_steps, stop, iterations, replays_after_stop=3):
    """The slots after a run of `iterations` (a multiple of acc_steps) as the launches leave them: one launch behind the
    initialisation, one behind every group, `replays_after_stop` more for a frame that stopped at iteration `stop` (0: never).
    A slot holds the number of optimiser steps the joints it received had been through, or None (NaN)."""
    slots = {s: None for s in saves}

    def launch(n, stopped):
        for s in saves:
            act = snapshot_action(s, acc_steps, n, stopped)
            if act == "write":
                slots[s] = n
            elif act == "clear":
                slots[s] = None
    n, it, stopped = 0, 0, 0
    launch(n, stopped)
    while it < iterations:
        end = it + acc_steps
        if stop and it < stop <= end:       # the criterion fires inside (or at the end of) this group: it steps at once
            it, stopped = stop, stop
        else:
            it = end
        n += 1
        launch(n, stopped)
        if stopped:
            for _ in range(replays_after_stop):
                launch(n, stopped)
            break
    return slots


def reference_snapshots(saves, acc_steps, stop, iterations):
    """train.py:130-233's control flow, literally: step at multiples of accumulation_steps or at the stop; save at the listed
    iterations or at the stop; break.  A saved iteration maps to the number of optimiser steps its parameters had been through."""
    saved, steps = {}, 0
    for iteration in range(1, iterations + 1):
        stopping = iteration == stop                    # early_stopping(loss) returns True at this iteration
        if iteration % acc_steps == 0 or stopping:
            steps += 1                                  # optimizer.step()
        if iteration in saves or stopping:
            saved[iteration] = steps                    # scene.save_h36m(iteration, ...)
        if stopping:
            break
    return saved
