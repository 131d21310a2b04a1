"""The device-side report (skelsplat_amd/report.py, csrc/sks_report.hip) without a device: the float64 references the GPU tests
compare against equal the host evaluator's numbers, the snapshot rule of sks_loop_report reproduces a literal model of the
reference's save / step / stop control flow, and the argument checks of the Python surface and of the C entry points refuse."""
import ctypes
import os
import re

import numpy as np
import pytest

from skelsplat_amd import _lib, io, report
from tests import report_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poses(N, P, seed):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(-3000.0, 3000.0, (N, P, 3))
    return gt + rng.normal(0.0, 40.0, (N, P, 3)), gt


@pytest.mark.parametrize("N,P", [(1, 1), (3, 17), (70, 19)])
def test_references_are_the_host_evaluator(N, P):
    pred, gt = _poses(N, P, N * 100 + P)
    pj, mean = rr.pose_errors_ref(pred, gt)
    assert pj.shape == (N, P, 2) and mean.shape == (N, 2)
    np.testing.assert_allclose(pj[..., 0].mean(), io.mpjpe(pred, gt), rtol=1e-14)
    np.testing.assert_allclose(pj[..., 1].mean(), io.mpjpe_root_relative(pred, gt), rtol=1e-14)
    for f in range(N):
        np.testing.assert_allclose(mean[f, 0], io.mpjpe(pred[f], gt[f]), rtol=1e-14)
        np.testing.assert_allclose(mean[f, 1], io.mpjpe_root_relative(pred[f], gt[f]), rtol=1e-14)
    assert (pj[:, 0, 1] == 0).all()                         # the root joint's relative error
    groups = np.arange(N) % 3
    valid = np.arange(N) % 4 != 1
    ev = rr.eval_sequence_ref(pred, gt, groups, 4, valid)
    assert ev.shape == (5, 2) and np.isnan(ev[4]).all()     # group 3 has no frames
    np.testing.assert_allclose(ev[0, 0], io.mpjpe(pred[valid], gt[valid]), rtol=1e-14)
    np.testing.assert_allclose(ev[0, 1], io.mpjpe_root_relative(pred, gt), rtol=1e-14)
    for g in range(3):
        sel = groups == g
        if sel.any():
            np.testing.assert_allclose(ev[1 + g, 1], io.mpjpe_root_relative(pred[sel], gt[sel]), rtol=1e-14)
        if (sel & valid).any():
            np.testing.assert_allclose(ev[1 + g, 0], io.mpjpe(pred[sel & valid], gt[sel & valid]), rtol=1e-14)
        else:
            assert np.isnan(ev[1 + g, 0])


def test_allowances_cover_float_arithmetic_done_on_the_host():
    """The same operations in numpy float32, in the kernel's order, stay inside the allowances (and are not far inside: the
    formulas are of the size of the arithmetic's own error, not a blanket tolerance)."""
    pred64, gt64 = _poses(50, 19, 5)
    pred, gt = pred64.astype(np.float32), gt64.astype(np.float32)
    d = pred - gt
    e_abs = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    r = (pred - pred[:, 0:1]) - (gt - gt[:, 0:1])
    e_rel = np.sqrt((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2])
    got = np.stack([e_abs, e_rel], axis=-1)
    assert got.dtype == np.float32
    want, _ = rr.pose_errors_ref(pred, gt)
    allow = rr.per_joint_allowance(pred, gt)
    assert (np.abs(got - want) <= allow).all()
    # (coordinates up to 3 000 mm: the operands of column 1's subtractions sum to < 3 x 6 x 6 000, times 2^-24)
    assert allow.max() < 3 * 6 * 6000 * rr.U32 + 1e-4
    m = got.sum(axis=1, dtype=np.float32) / np.float32(19)
    assert (np.abs(m - got.astype(np.float64).mean(axis=1)) <= rr.mean_allowance(got)).all()


SAVES = [(0, 4, 8, 12, 40), (0, 3, 10, 13, 39, 40), (1, 5, 6, 7, 9, 11)]


@pytest.mark.parametrize("acc", [4, 3])
@pytest.mark.parametrize("saves", SAVES)
def test_snapshot_rule_is_the_references_control_flow(acc, saves):
    """Per save iteration s >= 1 the slot holds what the reference's loop saved at s -- the parameters after the same number of
    optimiser steps -- or nothing where the reference saved nothing: stops inside a group, at the end of a group, never; save
    iterations that are multiples of acc_steps and that are not, one of them in the group behind the stop, one at the stop,
    one right behind it.  Iteration 0 (outside the reference's loop) is the initial joints."""
    iterations = 48                                         # a multiple of both acc_steps, past every save iteration
    stops = [0] + list(range(1, iterations + 1))
    for stop in stops:
        got = rr.device_snapshots(saves, acc, stop, iterations)
        want = rr.reference_snapshots(set(saves), acc, stop, iterations)
        for s in saves:
            if s == 0:
                assert got[0] == 0
            else:
                assert got[s] == want.get(s), (acc, saves, stop, s, got, want)
        # replays behind the stop change nothing
        assert got == rr.device_snapshots(saves, acc, stop, iterations, replays_after_stop=0)


def test_snapshot_rule_cases_by_hand():
    """acc_steps 4: iteration 10 is the state after 2 steps; a frame that stops at 9 never gets to 10 or 12; one that stops at 10
    saves its final joints there (3 steps: 4, 8 and the stop's own)."""
    assert rr.snapshot_action(10, 4, 2, 0) == "write" and rr.snapshot_action(10, 4, 3, 0) is None
    assert rr.device_snapshots((10, 12), 4, 0, 40) == {10: 2, 12: 3}
    assert rr.device_snapshots((8, 9, 10, 12), 4, 9, 40) == {8: 2, 9: 3, 10: None, 12: None}
    assert rr.device_snapshots((10, 11, 12), 4, 10, 40) == {10: 3, 11: None, 12: None}
    assert rr.device_snapshots((8, 9), 4, 8, 40) == {8: 2, 9: None}            # a stop at the end of a group
    assert rr.reference_snapshots({8, 9, 10, 12}, 4, 9, 40) == {8: 2, 9: 3}


def test_python_refusals():
    assert report.check_report_args(0, ()) == (0, ())
    assert report.check_report_args(41, [0, 4, np.int64(10)]) == (41, (0, 4, 10))
    with pytest.raises(ValueError, match="report_steps"):
        report.check_report_args(-1, ())
    with pytest.raises(ValueError, match="report_steps"):
        report.check_report_args(2.5, ())
    with pytest.raises(ValueError, match="at most 8"):
        report.check_report_args(0, range(9))
    with pytest.raises(ValueError, match="save_iterations"):
        report.check_report_args(0, (4, -1))
    import torch
    a = torch.zeros((2, 17, 3))
    with pytest.raises(ValueError, match="ROCm device"):
        report.pose_errors(a, a)
    with pytest.raises(ValueError, match="ROCm device"):
        report.evaluate_sequence(a, a)


def test_abi_tables_and_c_refusals():
    hdr = open(os.path.join(ROOT, "include", "skelsplat_hip.h")).read()
    assert int(re.search(r"#define\s+SKS_REPORT_MAX_SAVES\s+(\d+)", hdr).group(1)) == _lib.SKS_REPORT_MAX_SAVES == 8
    assert int(re.search(r"#define\s+SKS_EVAL_MAX_GROUPS\s+(\d+)", hdr).group(1)) == _lib.SKS_EVAL_MAX_GROUPS == 64
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for symbol in ("sks_pose_errors", "sks_loop_report", "sks_eval_sequence"):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % symbol, plain).group(1)
        kinds = [ctypes.c_void_p if "*" in p else ctypes.c_int for p in proto.split(",")]
        assert _lib.SIGNATURES[symbol] == (ctypes.c_int, kinds), symbol
    from skelsplat_amd import build
    assert "sks_report.hip" in build.SOURCES
    lib = _lib.load()
    x = 0x1000      # (never dereferenced: every call below is refused before anything is launched)

    def refused(fn, args, text):
        rc = fn(*args)
        assert rc < 0, (fn.__name__, args)
        assert text in lib.sks_last_error().decode(), (text, lib.sks_last_error())
    refused(lib.sks_pose_errors, (0, 17, x, x, None, x, None), "at least 1")
    refused(lib.sks_pose_errors, (2, 17, None, x, None, x, None), "pred")
    refused(lib.sks_pose_errors, (2, 17, x, None, None, x, None), "gt")
    refused(lib.sks_pose_errors, (2, 17, x, x, x, None, None), "mean")
    saves = (ctypes.c_int * 8)(0, 4, 8, 0, 0, 0, 0, 0)
    sp = ctypes.cast(saves, ctypes.c_void_p)
    ok = dict(frames=2, V=4, P=17, counters=x, es_state=None, es_window=0, xyz=x, gt=x, loss_sums=x, acc_steps=4, capacity=5,
              trace_err=x, trace_loss=x, final_err=x, K=3, save_iterations=sp, snaps=x, stream=None)
    for change, text in ((dict(frames=0), "at least 1"), (dict(counters=None), "counters"), (dict(xyz=None), "xyz"),
                         (dict(acc_steps=0), "acc_steps"), (dict(capacity=-1), "capacity"), (dict(K=9), "SKS_REPORT_MAX_SAVES"),
                         (dict(es_state=x, es_window=0), "es_window"), (dict(es_state=x, es_window=17), "es_window"),
                         (dict(final_err=None), "final_err"), (dict(trace_err=None), "trace_err"),
                         (dict(gt=None), "without gt"), (dict(loss_sums=None), "go together"),
                         (dict(trace_loss=None), "go together"), (dict(snaps=None), "snaps"),
                         (dict(save_iterations=None), "save_iterations")):
        refused(lib.sks_loop_report, tuple({**ok, **change}.values()), text)
    neg = (ctypes.c_int * 8)(0, -4, 8, 0, 0, 0, 0, 0)
    refused(lib.sks_loop_report, tuple({**ok, "save_iterations": ctypes.cast(neg, ctypes.c_void_p)}.values()), "negative")
    refused(lib.sks_eval_sequence, (0, 17, x, x, None, 0, None, x, None), "at least 1")
    refused(lib.sks_eval_sequence, (5, 17, x, x, x, 65, None, x, None), "SKS_EVAL_MAX_GROUPS")
    refused(lib.sks_eval_sequence, (5, 17, None, x, None, 0, None, x, None), "pred")
    refused(lib.sks_eval_sequence, (5, 17, x, x, None, 0, None, None, None), "out")
    refused(lib.sks_eval_sequence, (5, 17, x, x, None, 3, None, x, None), "without group_ids")
