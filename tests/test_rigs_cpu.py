"""The rig bank on the host (skelsplat_amd/rigs.py): its rows are what a one-rig loop uses, bit for bit; what it refuses; the
host restatement of the selection; the C ABI tables of the *_dv entry points against the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rigs(n=4, dataset="h36m", mixed=True):
    """n jittered ring rigs of 4 views whose rings differ in radius (so cameras_extent differs well beyond rounding); H36M
    mixes 1000- and 1002-wide sensors (views 1 and 3)."""
    from skelsplat_amd.scene import SyntheticScene, look_at_camera
    rigs = []
    for r in range(n):
        sc = SyntheticScene(dataset, n_views=4, seed=20 + r, ring=4000.0 + 700.0 * r)
        cams = sc.cameras
        if mixed:
            cams = [c if j % 2 == 0 else _resized(c, c.image_width + 2) for j, c in enumerate(cams)]
        rigs.append(cams)
    return rigs


def _resized(c, width):
    from skelsplat_amd.scene import Camera
    return Camera(c.uid, c.R, c.T, c.K, width, c.image_height)


def test_bank_rows_are_the_one_rig_loops():
    from skelsplat_amd.rigs import RigBank
    from skelsplat_amd.rasterizer import ViewBatch
    from skelsplat_amd.triangulation import device_projection_matrices
    rigs = _rigs()
    bank = RigBank(rigs)
    assert (bank.R, bank.V) == (4, 4) and bank.sizes == [(1000, 1000), (1002, 1000)] * 2
    assert bank.viewmatrix.dtype == bank.projmatrix.dtype == bank.tan.dtype == torch.float32
    assert bank.proj.dtype == bank.sched.dtype == bank.sched_log.dtype == torch.float64
    from skelsplat_amd import _lib
    for r, rig in enumerate(rigs):
        # ViewBatch.from_cameras(rig) holds exactly these (its constructor needs a ROCm device: tests/test_rigs_gpu.py compares
        # with the object itself): the stacked camera matrices and the tangents as the float arrays of the C ABI
        vm, pm, tanx, tany, sizes = ViewBatch.camera_rows(rig)
        assert torch.equal(bank.viewmatrix[r], vm) and torch.equal(bank.projmatrix[r], pm) and sizes == bank.sizes
        assert bank.tan[r, :, 0].tolist() == list(_lib.farray(tanx)) and bank.tan[r, :, 1].tolist() == list(_lib.farray(tany))
        assert torch.equal(bank.proj[r], device_projection_matrices(rig, "cpu"))
    assert not torch.equal(bank.viewmatrix[0], bank.viewmatrix[1])


def test_schedule_rows_are_training_setups():
    """Row r = what GaussianModel.training_setup and its ExponentialLR hold for spatial_lr_scale = cameras_extent(rig r)."""
    from skelsplat_amd.rigs import RigBank
    from skelsplat_amd.scene import GaussianModel, cameras_extent, skeleton_template
    rigs = _rigs()
    bank = RigBank(rigs)
    ext = [cameras_extent(rig) for rig in rigs]
    assert bank.extent == ext
    for a in range(len(ext)):
        for b in range(a + 1, len(ext)):
            assert abs(ext[a] - ext[b]) > 1e-3 * ext[a]        # far more than a rounding step: the rows really differ
    for r, rig in enumerate(rigs):
        gm = GaussianModel().create_from_points(skeleton_template("h36m"), ext[r], 17)
        gm.training_setup()
        cfg, lr = gm.opt_cfg, gm.xyz_scheduler_args
        want = [cfg["lr_init"], cfg["lr_final"], cfg["lr_delay_mult"], float(cfg["lr_delay_steps"]), float(cfg["lr_max_steps"])]
        assert bank.sched[r].tolist() == want
        assert bank.sched_log[r].tolist() == [lr.log_init, lr.log_final] + want[2:]
        assert (lr.delay_steps, lr.delay_mult, lr.max_steps) == (cfg["lr_delay_steps"], cfg["lr_delay_mult"], cfg["lr_max_steps"])


def test_zero_schedule_end_points_become_minus_infinity():
    from skelsplat_amd.rigs import RigBank
    from skelsplat_amd.scene import OptimizationParams

    class Off(OptimizationParams):
        position_lr_init = 0.0
        position_lr_final = 0.0
    bank = RigBank(_rigs(2), opt=Off)
    assert bank.sched[:, :2].abs().sum() == 0 and torch.isinf(bank.sched_log[:, :2]).all() and (bank.sched_log[:, :2] < 0).all()


def test_mismatching_rigs_are_refused():
    from skelsplat_amd.rigs import RigBank
    rigs = _rigs(3)
    bad = [list(r) for r in rigs]
    bad[2][1] = _resized(bad[2][1], 1000)                      # view slot 1 is 1002 wide in rig 0
    with pytest.raises(ValueError, match="rig 2, view 1 is 1000x1000.*fixed across rigs"):
        RigBank(bad)
    with pytest.raises(ValueError, match="same number of views"):
        RigBank([rigs[0], rigs[1][:3]])
    with pytest.raises(ValueError, match="at least one rig"):
        RigBank([])


def test_out_of_range_host_ids_are_refused():
    from skelsplat_amd.rigs import RigBank, validate_rig_ids
    bank = RigBank(_rigs(3))
    for bad in ([0, 3], [-1, 0], np.array([0, 1, 7]), torch.tensor([2, 3])):
        with pytest.raises(ValueError, match="outside the bank"):
            bank.select_host(bad)
    with pytest.raises(ValueError, match="integers"):
        validate_rig_ids([0.5, 1.0], 3)
    with pytest.raises(ValueError, match=r"must be \(4,\)"):
        validate_rig_ids([0, 1], 3, 4)
    with pytest.raises(ValueError, match="must be"):
        validate_rig_ids([[0, 1]], 3)
    assert validate_rig_ids(torch.tensor([2, 0, 1], dtype=torch.int32), 3).tolist() == [2, 0, 1]


def test_host_selection_is_indexing():
    """select_host, the host restatement of sks_rig_select: frame f holds rig ids[f]'s rows, the sizes are the slots'."""
    from skelsplat_amd.rigs import RigBank
    from skelsplat_amd.rasterizer import ViewBatch
    rigs = _rigs()
    bank = RigBank(rigs)
    ids = [3, 0, 0, 2, 1]
    sel = bank.select_host(ids)
    V = bank.V
    from skelsplat_amd import _lib
    for f, r in enumerate(ids):
        vm, pm, tanx, tany, sizes = ViewBatch.camera_rows(rigs[r])
        assert torch.equal(sel["viewmatrix"][f * V:(f + 1) * V], vm)
        assert torch.equal(sel["projmatrix"][f * V:(f + 1) * V], pm)
        assert sel["tanfovx"][f * V:(f + 1) * V].tolist() == list(_lib.farray(tanx))
        assert sel["tanfovy"][f * V:(f + 1) * V].tolist() == list(_lib.farray(tany))
        assert sel["wh"][f * V:(f + 1) * V].tolist() == [list(s) for s in sizes]
        assert torch.equal(sel["proj"][f], bank.proj[r]) and torch.equal(sel["sched_log"][f], bank.sched_log[r])


def test_loops_refuse_what_a_bank_cannot_do(monkeypatch):
    """rig_ids without a bank (the sequence helper every loop goes through), and a bank on a view-sharded loop."""
    from skelsplat_amd import loop as L
    from skelsplat_amd.rigs import RigBank
    with pytest.raises(ValueError, match="rig_ids needs a rig bank"):
        L._sequence_rig_ids(None, [0, 1], 2)
    assert L._sequence_rig_ids(None, None, 2) is None
    with pytest.raises(ValueError, match="either cameras= .* or rigs="):
        L.FrameBatchLoop(None, frames=2)
    monkeypatch.setattr(L.dist, "is_available", lambda: True)
    monkeypatch.setattr(L.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(L.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(L.dist, "get_rank", lambda group=None: 0)

    class Gm:
        _xyz = torch.zeros(17, 3)
    with pytest.raises(ValueError, match="view-sharded loop"):
        L.MultiViewLoop(Gm(), _rigs(1)[0], None, rigs=RigBank(_rigs(2)))


def test_dv_tables_are_the_headers():
    """The (parameter name, ctype) tables of the *_dv entry points and sks_rig_select in skelsplat_amd._lib are the header's
    prototypes, name for name, type for type and in order; the step entries differ from the by-value ones only in the documented
    slots; the library is the version that has them."""
    from skelsplat_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "skelsplat_hip.h")).read(), flags=re.S)
    scalars = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
               "unsigned long long": ctypes.c_ulonglong}

    def prototype(symbol):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % symbol, hdr).group(1)
        out = []
        for param in proto.split(","):
            ctype, name = re.fullmatch(r"\s*(.*?)(\w+)\s*", param, flags=re.S).groups()
            out.append((name, ctypes.c_void_p if "*" in ctype else scalars[" ".join(ctype.split())]))
        return out
    assert set(_lib.DV_PARAMS) == {"sks_rig_select", "sks_geometry_dv", "sks_heatmap_factors_dv", "sks_heatmap_totals_dv",
                                   "sks_loop_fused_step_dv", "sks_loop_fused_step_es_dv"}
    for symbol, table in _lib.DV_PARAMS.items():
        assert prototype(symbol) == list(table), symbol
        assert _lib.SIGNATURES[symbol] == (ctypes.c_int, [ct for _, ct in table])
    for dv, base, gone in (("sks_geometry_dv", "sks_geometry", ["tanfovx", "tanfovy", "view_wh"]),
                           ("sks_heatmap_factors_dv", "sks_heatmap_factors", ["tanfovx", "tanfovy", "view_wh"]),
                           ("sks_heatmap_totals_dv", "sks_heatmap_totals", ["view_wh"]),
                           ("sks_loop_fused_step_dv", "sks_loop_fused_step", ["tanfovx", "tanfovy"]),
                           ("sks_loop_fused_step_es_dv", "sks_loop_fused_step_es", ["tanfovx", "tanfovy"])):
        old = [n for n, _ in prototype(base)]
        new = [n for n, _ in _lib.DV_PARAMS[dv]]
        assert [n for n in old if n not in new] == gone + (["lr_sched"] if "step" in dv else []), dv
        assert [n for n in new if n not in old] == ["views_dev"] + (["lr_sched_dev"] if "step" in dv else []), dv
        assert [ct for _, ct in prototype(base)] == _lib.SIGNATURES[base][1]       # (the by-value entries are as they were)
    assert _lib.load().sks_version() >= 14
