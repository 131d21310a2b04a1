"""A bank of camera rigs on the device, for frame batches whose frames are seen by different cameras.

The reference hands every scene its own cameras (train.py:76; Human3.6M: one set of extrinsics per subject, Panoptic: one
calibration per activity, Occlusion-Person: one camera block per scene, triangulation.py:180), while a FrameBatchLoop built
from `cameras=` repeats ONE list of V cameras for all its frames.  A RigBank holds R rigs of V cameras each; per batch,
`rig_ids (F,)` picks one per frame and a single gather launch (sks_rig_select) fills the loop's persistent per-batch buffers
on the device, so graphs captured for one batch are replayed as they are for the next.

The bank is built ONCE, on the host, with the arithmetic a one-rig loop uses (`Camera`, `ViewBatch.from_cameras`,
`device_projection_matrices`, `cameras_extent`, `GaussianModel.training_setup`): its rows are bit for bit what
FrameBatchLoop(cameras=rig) would use, and so are the results.  What stays fixed is the image size of a view slot: sizes
decide buffer shapes and launch grids, so view j of every rig must have the same (W_j, H_j).
"""
import math

import numpy as np
import torch

from ._base import ViewBatch
from .scene import OptimizationParams, cameras_extent
from .triangulation import projection_matrices


def schedule_row(opt, spatial_lr_scale):
    """The five numbers of sks_loop_adam_step's `lr_sched` for one rig -- lr_init, lr_final, lr_delay_mult, lr_delay_steps,
    lr_max_steps -- exactly as GaussianModel.training_setup forms them for that spatial_lr_scale."""
    return (opt.position_lr_init * spatial_lr_scale, opt.position_lr_final * spatial_lr_scale,
            float(opt.position_lr_delay_mult), 0.0, float(opt.position_lr_max_steps))


def _log(x):
    """The logarithm the optimiser kernels take of a schedule end point (np.log(0) = -inf in the reference,
    general_utils.py:66; scene.ExponentialLR): libm's log, the function the library's host code calls."""
    return math.log(x) if x > 0.0 else (-math.inf if x == 0.0 else math.nan)


def validate_rig_ids(rig_ids, R, n=None):
    """Host-side ids -> int64 numpy array; refuses anything that is not `n` integers within [0, R)."""
    ids = np.asarray(rig_ids.cpu() if torch.is_tensor(rig_ids) else rig_ids)
    if ids.ndim != 1 or (n is not None and ids.shape[0] != n):
        raise ValueError(f"rig_ids must be ({'N' if n is None else n},) integers, got shape {tuple(ids.shape)}")
    if ids.dtype.kind not in "iu":
        if ids.dtype.kind != "f" or not np.all(ids == np.floor(ids)):
            raise ValueError(f"rig_ids must be integers, got {ids.dtype}")
    ids = ids.astype(np.int64)
    bad = np.nonzero((ids < 0) | (ids >= R))[0]
    if bad.size:
        raise ValueError(f"rig_ids[{int(bad[0])}] = {int(ids[bad[0]])} is outside the bank's [0, {R})")
    return ids


class RigBank:
    """R rigs of V cameras each.  `rigs`: a list of R lists of V `Camera`s; `opt`: the optimisation parameters the
    learning-rate schedule is formed from (what GaussianModel.training_setup takes).

    Host side (built here, whatever `device`): viewmatrix / projmatrix (R,V,16) fp32, tan (R,V,2) fp32 = {tan(FoVx/2),
    tan(FoVy/2)}, proj (R,V,3,4) float64 = K [R|t] or None when the cameras carry no K, extent (R,) =
    cameras_extent(rig), sched (R,5) float64 = schedule_row per rig, sched_log (R,5) = the same rows with the two end
    points replaced by their logarithms (the layout of sks_loop_fused_step_dv's lr_sched_dev), sizes = [(W_j, H_j)] per
    view slot.  `device` a ROCm device: the same tensors uploaded once, under the same names with a `_dev` suffix, plus
    wh_dev (V,2) int32."""

    def __init__(self, rigs, device=None, opt=OptimizationParams):
        rigs = [list(r) for r in rigs]
        if not rigs or not rigs[0]:
            raise ValueError("RigBank needs at least one rig of at least one camera")
        self.rigs = rigs
        self.R, self.V = len(rigs), len(rigs[0])
        self.sizes = [(int(c.image_width), int(c.image_height)) for c in rigs[0]]
        for r, rig in enumerate(rigs):
            if len(rig) != self.V:
                raise ValueError(f"rig {r} has {len(rig)} cameras, rig 0 has {self.V}: every rig needs the same number of views")
            for j, c in enumerate(rig):
                sz = (int(c.image_width), int(c.image_height))
                if sz != self.sizes[j]:
                    raise ValueError(f"rig {r}, view {j} is {sz[0]}x{sz[1]}, rig 0's view {j} is {self.sizes[j][0]}x"
                                     f"{self.sizes[j][1]}: the image size of a view slot is fixed across rigs (it decides "
                                     "buffer shapes and launch grids)")
        rows = [ViewBatch.camera_rows(rig) for rig in rigs]          # (the arithmetic of ViewBatch.from_cameras)
        self.viewmatrix = torch.stack([vm.to(device="cpu", dtype=torch.float32) for vm, *_ in rows]).contiguous()      # (R,V,16)
        self.projmatrix = torch.stack([pm.to(device="cpu", dtype=torch.float32) for _, pm, *_ in rows]).contiguous()
        # (doubles rounded to float32 once, as the ctypes float arrays of a ViewBatch round them)
        self.tan = torch.tensor([[[tx[j], ty[j]] for j in range(self.V)] for _, _, tx, ty, _ in rows], dtype=torch.float64).to(torch.float32)
        has_k = all(hasattr(c, "K") and hasattr(c, "R") and hasattr(c, "T") for rig in rigs for c in rig)
        self.proj = (torch.as_tensor(np.stack([projection_matrices(rig) for rig in rigs]), dtype=torch.float64).contiguous()
                     if has_k else None)
        self.extent = [cameras_extent(rig) for rig in rigs]
        self.sched = torch.tensor([schedule_row(opt, e) for e in self.extent], dtype=torch.float64)
        self.sched_log = self.sched.clone()
        for r in range(self.R):
            self.sched_log[r, 0] = _log(float(self.sched[r, 0]))
            self.sched_log[r, 1] = _log(float(self.sched[r, 1]))
        self.device = None
        if device is not None:
            self.to(device)

    def to(self, device):
        """Uploads the bank (once; a second call with the same device is free)."""
        device = torch.device(device)
        if self.device == device:
            return self
        self.viewmatrix_dev = self.viewmatrix.to(device)
        self.projmatrix_dev = self.projmatrix.to(device)
        self.tan_dev = self.tan.to(device)
        self.proj_dev = None if self.proj is None else self.proj.to(device)
        self.sched_log_dev = self.sched_log.to(device)
        self.wh_dev = torch.tensor(self.sizes, dtype=torch.int32).to(device)
        self.device = device
        return self

    def select_host(self, rig_ids):
        """What sks_rig_select writes for a batch, restated on the host by indexing (tests; nothing here is on the hot
        path): dict of viewmatrix / projmatrix (F*V,16), tanfovx / tanfovy (F*V,), wh (F*V,2), proj (F,V,3,4) or None,
        sched_log (F,5)."""
        ids = torch.as_tensor(validate_rig_ids(rig_ids, self.R))
        F = ids.shape[0]
        tan = self.tan[ids].reshape(F * self.V, 2)
        return dict(viewmatrix=self.viewmatrix[ids].reshape(F * self.V, 16), projmatrix=self.projmatrix[ids].reshape(F * self.V, 16),
                    tanfovx=tan[:, 0].contiguous(), tanfovy=tan[:, 1].contiguous(),
                    wh=torch.tensor(self.sizes, dtype=torch.int32).repeat(F, 1),
                    proj=None if self.proj is None else self.proj[ids], sched_log=self.sched_log[ids])


class RigSelection:
    """The persistent per-batch buffers of one FrameBatchLoop over a bank, and the launch that fills them.
    `viewmatrix` / `projmatrix`: the loop's (F*V,16) rows (its ViewBatch's own tensors), filled in place."""

    def __init__(self, bank, frames, viewmatrix, projmatrix):
        dev = viewmatrix.device
        if bank.device != dev:
            raise ValueError(f"the bank lives on {bank.device}, the loop on {dev}: RigBank(rigs, device) / bank.to(device)")
        self.bank, self.F = bank, int(frames)
        F, V = self.F, bank.V
        self.viewmatrix, self.projmatrix = viewmatrix, projmatrix
        self.table = torch.zeros((4, 64), dtype=torch.int32, device=dev)            # ViewTan: tanfovx, tanfovy, W_v, H_v
        self.proj = None if bank.proj is None else torch.zeros((F, V, 3, 4), dtype=torch.float64, device=dev)
        self.sched = torch.zeros((F, 5), dtype=torch.float64, device=dev)
        self.ids = torch.zeros(F, dtype=torch.int32, device=dev)
        # the kernel's error word: pinned host memory, read without waiting (final behind any synchronisation)
        self.error = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._error_np = self.error.numpy()

    def select(self, rig_ids):
        """`rig_ids` (F,): host data (list, array, CPU tensor) is validated here; a device tensor is taken as it is and
        bounds-checked by the kernel (check())."""
        from . import _lib
        F, bank = self.F, self.bank
        if torch.is_tensor(rig_ids) and rig_ids.device.type != "cpu":
            if rig_ids.dim() != 1 or rig_ids.shape[0] != F or rig_ids.is_floating_point():
                raise ValueError(f"rig_ids must be ({F},) integers, got {tuple(rig_ids.shape)} {rig_ids.dtype}")
            self.ids.copy_(rig_ids)
        else:
            self.ids.copy_(torch.as_tensor(validate_rig_ids(rig_ids, bank.R, F), dtype=torch.int32))
        dev = self.ids.device
        with torch.cuda.device(dev):
            rc = _lib.load().sks_rig_select(bank.R, bank.V, F, self.ids.data_ptr(), bank.viewmatrix_dev.data_ptr(),
                                            bank.projmatrix_dev.data_ptr(), bank.tan_dev.data_ptr(), bank.wh_dev.data_ptr(),
                                            _lib.ptr(bank.proj_dev), bank.sched_log_dev.data_ptr(), self.viewmatrix.data_ptr(),
                                            self.projmatrix.data_ptr(), self.table.data_ptr(), _lib.ptr(self.proj),
                                            self.sched.data_ptr(), self.error.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "sks_rig_select")

    def check(self):
        """Raises if a selection met an id outside the bank (its frame kept the cameras it had); clears the word."""
        e = int(self._error_np[0])
        if e:
            self._error_np[0] = 0
            raise RuntimeError(f"rig_ids: frame {e - 1} of a batch named a rig outside the bank's [0, {self.bank.R}); nothing "
                               "was written for it, so it ran with the cameras its slot held before")
