"""Multi-view optimisation loop of one scene (reference: train.py:130-222), MI355X layout.

What the reference does per iteration: pick view (iteration-1) % V, render it, masked-L2 against that view's heat-map
plus lambda * limb-symmetry loss, autograd.grad wrt (xyz, _scaling, _rotation, _opacity); store the xyz gradient in
slot `view` of a V-slot buffer, overwrite the other three .grad with this view's; every `accumulation_steps`
iterations: xyz.grad = mean over the V slots, Adam step.

Because the parameters only change at those steps, the views of one accumulation group are independent given the
parameters.  Here a group is ONE batched forward + ONE batched backward launch sequence (blockIdx.z = view), and
with torch.distributed the views are sharded over ranks (view v -> rank v % world): each rank renders its views and a
single all_gather of the (V_local, P, 11) per-view parameter gradients over RCCL rebuilds the V slots in view order
on every rank, so the mean uses the reference's summation order and every rank takes the identical Adam step
(no parameter broadcast).  Nothing in the group synchronises with the host.
"""
import ctypes
import os
from typing import Any, NamedTuple

import numpy as np

import torch
import torch.distributed as dist

from . import rasterizer as R
from ._group import next_group
from ._sequence import InitialJoints, JointSwitches, SequenceRun, SequenceSwitches, _checked_gt
# (callers and tests reach these as loop.<name>)
from ._sequence import _checked_reject, _debug_frames, _rejection, _sequence_predictions, _sequence_rig_ids     # noqa: F401
from .scene import DATASETS


def l2_loss_gaussian(rendering, gt_heatmap):
    """utils/loss_utils.py:86-100 ('mean' reduction): mean squared error over pixels where gt > 0 or rendering > 0."""
    mask = (gt_heatmap > 0) | (rendering > 0)
    error = (rendering - gt_heatmap) ** 2
    return error[mask].mean(), error


def limb_3d_consistency_loss(xyz, dataset):
    """utils/loss_utils.py:226-250."""
    (la0, la1), (ra0, ra1), (ll0, ll1), (rl0, rl1) = DATASETS[dataset]["limbs"]
    l_arm = torch.norm(xyz[la0] - xyz[la1], dim=-1)
    r_arm = torch.norm(xyz[ra0] - xyz[ra1], dim=-1)
    l_leg = torch.norm(xyz[ll0] - xyz[ll1], dim=-1)
    r_leg = torch.norm(xyz[rl0] - xyz[rl1], dim=-1)
    return torch.norm(l_arm - r_arm) + torch.norm(l_leg - r_leg)


def limb_consistency_observed(xyz, dataset):
    """limb_3d_consistency_loss as the loops apply it (DESIGN.md "Unobserved joints"): a pair (arms, legs) that holds a joint
    with a non-finite coordinate adds 0 to the loss and 0 to every gradient, the other pair is unaffected -- the rule of the device
    tail (sks_loop_dev.h).  The lengths of such a pair are taken from zeros in place of the missing rows, so that autograd
    never multiplies a NaN by the 0 it is weighted with.  For finite `xyz` the value and the gradient are
    limb_3d_consistency_loss's, bit for bit (the weights are 1.0)."""
    (la0, la1), (ra0, ra1), (ll0, ll1), (rl0, rl1) = DATASETS[dataset]["limbs"]
    seen = torch.isfinite(xyz).all(dim=-1)
    safe = torch.where(seen[:, None], xyz, torch.zeros_like(xyz))
    length = lambda a, b: torch.norm(safe[a] - safe[b], dim=-1)
    arms = (seen[la0] & seen[la1] & seen[ra0] & seen[ra1]).to(xyz.dtype)
    legs = (seen[ll0] & seen[ll1] & seen[rl0] & seen[rl1]).to(xyz.dtype)
    return torch.norm(length(la0, la1) - length(ra0, ra1)) * arms + torch.norm(length(ll0, ll1) - length(rl0, rl1)) * legs


def masked_l2_grad_torch(render, gt):
    """Plain-tensor-op statement of the masked-L2 gradient (device-side, no host sync); render, gt: (V,C,H,W).
    Returns (dL, per-view loss, per-view scale): the true gradient is dL * scale[v]."""
    mask = (gt > 0) | (render > 0)
    diff = render - gt
    n = mask.sum(dim=(1, 2, 3)).clamp_min(1).to(render.dtype)
    loss = (diff * diff * mask).sum(dim=(1, 2, 3)) / n
    dL = 2.0 * diff * mask
    return dL, loss, 1.0 / n


def activation_chain(gm, g):
    """Per-view gradients wrt the activated tensors -> wrt the raw parameters (what autograd does through
    exp / normalize / sigmoid in gaussian_model.py:39-47, 102-131).  g: dict of (V,P,...) tensors."""
    s = gm.get_scaling.detach()
    o = gm.get_opacity.detach()
    raw_q = gm._rotation.detach()
    nrm = raw_q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    q = raw_q / nrm
    d_scaling = g["scales"] * s[None]
    d_opacity = g["opacities"] * (o * (1 - o))[None]
    gq = g["rotations"]
    d_rotation = (gq - q[None] * (q[None] * gq).sum(-1, keepdim=True)) / nrm[None]
    return d_scaling, d_rotation, d_opacity


class OptEarlyStopping:
    """utils/general_utils.py:467-491: stop when the last `window_size` losses repeat the `window_size` before them to
    within `repeat_tolerance` (compared as fp32 tensors, like the reference's torch.tensor(list) of loss.item())."""

    def __init__(self, window_size=4, repeat_tolerance=1e-6):
        self.window_size = window_size
        self.repeat_tolerance = repeat_tolerance
        self.loss_history = []

    def __call__(self, current_loss):
        self.loss_history.append(current_loss)
        if len(self.loss_history) < 2 * self.window_size:
            return False
        w1 = torch.tensor(self.loss_history[-2 * self.window_size:-self.window_size])
        w2 = torch.tensor(self.loss_history[-self.window_size:])
        return bool(torch.all(torch.abs(w1 - w2) < self.repeat_tolerance))


class NotStopping:
    """utils/general_utils.py:493-498."""

    def __call__(self, current_loss):
        return False


early_stopping_strategy = {"opt_early_stopping": OptEarlyStopping, "no_stopping": NotStopping}   # utils/__init__.py:31-34


def _optimiser_arrays(cfg, dataset, lambda_consistency):
    """The HOST arrays of the optimiser block (`_sched`, `_lrs`, `_adam`, `_limb`) from a GaussianModel's opt_cfg."""
    sched = (ctypes.c_double * 5)(cfg["lr_init"], cfg["lr_final"], cfg["lr_delay_mult"],
                                  float(cfg["lr_delay_steps"]), float(cfg["lr_max_steps"]))
    lrs = (ctypes.c_double * 3)(cfg["lr_scaling"], cfg["lr_rotation"], cfg["lr_opacity"])
    adam = (ctypes.c_double * 3)(cfg["betas"][0], cfg["betas"][1], cfg["eps"])
    limbs = [i for pair in DATASETS[dataset]["limbs"] for i in pair]
    return sched, lrs, adam, (ctypes.c_int * 8)(*limbs) if lambda_consistency != 0.0 else None


class SizeGroup(NamedTuple):
    """One entry of a loop's `size_groups`: the local view slots of one image size, each one batched launch sequence of the dense
    path (and of the per-frame heat-map generation)."""
    slots: list     # local slots (FrameBatchLoop: frame-major)
    views: Any      # rasterizer.ViewBatch of them (None under a view_grad_fn)
    gt: Any         # their (Vg,C,H,W) pseudo-GT planes
    stats: Any      # rasterizer.GtStats of the planes, None where the sparse path is off
    idx: Any        # the slots as an index tensor on the device


class _GroupLoop(JointSwitches):
    """What MultiViewLoop and FrameBatchLoop share: run()'s groups, captured several to a hipGraph (`_enqueue`).  It calls the loop's
    own `step_group()`, `_device_group(group_mask, last_view, n_iters)` and `_all_stopped()`, and `_after_replay()` after every replay.
    Each loop also has `_optimiser_block(group_mask, last_view, n_iters)`: _lib.OPTIMISER_PARAMS of one group, tensors as tensors."""

    def _after_replay(self):
        pass

    def _init_view_weighting(self, view_weighting, view_threshold):
        """`view_weighting` = None | "scale" | "select": each view's xyz gradient weighted by its agreement with the others' in the
        optimiser step (include/skelsplat_hip.h "View agreement").  `view_weights` / `view_similarity`: the last step's, None when off."""
        from . import _lib
        self.view_weighting = view_weighting
        self._vw_mode = _lib.vw_mode(view_weighting)
        self.view_threshold = float(view_threshold)
        self.view_weights = self.view_similarity = None

    def _view_weight_args(self):
        """sparse.loop_fused_step's `view_weights`."""
        return (self._vw_mode, self.view_threshold, self.view_weights, self.view_similarity) if self._vw_mode else None

    def _enqueue(self, iterations, groups_per_graph, graphs=True):
        """run() without its final synchronisation (FramePipeline drives several loops with it).  With use_graph, while every group
        is the same one (all views, acc_steps iterations), G = `groups_per_graph` of them are ONE hipGraph: an eager group warms
        allocations and counts as a real step, G groups are captured, and the graph is replayed while G groups remain."""
        # The eager group and every replay start by refreshing the geometry from the parameters: nobody has said that they were
        # left untouched (new_scene(s), eager steps, a caller's write between two runs that capture).
        if graphs and self.use_graph and self.acc_steps % self.V == 0 and self.iteration % self.acc_steps == 0:
            key = next_group(self.iteration, self.acc_steps, self.V).key
            remaining = (iterations - self.iteration) // self.acc_steps
            G = min(int(groups_per_graph), remaining)
            if G > 1:
                if self._multi is None or self._multi[0] != (key, G):
                    self._geom_valid = False
                    self._device_group(*key)
                    self.iteration += self.acc_steps
                    remaining -= 1
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        self._geom_valid = False
                        for _ in range(G):
                            self._device_group(*key)
                    self._multi = ((key, G), graph)
                while remaining >= G and not self._all_stopped():
                    self._multi[1].replay()
                    self.iteration += G * self.acc_steps
                    remaining -= G
                    self._after_replay()
        chained = False       # (between a run's own consecutive groups nobody else touches the parameters)
        while self.iteration < iterations and not self._all_stopped():
            self.step_group(parameters_untouched=chained)
            chained = True


class MultiViewLoop(_GroupLoop):
    """One scene.  `heatmaps`: (V,C,H,W) pseudo-GT on this rank's device, or a list of V (C,H_v,W_v) tensors when the
    cameras differ in size (only the local views are read).
    `loss_grad`: callable (render, gt) -> (dL_unscaled, per-view loss, per-view scale); default: the fused HIP kernel
    (ops.masked_l2_grad_fused); loop.masked_l2_grad_torch is the same thing in tensor ops.
    `shard_views=False`: this process runs all V views itself even when torch.distributed is initialised (frame
    sharding: every rank optimises its own frames, no communication at all -- SURVEY §8e axis 2).
    `early_stopping`: a key of `early_stopping_strategy` (configs/*.yaml `training.early_stopping`), an OptEarlyStopping
    instance, or a callable loss -> bool.  The reference's criterion (OptEarlyStopping, window <= 16) runs ON THE DEVICE, inside
    the optimiser kernel (sks_loop_adam_step_es): no loss is read back, the group stays a fixed launch sequence (use_graph works,
    view-sharded ranks decide identically from the gathered sums -- they ride in the step's one all_gather), and the host learns
    the stopping iteration from a pinned flag it polls without waiting (run() synchronises once, at its end).  Any other
    callable is a host decision: one read-back per group, no use_graph.
    `view_weighting`: None (the reference's plain mean of the V slots), "scale" or "select": each view's xyz gradient is weighted
    per joint by its agreement with the other views' (utils/similarity_utils.py; DESIGN.md "View agreement"), inside the step's own
    launch on the device tail and by the same definition in tensor ops on the host tail; `view_threshold`: select's cosine
    threshold.  `view_weights` (V,P) and `view_similarity` (P,V,V) hold the last step's."""

    def __init__(self, gaussians, cameras, heatmaps, dataset="h36m", accumulation_steps=4, lambda_consistency=1e-5,
                 bg=None, antialiasing=False, loss_grad=None, group=None, view_grad_fn=None, device_tail=None,
                 use_graph=False, sparse=None, fused_tail=None, shard_views=True, graph_collectives=None,
                 early_stopping="no_stopping", rigs=None, view_weighting=None, view_threshold=0.5):
        self.gm = gaussians
        self.dataset = dataset
        self.V = len(cameras)
        self._init_view_weighting(view_weighting, view_threshold)
        self.acc_steps = int(accumulation_steps)
        self.lambda_consistency = float(lambda_consistency)
        self.antialiasing = antialiasing
        self.group = group
        sharded = bool(shard_views) and dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if sharded else 1
        self.rank = dist.get_rank(group) if sharded else 0
        if rigs is not None:
            # a rig bank selects cameras per FRAME of a batch; this loop runs one frame on one list of cameras
            if self.world > 1:
                raise ValueError("a rig bank on a view-sharded loop (world > 1): every rank holds only its own views' rows; "
                                 "rigs per frame need all views on one GPU (FrameBatchLoop / FramePipeline with rigs=)")
            raise ValueError("MultiViewLoop runs one frame on one rig (cameras=); a rig bank goes to "
                             "FrameBatchLoop(gaussians, rigs=bank, frames=F) -- frames=1 for one frame at a time")
        # the exchange step runs whenever views are sharded over a process group -- also a group of ONE rank, which is how
        # the single-GPU tests drive the very code path 8 GPUs take (RCCL all_gather included)
        self.exchange = sharded
        dev = gaussians._xyz.device
        self.device = dev
        self.local_ids = [v for v in range(self.V) if v % self.world == self.rank]
        # view_grad_fn(loop) -> ((V_local,P,11) raw-parameter gradients, per-view losses) replaces the HIP path;
        # only the multi-process CPU tests use it (gloo has no GPU), the product path is _local_view_grads.
        self.view_grad_fn = view_grad_fn
        self.cameras = cameras
        # K [R|t] of all V views, float64 on the device: new_scene(points=None) triangulates the initial joints with them
        from .triangulation import device_projection_matrices
        self._proj = device_projection_matrices(cameras, dev)
        self._reject = None                         # set_outlier_rejection's (reject_px, min_inliers)
        self._refine = None                         # set_refinement's (huber_px, max_iters)
        self.inliers = self.n_consensus = None      # new_scene(points=None) with rejection: (V,J) bool, (J,) int32, allocated once
        P = gaussians._xyz.shape[0]
        self.P = P
        self._init_heatmaps(heatmaps)
        self.bg = bg
        default_loss = loss_grad is None
        if loss_grad is None and view_grad_fn is None:
            from .ops import masked_l2_grad_fused
            loss_grad = masked_l2_grad_fused
        self.loss_grad = loss_grad
        # V-slot buffer of per-view xyz gradients (train.py:121); persists across groups (quirk Q8)
        self.accumulated_grads = torch.zeros((self.V, P, 3), device=dev)
        self.iteration = 0
        self.last_losses = None
        self.stopped_at = None       # iteration at which early stopping ended the scene (train.py:155,227-233)
        self._es_groups = 0          # groups enqueued since the scene began (view-sharded early stopping: step_group)
        # all_gather needs equal shard sizes: pad every rank to ceil(V / world) views
        self.vmax = (self.V + self.world - 1) // self.world
        # device-side tail (sks_loop_pack_grads + sks_loop_adam_step): default whenever the HIP path is used with the
        # fused loss; the tensor-op tail + torch.optim.Adam below is the same algorithm and stays for custom losses
        if device_tail is None:
            device_tail = view_grad_fn is None and default_loss and dev.type == "cuda" and P <= 256
        self.device_tail = bool(device_tail)
        if callable(early_stopping):
            self.early_stopping = early_stopping
        else:
            self.early_stopping = early_stopping_strategy[early_stopping]()
        self._stopping = not isinstance(self.early_stopping, NotStopping)
        # the reference's criterion on the device (sks_loop_adam_step_es); anything else is a host decision per group
        self._es_device = (self._stopping and type(self.early_stopping) is OptEarlyStopping and self.device_tail
                           and 1 <= self.early_stopping.window_size <= 16 and not self.early_stopping.loss_history)
        if self._stopping and not self._es_device and use_graph:
            raise ValueError("a custom early-stopping callable reads every iteration's loss on the host (train.py:155): "
                             "use_graph must be False")
        # hipGraph capture of a group that contains the RCCL all_gather: opt-in (graph_collectives=True or
        # SKS_GRAPH_COLLECTIVES=1); the sequence itself is fixed and allocation-free either way
        if graph_collectives is None:
            graph_collectives = os.environ.get("SKS_GRAPH_COLLECTIVES") == "1"
        self.use_graph = bool(use_graph) and self.device_tail and (not self.exchange or bool(graph_collectives))
        self._graphs = {}            # step_group's: (group key, chained) -> graph of one group
        self._multi = None           # run()'s: ((group key, G), graph of G groups)
        self._rows = None            # the exchange on the host's word: row of view v in a gathered table (_gathered_rows)
        # sparse fused step: render + clamp + masked-L2 + backward only on the tiles some Gaussian rect covers, using
        # per-view statistics of the constant heat-maps (sks_gt_tile_stats); no dense image / gradient is ever written
        if sparse is None:
            sparse = self.device_tail and P <= 64
        self.sparse = bool(sparse) and self.device_tail and P <= 64
        self._init_sparse_stats()
        if self.device_tail:
            self._init_device_tail()
            self._init_exchange_buffers()
        # (without the device tail -- a custom loss_grad / view_grad_fn -- the criterion is a host decision per group: the views'
        # losses ride in the gradients' all_gather as one more column, every rank feeds the same numbers in iteration order)
        # the dense step renders into fresh tensors every group: its forward's fill configuration is measured once per image size
        # (rasterizer.tune_forward; forward_views then launches with the pick) -- the library's own tuner, no caller-side knob
        if view_grad_fn is None and dev.type == "cuda" and not self.sparse and R.AUTOTUNE and P <= 256:
            with torch.no_grad():
                feats = gaussians.get_features.reshape(P, -1)
                for slots, vb, gt, _, idx in self.size_groups:
                    R.tune_forward(vb, gaussians._xyz.detach(), feats, gaussians.get_opacity.detach(), gaussians.get_scaling.detach(),
                                   gaussians.get_rotation.detach(), None, antialiasing=self.antialiasing, clamp01=True)
        self._init_fused_tail(fused_tail)

    # -- the constructor's steps, in the order they run ------------------------------------------------------------
    def _init_heatmaps(self, heatmaps):
        """Heat-map layout and size groups."""
        # Local heat-maps live in ONE flat buffer (rasterizer.HeatmapSet): views of one size are adjacent -- a (Vg,C,H,W)
        # tensor for the dense entry points -- and the sparse fused step addresses all of them, whatever their sizes,
        # through per-view offsets in a single launch (H36M mixes 1000x1000 and 1002x1000 sensors, quirk Q11).
        cameras, Vl = self.cameras, len(self.local_ids)
        sizes = [(int(cameras[v].image_width), int(cameras[v].image_height)) for v in self.local_ids]
        if torch.is_tensor(heatmaps) and heatmaps.dim() == 4 and Vl == self.V and heatmaps.is_contiguous() \
                and heatmaps.dtype == torch.float32 and len(set(sizes)) == 1:
            self.hset = R.HeatmapSet.adopt(heatmaps)            # all views local, one size: no copy
        elif Vl:
            C_hm = int(heatmaps[self.local_ids[0]].shape[0])
            self.hset = R.HeatmapSet(sizes, C_hm, heatmaps[self.local_ids[0]].device)
            for k, v in enumerate(self.local_ids):
                self.hset.planes[k].copy_(heatmaps[v])
        else:
            self.hset = None
        self.size_groups = []       # SizeGroup per image size
        if self.hset is not None:
            for key, slots in self.hset.groups.items():
                vb = (R.ViewBatch.from_cameras([cameras[self.local_ids[k]] for k in slots]) if self.view_grad_fn is None else None)
                idx = torch.tensor(slots, dtype=torch.long, device=self.device)
                self.size_groups.append(SizeGroup(slots, vb, self.hset.group(key), None, idx))
        single = len(self.size_groups) == 1
        self.gt = self.size_groups[0].gt if single else None   # single-size convenience (tests, view_grad_fn)
        self.views = self.size_groups[0].views if single else None

    def _init_sparse_stats(self):
        """Sparse path: the heat-maps' statistics per size group, and ALL local views in one batch (sizes may differ)."""
        self.views_all = self.stats_all = None
        if self.sparse and self.local_ids:
            self.size_groups = [grp._replace(stats=R.gt_tile_stats(grp.gt)) for grp in self.size_groups]
            if len(self.size_groups) == 1:
                self.views_all, self.stats_all = self.size_groups[0].views, self.size_groups[0].stats
            else:
                self.views_all = R.ViewBatch.from_cameras([self.cameras[v] for v in self.local_ids], allow_mixed=True)
                self.stats_all = R.GtStats.of_set(self.hset)
                self._merge_totals()

    def _init_device_tail(self):
        """The optimiser's state on the device (sks_loop_adam_step), and the criterion's when it runs there."""
        P, dev = self.P, self.device
        self._sched, self._lrs, self._adam, self._limb = _optimiser_arrays(self.gm.opt_cfg, self.dataset, self.lambda_consistency)
        self.exp_avg = torch.zeros((P, 11), device=dev)
        self.exp_avg_sq = torch.zeros((P, 11), device=dev)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)
        if self._vw_mode:       # the step's own launch writes them (persistent: a captured graph keeps their addresses)
            self.view_weights = torch.zeros((self.V, P), device=dev)
            self.view_similarity = torch.zeros((P, self.V, self.V), device=dev)
        self._es_state = self._es_flag = None
        if self._es_device:
            w = self.early_stopping.window_size
            self._es_state = torch.zeros(2 + 2 * w, dtype=torch.int32, device=dev)
            self._es_flag = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._es_flag_np = self._es_flag.numpy()

    def _init_exchange_buffers(self):
        """The group's gradient and loss buffers, and the exchange's."""
        # persistent buffers of the group (allocated here, never inside a graph capture): this rank's packed
        # raw-parameter gradients -- with the exchange padded to vmax rows, the pad rows stay zero for ever -- and what
        # all_gather_into_tensor leaves, which sks_loop_adam_step reads in place (rank-major layout, `shard_world`)
        P, dev, Vl = self.P, self.device, len(self.local_ids)
        if self.exchange and self._es_device:
            # a rank's block = its vmax x P x 11 gradient rows (padded to an even float count) + its views' {S, N} doubles:
            # gradients and losses cross in ONE all_gather, every rank runs the same criterion (sks_loop_shard_floats)
            from . import _lib
            nfl = int(_lib.load().sks_loop_shard_floats(self.V, P, self.world))
            tail = nfl - 4 * self.vmax
            self._shard_flat = torch.zeros(nfl, device=dev)
            self._shard = self._shard_flat[:self.vmax * P * 11].view(self.vmax, P, 11)
            self._sums = self._shard_flat[tail:].view(torch.float64).view(self.vmax, 2)
            self._allg = torch.empty(self.world * nfl, device=dev)
        else:
            self._shard_flat = None
            self._shard = torch.zeros((self.vmax if self.exchange else max(Vl, 1), P, 11), device=dev)
            self._allg = torch.empty((self.world * self.vmax, P, 11), device=dev) if self.exchange else None
            self._sums = torch.zeros((max(Vl, 1), 2), dtype=torch.float64, device=dev)
        self._sums_all = (torch.zeros((self.world * self.vmax, 2), dtype=torch.float64, device=dev)
                          if self.exchange and self._stopping and not self._es_device else None)
        self._direct = None
        if self.exchange:
            # RCCL builds its communicator on the first collective: do that here, eagerly, never inside a graph
            # capture or a timed step (the gathered rows are overwritten by every group)
            dist.all_gather_into_tensor(self._allg, self._shard if self._shard_flat is None else self._shard_flat, group=self.group)
            # ... and, when asked for (SKS_RCCL_DIRECT=1), a communicator of our own, so that the group's one all_gather is
            # enqueued on the stream its neighbours run on (torch's process group runs it on an internal stream: two event
            # hand-overs, ~7 us of the GPU timeline per step at world 1); None by default and when the backend is not RCCL
            if dev.type == "cuda":
                from .rccl_direct import DirectGather
                self._direct = DirectGather.create(dev, self.group)

    def _init_fused_tail(self, fused_tail):
        """The fused tail: whether it runs, and its persistent geometry."""
        # one GPU, sparse step: the whole group is two launches (sks_loop_fused_step); the geometry of the current
        # parameters lives in a persistent state that every step leaves up to date for the next one
        # (the single-workgroup tail walks the views four at a time: a win for a handful of views -- H36M's 4 --, a loss
        # for Panoptic's 31, where the one-block-per-view kernels stay)
        self.fused_tail = (self.sparse and not self.exchange and len(self.local_ids) > 0 and self.bg is None and not self._stopping
                           and (fused_tail is True or (fused_tail is None and self.V <= 8)))
        self._fstate = None          # persistent ForwardState (geom + radii) of the fused tail
        self._geom_valid = False     # does it describe the current parameters?
        if self.fused_tail:          # persistent buffers are allocated here, never inside a graph capture
            with torch.no_grad():
                self._refresh_geometry()
            self._fbuf = (self._shard, self._sums)

    # -- the reference's debug pictures (train.py:279-304, `debug.save_images`) of the loop's current scene --------
    def _local_pictures(self, pictures_of):
        """(V_local,H,W) uint8 from `pictures_of(slots, views, planes)` per size group: H, W the largest local view, a smaller
        view in the leading part of its slab."""
        if len(self.size_groups) == 1:
            return pictures_of(*self.size_groups[0][:3])
        W, H = max(w for w, _ in self.hset.sizes), max(h for _, h in self.hset.sizes)
        out = torch.zeros((len(self.local_ids), H, W), dtype=torch.uint8, device=self.device)
        for slots, vb, gt, _, idx in self.size_groups:
            out[idx, :gt.shape[2], :gt.shape[3]] = pictures_of(slots, vb, gt)
        return out

    def _save_local(self, directory, name, pictures):
        from .io import write_png_gray
        host = pictures.cpu().numpy()
        for k, v in enumerate(self.local_ids):      # (view-sharded: every rank writes its own views' files)
            w, h = self.hset.sizes[k]
            write_png_gray(os.path.join(directory, f"{name}_{v}.png"), host[k, :h, :w])
        return pictures

    def save_heatmaps(self, output_dir, name="heatmap"):
        """train.py:294-304 for the current scene: {output_dir}/heatmaps/{name}_{view}.png, the channel sum of each local view's
        pseudo-GT planes, min-max normalised, 8-bit grey (preview.channel_sum_u8).  Returns the (V_local,H,W) uint8 pictures on
        the device.  Reads them back once; the loop's state is not touched."""
        from .preview import channel_sum_u8
        if self.hset is None:
            raise ValueError("save_heatmaps: this rank holds no view")
        with torch.no_grad():
            pictures = self._local_pictures(lambda slots, vb, gt: channel_sum_u8(gt))
        return self._save_local(os.path.join(output_dir, "heatmaps"), name, pictures)

    def save_images(self, output_dir, name="render"):
        """train.py:279-291 for the current parameters: {output_dir}/images/{name}_{view}.png, each local view rendered over a
        black background, clamped to [0, 1], channels summed, min-max normalised, 8-bit grey (preview.render_preview: a
        workspace of its own -- the loop's recorded plans and captured graphs are not touched).  name="render_1" after the first
        iteration is the reference's other call.  Returns the (V_local,H,W) uint8 pictures on the device."""
        from .preview import render_preview
        if self.hset is None or self.view_grad_fn is not None:
            raise ValueError("save_images: this rank renders no view")
        gm, P = self.gm, self.P
        with torch.no_grad():
            args = (gm._xyz.detach(), gm.get_scaling.detach(), gm.get_rotation.detach(), gm.get_opacity.detach(),
                    gm.get_features.detach().reshape(P, -1))
            pictures = self._local_pictures(lambda slots, vb, gt: render_preview(vb, *args, antialiasing=self.antialiasing))
        return self._save_local(os.path.join(output_dir, "images"), name, pictures)

    def _refresh_geometry(self):
        """The fused tail's persistent geometry from the parameters as they are now (in place once it exists)."""
        gm = self.gm
        self._fstate = R.geometry_views(self.views_all, gm._xyz.detach(), gm.get_features.reshape(self.P, -1).shape[1], gm._opacity,
                                        gm._scaling, gm._rotation, None, antialiasing=self.antialiasing, raw_params=True,
                                        out=self._fstate)

    def _merge_totals(self):
        """Mixed sizes: the per-size-group heat-map totals -> the (V_local,2) table of the all-views batch."""
        for slots, vb, gt, stats, idx in self.size_groups:
            self.stats_all.totals.index_copy_(0, idx, stats.totals)

    # -- scene streaming ---------------------------------------------------------------------------------------
    def new_scene(self, points, poses_2d=None, heatmaps=None, dropout=False, poses_3d=None):
        """Next frame seen by the SAME cameras (the reference's outer loop, train.py:74-99: new GaussianModel, new
        heat-maps, iteration counter back to 0).  Everything is re-initialised in place -- parameters, Adam moments,
        step counters, V-slot buffer, heat-maps and their tile statistics keep their storage -- so the hipGraphs
        captured for the previous frame are replayed as they are.  Give either `poses_2d` (V,J,2) (the heat-maps are
        generated from the re-initialised Gaussians like general_utils.py:175-304) or ready `heatmaps`.
        `points=None`, optionally with `poses_3d` (V,J,3): the initial joints are estimated from the detections as
        FrameBatchLoop.new_scenes says, for this one frame, on the device, on the current stream, bit for bit what that frame gets
        in a batch; with `dropout` the dropped planes' detections stay out of it.  It needs all V views' detections, so a
        view-sharded loop (world > 1) refuses it; a joint that comes out NaN is then UNOBSERVED for the whole loop, on every
        path of this class (DESIGN.md "Unobserved joints").  The same holds for a NaN row of explicit `points`.
        After `set_outlier_rejection` the views each joint was solved from are in `self.inliers` (V,J) bool, the consensus
        counts in `self.n_consensus` (J,) int32; `set_refinement` acts here as it does there."""
        from .heatmaps import generate_heatmaps
        gm = self.gm
        plan = InitialJoints.check("new_scene", points, poses_2d, poses_3d, (None, self.V, self.P), self._reject, self._refine,
                                   self._proj, self.device)
        if plan.estimated and self.world > 1:
            raise ValueError("new_scene(points=None): a view-sharded loop (world > 1) sees only its own views' "
                             "detections; triangulate on one rank (triangulation.triangulate_sequence) and pass points")
        with torch.no_grad():
            self.accumulated_grads.zero_()
            if self.device_tail:
                self.exp_avg.zero_()
                self.exp_avg_sq.zero_()
                self.counters.zero_()
            elif gm.optimizer is not None:
                gm.training_setup()
            drop = None
            if dropout and poses_2d is not None:
                from .heatmaps import draw_dropout
                drop = draw_dropout(self.V, self.P)
                if self.exchange and self.world > 1:
                    # the reference makes ONE draw shared by all cameras (general_utils.py:267-283); the ranks' default
                    # generators are not synchronised, so rank 0's draw is the scene's
                    buf = drop.to(device=self.device, dtype=torch.uint8)
                    dist.broadcast(buf, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0,
                                   group=self.group)
                    drop = buf.to(device="cpu", dtype=torch.bool)
            if not plan.estimated:
                gm.reset_from_points(plan.points[0])
            else:
                if plan.reject[0] is not None and self.inliers is None:
                    self.inliers = torch.zeros((self.V, self.P), dtype=torch.bool, device=self.device)
                    self.n_consensus = torch.zeros((self.P,), dtype=torch.int32, device=self.device)
                pts = torch.empty((self.P, 3), dtype=torch.float32, device=self.device)
                gm.reset_from_points(plan.write(None if drop is None else ~drop, pts, (self.inliers, self.n_consensus)))
            for slots, vb, gt, stats, idx in self.size_groups:
                ids = [self.local_ids[k] for k in slots]
                if heatmaps is not None:
                    for i, v in enumerate(ids):
                        gt[i].copy_(heatmaps[v])
                elif poses_2d is not None:
                    p2d = torch.as_tensor(poses_2d, device=self.device)[ids]
                    # the planes and (when the sparse path wants them) their per-view totals in one pass
                    fused = stats is not None and stats.tile_S is None
                    generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(), p2d,
                                      [self.cameras[v] for v in ids], out=gt, views=vb,
                                      totals=stats.totals if fused else None,
                                      drop_mask=None if drop is None else drop[ids])
                    if fused:
                        continue
                else:
                    raise ValueError("new_scene needs poses_2d or heatmaps")
                if stats is not None:
                    R.gt_tile_stats(gt, out=stats)
            if self.sparse and len(self.size_groups) > 1:
                self._merge_totals()
        if self.device_tail and self._es_device:
            torch.cuda.current_stream(self.device).synchronize()    # (nothing of the last scene may still write the flag)
            self._es_state.zero_()
            self._es_flag_np[0] = 0
        elif isinstance(self.early_stopping, (OptEarlyStopping, NotStopping)):
            self.early_stopping = type(self.early_stopping)()
        self.stopped_at = None
        self._es_groups = 0
        self._geom_valid = False
        self.iteration = 0    # (last_losses keeps pointing at the buffers the captured graphs write)
        return self

    # -- one accumulation group --------------------------------------------------------------------------
    def _local_view_grads(self):
        """Renders this rank's views and returns (V_local, P, 11) raw-parameter gradients + per-view losses."""
        gm = self.gm
        P = self.P
        with torch.no_grad():
            means = gm._xyz.detach()
            feats = gm.get_features.reshape(P, -1)
            opac = gm.get_opacity.detach()
            scales = gm.get_scaling.detach()
            quats = gm.get_rotation.detach()
            packed = torch.empty((len(self.local_ids), P, 11), device=means.device)
            losses = torch.empty(len(self.local_ids), device=means.device)
            for slots, vb, gt, _, idx in self.size_groups:
                color, inv, radii, st = R.forward_views(vb, means, feats, opac, scales, quats, None,
                                                        antialiasing=self.antialiasing, clamp01=True)
                dL, lv, scale = self.loss_grad(color, gt)
                g = R.backward_views(st, means, feats, opac, scales, quats, None, dL, None, bg=self.bg)
                d_scaling, d_rotation, d_opacity = activation_chain(gm, g)
                pk = torch.cat([g["means3D"], d_scaling, d_rotation, d_opacity], dim=-1)  # (Vg, P, 11)
                packed.index_copy_(0, idx, pk * scale[:, None, None])   # 1 / N_mask of each view (the backward is linear in dL)
                losses.index_copy_(0, idx, lv.to(losses.dtype))
        return packed, losses

    def _consistency_grad(self):
        xyz = self.gm._xyz.detach().clone().requires_grad_(True)
        loss = limb_consistency_observed(xyz, self.dataset) * self.lambda_consistency
        (gx,) = torch.autograd.grad(loss, xyz)
        return gx, loss.detach()

    # -- device-side tail ----------------------------------------------------------------------------------
    def _device_grads(self):
        """This rank's views -> self._shard[:V_local] (packed raw-parameter gradients) and self._sums ({S, N} per view):
        a fixed, allocation-light launch sequence (sparse: sks_geometry + sks_backward_fused_loss for ALL local views,
        whatever their sizes; dense: forward + masked-L2 + backward + pack per size group)."""
        from . import _lib
        from .ops import masked_l2
        lib = _lib.load()
        gm, P, dev = self.gm, self.P, self.device
        Vl = len(self.local_ids)
        stream = torch.cuda.current_stream(dev).cuda_stream
        means = gm._xyz.detach()
        feats = gm.get_features.reshape(P, -1)
        packed = self._shard[:Vl]
        if self.sparse:
            # leaf parameters straight into the kernels: activations, their Jacobians and the 1/N scale all run inside
            # sks_geometry / sks_backward_fused_loss (SKS_RAW_PARAMS)
            st = R.geometry_views(self.views_all, means, feats.shape[1], gm._opacity, gm._scaling, gm._rotation, None,
                                  antialiasing=self.antialiasing, raw_params=True)
            R.backward_fused_loss(st, self.stats_all, means, feats, gm._opacity, gm._scaling, gm._rotation, None,
                                  bg=self.bg, packed_out=packed, sums_out=self._sums)
            return
        opac, scales, quats = gm.get_opacity.detach(), gm.get_scaling.detach(), gm.get_rotation.detach()
        single = len(self.size_groups) == 1
        for slots, vb, gt, stats, idx in self.size_groups:
            color, inv, radii, st = R.forward_views(vb, means, feats, opac, scales, quats, None,
                                                    antialiasing=self.antialiasing, clamp01=True)
            dL, S, N = masked_l2(color, gt)
            g = R.backward_views(st, means, feats, opac, scales, quats, None, dL, None, bg=self.bg)
            sums = torch.stack([S, N], dim=1).contiguous()
            Vg = len(slots)
            pk = packed if single else torch.empty((Vg, P, 11), device=dev)
            _lib.check(lib.sks_loop_pack_grads(Vg, P, g["means3D"].data_ptr(), g["scales"].data_ptr(),
                                               g["rotations"].data_ptr(), g["opacities"].data_ptr(),
                                               gm._scaling.data_ptr(), gm._rotation.data_ptr(), gm._opacity.data_ptr(),
                                               sums.data_ptr(), pk.data_ptr(), stream), "sks_loop_pack_grads")
            if not single:
                packed.index_copy_(0, idx, pk)
            self._sums[:Vl].index_copy_(0, idx, sums)

    def _device_adam(self, group_mask, last_view, n_iters):
        """[all_gather of the shards ->] sks_loop_adam_step on the view-major (one rank) or rank-major (gathered) table."""
        from . import _lib
        lib = _lib.load()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.exchange:
            # every rank needs every view's gradients (train.py:175, 215-218): ONE all_gather of the padded shards over
            # RCCL; the optimiser kernel reads the gathered buffer in place (view v = row (v % world) * vmax + v // world)
            src = self._shard if self._shard_flat is None else self._shard_flat
            if self._direct is not None:
                self._direct.all_gather_into_tensor(self._allg, src)     # RCCL on THIS stream (rccl_direct.py)
            else:
                dist.all_gather_into_tensor(self._allg, src, group=self.group)
            full, world = self._allg, self.world
        else:
            full, world = self._shard, 1
        block = self._optimiser_block(group_mask, last_view, n_iters)      # (this entry point takes its tensors as pointers)
        args = (self.V, self.P, full.data_ptr(), *[a.data_ptr() if torch.is_tensor(a) else a for a in block], world)
        step, what = lib.sks_loop_adam_step, "sks_loop_adam_step"
        if self._es_device:
            es = self.early_stopping
            step, what = lib.sks_loop_adam_step_es, "sks_loop_adam_step_es"
            args += (None if world > 1 else self._sums.data_ptr(), self._es_state.data_ptr(), int(es.window_size),
                     float(es.repeat_tolerance), self._es_flag.data_ptr())
        if self._vw_mode:       # (one entry for both forms: es_state == NULL is the step without a criterion)
            if not self._es_device:
                args += (None, None, 0, 0.0, None)
            step, what = lib.sks_loop_adam_step_vw, "sks_loop_adam_step_vw"
            args += (self._vw_mode, self.view_threshold, self.view_weights.data_ptr(), self.view_similarity.data_ptr())
        _lib.check(step(*args, stream), what)

    def _optimiser_block(self, group_mask, last_view, n_iters):
        gm = self.gm
        return (self.accumulated_grads, group_mask, last_view, gm._xyz, gm._scaling, gm._rotation, gm._opacity, self.exp_avg,
                self.exp_avg_sq, self.counters, n_iters, self._sched, self._lrs, self._adam, self.lambda_consistency, self._limb)

    def _device_group(self, group_mask, last_view, n_iters, grp=None):
        """forward -> fused masked-L2 -> backward -> pack -> [all_gather] -> Adam, all enqueued, no host sync.
        `grp`: the Group the key is of; step_group hands it over for a host criterion, which may cut it."""
        gm, P = self.gm, self.P
        with torch.no_grad():
            if self.fused_tail:
                feats = gm.get_features.reshape(P, -1)
                if not self._geom_valid:
                    self._refresh_geometry()
                    self._geom_valid = True
                packed, sums = self._fbuf
                R.loop_fused_step(self._fstate, self.stats_all, feats, packed, sums,
                                  *self._optimiser_block(group_mask, last_view, n_iters), view_weights=self._view_weight_args())
                self.last_losses = (sums[:, 0], sums[:, 1])
                return
            if self.local_ids:
                self._device_grads()
                Vl = len(self.local_ids)
                self.last_losses = (self._sums[:Vl, 0], self._sums[:Vl, 1])
            if self._stopping and not self._es_device:
                group_mask, last_view, n_iters = self._early_stop_cut(grp)
            self._device_adam(group_mask, last_view, n_iters)

    ES_SYNC_GROUPS = 8      # view-sharded ranks look at the device criterion's flag every this many groups (step_group)

    def _poll_stop(self, wait=False):
        """Device-side criterion: has it fired?  The kernel stores the stopping iteration into pinned host memory; `wait`
        first lets the stream drain (run() does, once, when it has enqueued everything it was asked for)."""
        if wait:
            torch.cuda.current_stream(self.device).synchronize()
        it = int(self._es_flag_np[0])
        if it:
            self.stopped_at = it
            self.iteration = it
        return self.stopped_at

    def _early_stop_cut(self, grp):
        """train.py:155-233 with the group's views batched: feed the criterion the losses of the group's iterations in
        order; if it fires at the k-th, only the first k views' slots are refreshed, view k's scaling / rotation /
        opacity gradients win, the optimiser steps at once and the scene ends.  One host sync per group.  Returns the key of the
        group that steps: `grp`'s, cut where the criterion fired."""
        Vl = len(self.local_ids)
        if self.exchange:
            pad = torch.zeros((self.vmax, 2), dtype=torch.float64, device=self.device)
            pad[:Vl] = self._sums[:Vl]
            dist.all_gather_into_tensor(self._sums_all, pad, group=self.group)
            sums = self._sums_all.index_select(0, self._gathered_rows()).cpu()
        else:
            sums = self._sums[:Vl].cpu()
        l2 = (sums[:, 0] / sums[:, 1].clamp_min(1.0)).to(torch.float32)
        cons = torch.zeros((), dtype=torch.float32)
        if self.lambda_consistency != 0.0:
            cons = (limb_consistency_observed(self.gm._xyz.detach(), self.dataset) * self.lambda_consistency).float().cpu()
        return self._cut_where_stopped(grp, l2, cons).key

    def _gathered_rows(self):
        """rank r, slot k  <->  view r + k * world: the row of every view in a gathered table, in view order (built once)."""
        if self._rows is None:
            self._rows = torch.tensor([(v % self.world) * self.vmax + v // self.world for v in range(self.V)],
                                      dtype=torch.long, device=self.device)
        return self._rows

    def _cut_where_stopped(self, grp, l2, cons):
        """The host criterion sees the losses of the group's iterations in order; where it fires, the group is cut and the scene ends."""
        for k, v in enumerate(grp.views):
            if self.early_stopping(float(l2[v] + cons)):
                grp = grp.cut(k)
                self.stopped_at = grp.end
                break
        return grp

    def step_group(self, parameters_untouched=False):
        """Runs iterations self.iteration+1 .. up to the next optimiser step (train.py:130-222).
        parameters_untouched=True: the caller states that nothing has written the parameters since this object's previous
        step_group() -- the fused step's tail left the geometry of the updated parameters behind, and this step then starts from
        it instead of launching a geometry pass of its own (what run() does between its own consecutive groups, and what a
        captured graph of several groups does inside).  There is no way to see a write through `.data` or a raw pointer from here,
        so the default is to recompute."""
        gm = self.gm
        if self.stopped_at is not None:
            return self.iteration
        grp = next_group(self.iteration, self.acc_steps, self.V)
        if self.device_tail:
            if self.use_graph:
                # (two graphs per group shape: one that first refreshes the geometry from the parameters, one -- replayed on the
                # caller's word, parameters_untouched -- that starts from what the previous group's tail left)
                chained = bool(parameters_untouched and self.fused_tail and self._geom_valid)
                gkey = grp.key + (chained,)
                if self._graphs.get(gkey) is None:
                    # capture one group; replays advance the device counters themselves
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        if not chained:
                            self._geom_valid = False    # (see _enqueue: a replay never assumes who ran before it)
                        self._device_group(*grp.key)
                    self._graphs[gkey] = graph          # the capture itself does not execute: replay below
                self._graphs[gkey].replay()
            else:
                if not parameters_untouched:
                    self._geom_valid = False    # eager steps never assume the parameters were left untouched since the last one
                self._device_group(*grp.key, grp)
            if self._es_device:
                if self.exchange and self.world > 1:
                    # Sharded: every group holds a collective, so every rank must enqueue the SAME number of groups.  A free-running
                    # poll would not give that -- each host runs ahead of its GPU by its own amount and would see the flag a
                    # different number of groups late.  So the flag is only looked at behind a stream synchronisation, every
                    # ES_SYNC_GROUPS-th group: there the state the criterion ran on (gathered sums, es_state) is the same on
                    # every rank, and so is what each of them reads.
                    self._es_groups += 1
                    if self._es_groups % self.ES_SYNC_GROUPS == 0:
                        self._poll_stop(wait=True)
                else:
                    self._poll_stop()       # (never waits: the groups enqueued behind a stop do nothing to the parameters)
            self.iteration = grp.end if self.stopped_at is None else self.stopped_at
            return self.iteration
        if not self.local_ids:
            packed, losses = None, None
        elif self.view_grad_fn is not None:
            packed, losses = self.view_grad_fn(self)
        else:
            packed, losses = self._local_view_grads()
        dev = self.device
        n11 = self.P * 11
        if self.exchange:
            # ONE collective per group here too: a rank's block = its views' gradient rows, each followed by that view's loss
            shard = torch.zeros((self.vmax, n11 + 1), device=dev)
            if packed is not None:
                shard[:packed.shape[0], :n11] = packed.reshape(packed.shape[0], n11)
                shard[:packed.shape[0], n11] = losses.to(shard.dtype)
            allg = torch.empty((self.world * self.vmax, n11 + 1), device=dev)
            dist.all_gather_into_tensor(allg, shard, group=self.group)
            rows = allg.index_select(0, self._gathered_rows())
            full, losses_all = rows[:, :n11].reshape(self.V, self.P, 11), rows[:, n11]
        else:
            full, losses_all = packed, losses
        gcons, lcons = self._consistency_grad() if self.lambda_consistency != 0.0 else (0.0, None)
        if self._stopping:
            # train.py:155-233 with the group's views batched: the criterion sees the losses of the group's iterations in order;
            # if it fires at the k-th, only the first k views' slots are refreshed, view k's scaling / rotation / opacity
            # gradients win, the optimiser steps at once and the scene ends (the same numbers on every rank: the same decision)
            l2 = losses_all.detach().to(torch.float32).cpu()
            cons = torch.zeros((), dtype=torch.float32) if lcons is None else lcons.detach().to(torch.float32).cpu()
            grp = self._cut_where_stopped(grp, l2, cons)
        # every view's loss contains the consistency term, so every slot carries its gradient (train.py:150-152,175)
        for v in dict.fromkeys(grp.views):
            self.accumulated_grads[v] = full[v, :, 0:3] + gcons
        last = grp.last_view                                               # quirk Q7: last view's grads win
        if gm._xyz.grad is None:
            for p in (gm._xyz, gm._scaling, gm._rotation, gm._opacity):
                p.grad = torch.zeros_like(p)
        gm._scaling.grad = full[last, :, 3:6].contiguous()
        gm._rotation.grad = full[last, :, 6:10].contiguous()
        gm._opacity.grad = full[last, :, 10:11].contiguous()
        if self._vw_mode:                                                  # the same definition as the device tail's, in tensor ops
            from .view_agreement import weighted_mean
            gm._xyz.grad, self.view_weights, self.view_similarity = weighted_mean(self.accumulated_grads, self.view_weighting,
                                                                                   self.view_threshold)
        else:
            gm._xyz.grad = self.accumulated_grads.mean(dim=0)              # train.py:215-218
        gm.update_learning_rate(grp.end)                                   # quirk Q9: schedule indexed by iteration
        with torch.no_grad():
            gm.optimizer.step()
            gm.optimizer.zero_grad(set_to_none=True)
        self.iteration = grp.end
        self.last_losses = losses
        return grp.end

    def _all_stopped(self):
        return self.stopped_at is not None

    def _after_replay(self):
        if self._es_device:
            self._poll_stop(wait=self.exchange and self.world > 1)     # (sharded: see step_group)

    def run(self, iterations=500, groups_per_graph=25):
        """Runs the loop up to `iterations`.  With use_graph, `groups_per_graph` consecutive accumulation groups are
        captured into ONE hipGraph (the step has no host state: counters, LR schedule and Adam live on the device), so
        a 500-iteration scene is a handful of graph launches."""
        self._enqueue(iterations, groups_per_graph, graphs=self.stopped_at is None)
        if self.device_tail and self._es_device and self.stopped_at is None:
            self._poll_stop(wait=True)      # the ONE synchronisation of a scene with the criterion on the device
        return self.gm._xyz.detach()


def _frame_criterion(early_stopping):
    """FrameBatchLoop's `early_stopping` -> None (off) or (window, tolerance) of the reference's criterion, which the frame
    batch runs per frame on the device; anything else is refused."""
    es = early_stopping
    if isinstance(es, str):
        if es not in early_stopping_strategy:
            raise ValueError(f"early_stopping = {es!r}: expected one of {sorted(early_stopping_strategy)}")
        es = early_stopping_strategy[es]()
    if type(es) is NotStopping:
        return None
    if type(es) is not OptEarlyStopping:
        raise ValueError("FrameBatchLoop runs the early-stopping criterion per frame on the device: it takes "
                         "'opt_early_stopping' or an OptEarlyStopping; a host-side callable needs MultiViewLoop")
    w = es.window_size
    if not isinstance(w, (int, np.integer)) or not 1 <= int(w) <= 16:
        raise ValueError(f"OptEarlyStopping.window_size = {w!r}: the device criterion keeps 1 .. 16")
    if es.loss_history:
        raise ValueError("OptEarlyStopping has a loss history already: every frame starts from an empty one")
    return int(w), float(es.repeat_tolerance)


class FrameBatchLoop(_GroupLoop, SequenceSwitches):
    """F independent frames, optimised side by side in the sparse fused step -- seen by the SAME cameras (`cameras=`), or each
    by one rig of a bank (`rigs=` a rigs.RigBank; then `new_scenes(..., rig_ids=)` names every frame's rig).

    The reference optimises one frame after the other (train.py:74-99: a fresh GaussianModel and fresh heat-maps per
    scene, nothing carried over), and one 17-Gaussian skeleton keeps only a fraction of an MI355X busy: the fused
    render+loss+backward kernel of a 4-view group launches 4 x 17 x 16 workgroups for 256 CUs, and the single-workgroup
    tail (geometry backward, Adam, next geometry) runs on ONE.  Frames being independent, F of them go through the same
    two launches: `sks_loop_fused_step(frames=F)` renders F x V views and steps F optimisers, one workgroup per frame.
    Every frame's trajectory is bit-identical to a MultiViewLoop running it alone (tests/test_ops_gpu.py).

    `gaussians`: a GaussianModel of ONE frame after training_setup() -- the template for the initial scaling /
    rotation / opacity, the one-hot features and the optimiser's configuration; its own tensors are not touched.
    Parameters live stacked: xyz / scaling (F,P,3), rotation (F,P,4), opacity (F,P,1).  F x V <= 64 views per launch.

    `early_stopping` (configs/*.yaml `training.early_stopping`): "no_stopping", "opt_early_stopping", or an OptEarlyStopping
    with 1 <= window_size <= 16 and an empty history.  The criterion runs per frame on the device, inside the step's tail
    (sks_loop_fused_step_es): each frame stops at its own iteration, exactly as a MultiViewLoop running it alone with the
    same criterion, and a stopped frame's workgroups leave at once from then on.  `stopped_at` reads each frame's stopping
    iteration from pinned memory without waiting; `counters[f, 0]` is frame f's own iteration, while `iteration` stays the
    number of iterations enqueued.  Host-side criteria (any other callable) read every loss back: MultiViewLoop runs those.

    `rigs`: a RigBank on the parameters' device, instead of `cameras`.  The view and projection rows, the per-view scalars, the
    DLT's projection matrices and the learning-rate schedule of the batch are then persistent DEVICE buffers which
    `new_scenes(rig_ids=)` refills by one gather launch (sks_rig_select), and the step reads them through the library's *_dv
    entry points -- nothing of a rig is baked into a captured graph, so `_graph` / `_multi` are replayed as they are for a batch
    with other rigs.  `gaussians.opt_cfg` supplies every hyper-parameter except the spatial scale of the xyz learning rate,
    which is each frame's own rig's `cameras_extent` (build the bank with the same `opt`).  A frame's trajectory is bit-identical
    to FrameBatchLoop(cameras=that rig) running it alone.  The image size of a view slot stays fixed across rigs.

    `keep_gaussians=True`: `optimize_sequence` keeps every frame's scaling, rotation and opacity next to its joints
    (`self.gaussians`, an uncertainty.SequenceGaussians) -- the Gaussian per joint the reference saves per scene, and what
    skelsplat_amd/uncertainty.py reads back as the pose's uncertainty.  Off (default): nothing is allocated or enqueued for it.

    `view_weighting` / `view_threshold`: as MultiViewLoop's, per frame, inside the fused step's tail (sks_loop_fused_step_vw);
    `view_weights` (F,V,P) and `view_similarity` (F,P,V,V) hold each frame's last step's.  A frame's trajectory stays bit-identical
    to a MultiViewLoop with the same keyword running it alone."""

    def __init__(self, gaussians, cameras=None, frames=None, dataset="h36m", accumulation_steps=4, lambda_consistency=1e-5,
                 antialiasing=False, use_graph=False, factored=True, early_stopping="no_stopping", rigs=None, report_steps=0,
                 save_iterations=(), keep_gaussians=False, view_weighting=None, view_threshold=0.5):
        from .report import check_report_args
        check_report_args(report_steps, save_iterations)
        self._init_view_weighting(view_weighting, view_threshold)
        if (cameras is None) == (rigs is None):
            raise ValueError("FrameBatchLoop takes either cameras= (one rig for all frames) or rigs= (a RigBank)")
        if frames is None:
            raise ValueError("FrameBatchLoop needs frames=F")
        if rigs is not None:
            rigs.to(gaussians._xyz.device)      # (uploaded once; free when the bank already lives there)
            cameras = rigs.rigs[0]      # (sizes and counts; every row a kernel reads comes from the bank, per batch)
        gm = gaussians
        self.gm = gm
        self.dataset = dataset
        self.cameras = cameras
        self.F, self.V = int(frames), len(cameras)
        F, V = self.F, self.V
        if F < 1 or F * V > R._lib.SKS_MAX_VIEWS:
            raise ValueError(f"frames x views = {F} x {V} exceeds the {R._lib.SKS_MAX_VIEWS} views of one launch")
        P = gm._xyz.shape[0]
        if P > 64:
            raise ValueError("frame batching runs the sparse fused step: P <= 64 Gaussians per frame")
        self.P = P
        dev = gm._xyz.device
        self.device = dev
        self.acc_steps = int(accumulation_steps)
        self.lambda_consistency = float(lambda_consistency)
        self.antialiasing = antialiasing
        self.use_graph = bool(use_graph)
        self.features = gm.get_features.detach().reshape(P, -1).contiguous()
        self.C = self.features.shape[1]
        init = gm._initial
        self._init = (init[0].reshape(1, P, 3), init[1].reshape(1, P, 4), init[2].reshape(1, P, 1))
        self.xyz = gm._xyz.detach().reshape(1, P, 3).repeat(F, 1, 1).contiguous()
        self.scaling = self._init[0].repeat(F, 1, 1).contiguous()
        self.rotation = self._init[1].repeat(F, 1, 1).contiguous()
        self.opacity = self._init[2].repeat(F, 1, 1).contiguous()
        self.exp_avg = torch.zeros((F, P, 11), device=dev)
        self.exp_avg_sq = torch.zeros((F, P, 11), device=dev)
        self.counters = torch.zeros((F, 2), dtype=torch.int32, device=dev)
        self.accumulated_grads = torch.zeros((F, V, P, 3), device=dev)    # train.py:121, one V-slot buffer per frame
        if self._vw_mode:       # each frame's weights and cosines of its last step (a stopped frame's rows stay as its last step left them)
            self.view_weights = torch.zeros((F, V, P), device=dev)
            self.view_similarity = torch.zeros((F, P, V, V), device=dev)
        # per-frame early stopping on the device: (window, tolerance) or None; the state of every frame's criterion (the
        # layout of sks_loop_adam_step_es's, one row per frame) and the pinned flags the tail writes the stopping iteration to
        self._es = _frame_criterion(early_stopping)
        self._es_state = self._es_flags = None
        if self._es is not None:
            self._es_state = torch.zeros((F, 2 + 2 * self._es[0]), dtype=torch.int32, device=dev)
            self._es_flags = torch.zeros(F, dtype=torch.int32).pin_memory()
            self._es_flags_np = self._es_flags.numpy()
        self._packed = torch.zeros((F * V, P, 11), device=dev)
        self._sums = torch.zeros((F * V, 2), dtype=torch.float64, device=dev)
        # reporting (report.LoopReport): None = off, and then the launch sequence of a group is the one without it
        self._report = None
        if report_steps or save_iterations:
            from .report import LoopReport
            self._report = LoopReport(F, V, P, report_steps, save_iterations, dev)
        self.report = None      # optimize_sequence's report.SequenceReport of the last sequence
        # keep_gaussians: optimize_sequence keeps every frame's scaling / rotation / opacity next to its joints
        # (uncertainty.SequenceGaussians in `gaussians`); off: nothing is allocated and nothing more is enqueued
        self.keep_gaussians = bool(keep_gaussians)
        self.gaussians = None
        self._gt_next = None    # set_ground_truth's tensor, until the next new_scenes / optimize_sequence takes it
        # set_debug_images: the sequence indices optimize_sequence pictures (preview.SequenceImages in `images`); off: nothing is
        # allocated and nothing more is enqueued
        self._debug_frames = None
        self.images = None
        self._frame_views = None
        self._sched, self._lrs, self._adam, self._limb = _optimiser_arrays(gm.opt_cfg, dataset, self.lambda_consistency)
        cams_all = [cameras[k % V] for k in range(F * V)]
        self._cams_all = cams_all

        def views_of(slots, allow_mixed=False):
            if rigs is None:
                return R.ViewBatch.from_cameras([cams_all[k] for k in slots], allow_mixed=allow_mixed)
            # rows of the bank's rig 0 in buffers of the loop's own (filled per batch by sks_rig_select)
            j = [k % V for k in slots]
            sz = [rigs.sizes[i] for i in j]
            return R.ViewBatch(rigs.viewmatrix_dev[0, j].clone(), rigs.projmatrix_dev[0, j].clone(), rigs.tan[0, j, 0].tolist(),
                               rigs.tan[0, j, 1].tolist(), max(s[0] for s in sz), max(s[1] for s in sz), sz)
        # K [R|t] per view, float64 on the device, built once: new_scenes(points=None) triangulates with them
        from .triangulation import device_projection_matrices
        self._proj = device_projection_matrices(cameras, dev)
        self._reject = None     # set_outlier_rejection's (reject_px, min_inliers)
        self._refine = None     # set_refinement's (huber_px, max_iters)
        self._reproject = False     # set_reprojection_report
        self.reprojection = None    # optimize_sequence's reprojection.SequenceReprojection of the last sequence
        self._smooth = None         # set_smoothing's settings
        self.smoothed = None        # optimize_sequence's smoothing.Smoothed of the last sequence
        self._bones = None          # set_bone_constraint's settings
        self.bone_lengths = self.constrained = None     # optimize_sequence's skeleton.BoneLengths / Projected of the last sequence
        # new_scenes(points=None) with rejection: the views each joint of the batch was triangulated from, the winners' counts
        self.inliers = torch.ones((F, V, self.P), dtype=torch.bool, device=dev)
        self.n_consensus = torch.zeros((F, self.P), dtype=torch.int32, device=dev)
        self.seq_inliers = self.seq_n_consensus = None     # optimize_sequence with rejection: the same for its N frames
        self.seq_view_weights = None                       # optimize_sequence with view weighting: (N,V,P) final weights
        sizes = [(int(c.image_width), int(c.image_height)) for c in cams_all]
        # factored (default): the pseudo-GT stays in its separable form (rasterizer.HeatmapFactors) -- the fused step
        # evaluates the pixels it needs, the per-view loss constants come from the factors (sks_heatmap_totals), and no
        # heat-map plane is ever written: 68 MB per H36M view and a frame's largest memory pass are gone
        self.factored = bool(factored)
        self.hset, self.size_groups, self.factors = None, [], None
        if self.factored:
            self.views_all = views_of(range(F * V), allow_mixed=True)
            self.factors = R.HeatmapFactors(F * V, self.C, self.views_all.W, self.views_all.H, dev)
            self.stats_all = R.GtStats.of_factors(self.factors)
        else:
            # planes of all F x V views (frame-major) in one flat buffer; views of one size adjacent (H36M: two sizes)
            self.hset = R.HeatmapSet(sizes, self.C, dev)
            for key, slots in self.hset.groups.items():
                vb = views_of(slots)
                gt = self.hset.group(key)
                gt.zero_()
                self.size_groups.append(SizeGroup(slots, vb, gt, R.gt_tile_stats(gt), torch.tensor(slots, dtype=torch.long, device=dev)))
            if len(self.size_groups) == 1:
                self.views_all, self.stats_all = self.size_groups[0].views, self.size_groups[0].stats
            else:
                self.views_all = views_of(range(F * V), allow_mixed=True)
                self.stats_all = R.GtStats.of_set(self.hset)
        self.rigs, self._sel, self._hf_all = rigs, None, None
        if rigs is not None:
            from .rigs import RigSelection
            self._sel = RigSelection(rigs, F, self.views_all.viewmatrix, self.views_all.projmatrix)
            self.views_all.table = self._sel.table
            self._sched, self._proj = self._sel.sched, self._sel.proj      # per frame, on the device
            self._sel.select([0] * F)
            if not self.factored:   # the factors of ALL views in one launch; the planes are written from them per image size
                self._hf_all = R.HeatmapFactors(F * V, self.C, self.views_all.W, self.views_all.H, dev)
        with torch.no_grad():
            self._fstate = R.geometry_views(self.views_all, self.xyz, self.C, self.opacity, self.scaling, self.rotation, None,
                                            antialiasing=antialiasing, raw_params=True, frames=F)
        self._geom_valid = False
        self._graph = None
        self._multi = None
        self.iteration = 0
        self.last_losses = None

    def new_scenes(self, points, poses_2d=None, heatmaps=None, drop_masks=None, rig_ids=None, poses_3d=None):
        """The next F frames: `points` (F,P,3) initial joints; either `poses_2d` (F,V,J,2) -- the heat-maps are generated
        from the re-initialised Gaussians like general_utils.py:175-304, all frames in two launches per image size -- or
        ready `heatmaps` (F,V,C,H,W) / a list of F lists of V (C,H_v,W_v) planes.  `drop_masks`: optional (F,V,J) bool of
        dropped heat-map planes (heatmaps.draw_dropout per frame).  Everything is re-initialised in place, so captured
        hipGraphs are replayed as they are.
        `points=None`: the initial joints are the DLT triangulation of `poses_2d` (triangulation.triangulate_sequence),
        written straight into `self.xyz` by one launch on the current stream, in front of the heat-map factors that read
        them: detections already on the device never touch the host.  `drop_masks` are then also the DLT's
        `valid = ~drop_masks` -- a dropped plane is a detection the caller does not trust --, and a joint kept in fewer than
        two views has no triangulation: it starts as NaN, and is then UNOBSERVED for the whole loop (DESIGN.md "Unobserved
        joints": it renders nothing, its planes are zero, its limb pair leaves the loss, it stays NaN, and neither the frame's
        other joints nor any other frame notice).  Ready `heatmaps` carry no detections: refused.
        `poses_3d` (F,V,J,3), with `points=None`: the initial joints are instead the reprojection-error-weighted mean of the
        views' 3D predictions (initial_guess.fuse_predictions, the reference's "metrabs" guess), written into `self.xyz` by one
        launch in the same place with the same `valid = ~drop_masks`; a joint whose views are all dropped starts as NaN.
        Together with explicit `points` it is refused.
        `set_outlier_rejection` and `set_refinement` say what they add to the triangulation, in the same place: the views each joint
        was solved from are then in `self.inliers` (F,V,J) bool, the winners' counts in `self.n_consensus` (F,J) int32.
        `rig_ids` (F,) ints, host or device (a loop over a rig bank): frame f is seen by rig rig_ids[f] -- one gather launch on
        the current stream fills the batch's camera rows, per-view scalars, projection matrices and schedule rows in place, in
        front of the triangulation and the heat-map factors that read them.  Host ids are validated here; ids in a device
        tensor are bounds-checked by the kernel, which skips a frame whose id is outside the bank (it keeps the cameras its
        slot had) and raises an error word that `check_rigs()` reports.  None: the frames keep the rigs they have.
        A loop that reports (`report_steps` / `save_iterations`): the ground truth given to `set_ground_truth` since the last batch,
        (F,P,3), is copied in place -- without one the errors of this batch are NaN, losses and snapshots are reported all the
        same --, the traces and snapshots go back to NaN and one report launch behind everything above writes row 0 and the
        snapshots of iteration 0 from the initial joints."""
        from .heatmaps import generate_heatmaps, heatmap_factors, heatmap_planes
        F, V, P = self.F, self.V, self.P
        if self.factored and heatmaps is not None:
            raise ValueError("ready heat-map planes need FrameBatchLoop(..., factored=False)")
        if rig_ids is not None and self._sel is None:
            raise ValueError("rig_ids needs a rig bank: FrameBatchLoop(gaussians, rigs=RigBank(rigs, device), frames=F)")
        if self._reproject and heatmaps is not None:
            raise ValueError("new_scenes: the reprojection report (set_reprojection_report) measures against detections, and ready "
                             "heatmaps carry none -- give poses_2d, or switch it off with set_reprojection_report(False)")
        gt_pose, self._gt_next = _checked_gt(self, self._gt_next, F, "new_scenes"), None      # (`gt` below: heat-map planes)
        with torch.no_grad():
            if self._sel is not None:
                self._sel.check()       # (an id a device tensor of an earlier batch held outside the bank; never waits)
                if rig_ids is not None:
                    self._sel.select(rig_ids)
            plan = InitialJoints.check("new_scenes", points, poses_2d, poses_3d, (F, V, P), self._reject, self._refine, self._proj,
                                       self.device)
            if plan.estimated:
                poses_2d = plan.p2d[..., :2]
            if self._es is not None:
                # a frame still running may yet write its flag from work enqueued before: let it drain first (once every
                # frame has stopped, nothing writes a flag any more, and the next frames start at once)
                if not self._es_flags_np.all():
                    torch.cuda.current_stream(self.device).synchronize()
                self._es_flags_np[:] = 0
                self._es_state.zero_()
            keep = None
            if plan.estimated and drop_masks is not None:
                keep = ~torch.as_tensor(drop_masks).to(device=self.device, dtype=torch.bool).reshape(F, V, P)
            plan.write(keep, self.xyz, (self.inliers, self.n_consensus))
            self.scaling.copy_(self._init[0].expand(F, P, 3))
            self.rotation.copy_(self._init[1].expand(F, P, 4))
            self.opacity.copy_(self._init[2].expand(F, P, 1))
            self.exp_avg.zero_(); self.exp_avg_sq.zero_(); self.counters.zero_(); self.accumulated_grads.zero_()
            if poses_2d is not None:
                p2d_all = torch.as_tensor(poses_2d, device=self.device).reshape(F * V, -1, 2)
                drop_all = None if drop_masks is None else torch.as_tensor(drop_masks).reshape(F * V, -1)
            elif heatmaps is None:
                raise ValueError("new_scenes needs poses_2d or heatmaps")
            if self.factored:
                # two small launches for all frames and image sizes: the factors, then the loss constants from them
                heatmap_factors(self.xyz, torch.exp(self.scaling), self.rotation, p2d_all, self._cams_all,
                                views=self.views_all, frames=F, out=self.factors, drop_mask=drop_all)
                self.factors.totals(self.views_all, self.stats_all.totals)
            if self._hf_all is not None and heatmaps is None:
                heatmap_factors(self.xyz, torch.exp(self.scaling), self.rotation, p2d_all, self._cams_all,
                                views=self.views_all, frames=F, out=self._hf_all, drop_mask=drop_all)
            for slots, vb, gt, stats, idx in self.size_groups:
                if heatmaps is not None:
                    for i, k in enumerate(slots):
                        gt[i].copy_(heatmaps[k // V][k % V])
                    R.gt_tile_stats(gt, out=stats)
                elif self._hf_all is not None:
                    hf = self._hf_all       # (a view's factors do not depend on which views share its launch)
                    heatmap_planes(hf.row[idx][:, :, :vb.H].contiguous(), hf.col[idx][:, :, :vb.W].contiguous(), hf.cmin[idx],
                                   hf.den[idx], out=gt, totals=stats.totals)
                else:
                    generate_heatmaps(self.xyz, torch.exp(self.scaling), self.rotation, p2d_all[idx],
                                      [self.cameras[k % V] for k in slots], out=gt, views=vb, totals=stats.totals,
                                      drop_mask=None if drop_all is None else drop_all[idx.cpu()], frames=F)
                if len(self.size_groups) > 1:
                    self.stats_all.totals.index_copy_(0, idx, stats.totals)
            if self._report is not None:
                self._report.reset(gt_pose)
                self._report.launch(self, losses=False)
        self._geom_valid = False
        self.iteration = 0
        return self

    def frame_views(self, i):
        """The ViewBatch of frame i's V views for a dense forward of that frame alone (the debug pictures): the loop's cameras,
        which every frame of a batch shares."""
        if self._frame_views is None:
            self._frame_views = R.ViewBatch.from_cameras(self._cams_all[:self.V], allow_mixed=True)
        return self._frame_views

    def heatmap_pictures(self):
        """((F x V,H,W) uint8, (F x V,2) float32 {min, max}) of the batch's pseudo-GT as it stands: preview.heatmap_preview of
        the factors, or preview.channel_sum_u8 of the planes (factored=False); H, W the largest view."""
        from .preview import channel_sum_u8, heatmap_preview
        if self.factored:
            return heatmap_preview(self.factors, self.views_all, return_minmax=True)
        if len(self.size_groups) == 1:
            return channel_sum_u8(self.size_groups[0].gt, return_minmax=True)
        va = self.views_all
        out = torch.zeros((va.V, va.H, va.W), dtype=torch.uint8, device=self.device)
        mm = torch.empty((va.V, 2), dtype=torch.float32, device=self.device)
        for slots, vb, gt, stats, idx in self.size_groups:
            out[idx, :vb.H, :vb.W], mm[idx] = channel_sum_u8(gt, return_minmax=True)
        return out, mm

    def _optimiser_block(self, group_mask, last_view, n_iters):
        return (self.accumulated_grads, group_mask, last_view, self.xyz, self.scaling, self.rotation, self.opacity, self.exp_avg,
                self.exp_avg_sq, self.counters, n_iters, self._sched, self._lrs, self._adam, self.lambda_consistency, self._limb)

    def _set_view_weighting(self, mode, threshold):
        """set_view_weighting for this loop: the step's entry point changes, so the captured graphs go."""
        self._init_view_weighting(mode, threshold)
        if self._vw_mode:
            self.view_weights = torch.zeros((self.F, self.V, self.P), device=self.device)
            self.view_similarity = torch.zeros((self.F, self.P, self.V, self.V), device=self.device)
        self._graph = self._multi = None

    def _device_group(self, group_mask, last_view, n_iters):
        with torch.no_grad():
            if not self._geom_valid:
                self._fstate = R.geometry_views(self.views_all, self.xyz, self.C, self.opacity, self.scaling, self.rotation,
                                                None, antialiasing=self.antialiasing, raw_params=True, out=self._fstate,
                                                frames=self.F)
                self._geom_valid = True
            es = {} if self._es is None else dict(es_state=self._es_state, es_window=self._es[0], es_tolerance=self._es[1],
                                                  es_flags=self._es_flags)
            R.loop_fused_step(self._fstate, self.stats_all, self.features, self._packed, self._sums,
                              *self._optimiser_block(group_mask, last_view, n_iters), **es, view_weights=self._view_weight_args())
            if self._report is not None:
                self._report.launch(self)
        s = self._sums.view(self.F, self.V, 2)
        self.last_losses = (s[..., 0], s[..., 1])       # per (frame, view) {S, N}: loss = S / N

    def step_group(self, parameters_untouched=False):
        """(parameters_untouched: as MultiViewLoop.step_group)
        Iterations self.iteration+1 .. the next optimiser step of EVERY frame (train.py:130-222; the frames share the
        iteration counter, the view order and therefore the group's view mask).  With early stopping, nothing is enqueued
        once every frame has stopped."""
        if self._all_stopped():
            return self.iteration
        grp = next_group(self.iteration, self.acc_steps, self.V)
        key = grp.key
        if self.use_graph:
            if self._graph is None or self._graph[0] != key:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self._geom_valid = False
                    self._device_group(*key)
                self._graph = (key, graph)
            self._graph[1].replay()
        else:
            if not parameters_untouched:
                self._geom_valid = False
            self._device_group(*key)
        self.iteration = grp.end
        return grp.end

    @property
    def stopped_at(self):
        """Per frame: the iteration early stopping ended it at, or None (so far: read from the pinned flags without waiting;
        after run() returns, final)."""
        if self._es is None:
            return [None] * self.F
        return [int(x) or None for x in self._es_flags_np]

    def _all_stopped(self):
        return self._es is not None and bool(self._es_flags_np.all())

    # What the loop reports (report_steps / save_iterations; report.LoopReport says what each holds): the loop's own buffers,
    # as they stand on the stream -- none of these waits.  None for what is switched off.
    @property
    def trace_errors(self):
        """(F,report_steps,2): row n = mean absolute / root-relative error after n optimiser steps."""
        return None if self._report is None else self._report.trace_err

    @property
    def trace_losses(self):
        """(F,report_steps,V): row n >= 1 = every view's loss in the group that led to step n."""
        return None if self._report is None else self._report.trace_loss

    @property
    def final_errors(self):
        """(F,P,2): per-joint absolute / root-relative error of the current joints."""
        return None if self._report is None else self._report.final_err

    @property
    def snapshots(self):
        """(F,K,P,3): the joints at the end of iteration save_iterations[k]; NaN for a frame that stopped before it."""
        return None if self._report is None else self._report.snaps

    @property
    def steps(self):
        """(F,) int32: optimiser steps every frame has made (the last row of its traces)."""
        return self.counters[:, 1]

    def run(self, iterations=500, groups_per_graph=25):
        """All F frames up to `iterations`; returns the joints (F,P,3).  With use_graph, `groups_per_graph` groups are one
        hipGraph, as in MultiViewLoop.run.  With early stopping, the flags are polled between launches without waiting,
        enqueuing ends once every frame has stopped, and the stream is synchronised once, at the end."""
        self._enqueue(iterations, groups_per_graph)
        if self._es is not None:
            torch.cuda.current_stream(self.device).synchronize()
            self.check_rigs()
        return self.xyz

    def check_rigs(self):
        """A loop over a rig bank: raises if a `rig_ids` device tensor named a rig outside the bank (that frame was skipped by
        the gather and ran with the cameras its slot held before).  Reads a pinned word and never waits: final once the
        stream has been synchronised, which run() with early stopping does itself."""
        if self._sel is not None:
            self._sel.check()

    def optimize_sequence(self, points, poses_2d, iterations=500, groups_per_graph=25, return_initial=False, rig_ids=None,
                          poses_3d=None):
        """The reference's outer loop over the frames of a sequence (train.py:74-99) F frames at a time: `points`
        (N,P,3) initial joints and `poses_2d` (N,V,J,2) detections of N frames -> (N,P,3) optimised joints.  A last batch
        with fewer than F frames is filled up by repeating its final frame (frames are independent: the filler changes
        nothing and is dropped).  `points=None`: every batch's initial joints are triangulated from its detections on
        the device (new_scenes); `poses_2d` may be a device tensor and is then never copied to the host.
        `return_initial=True`: returns (joints, initial joints), both (N,P,3) on the device.
        `rig_ids` (N,) ints, host or device (a loop over a rig bank): the rig of every frame, see new_scenes.
        `poses_3d` (N,V,J,3), with `points=None`: every batch's initial joints are fused from the views' 3D predictions
        instead (new_scenes); a device tensor is never copied to the host.
        What the switches add -- set_outlier_rejection (`self.seq_inliers`, `self.seq_n_consensus`), set_refinement,
        set_reprojection_report (`self.reprojection`), set_smoothing (`self.smoothed`), set_bone_constraint (`self.bone_lengths`,
        `self.constrained`), set_debug_images (`self.images`) -- is said
        there; each result is None after a sequence without its switch.
        A loop that reports: the return value is the same, and `self.report` (a report.SequenceReport) holds the loop's traces,
        final errors, snapshots and step counts for all N frames -- the errors against the (N,P,3) ground truth given to
        `set_ground_truth` before this call, NaN without one.
        A loop built with keep_gaussians=True: afterwards `self.gaussians` (an uncertainty.SequenceGaussians) holds every frame's
        xyz -- the tensor returned --, scaling, rotation and opacity as the frame ended, what scene.save_h36m writes
        (io.save_ply_arrays) and uncertainty.joint_uncertainty reads; None otherwise."""
        run, self._gt_next = SequenceRun(self, self._gt_next, points, poses_2d, poses_3d, rig_ids, return_initial), None
        run.publish(self, ("seq_inliers", "seq_n_consensus"))
        for b in run.starts():
            run.begin(self, b)
            self.run(iterations, groups_per_graph)      # (returns self.xyz, which take() copies)
            run.take(self, b)
        self.smoothed = run.smoothed()
        self.bone_lengths, self.constrained = run.constrained(self.smoothed)
        self.check_rigs()
        return run.result()


class FramePipeline(SequenceSwitches):
    """A sequence of frames through `streams` FrameBatchLoops of `frames` frames each, one HIP stream per loop.

    Inside one FrameBatchLoop a group is two dependent launches: the compositing backward of all its frames, then one
    workgroup per frame for geometry backward + Adam + next geometry (~14 us during which the chip is nearly idle).  Several
    loops on separate streams fill that hole with each other's backward kernels: on one MI355X (H36M, 4 views, 500
    iterations per frame, heat-map generation included) 292 frames/s one frame at a time, 1 480 with 16 frames per launch,
    1 900-2 100 with 2-4 such loops in flight (tools/bench_frames.py).  Results do not depend on `frames` / `streams`:
    every frame's trajectory is bit-identical to a MultiViewLoop running it alone.
    `early_stopping` (as FrameBatchLoop's) goes to every loop; then a stream whose batch has stopped entirely takes the next
    batch at once, and `stopped_at` holds the last sequence's stopping iterations."""

    def __init__(self, gaussians, cameras=None, frames=16, streams=2, **kw):
        kw.setdefault("use_graph", True)
        self.loops = [FrameBatchLoop(gaussians, cameras, frames, **kw) for _ in range(int(streams))]
        self.device = self.loops[0].device
        self.streams = [torch.cuda.Stream(self.device) for _ in self.loops]
        self.F, self.P = self.loops[0].F, self.loops[0].P
        self.stopped_at = None       # early stopping: (N,) int64 of the last optimize_sequence, 0 = ran to the end
        self.report = None           # loops that report: report.SequenceReport of the last optimize_sequence
        self.gaussians = None        # keep_gaussians=True: uncertainty.SequenceGaussians of the last optimize_sequence
        self._gt_next = None         # set_ground_truth's tensor, until the next optimize_sequence takes it
        self.images = None           # set_debug_images: preview.SequenceImages of the last optimize_sequence
        self.inliers = self.n_consensus = None     # optimize_sequence with rejection: (N,V,J) bool, (N,J) int32
        self.reprojection = None     # set_reprojection_report: reprojection.SequenceReprojection of the last optimize_sequence
        self.smoothed = None         # set_smoothing: smoothing.Smoothed of the last optimize_sequence
        self.bone_lengths = self.constrained = None     # set_bone_constraint: skeleton.BoneLengths / Projected of the last one
        self.view_weights = None     # view weighting on: (N,V,P) final weights of the last optimize_sequence

    def _driven(self):
        return self.loops       # (the switches set every loop: JointSwitches, SequenceSwitches)

    def optimize_sequence(self, points, poses_2d, iterations=500, groups_per_graph=25, interleave=100,
                          return_initial=False, rig_ids=None, poses_3d=None):
        """(N,P,3) initial joints + (N,V,J,2) detections -> (N,P,3) optimised joints (train.py:74-99 over the frames).
        The loops' graph launches are issued round-robin, `interleave` iterations at a time, so that every stream always
        has work queued; a last batch with fewer than `frames` frames is padded by repeating its final frame.
        `points=None`: every batch's initial joints are triangulated from its detections by one launch on the batch's own
        stream (FrameBatchLoop.new_scenes), behind whatever the caller's stream did to `poses_2d`; detections given as a
        device tensor are never copied to the host.  `return_initial=True`: returns (joints, initial joints).
        `rig_ids` (N,) ints, host or device (loops over a rig bank, `rigs=`): the rig of every frame, see
        FrameBatchLoop.new_scenes; check_rigs() reports an id a device tensor held outside the bank.
        `poses_3d` (N,V,J,3), with `points=None`: every batch's initial joints are fused from the views' 3D predictions
        instead of triangulated, by one launch in the same place (initial_guess.fuse_predictions).
        The switches, the loops' reports and kept Gaussians fill the results FrameBatchLoop.optimize_sequence names, here with the
        consensus pair in `self.inliers` (N,V,J) bool / `self.n_consensus` (N,J) int32; every batch's rows are made or copied on the
        batch's own stream (the reprojection report: two launches per batch), the smoothing is enqueued on the caller's stream
        once it waits for every batch.  The return value is the same with and without them."""
        run, self._gt_next = SequenceRun(self.loops[0], self._gt_next, points, poses_2d, poses_3d, rig_ids, return_initial), None
        run.publish(self)
        cur = torch.cuda.current_stream(self.device)
        es = self.loops[0]._es is not None
        if es:
            self.stopped_at = run.stopped_at = torch.zeros(run.N, dtype=torch.int64, device=self.device)
        for st in self.streams:
            st.wait_stream(cur)                      # inputs and `out` were produced on the caller's stream
        schedule = self._sequence_es if es else self._sequence_waves
        schedule(run, iterations, groups_per_graph, interleave)
        for st in self.streams:
            cur.wait_stream(st)
        self.smoothed = run.smoothed()
        self.bone_lengths, self.constrained = run.constrained(self.smoothed)
        self.check_rigs()
        return run.result()

    def check_rigs(self):
        """FrameBatchLoop.check_rigs of every loop (never waits: final once the device has been synchronised)."""
        for fb in self.loops:
            fb.check_rigs()

    def _sequence_waves(self, run, iterations, groups_per_graph, interleave):
        """optimize_sequence without early stopping: waves of one batch per stream, begun, run round-robin and taken together."""
        starts, S = run.starts(), len(self.loops)
        for w in range(0, len(starts), S):
            active = list(zip(self.loops, self.streams, starts[w:w + S]))
            for fb, st, b in active:
                with torch.cuda.stream(st):
                    run.begin(fb, b)
            for k in range(0, iterations, max(int(interleave), 1)):
                for fb, st, b in active:
                    with torch.cuda.stream(st):
                        fb.run(min(iterations, k + interleave), groups_per_graph)
            for fb, st, b in active:
                with torch.cuda.stream(st):
                    run.take(fb, b)

    def _sequence_es(self, run, iterations, groups_per_graph, interleave):
        """optimize_sequence with early stopping: every stream keeps its own batch and takes the next one as soon as its
        batch is done -- all frames stopped (seen in the pinned flags, without waiting) or `iterations` enqueued -- instead
        of waiting for the other streams' batches.  Results and stopping iterations are copied on the batch's stream."""
        pending = iter(run.starts())

        def take(fb, st):
            b = next(pending, None)
            if b is None:
                return None
            with torch.cuda.stream(st):
                run.begin(fb, b)
            return [fb, st, b, 0]

        step = max(int(interleave), 1)
        active = [a for a in (take(fb, st) for fb, st in zip(self.loops, self.streams)) if a is not None]
        while active:
            nxt = []
            for slot in active:
                fb, st, b, k = slot
                k = min(iterations, k + step)
                with torch.cuda.stream(st):
                    fb._enqueue(k, groups_per_graph)
                    slot[3] = k
                    if k >= iterations or fb._all_stopped():
                        run.take(fb, b)
                        slot = take(fb, st)
                if slot is not None:
                    nxt.append(slot)
            active = nxt


def mpjpe(pred, gt):
    """eval.py:123-124: mean Euclidean joint error (same units as the inputs, mm)."""
    return torch.norm(pred - gt, dim=1).mean()
