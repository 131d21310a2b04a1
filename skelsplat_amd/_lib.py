"""ctypes binding of libskelsplat_hip.so (include/skelsplat_hip.h).

The library is the product: there is NO CPU or PyTorch fallback.  Loading fails loudly if the shared object is
missing and cannot be built, and every op raises if it is handed non-ROCm tensors.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libskelsplat_hip.so")
_lib = None

SKS_MAX_VIEWS = 64
SKS_MAX_CHANNELS = 32
SKS_SMALL_P = 256
SKS_ANTIALIASING = 1
SKS_CLAMP01 = 2
SKS_FORCE_BINNED = 4
SKS_DEBUG_SYNC = 8
SKS_NO_NT_STORES = 16
SKS_RAW_PARAMS = 32
SKS_BIN_CLEAN = 64
SKS_RAW_GRADS = 128
SKS_FB_NO_JOIN = 1
SKS_BIN_GROUPS_SHIFT = 16
SKS_BWD_WG_SHIFT = 23     # bits 23..25: workgroups per (view, Gaussian) of the wave-resident backward = 16 >> (value - 1); 0 = automatic
SKS_SSIM_SCRATCH_BYTES = 64 * 8
SKS_SOFTARGMAX_STATS = 6
SKS_REPORT_MAX_SAVES = 8
SKS_EVAL_MAX_GROUPS = 64
SKS_CALIBRATION_MAX_K = 8
SKS_REFINE_MAX_ITERS = 16
SKS_SMOOTH_MAX_JOINTS = 256
SKS_SMOOTH_MAX_HALF_WINDOW = 32
SKS_SMOOTH_BOX, SKS_SMOOTH_TRICUBE = 0, 1
SKS_SMOOTH_LAUNCH_INTS = 4
SKS_BONES_MAX_JOINTS = 32
SKS_BONES_MAX_GROUPS = 256
SKS_BONES_MAX_ITERS = 16
SKS_BONES_LAUNCH_INTS = 8
SKS_PEOPLE_MAX_DETS = 128
SKS_PEOPLE_MAX_SLOTS = 16
SKS_PEOPLE_MAX = 8
SKS_PEOPLE_MAX_GROUPS = 65535
SKS_PEOPLE_LAUNCH_INTS = 4
SKS_ALIGN_RIGID, SKS_ALIGN_SIMILARITY, SKS_ALIGN_SCALE = 0, 1, 2
SKS_PREVIEW_LAUNCH_INTS = 4
SKS_HEATMAP_MAX_RADIUS = 1 << 18     # a truncation radius beyond it draws no impulse (sks_heatmap_factors, DESIGN.md "Degenerate footprints")


SKS_NO_EARLY_FILL = 1 << 30
SKS_BWD_LDS_LIST = 1 << 20     # tests: the LDS-list backward even when P <= 64
SKS_FILL_LINEAR = 1 << 21      # tuning/tests: forward fill blocks always in linear (pass-major) mode
SKS_FILL_ROWS = 1 << 22        # tuning/tests: row-aligned fill blocks whenever W % 4 == 0


def SKS_EARLY_FILL(n):
    """Tuning/tests, small path: the geometry launch zeroes n sixteenths of the call's planes (n = 1..6), all of them (7); 0 = automatic."""
    return (int(n) & 7) << SKS_BIN_GROUPS_SHIFT


def SKS_BIN_GROUPS(n):
    """Flag bits for `n` view groups on the binned path (include/skelsplat_hip.h)."""
    return ((int(n) - 1) & 7) << SKS_BIN_GROUPS_SHIFT


_vp, _i, _u, _f, _sz = C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_size_t

# The three entry points whose calls rasterizer.py records and replays: (parameter name, ctype) as in include/skelsplat_hip.h
# (tests/test_cpu.py holds the tables to it).  A slot of a recorded argument block is addressed through FWD / BWD / FWD_BWD below.
_CAMERAS = (("V", _i), ("P", _i), ("C", _i), ("W", _i), ("H", _i), ("viewmatrix", _vp), ("projmatrix", _vp),
            ("tanfovx", _vp), ("tanfovy", _vp))
_GAUSSIANS = (("means3D", _vp), ("features", _vp), ("opacities", _vp), ("scales", _vp), ("rotations", _vp),
              ("cov3D_precomp", _vp), ("scale_modifier", _f), ("flags", _u))
_UPSTREAM = (("dL_dout_color", _vp), ("dL_dout_invdepth", _vp), ("accum", _vp))
_GRADS = (("dL_dmeans3D", _vp), ("dL_dmeans2D", _vp), ("dL_dopacity", _vp), ("dL_dscales", _vp), ("dL_drotations", _vp),
          ("dL_dcov3D", _vp), ("dL_dfeatures", _vp), ("dL_dmeans3D_mean", _vp))
_FORWARD_IO = (("out_color", _vp), ("out_invdepth", _vp), ("radii", _vp), ("geom", _vp), ("binning", _vp),
               ("bin_capacity", _sz), ("num_rendered_dev", _vp))
FORWARD_PARAMS = _CAMERAS + _GAUSSIANS + _FORWARD_IO + (("final_T", _vp), ("n_contrib", _vp), ("stream", _vp))
BACKWARD_PARAMS = _CAMERAS + (("bg", _vp),) + _GAUSSIANS + (("radii", _vp), ("geom", _vp), ("binning", _vp), ("bin_capacity", _sz)) \
    + _UPSTREAM + _GRADS + (("stream", _vp),)
# the prefill pair (include/skelsplat_hip.h): the same blocks with their extra parameters in front of `stream`, so a recorded block of
# sks_forward / sks_backward becomes theirs by inserting the extras at FWD["stream"] / BWD["stream"]
FORWARD_PREFILLED_PARAMS = FORWARD_PARAMS[:-1] + (("prefilled_planes", _i), ("stream", _vp))
BACKWARD_PREFILL_PARAMS = BACKWARD_PARAMS[:-1] + (("next_color", _vp), ("next_invdepth", _vp), ("planes_wave", _i), ("planes_geom", _i),
                                                  ("stream", _vp))
FORWARD_BACKWARD_PARAMS = _CAMERAS + _GAUSSIANS + _FORWARD_IO + (("bg", _vp),) + _UPSTREAM + _GRADS \
    + (("stream", _vp), ("aux_stream", _vp), ("fb_flags", _u))

FWD, BWD, FWD_BWD = ({name: i for i, (name, _) in enumerate(params)}      # parameter name -> slot
                     for params in (FORWARD_PARAMS, BACKWARD_PARAMS, FORWARD_BACKWARD_PARAMS))
# sks_forward_backward's block from the two calls' records, BY NAME: the forward record's slot if sks_forward has the name, else the
# backward record's; None = in neither, the caller sets it per call.
FWD_BWD_SOURCES = tuple(("fwd", FWD[n]) if n in FWD else ("bwd", BWD[n]) if n in BWD else None for n in FWD_BWD)

# The entry points that read per-view scalars and the LR schedule from DEVICE memory (frame batches over a rig bank), in the same
# style: (parameter name, ctype) as in include/skelsplat_hip.h (tests/test_rigs_cpu.py holds the tables to it).
_ull = C.c_ulonglong
_VIEWS_DV = (("viewmatrix", _vp), ("projmatrix", _vp), ("views_dev", _vp))
RIG_SELECT_PARAMS = (("R", _i), ("V", _i), ("frames", _i), ("rig_ids", _vp), ("bank_viewmatrix", _vp), ("bank_projmatrix", _vp),
                     ("bank_tan", _vp), ("slot_wh", _vp), ("bank_proj", _vp), ("bank_sched", _vp), ("viewmatrix", _vp),
                     ("projmatrix", _vp), ("views_dev", _vp), ("proj", _vp), ("lr_sched_dev", _vp), ("error_word", _vp),
                     ("stream", _vp))
GEOMETRY_DV_PARAMS = (("V", _i), ("P", _i), ("C", _i), ("W", _i), ("H", _i)) + _VIEWS_DV + (
    ("means3D", _vp), ("opacities", _vp), ("scales", _vp), ("rotations", _vp), ("cov3D_precomp", _vp), ("scale_modifier", _f),
    ("flags", _u), ("radii", _vp), ("geom", _vp), ("frames", _i), ("stream", _vp))
HEATMAP_FACTORS_DV_PARAMS = (("V", _i), ("J", _i), ("W", _i), ("H", _i), ("means3D", _vp), ("scales", _vp), ("rotations", _vp),
                             ("scale_modifier", _f), ("poses_2d", _vp), ("viewmatrix", _vp), ("views_dev", _vp), ("row", _vp),
                             ("col", _vp), ("cmin", _vp), ("den", _vp), ("frames", _i), ("stream", _vp))
HEATMAP_TOTALS_DV_PARAMS = (("V", _i), ("J", _i), ("W", _i), ("H", _i), ("row", _vp), ("col", _vp), ("cmin", _vp), ("den", _vp),
                            ("views_dev", _vp), ("gt_totals", _vp), ("stream", _vp))
# The optimiser block of the loop's step entry points (sks_loop_adam_step*, sks_loop_fused_step*): one run of every prototype, which
# loop.py fills from one place per loop; the early-stopping entries append _ES and their host flag(s).  tests/test_cpu.py holds the
# tables to the header.
OPTIMISER_PARAMS = (("slots", _vp), ("group_mask", _ull), ("last_view", _i), ("xyz", _vp), ("scaling", _vp), ("rotation", _vp),
                    ("opacity", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("counters", _vp), ("acc_steps", _i),
                    ("lr_sched", _vp), ("lrs", _vp), ("adam", _vp), ("lambda_consistency", _f), ("limb", _vp))
OPTIMISER_DV_PARAMS = tuple(("lr_sched_dev", ct) if name == "lr_sched" else (name, ct) for name, ct in OPTIMISER_PARAMS)
_ES = (("es_state", _vp), ("es_window", _i), ("es_tolerance", _f))
ES_PARAMS, ES_FRAMES_PARAMS = _ES + (("es_host_flag", _vp),), _ES + (("es_host_flags", _vp),)
_ADAM_STEP = (("V", _i), ("P", _i), ("grads", _vp)) + OPTIMISER_PARAMS + (("shard_world", _i),)
_STEP_RENDER = (("features", _vp), ("scale_modifier", _f), ("flags", _u), ("radii", _vp), ("geom", _vp), ("gt", _vp),
                ("gt_totals", _vp), ("accum", _vp), ("loss_sums", _vp), ("packed", _vp))
_STEP_HEATMAPS = (("view_wh", _vp), ("gt_offsets", _vp), ("frames", _i), ("hm_factors", _vp))
_STEP = _CAMERAS + _STEP_RENDER + OPTIMISER_PARAMS + _STEP_HEATMAPS
_STEP_DV = (("V", _i), ("P", _i), ("C", _i), ("W", _i), ("H", _i)) + _VIEWS_DV + _STEP_RENDER + OPTIMISER_DV_PARAMS + _STEP_HEATMAPS
LOOP_ADAM_STEP_PARAMS = _ADAM_STEP + (("stream", _vp),)
LOOP_ADAM_STEP_ES_PARAMS = _ADAM_STEP + (("loss_sums", _vp),) + ES_PARAMS + (("stream", _vp),)
LOOP_FUSED_STEP_PARAMS = _STEP + (("stream", _vp),)
LOOP_FUSED_STEP_ES_PARAMS = _STEP + ES_FRAMES_PARAMS + (("stream", _vp),)
LOOP_FUSED_STEP_DV_PARAMS = _STEP_DV + (("stream", _vp),)
LOOP_FUSED_STEP_ES_DV_PARAMS = _STEP_DV + ES_FRAMES_PARAMS + (("stream", _vp),)
STEP_PARAMS = {"sks_loop_adam_step": LOOP_ADAM_STEP_PARAMS, "sks_loop_adam_step_es": LOOP_ADAM_STEP_ES_PARAMS,
               "sks_loop_fused_step": LOOP_FUSED_STEP_PARAMS, "sks_loop_fused_step_es": LOOP_FUSED_STEP_ES_PARAMS}
DV_PARAMS = {"sks_rig_select": RIG_SELECT_PARAMS, "sks_geometry_dv": GEOMETRY_DV_PARAMS,
             "sks_heatmap_factors_dv": HEATMAP_FACTORS_DV_PARAMS, "sks_heatmap_totals_dv": HEATMAP_TOTALS_DV_PARAMS,
             "sks_loop_fused_step_dv": LOOP_FUSED_STEP_DV_PARAMS, "sks_loop_fused_step_es_dv": LOOP_FUSED_STEP_ES_DV_PARAMS}
# View agreement (include/skelsplat_hip.h "View agreement"): the early-stopping prototypes with VW_PARAMS in front of `stream`;
# es_state == NULL there is the step without a criterion, vw_mode 0 the plain mean.  tests/test_view_weights_cpu.py holds the tables
# to the header.
VW_PARAMS = (("vw_mode", _i), ("vw_threshold", _f), ("vw_weights", _vp), ("vw_similarity", _vp))
VW_MODES = {None: 0, "scale": 1, "select": 2}
LOOP_ADAM_STEP_VW_PARAMS = LOOP_ADAM_STEP_ES_PARAMS[:-1] + VW_PARAMS + (("stream", _vp),)
LOOP_FUSED_STEP_VW_PARAMS = LOOP_FUSED_STEP_ES_PARAMS[:-1] + VW_PARAMS + (("stream", _vp),)
LOOP_FUSED_STEP_VW_DV_PARAMS = LOOP_FUSED_STEP_ES_DV_PARAMS[:-1] + VW_PARAMS + (("stream", _vp),)
VW_STEP_PARAMS = {"sks_loop_adam_step_vw": LOOP_ADAM_STEP_VW_PARAMS, "sks_loop_fused_step_vw": LOOP_FUSED_STEP_VW_PARAMS,
                  "sks_loop_fused_step_vw_dv": LOOP_FUSED_STEP_VW_DV_PARAMS}


def vw_mode(view_weighting):
    """The C ABI's vw_mode of a `view_weighting` keyword (None | "scale" | "select")."""
    if view_weighting not in VW_MODES:
        raise ValueError(f"view_weighting = {view_weighting!r}: expected None, 'scale' or 'select'")
    return VW_MODES[view_weighting]


# symbol -> (restype, argtypes); mirrors include/skelsplat_hip.h (tests check every declared symbol is exported)
SIGNATURES = {
    "sks_last_error": (C.c_char_p, []),
    "sks_version": (_i, []),
    "sks_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _sz, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)]),
    "sks_launch_regime": (_i, [_i, _i, _i, _i, _i, _u, _i, C.POINTER(_i)]),
    "sks_list_regime": (_i, [C.POINTER(_i)]),
    "sks_forward": (_i, [ct for _, ct in FORWARD_PARAMS]),
    "sks_backward": (_i, [ct for _, ct in BACKWARD_PARAMS]),
    "sks_forward_backward": (_i, [ct for _, ct in FORWARD_BACKWARD_PARAMS]),
    "sks_forward_prefilled": (_i, [ct for _, ct in FORWARD_PREFILLED_PARAMS]),
    "sks_backward_prefill": (_i, [ct for _, ct in BACKWARD_PREFILL_PARAMS]),
    "sks_prefill_planes": (_i, [_i, _i, _i, _i, _i, _u, C.POINTER(_i), C.POINTER(_i)]),
    "sks_mark_visible": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    "sks_mean_views": (_i, [_i, _i, _vp, _i, _vp, _vp]),
    "sks_export_lists": (_i, [_i, _i, _i, _vp, _sz, _vp, _vp, _vp]),
    "sks_masked_l2": (_i, [_i, _sz, _vp, _vp, _vp, _vp, _vp]),
    "sks_masked_l2_launch": (_i, [_sz, C.POINTER(_i)]),
    "sks_masked_l2_loss": (_i, [_i, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "sks_fused_ssim_fwd": (_i, [_i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_fused_ssim_bwd": (_i, [_i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_fused_ssim_bwd_uniform": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "sks_fused_ssim_mean": (_i, [_i, _i, _i, _i, _f, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_knn3_meandist2": (_i, [_i, _vp, _vp, _vp]),
    "sks_knn3_scratch_bytes": (_sz, [_i]),
    "sks_knn3_meandist2_grid": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
    "sks_softargmax_scratch_bytes": (_sz, [_i, _i, _i]),
    "sks_softargmax_fwd": (_i, [_i, _i, _i, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sks_softargmax_bwd": (_i, [_i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "sks_heatmaps": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_heatmap_factors": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "sks_heatmap_totals": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_gt_tile_stats": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "sks_geometry": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _u, _vp, _vp, _vp, _i, _vp]),
    "sks_backward_fused_loss": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _u,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_loop_pack_grads": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_loop_shard_floats": (_sz, [_i, _i, _i]),
    "sks_adam_multi": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, _vp]),
    "sks_triangulate": (_i, [_i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_triangulate_robust": (_i, [_i, _i, _i, _vp, _sz, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_fuse_predictions": (_i, [_i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "sks_reproject": (_i, [_i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_eval_reprojection": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "sks_triangulate_refine": (_i, [_i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, _vp, _vp, _vp]),
    "sks_smooth_sequence": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "sks_smooth_launch": (_i, [_i, _i, _i, _vp]),
    "sks_eval_accel": (_i, [_i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "sks_bone_measure": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp]),
    "sks_bone_lengths": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "sks_bone_project": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, C.c_double, _i, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "sks_bones_launch": (_i, [_i, _i, _i, _i, _vp]),
    "sks_associate_people": (_i, [_i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, C.c_double, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp]),
    "sks_track_people": (_i, [_i, _i, _i, _vp, _vp, _i, C.c_double, _i, _i, _vp, _vp, _vp, _vp]),
    "sks_people_launch": (_i, [_i, _i, _vp]),
    **{name: (_i, [ct for _, ct in params]) for name, params in {**STEP_PARAMS, **DV_PARAMS, **VW_STEP_PARAMS}.items()},
    "sks_pose_errors": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp]),
    "sks_loop_report": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "sks_eval_sequence": (_i, [_i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "sks_joint_uncertainty": (_i, [_i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    "sks_view_footprints": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "sks_calibration": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "sks_align_poses": (_i, [_i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "sks_eval_sequence_aligned": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp, _vp]),
    "sks_eval_sequence_aligned_scratch_bytes": (_sz, [_i, _i]),
    "sks_preview_planes": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "sks_preview_factors": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sks_preview_scratch_bytes": (_sz, [_i, _i, _i]),
    "sks_preview_launch": (_i, [_i, _i, _i, _vp]),
    "sks_prof_enable": (_i, [_i]),
    "sks_prof_spin": (_i, [C.c_double, _vp]),
    "sks_prof_read": (_i, [_i, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "sks_prof_count": (_i, [_i, C.POINTER(C.c_longlong)]),
    "sks_prof_read_quantiles": (_i, [_i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
}


_PREFILL_SYMBOLS = ("sks_forward_prefilled", "sks_backward_prefill", "sks_prefill_planes")
HAS_PREFILL = True      # False only for an SKS_LIB_OVERRIDE library that predates the prefill pair (load)


def load(build_if_missing=True):
    """Returns the loaded CDLL; raises ImportError with the build error if it cannot be produced."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing:
        try:
            from . import build as _b
            if _b._stale():
                _b.build()
        except Exception as e:  # no hipcc on this box: fall through to the prebuilt .so
            if not os.path.exists(LIB_PATH):
                raise ImportError(f"libskelsplat_hip.so is missing and could not be built: {e}") from e
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found; run `python -m skelsplat_amd.build`")
    override = os.environ.get("SKS_LIB_OVERRIDE")
    lib = C.CDLL(override or LIB_PATH)   # override: A/B of build variants (tools/ab_libs.sh)
    global HAS_PREFILL
    for name, (res, args) in SIGNATURES.items():
        if override and name in _PREFILL_SYMBOLS and not hasattr(lib, name):
            HAS_PREFILL = False      # an A/B against a build from before the prefill pair: its Workspace keeps one output set
            continue
        if override and name in VW_STEP_PARAMS and not hasattr(lib, name):
            continue                 # an A/B against a build from before view agreement: only view_weighting=None runs on it
        fn = getattr(lib, name)  # AttributeError = ABI drift, fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().sks_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def scratch_bytes(V, P, C_, W, H, bin_capacity=0):
    g, b, a = _sz(0), _sz(0), _sz(0)
    check(load().sks_scratch_bytes(V, P, C_, W, H, bin_capacity, C.byref(g), C.byref(b), C.byref(a)), "sks_scratch_bytes")
    return g.value, b.value, a.value


# sks_launch_regime's record: field name -> index (include/skelsplat_hip.h, SKS_REGIME_*)
REGIME_FIELDS = ("path", "cover", "cw", "ppt", "half", "rowmode", "pb", "fsplit", "w_magic", "bwd", "gx", "gy", "bpc", "wave_groups",
                 "lead")
REGIME_INTS = 16
PATH_SMALL, PATH_BINNED = 0, 1
COVER_NONE, COVER_PER_VIEW, COVER_PER_PLANE = 0, 1, 2
BWD_WAVE, BWD_GATHER, BWD_TILE = 0, 1, 2


def launch_regime(V, P, C_, W, H, flags=0, out_aligned128=True):
    """Which launch forms a call of this shape takes, as a dict over REGIME_FIELDS (the library's own answer, host only:
    sks_launch_regime)."""
    out = (_i * REGIME_INTS)()
    check(load().sks_launch_regime(V, P, C_, W, H, flags, 1 if out_aligned128 else 0, out), "sks_launch_regime")
    return {name: out[i] for i, name in enumerate(REGIME_FIELDS)}


# sks_list_regime's record: field name -> index (include/skelsplat_hip.h, SKS_LIST_*)
LIST_REGIME_FIELDS = ("wave_sort", "wave_k", "sort_lds", "long_list", "classes", "band_threads")
LIST_REGIME_INTS = 8


def list_regime():
    """The list lengths at which the binned path switches sorter or walk, as a dict over LIST_REGIME_FIELDS (host only:
    sks_list_regime)."""
    out = (_i * LIST_REGIME_INTS)()
    check(load().sks_list_regime(out), "sks_list_regime")
    return {name: out[i] for i, name in enumerate(LIST_REGIME_FIELDS)}


def masked_l2_launch(n_per_view):
    """(workgroups per view, threads per workgroup) of sks_masked_l2 for views of n_per_view elements (host only:
    sks_masked_l2_launch)."""
    out = (_i * 2)()
    check(load().sks_masked_l2_launch(n_per_view, out), "sks_masked_l2_launch")
    return out[0], out[1]


# sks_preview_launch's record: field name -> index (include/skelsplat_hip.h, SKS_PREVIEW_*)
PREVIEW_LAUNCH_FIELDS = ("load_bytes", "store_bytes", "groups_sum", "groups_pack")


def preview_launch(W, H, aligned=True):
    """Which forms sks_preview_planes takes for views of W x H, as a dict over PREVIEW_LAUNCH_FIELDS (host only:
    sks_preview_launch).  aligned: every base pointer is a multiple of 16."""
    out = (_i * SKS_PREVIEW_LAUNCH_INTS)()
    check(load().sks_preview_launch(W, H, 1 if aligned else 0, C.cast(out, _vp)), "sks_preview_launch")
    return {name: out[i] for i, name in enumerate(PREVIEW_LAUNCH_FIELDS)}


# sks_smooth_launch's record: field name -> index (include/skelsplat_hip.h, SKS_SMOOTH_*)
SMOOTH_LAUNCH_FIELDS = ("tile", "groups", "threads", "lds_bytes")


def smooth_launch(N, J, half_window):
    """The launch sks_smooth_sequence makes for N frames of J joints, as a dict over SMOOTH_LAUNCH_FIELDS: the tile length T in
    frames, the workgroups, the threads per workgroup and a workgroup's LDS bytes (host only: sks_smooth_launch)."""
    out = (_i * SKS_SMOOTH_LAUNCH_INTS)()
    check(load().sks_smooth_launch(N, J, half_window, C.cast(out, _vp)), "sks_smooth_launch")
    return {name: out[i] for i, name in enumerate(SMOOTH_LAUNCH_FIELDS)}


# sks_bones_launch's record: field name -> index (include/skelsplat_hip.h, SKS_BONES_*)
BONES_LAUNCH_FIELDS = ("measure_groups", "measure_threads", "lengths_groups", "lengths_threads", "lengths_lds_bytes",
                       "project_groups", "project_threads", "project_lds_bytes")


def bones_launch(N, J, B, n_groups=1):
    """The three launches of sks_bone_measure / sks_bone_lengths / sks_bone_project for N frames of J joints, B bones and
    n_groups recordings, as a dict over BONES_LAUNCH_FIELDS: workgroups, threads per workgroup and a workgroup's LDS bytes (host
    only: sks_bones_launch)."""
    out = (_i * SKS_BONES_LAUNCH_INTS)()
    check(load().sks_bones_launch(N, J, B, n_groups, C.cast(out, _vp)), "sks_bones_launch")
    return {name: out[i] for i, name in enumerate(BONES_LAUNCH_FIELDS)}


# sks_people_launch's record: field name -> index (include/skelsplat_hip.h, SKS_PEOPLE_*)
PEOPLE_LAUNCH_FIELDS = ("assoc_threads", "assoc_lds_bytes", "assoc_list_entries", "track_threads")


def people_launch(V, M):
    """The association's workgroup for V views of M candidate slots, as a dict over PEOPLE_LAUNCH_FIELDS: its threads, its LDS
    bytes and the entries of its edge list; and the tracker's threads (host only: sks_people_launch)."""
    out = (_i * SKS_PEOPLE_LAUNCH_INTS)()
    check(load().sks_people_launch(V, M, C.cast(out, _vp)), "sks_people_launch")
    return {name: out[i] for i, name in enumerate(PEOPLE_LAUNCH_FIELDS)}


def prefill_planes(V, P, C_, W, H, flags=0):
    """(planes_wave, planes_geom): how many of the call's last planes the small-path backward's two launches zero for the next forward
    (the library's rule, sks_prefill_planes; (0, 0) = no prefill for this call)."""
    nw, ng = _i(0), _i(0)
    check(load().sks_prefill_planes(V, P, C_, W, H, flags, C.byref(nw), C.byref(ng)), "sks_prefill_planes")
    return nw.value, ng.value


def ptr(t):
    """Device pointer of a tensor, or None.  Empty tensors are the reference's "not provided" sentinel."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def farray(vals):
    return (C.c_float * len(vals))(*[float(v) for v in vals])


def prof_count(kind):
    """Bracketed launches of one kind collected since the last read."""
    n = C.c_longlong(0)
    check(load().sks_prof_count(kind, C.byref(n)), "sks_prof_count")
    return n.value


def prof_enable(on, every=1, kinds=(0, 1), recorded=False):
    """Bracket the forward (kind 0) / backward (kind 1) compositor launches with hipEvents: every `every`-th launch of each
    kind in `kinds`.  What was collected so far stays until it is read (a caller may change the stride mid-collection)."""
    skip = sum(1 << (16 + k) for k in (0, 1) if k not in kinds)
    check(load().sks_prof_enable((min(0xffff, max(1, int(every))) | skip | ((1 << 18) if recorded else 0)) if on else 0),
          "sks_prof_enable")


def prof_read_quantiles(kind):
    """(total_ms, launches, (p10_ms, p50_ms, p90_ms)) of the bracketed launches of one kind since the last read."""
    q = (C.c_double * 3)()
    ms, n = C.c_double(0), C.c_longlong(0)
    check(load().sks_prof_read_quantiles(kind, q, C.byref(ms), C.byref(n)), "sks_prof_read_quantiles")
    return ms.value, n.value, (q[0], q[1], q[2])


def prof_read(kind):
    """(total_ms, launches) of the forward (kind 0) / backward (kind 1) compositor kernel since the last read."""
    ms, n = C.c_double(0), C.c_longlong(0)
    check(load().sks_prof_read(kind, C.byref(ms), C.byref(n)), "sks_prof_read")
    return ms.value, n.value
