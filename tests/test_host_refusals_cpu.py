"""What the host layer of the rasterizer refuses, and in which order (csrc/sks_raster.hip, csrc/sks_loop.hip): for each of 14
entry points a table of calls that are refused BEFORE the first HIP runtime call, each row with its exact return code and its
exact sks_last_error() text.  Rows that break two rules at once pin which refusal wins.

No device is needed and none may be present: host-read arguments (the tangents, lr_sched, lrs, adam, limb, view_wh, gt_offsets,
the hm_factors row) are real ctypes arrays, every device pointer is a placeholder address -- a refusal that went missing would
launch on made-up pointers, so the module is skipped where a GPU is available.

Not covered: P == 0 (it reaches hipMemsetAsync), and backward_impl's "view group %d of %d" (no entry point of the C ABI can ask
for a group the call does not have: sks_backward passes none, sks_forward_backward's hook counts with the same bin_groups)."""
import ctypes

import pytest
import torch

from skelsplat_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="a refusal that went missing would launch on made-up pointers")

X = 0x10000          # a device pointer no refused call touches (128-byte aligned)
_KEEP = []           # the host arrays stay alive for the module's life


def _host(ctype, vals):
    arr = (ctype * len(vals))(*vals)
    _KEEP.append(arr)
    return ctypes.cast(arr, ctypes.c_void_p)


TAN = _host(ctypes.c_float, [1.0] * 64)
LR_SCHED = _host(ctypes.c_double, [1e-3, 1e-5, 0.01, 0.0, 100.0])
LRS = _host(ctypes.c_double, [5e-3, 1e-3, 5e-2])
ADAM = _host(ctypes.c_double, [0.9, 0.999, 1e-15])
LIMB_OK = _host(ctypes.c_int, [0, 1, 2, 3, 4, 5, 6, 16])
LIMB_HIGH = _host(ctypes.c_int, [0, 1, 2, 3, 4, 5, 6, 17])
LIMB_NEG = _host(ctypes.c_int, [0, -1, 2, 3, 4, 5, 6, 7])
WH_OK = _host(ctypes.c_int, [64, 48, 60, 40])
WH_WIDE = _host(ctypes.c_int, [64, 48, 65, 48])
WH_ZERO = _host(ctypes.c_int, [64, 48, 64, 0])
GT_OFF = _host(ctypes.c_size_t, [0, 4 * 64 * 48])
HM_OK = _host(ctypes.c_void_p, [X, X, X, X])
HM_HOLES = [_host(ctypes.c_void_p, [X if k != i else None for k in range(4)]) for i in range(4)]

# the calls every table starts from: V=2 P=17 C=4 64x48, small path, every pointer given except the optional ones
SHAPE = dict(V=2, P=17, C=4, W=64, H=48)
OPTIONAL = ("cov3D_precomp", "final_T", "n_contrib", "stream", "aux_stream", "view_wh", "gt_offsets", "hm_factors", "limb", "bg")
VALUES = dict(SHAPE, tanfovx=TAN, tanfovy=TAN, scale_modifier=1.0, flags=0, bin_capacity=0, prefilled_planes=0, planes_wave=0,
              planes_geom=0, fb_flags=0, frames=1, group_mask=3, last_view=1, acc_steps=1, lr_sched=LR_SCHED, lrs=LRS, adam=ADAM,
              lambda_consistency=0.0, shard_world=1, es_window=4, es_tolerance=1e-4)

FUSED_LOSS = ("V P C W H viewmatrix projmatrix tanfovx tanfovy bg means3D features opacities scales rotations cov3D_precomp "
              "scale_modifier flags radii geom gt tile_S tile_N gt_totals accum dL_dmeans3D dL_dmeans2D dL_dopacity dL_dscales "
              "dL_drotations dL_dcov3D loss_sums packed_raw_grads view_wh gt_offsets hm_factors stream").split()
GEOMETRY = ("V P C W H viewmatrix projmatrix tanfovx tanfovy means3D opacities scales rotations cov3D_precomp scale_modifier "
            "flags radii geom view_wh frames stream").split()
NAMES = {
    "sks_forward": [n for n, _ in _lib.FORWARD_PARAMS],
    "sks_forward_prefilled": [n for n, _ in _lib.FORWARD_PREFILLED_PARAMS],
    "sks_backward": [n for n, _ in _lib.BACKWARD_PARAMS],
    "sks_backward_prefill": [n for n, _ in _lib.BACKWARD_PREFILL_PARAMS],
    "sks_forward_backward": [n for n, _ in _lib.FORWARD_BACKWARD_PARAMS],
    "sks_backward_fused_loss": FUSED_LOSS,
    "sks_geometry": GEOMETRY,
    "sks_geometry_dv": [n for n, _ in _lib.GEOMETRY_DV_PARAMS],
    **{name: [n for n, _ in params] for name, params in _lib.STEP_PARAMS.items()},
    "sks_loop_fused_step_dv": [n for n, _ in _lib.LOOP_FUSED_STEP_DV_PARAMS],
    "sks_loop_fused_step_es_dv": [n for n, _ in _lib.LOOP_FUSED_STEP_ES_DV_PARAMS],
}

MISSING = (-2, "missing required pointer")
NEED_COV = (-2, "need scales+rotations or cov3D_precomp")
HM_ROW = (-2, "hm_factors: row, col, cmin, den must all be given")
VIEW_WH = (-1, "view_wh: every view's size must be within [1, W] x [1, H] (pass the largest as W, H)")
TOGETHER = (-2, "view_wh and gt_offsets go together")
NO_PREFILL = (-1, "sks_backward_prefill: no prefill for this call (wave-resident small path with 16-byte non-temporal stores only: "
                  "1 <= P <= 64, W % 4 == 0 or W % 4 == 2 with an even H, no SKS_NO_NT_STORES / SKS_DEBUG_SYNC / SKS_FORCE_BINNED)")
ADAM_MISSING = (-2, "loop_adam: missing pointer")
LAST_VIEW = (-2, "loop_adam: last_view out of range")
LIMB = (-2, "loop_adam: limb index out of range")


def common_rows():
    """Each range check of check_common, and that the first one in V, P, C, W x H order wins."""
    return [(dict(V=0), -1, "V=0 out of range [1,64]"), (dict(V=65), -1, "V=65 out of range [1,64]"),
            (dict(P=-1), -1, "P=-1 negative"), (dict(C=0), -1, "C=0 out of range [1,32]"), (dict(C=33), -1, "C=33 out of range [1,32]"),
            (dict(W=0), -1, "image 0x48 out of range"), (dict(H=0), -1, "image 64x0 out of range"),
            (dict(W=4096 * 16 + 1), -1, "image 65537x48 out of range"), (dict(H=65535 * 16 + 1), -1, "image 64x1048561 out of range"),
            (dict(V=0, C=0), -1, "V=0 out of range [1,64]"), (dict(C=33, W=0), -1, "C=33 out of range [1,32]")]


def each_missing(names, refusal=MISSING, **also):
    return [({n: None, **also}, *refusal) for n in names]


def cov_rows():
    return [(dict(scales=None), *NEED_COV), (dict(rotations=None), *NEED_COV), (dict(scales=None, rotations=None), *NEED_COV)]


def forward_rows():
    """forward_impl, reached through sks_forward, sks_forward_prefilled and (no second stream) sks_forward_backward."""
    aligned = "out_color / out_invdepth must be 16-byte aligned (the planes are written with 16-byte stores)"
    binned = _lib.SKS_FORCE_BINNED
    return common_rows() + [
        (dict(out_color=None), -2, "out_color / out_invdepth must be provided"),
        (dict(out_invdepth=None), -2, "out_color / out_invdepth must be provided"),
        (dict(out_color=X + 4), -2, aligned), (dict(out_invdepth=X + 8), -2, aligned),
        *each_missing(("viewmatrix", "projmatrix", "tanfovx", "tanfovy", "means3D", "features", "opacities", "radii", "geom")),
        *cov_rows(),
        (dict(flags=binned, binning=None), -2, "binned path needs a binning buffer"),
        (dict(P=257, binning=None), -2, "binned path needs a binning buffer"),
        (dict(flags=binned), -1, "binned path needs bin_capacity >= 1"),
        (dict(P=257), -1, "binned path needs bin_capacity >= 1"),
        # two rules at once
        (dict(V=0, out_color=None), -1, "V=0 out of range [1,64]"),
        (dict(C=0, out_color=X + 4), -1, "C=0 out of range [1,32]"),
        (dict(out_color=None, out_invdepth=X + 4), -2, "out_color / out_invdepth must be provided"),
        (dict(out_invdepth=X + 4, viewmatrix=None), -2, aligned),
        (dict(geom=None, scales=None), *MISSING),
        (dict(scales=None, flags=binned, binning=None), *NEED_COV),
        (dict(flags=binned, binning=None, bin_capacity=0), -2, "binned path needs a binning buffer")]


def backward_rows():
    """backward_impl, through sks_backward and sks_backward_prefill."""
    return common_rows() + [
        *each_missing(("viewmatrix", "projmatrix", "tanfovx", "tanfovy", "means3D", "features", "opacities", "radii", "geom",
                       "dL_dout_color", "accum", "dL_dmeans3D", "dL_dmeans2D", "dL_dopacity")),
        *cov_rows(),
        (dict(flags=_lib.SKS_FORCE_BINNED, binning=None), -2, "binned path needs the forward's binning buffer"),
        (dict(P=257, binning=None), -2, "binned path needs the forward's binning buffer"),
        (dict(V=65, accum=None), -1, "V=65 out of range [1,64]"),
        (dict(dL_dopacity=None, rotations=None), *MISSING),
        (dict(rotations=None, P=257, binning=None), *NEED_COV)]


def prefill_rows():
    count = "sks_backward_prefill: planes_wave=%d planes_geom=%d out of range (the call has 10 planes)"
    given = "sks_backward_prefill: next_color / next_invdepth must be provided"
    aligned = "next_color / next_invdepth must be 16-byte aligned"
    huge = dict(P=1, C=32, W=4096, H=4096)     # 8192 fill-block rows per plane
    return backward_rows() + [
        (dict(planes_wave=-1), -1, count % (-1, 0)), (dict(planes_geom=-1), -1, count % (0, -1)),
        (dict(planes_wave=6, planes_geom=5), -1, count % (6, 5)), (dict(planes_wave=11), -1, count % (11, 0)),
        (dict(planes_wave=1, W=63), *NO_PREFILL), (dict(planes_geom=1, W=62, H=47), *NO_PREFILL),
        (dict(planes_wave=1, P=65), *NO_PREFILL), (dict(planes_wave=1, flags=_lib.SKS_FORCE_BINNED), *NO_PREFILL),
        (dict(planes_wave=1, flags=_lib.SKS_DEBUG_SYNC), *NO_PREFILL), (dict(planes_wave=1, flags=_lib.SKS_BWD_LDS_LIST), *NO_PREFILL),
        (dict(planes_wave=1, next_color=None), -2, given), (dict(planes_geom=1, next_invdepth=None), -2, given),
        (dict(planes_wave=1, next_color=X + 4), -2, aligned), (dict(planes_geom=1, next_invdepth=X + 8), -2, aligned),
        ({**huge, "V": 1, "planes_wave": 10}, -1,
         "sks_backward_prefill: 10 planes of 4096x4096 do not fit the compositing backward's launch"),
        ({**huge, "V": 2, "planes_geom": 64}, -1,
         "sks_backward_prefill: 64 planes of 4096x4096 do not fit the geometry backward's launch"),
        # two rules at once
        (dict(V=0, planes_wave=-1), -1, "V=0 out of range [1,64]"),
        (dict(planes_wave=-1, W=63), -1, count % (-1, 0)),
        (dict(planes_wave=1, W=63, next_color=None), *NO_PREFILL),
        (dict(planes_wave=1, next_color=None, next_invdepth=X + 4), -2, given),
        (dict(planes_wave=1, next_color=X + 4, viewmatrix=None), -2, aligned),
        (dict(planes_wave=1, viewmatrix=None), *MISSING),
        ({**huge, "V": 1, "planes_wave": 10, "scales": None}, *NEED_COV)]


def prefilled_rows():
    count = "prefilled_planes=%d out of range [0,10]"
    return forward_rows() + [
        (dict(prefilled_planes=-1), -1, count % -1), (dict(prefilled_planes=11), -1, count % 11),
        (dict(V=0, prefilled_planes=-1), -1, "V=0 out of range [1,64]"),
        (dict(prefilled_planes=11, out_color=None), -1, count % 11)]


def heatmap_rows():
    """The hm_factors and view_wh checks of the fused-loss entries (after their required pointers, in this order)."""
    return [*[(dict(hm_factors=h), *HM_ROW) for h in HM_HOLES],
            (dict(hm_factors=HM_HOLES[0], gt=None), *HM_ROW),
            (dict(view_wh=WH_WIDE, gt_offsets=GT_OFF), *VIEW_WH), (dict(view_wh=WH_ZERO, gt_offsets=GT_OFF), *VIEW_WH),
            (dict(view_wh=WH_OK), *TOGETHER), (dict(gt_offsets=GT_OFF), *TOGETHER),
            (dict(view_wh=WH_WIDE), *VIEW_WH), (dict(hm_factors=HM_HOLES[2], view_wh=WH_WIDE), *HM_ROW),
            (dict(hm_factors=HM_OK, gt=None, view_wh=WH_WIDE), *VIEW_WH)]


def fused_loss_rows():
    bad_p = "fused-loss backward needs 1 <= P <= 64 (got %d)"
    return common_rows() + [
        (dict(P=0), -1, bad_p % 0), (dict(P=65), -1, bad_p % 65),
        *each_missing(("viewmatrix", "projmatrix", "tanfovx", "tanfovy", "means3D", "features", "opacities", "radii", "geom", "gt",
                       "gt_totals", "accum", "dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "loss_sums")),
        *heatmap_rows(), *cov_rows(),
        (dict(P=65, viewmatrix=None), -1, bad_p % 65),
        (dict(loss_sums=None, hm_factors=HM_HOLES[1]), *MISSING),
        (dict(hm_factors=HM_HOLES[3], scales=None), *HM_ROW),
        (dict(scales=None, view_wh=WH_WIDE), *NEED_COV)]


def geometry_rows(dv):
    frames = "frames must divide the number of views (V = 2, frames = %d)"
    views = ("views_dev",) if dv else ("tanfovx", "tanfovy")
    rows = common_rows() + [
        (dict(P=0), -1, "P must be positive"), (dict(frames=0), -1, frames % 0), (dict(frames=3), -1, frames % 3),
        *each_missing(("viewmatrix", "projmatrix", *views, "means3D", "opacities", "radii", "geom")), *cov_rows(),
        (dict(P=0, frames=0), -1, "P must be positive"), (dict(frames=3, geom=None), -1, frames % 3),
        (dict(radii=None, rotations=None), *MISSING)]
    if not dv:
        rows += [(dict(view_wh=WH_WIDE), *VIEW_WH), (dict(view_wh=WH_ZERO), *VIEW_WH), (dict(scales=None, view_wh=WH_WIDE), *NEED_COV)]
    return rows


def adam_block_rows(sched):
    """fill_adam_args's texts, as every caller of it reports them (`sched`: the name of the host-read schedule, or None)."""
    ptrs = ("slots", "xyz", "scaling", "rotation", "opacity", "exp_avg", "exp_avg_sq", "counters", "lrs", "adam") + ((sched,) if sched else ())
    return [*each_missing(ptrs, ADAM_MISSING), (dict(last_view=-1), *LAST_VIEW), (dict(last_view=2), *LAST_VIEW),
            (dict(limb=LIMB_HIGH), *LIMB), (dict(limb=LIMB_NEG), *LIMB),
            (dict(counters=None, last_view=2), *ADAM_MISSING), (dict(last_view=2, limb=LIMB_HIGH), *LAST_VIEW),
            (dict(limb=LIMB_OK, last_view=-1), *LAST_VIEW)]


def fused_step_rows(name):
    es, dv = "_es" in name, name.endswith("_dv")
    tag = name[len("sks_"):]
    bad_p = "fused step needs 1 <= P <= 64 (got %d)"
    frames = "frames must divide the number of views (V = 2, frames = %d)"
    rows = []
    if dv:
        tables = (-2, tag + ": views_dev and lr_sched_dev are required")
        rows += [(dict(views_dev=None), *tables), (dict(lr_sched_dev=None), *tables), (dict(views_dev=None, V=0), *tables)]
    if es:
        state = (-2, "%s: es_state is required (%s is the step without a criterion)" % (tag, name.replace("_es", "")))
        window = tag + ": window %d out of range [1, 16]"
        rows += [(dict(es_state=None), *state), (dict(es_window=0), -1, window % 0), (dict(es_window=17), -1, window % 17),
                 (dict(es_state=None, es_window=0), *state), (dict(es_window=17, V=0), -1, window % 17)]
    if es and dv:
        rows += [(dict(lr_sched_dev=None, es_state=None), *tables)]
    rows += common_rows() + [
        (dict(P=0), -1, bad_p % 0), (dict(P=65), -1, bad_p % 65), (dict(frames=0), -1, frames % 0), (dict(frames=3), -1, frames % 3),
        *each_missing(("viewmatrix", "projmatrix", *(() if dv else ("tanfovx", "tanfovy")), "features", "radii", "geom", "gt",
                       "gt_totals", "accum", "loss_sums", "packed")),
        *heatmap_rows(),
        *adam_block_rows(None if dv else "lr_sched"),
        (dict(last_view=1, frames=2), *LAST_VIEW),          # (the optimiser's V is the views of ONE frame)
        (dict(P=65, frames=0), -1, bad_p % 65), (dict(frames=3, packed=None), -1, frames % 3),
        (dict(accum=None, xyz=None), *MISSING), (dict(view_wh=WH_OK, xyz=None), *TOGETHER),
        (dict(view_wh=WH_WIDE, gt_offsets=GT_OFF, last_view=2), *VIEW_WH)]
    return rows


def adam_step_rows(name):
    es = name.endswith("_es")
    shape = (-1, "loop_adam: V or P out of range")
    rows = [(dict(V=0), *shape), (dict(V=65), *shape), (dict(P=0), *shape), (dict(P=257), *shape),
            (dict(shard_world=0), -2, "loop_adam: shard_world must be >= 1"),
            *adam_block_rows("lr_sched"), (dict(grads=None), *ADAM_MISSING),
            (dict(V=0, shard_world=0), *shape), (dict(shard_world=0, grads=None), -2, "loop_adam: shard_world must be >= 1")]
    if es:
        state = (-2, "loop_adam_es: es_state is required (sks_loop_adam_step is the step without a criterion)")
        window = (-1, "loop_adam_es: window out of range [1, 16]")
        sums = (-2, "loop_adam_es: loss_sums is required on one rank")
        rows += [(dict(es_state=None), *state), (dict(es_window=0), *window), (dict(es_window=17), *window), (dict(loss_sums=None), *sums),
                 (dict(P=257, es_state=None), *shape), (dict(es_state=None, es_window=0), *state),
                 (dict(es_window=0, loss_sums=None), *window), (dict(loss_sums=None, shard_world=0), -2, "loop_adam: shard_world must be >= 1")]
    return rows


TABLES = {
    "sks_forward": forward_rows(),
    "sks_forward_prefilled": prefilled_rows(),
    "sks_backward": backward_rows(),
    "sks_backward_prefill": prefill_rows(),
    "sks_forward_backward": forward_rows(),
    "sks_backward_fused_loss": fused_loss_rows(),
    "sks_geometry": geometry_rows(False),
    "sks_geometry_dv": geometry_rows(True),
    "sks_loop_fused_step": fused_step_rows("sks_loop_fused_step"),
    "sks_loop_fused_step_es": fused_step_rows("sks_loop_fused_step_es"),
    "sks_loop_fused_step_dv": fused_step_rows("sks_loop_fused_step_dv"),
    "sks_loop_fused_step_es_dv": fused_step_rows("sks_loop_fused_step_es_dv"),
    "sks_loop_adam_step": adam_step_rows("sks_loop_adam_step"),
    "sks_loop_adam_step_es": adam_step_rows("sks_loop_adam_step_es"),
}
ROWS = {"sks_forward": 38, "sks_forward_prefilled": 42, "sks_backward": 33, "sks_backward_prefill": 56, "sks_forward_backward": 38,
        "sks_backward_fused_loss": 48, "sks_geometry": 31, "sks_geometry_dv": 27, "sks_loop_fused_step": 63,
        "sks_loop_fused_step_es": 68, "sks_loop_fused_step_dv": 63, "sks_loop_fused_step_es_dv": 69, "sks_loop_adam_step": 26,
        "sks_loop_adam_step_es": 34}


def test_the_tables_are_whole():
    assert {name: len(rows) for name, rows in TABLES.items()} == ROWS
    assert len(TABLES) == 14 and sum(len(rows) for rows in TABLES.values()) == 636
    two = sum(1 for rows in TABLES.values() for change, _, _ in rows if len(change) >= 2)
    assert two >= 6
    for name in TABLES:
        assert len(NAMES[name]) == len(_lib.SIGNATURES[name][1]), name


@pytest.mark.parametrize("name", list(TABLES))
def test_refusals(name):
    lib = _lib.load()
    fn = getattr(lib, name)
    names = NAMES[name]
    done = 0
    for change, rc_want, text in TABLES[name]:
        assert set(change) <= set(names), (name, change)
        args = [change[n] if n in change else VALUES.get(n, None if n in OPTIONAL else X) for n in names]
        lib.sks_set_error_(b"")
        rc = fn(*args)
        assert rc != 0, (name, change)
        assert rc == rc_want, (name, change, rc, lib.sks_last_error().decode())
        assert lib.sks_last_error().decode() == text, (name, change)
        done += 1
    assert done == ROWS[name]
