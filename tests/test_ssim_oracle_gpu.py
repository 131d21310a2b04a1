"""Fused SSIM on the GPU against the fixed-sequence CPU oracle (oracle/sks_ssim_oracle.c, float build), bit for bit.

Comparison is by value (-0 equals +0, nan equals nan).  Every pixel is exact, except where the oracle flags a quotient
outside the range in which the kernels' division sequence is IEEE `/` (a nonzero |n| < 2^-100, or d outside
[2^-100, 2^100); tests/test_ssim_oracle_cpu.py::test_division_sequence_is_ieee_division_in_its_range).  There each quotient
is within one ulp of the oracle's, so ssim_map, dm_dsigma1_sq and dm_dsigma12 (one quotient each) are within one ulp of the
oracle's value, and dm_dmu1 = ((q1 - q2) - q3) + q4 within 2 x sum ulp(q_i): the quotients' own ulps, and the three
additions, each of which rounds once more and moves by no more than what came in.  Nothing is measured on the kernels to
set these bounds.  The backward contains no division: exact everywhere.

Each test prints what it saw on flagged pixels ("ssim-oracle ..." lines, pytest -s) for MEASUREMENTS.md.

Not compared: the uniform backward with crop > 0 on non-finite partial maps.  The kernel skips the rows outside the crop
altogether (contributing 0) where the materialised gradient gives 0 x nan = nan; on finite maps the two are the same bits.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ssim_ref
from skelsplat_amd import _lib
from tests import ssim_cases as sc

pytestmark = pytest.mark.gpu

PARTS = ("dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12")
FLAG = dict(map=ssim_ref.FLAG_MAP, dm_dmu1=ssim_ref.FLAG_DMU1, dm_dsigma1_sq=ssim_ref.FLAG_DSIGMA1_SQ,
            dm_dsigma12=ssim_ref.FLAG_DSIGMA12)
CASES = sc.case_list()


@functools.lru_cache(maxsize=None)
def _oracle(name, shape):
    c = sc.make(name, shape)
    o = ssim_ref.forward(c.img1, c.img2, c.C1, c.C2)
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, o


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev(a, dev, offset=False):
    """The array on the device; offset: a contiguous view 4 bytes into its buffer (not 16-byte aligned)."""
    t = torch.tensor(np.asarray(a, dtype=np.float32))
    if not offset:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _empty(shape, dev, offset=False):
    return _dev(np.zeros(shape, np.float32), dev, offset)


def gpu_forward(dev, c, train=True, offset=False):
    B, CH, H, W = c.shape
    a, b = _dev(c.img1, dev, offset), _dev(c.img2, dev, offset)
    out = [_empty(c.shape, dev, offset) for _ in range(4 if train else 1)]
    ptrs = [t.data_ptr() for t in out] + [None] * (4 - len(out))
    rc = _lib.load().sks_fused_ssim_fwd(B, CH, H, W, c.C1, c.C2, a.data_ptr(), b.data_ptr(), *ptrs, _stream(dev))
    _lib.check(rc, "sks_fused_ssim_fwd")
    return dict(zip(("map",) + PARTS, (t.cpu().numpy() for t in out)))


def gpu_mean(dev, c, crop, train, scratch):
    B, CH, H, W = c.shape
    a, b = _dev(c.img1, dev), _dev(c.img2, dev)
    parts = [_empty(c.shape, dev) for _ in range(3)] if train else []
    ptrs = [t.data_ptr() for t in parts] + [None] * (3 - len(parts))
    mean = torch.empty((), dtype=torch.float32, device=dev)
    rc = _lib.load().sks_fused_ssim_mean(B, CH, H, W, c.C1, c.C2, a.data_ptr(), b.data_ptr(), crop, *ptrs,
                                         scratch.data_ptr(), mean.data_ptr(), _stream(dev))
    _lib.check(rc, "sks_fused_ssim_mean")
    return np.float32(mean.item()), dict(zip(PARTS, (t.cpu().numpy() for t in parts)))


def gpu_backward(dev, c, dL, parts, offset=False):
    B, CH, H, W = c.shape
    ts = [_dev(x, dev, offset) for x in (c.img1, c.img2, dL, *parts)]
    out = _empty(c.shape, dev, offset)
    rc = _lib.load().sks_fused_ssim_bwd(B, CH, H, W, c.C1, c.C2, *[t.data_ptr() for t in ts], out.data_ptr(), _stream(dev))
    _lib.check(rc, "sks_fused_ssim_bwd")
    return out.cpu().numpy()


def gpu_backward_uniform(dev, c, dL_value, dL_scale, crop, parts):
    B, CH, H, W = c.shape
    a, b = _dev(c.img1, dev), _dev(c.img2, dev)
    g = torch.tensor(dL_value, dtype=torch.float32, device=dev)
    ps = [_dev(x, dev) for x in parts]
    out = _empty(c.shape, dev)
    rc = _lib.load().sks_fused_ssim_bwd_uniform(B, CH, H, W, a.data_ptr(), b.data_ptr(), g.data_ptr(), dL_scale, crop,
                                                *[t.data_ptr() for t in ps], out.data_ptr(), _stream(dev))
    _lib.check(rc, "sks_fused_ssim_bwd_uniform")
    return out.cpu().numpy()


def same(a, b):
    """Elementwise equality by value: -0 == +0, nan == nan."""
    return (a == b) | (np.isnan(a) & np.isnan(b))


def assert_same(tag, got, want):
    ok = same(got, want)
    assert ok.all(), f"{tag}: {(~ok).sum()} / {ok.size} pixels differ from the oracle, first at {np.argwhere(~ok)[0].tolist()}"


def assert_forward(tag, got, o, keys, nonfinite=False):
    """Exact where the oracle raises no flag for that output; within the derived bound where it does."""
    for k in keys:
        want = o[k]
        if nonfinite:   # the same non-finite pixels, every finite pixel exact
            assert np.array_equal(np.isfinite(got[k]), np.isfinite(want)), f"{tag} {k}: the non-finite pixels differ"
            assert_same(f"{tag} {k}", got[k], want)
            continue
        fl = (o["flags"] & FLAG[k]) != 0
        assert_same(f"{tag} {k} (unflagged)", got[k][~fl], want[~fl])
        if fl.any():
            with np.errstate(invalid="ignore"):
                bound = 2.0 * o["ulp_sum"][fl].astype(np.float64) if k == "dm_dmu1" else np.spacing(np.abs(want[fl])).astype(np.float64)
                err = np.abs(got[k][fl].astype(np.float64) - want[fl].astype(np.float64))
            worst = float(np.max(err / bound))
            print(f"ssim-oracle {tag} {k}: {int(fl.sum())} flagged, {int((err > 0).sum())} of them differ, "
                  f"worst deviation {worst:.3f} x its bound")
            assert (err <= bound).all(), f"{tag} {k}: {(err > bound).sum()} flagged pixels beyond their bound, worst {worst:.2f} x"


def windows(c, half):
    """Pixels within `half` of a non-finite input pixel, per plane."""
    bad = ~np.isfinite(c.img1) | ~np.isfinite(c.img2)
    out = np.zeros(c.shape, bool)
    for b, ch, y, x in np.argwhere(bad):
        out[b, ch, max(y - half, 0):y + half + 1, max(x - half, 0):x + half + 1] = True
    return out


# ---- forward ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", CASES, ids=sc.case_id)
def test_forward_is_the_oracle(device, name, shape):
    """sks_fused_ssim_fwd (train, inference) and sks_fused_ssim_mean (with and without the partial maps)."""
    c, o = _oracle(name, shape)
    nf = name == "nonfinite"
    tag = f"{name} {sc.case_id(shape)}"
    print(f"ssim-oracle {tag}: {int((o['flags'] != 0).sum())} / {o['flags'].size} pixels flagged, "
          f"{o['outside_documented']} quotients outside d in [2^-40, 2^8), |n| in [2^-60, 2^12)")
    got = gpu_forward(device, c, train=True)
    assert_forward(tag + " train", got, o, ("map",) + PARTS, nf)
    assert_forward(tag + " inference", gpu_forward(device, c, train=False), o, ("map",), nf)
    if nf:
        for k in ("map",) + PARTS:
            assert not (~np.isfinite(got[k]) & ~windows(c, 5)).any(), f"{k}: non-finite outside the 11 x 11 windows"
    scratch = torch.zeros(64, dtype=torch.float64, device=device)
    H, W = shape[2:]
    for crop in (0, 5):
        want = ssim_ref.mean(o["map"], crop)
        m_train, parts = gpu_mean(device, c, crop, True, scratch)
        assert_forward(f"{tag} mean crop {crop}", parts, o, PARTS, nf)   # the mean form's partial maps are the map form's
        means = [m_train] + [gpu_mean(device, c, crop, False, scratch)[0] for _ in range(2)]
        if H <= 2 * crop or W <= 2 * crop or nf and not np.isfinite(want):
            assert np.isnan(want) and all(np.isnan(m) for m in means)   # an empty "valid" map
            continue
        # the scratch is zero again after every call: three calls in a row agree (the slots' sums depend on the
        # order the workgroups arrive in, so "agree" is to the last place of the double sum: the same float or its neighbour)
        for m in means:
            assert abs(float(m) - float(want)) <= float(np.spacing(np.abs(want))), (tag, crop, means, want)
    assert float(scratch.abs().max().item()) == 0.0


@pytest.mark.parametrize("min_blocks", sc.MIN_BLOCKS, ids=["strips-of-8", "strips-of-2", "strips-of-1"])
@pytest.mark.parametrize("name", ["seams", "checker-shift", "heatmaps", "noise"])
def test_strips_of_every_length_are_the_oracle(device, name, min_blocks, monkeypatch):
    """10 tile rows: the 10 filtered rows handed from tile to tile, forward and backward."""
    monkeypatch.setenv("SKS_SSIM_MIN_BLOCKS", min_blocks)
    c, o = _oracle(name, sc.SHAPE_TALL)
    tag = f"{name} strips {min_blocks}"
    got = gpu_forward(device, c, train=True)
    assert_forward(tag, got, o, ("map",) + PARTS)
    dL = np.random.default_rng(3).uniform(-1, 1, c.shape).astype(np.float32)
    parts = [o[k] for k in PARTS]
    assert_same(tag + " dL_dimg1", gpu_backward(device, c, dL, parts), ssim_ref.backward(c.img1, c.img2, dL, *parts))
    scratch = torch.zeros(64, dtype=torch.float64, device=device)
    want = ssim_ref.mean(o["map"], 5)
    assert abs(float(gpu_mean(device, c, 5, False, scratch)[0]) - float(want)) <= float(np.spacing(np.abs(want)))


@pytest.mark.parametrize("name", ["seams", "heatmaps", "checker-shift"])
def test_unaligned_buffers_are_the_oracle(device, name):
    """W % 4 == 0 but every pointer 4 bytes past a 16-byte boundary: the scalar-load path."""
    c, o = _oracle(name, sc.SHAPE_VEC)
    assert_forward(f"{name} unaligned", gpu_forward(device, c, train=True, offset=True), o, ("map",) + PARTS)
    dL = np.random.default_rng(4).uniform(-1, 1, c.shape).astype(np.float32)
    parts = [o[k] for k in PARTS]
    assert_same(f"{name} unaligned dL_dimg1", gpu_backward(device, c, dL, parts, offset=True),
                ssim_ref.backward(c.img1, c.img2, dL, *parts))


# ---- backward --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", CASES, ids=sc.case_id)
def test_backward_is_the_oracle(device, name, shape):
    """sks_fused_ssim_bwd called directly, (a) on the kernel's own partial maps under a random dL_dmap, (b) on arbitrary
    partial maps (magnitudes up to 1e4, mixed signs, unrelated to any image): exact everywhere, in every class."""
    c, _ = _oracle(name, shape)
    rng = np.random.default_rng(7)
    dL = rng.uniform(-1, 1, c.shape).astype(np.float32)
    own = gpu_forward(device, c, train=True)
    parts = [own[k] for k in PARTS]
    got, want = gpu_backward(device, c, dL, parts), ssim_ref.backward(c.img1, c.img2, dL, *parts)
    assert_same(f"{name} (a) dL_dimg1", got, want)
    if name == "nonfinite":
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
        assert not (~np.isfinite(got) & ~windows(c, 10)).any(), "non-finite outside the 21 x 21 windows"
        assert np.isfinite(got).any() or min(shape[2:]) < 21
    rand = [(rng.uniform(-1, 1, c.shape) * 10.0 ** rng.uniform(-4, 4, c.shape)).astype(np.float32) for _ in range(3)]
    assert_same(f"{name} (b) dL_dimg1", gpu_backward(device, c, dL, rand), ssim_ref.backward(c.img1, c.img2, dL, *rand))


@pytest.mark.parametrize("name,shape", [(n, s) for n in ("heatmaps", "noise", "seams", "flat-noisy-hi") for s in sc.MAIN_SHAPES] +
                         [("checker-shift", sc.SHAPE_SHORT), ("checker-shift", sc.SHAPE_TINY)], ids=sc.case_id)
@pytest.mark.parametrize("crop", [0, 5])
def test_uniform_backward_is_the_oracle(device, name, shape, crop):
    """sks_fused_ssim_bwd_uniform with dL_scale != 1: the same bits as sks_fused_ssim_bwd on the materialised gradient
    image, and as the oracle's uniform backward."""
    c, o = _oracle(name, shape)
    parts = [o[k] for k in PARTS]
    H, W = shape[2:]
    value, scale = 0.75, 1.0 / 77
    got = gpu_backward_uniform(device, c, value, scale, crop, parts)
    dL = np.zeros(c.shape, np.float32)
    if H > 2 * crop and W > 2 * crop:
        dL[:, :, crop:H - crop, crop:W - crop] = np.float32(value) * np.float32(scale)
    assert_same(f"{name} crop {crop} against the materialised gradient", got, gpu_backward(device, c, dL, parts))
    assert_same(f"{name} crop {crop} against the oracle", got, ssim_ref.backward_uniform(c.img1, c.img2, value, scale, crop, *parts))
    assert (got != 0).any() or not dL.any()


# ---- the public surface ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["heatmaps", "constants"])
@pytest.mark.parametrize("shape", sc.MAIN_SHAPES, ids=sc.case_id)
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_map_function_is_the_oracle(device, name, shape, padding):
    """FusedSSIMMap.apply(...).backward(): constants are arguments, the "valid" crop is the oracle's map [5:-5, 5:-5]."""
    from fused_ssim import FusedSSIMMap
    c, o = _oracle(name, shape)
    x = torch.tensor(c.img1, device=device).requires_grad_(True)
    m = FusedSSIMMap.apply(c.C1, c.C2, x, torch.tensor(c.img2, device=device), padding, True)
    want = o["map"][:, :, 5:-5, 5:-5] if padding == "valid" else o["map"]
    assert m.shape == want.shape
    assert_same(f"{name} {padding} map", m.detach().cpu().numpy(), want)
    w = np.random.default_rng(8).uniform(-1, 1, want.shape).astype(np.float32)
    m.backward(torch.tensor(w, device=device))
    dL = np.zeros(c.shape, np.float32)
    if padding == "valid":
        dL[:, :, 5:-5, 5:-5] = w
    else:
        dL[:] = w
    assert_same(f"{name} {padding} dL_dimg1", x.grad.cpu().numpy(), ssim_ref.backward(c.img1, c.img2, dL, *[o[k] for k in PARTS]))


@pytest.mark.parametrize("shape", sc.MAIN_SHAPES, ids=sc.case_id)
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_fused_ssim_is_the_oracle(device, shape, padding):
    """fused_ssim(...) and its backward on the heat-map class: the mean within one fp32 ulp (double sums in another
    order, count x 2^-53 relative), the gradient the oracle's uniform backward bit for bit."""
    from fused_ssim import fused_ssim
    c, o = _oracle("heatmaps", shape)
    crop = 5 if padding == "valid" else 0
    x = torch.tensor(c.img1, device=device).requires_grad_(True)
    val = fused_ssim(x, torch.tensor(c.img2, device=device), padding=padding)
    want = ssim_ref.mean(o["map"], crop)
    assert abs(float(val.item()) - float(want)) <= float(np.spacing(np.abs(want)))
    (3.0 * val).backward()
    B, CH, H, W = shape
    count = B * CH * (H - 2 * crop) * (W - 2 * crop)
    assert_same(f"heatmaps {padding} dL_dimg1", x.grad.cpu().numpy(),
                ssim_ref.backward_uniform(c.img1, c.img2, 3.0, 1.0 / count, crop, *[o[k] for k in PARTS]))
