"""GPU tests of skelsplat_amd.keypoints (csrc/sks_keypoint.hip): softargmax2d and the four keypoint criteria against the
float64 restatement of tests/keypoint_ref.py, which tests/test_keypoints_cpu.py holds to the reference's own fp32 results.

Bars.  Coordinates (relative to W - 1 / H - 1) and loss values (relative to the value): DEVICE_FACTOR = 4 times the deviation
of the REFERENCE'S fp32 CPU results from the same restatement over the same cases (keypoint_ref.REF_FP32_DEV_*, measured and
pinned by test_keypoints_cpu.py; MEASUREMENTS.md "softargmax2d").  Gradients with respect to the image: the project's standing
util.assert_close(rtol=1e-3, atol_scale=1e-4) against float64 autograd of the restatement.
Measured on an MI355X: coordinates within 1.1e-7 of the extent on every case, 'mean' / 'sum' values within 3e-7, single 'none'
elements within 2e-4 (every test prints its figures before it asserts)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import guarded
from tests import keypoint_cases as kc
from tests import keypoint_ref as kr
from tests import util

pytestmark = pytest.mark.gpu

COORD_BAR = kr.DEVICE_FACTOR * kr.REF_FP32_DEV_COORD      # of W - 1 / H - 1
LOSS_BAR = kr.DEVICE_FACTOR * kr.REF_FP32_DEV_LOSS        # of the value
REDUCTIONS = ("mean", "sum", "none")
_REF = {}


def reference(name, regime):
    """Float64 references of one case, computed once and shared: image, detections, keypoints, softargmax2d's gradient under
    keypoint_cases.cotangent, and per (criterion, reduction) the value and the gradient (under the same cotangent for the
    elementwise 'none' forms)."""
    key = (name, regime)
    if key not in _REF:
        img = kc.make_image(name, regime)
        x = torch.from_numpy(img).double().requires_grad_(True)
        xy = kr.softargmax2d(x)
        cot = torch.from_numpy(kc.cotangent(img.shape[:2]))
        gt = torch.from_numpy(kc.detections(xy.detach().numpy()))
        ref = {"img": img, "gt_2d": gt, "xy": xy.detach().numpy(), "cot": cot,
               "g_xy": torch.autograd.grad((xy * cot).sum(), x, retain_graph=True)[0].numpy()}
        for c in kr.CRITERIA:
            for red in REDUCTIONS:
                val = kr.reduce(kr.criterion_xy(c, xy, gt), red)
                out = (val * cot).sum() if val.dim() else val
                ref[c, red] = (val.detach().numpy(), torch.autograd.grad(out, x, retain_graph=True)[0].numpy())
        _REF[key] = ref
    return _REF[key]


def coord_dev(got, want, W, H):
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    return max(d[..., 0].max() / max(W - 1, 1), d[..., 1].max() / max(H - 1, 1))


@pytest.mark.parametrize("name,regime", kc.CASES, ids=[f"{n}-{r}" for n, r in kc.CASES])
def test_softargmax2d_values_and_gradients(device, name, regime):
    from skelsplat_amd.keypoints import softargmax2d
    ref = reference(name, regime)
    H, W = ref["img"].shape[2:]
    x = torch.from_numpy(ref["img"]).to(device).requires_grad_(True)
    xy = softargmax2d(x)
    assert xy.shape == ref["xy"].shape and xy.dtype == torch.float32
    (xy * ref["cot"].float().to(device)).sum().backward()
    dev = coord_dev(xy.detach().cpu().numpy(), ref["xy"], W, H)
    print(f"{name}-{regime}: coordinates off by {dev:.3e} of the extent (bar {COORD_BAR:.3e})")
    assert dev <= COORD_BAR
    util.assert_close("d softargmax2d / d image", x.grad.cpu().numpy(), ref["g_xy"], rtol=1e-3, atol_scale=1e-4)
    for v, c in kc.ZERO_PLANES.get(name, ()):        # uniform softmax: the exact centre
        np.testing.assert_allclose(xy[v, c].detach().cpu().numpy(), [(W - 1) / 2, (H - 1) / 2], rtol=1e-6)


@pytest.mark.parametrize("name,regime", kc.CASES, ids=[f"{n}-{r}" for n, r in kc.CASES])
def test_criteria_values_and_gradients(device, name, regime):
    """The four criteria x three reductions: the reference's return forms, values within LOSS_BAR, gradients with respect to the
    rendering at the standing tolerance."""
    from skelsplat_amd import keypoints
    ref = reference(name, regime)
    gt = ref["gt_2d"].to(device)
    cot = ref["cot"].float().to(device)
    for c in kr.CRITERIA:
        for red in REDUCTIONS:
            want, want_g = ref[c, red]
            x = torch.from_numpy(ref["img"]).to(device).requires_grad_(True)
            val = keypoints.losses[c](x, None, gt, reduction=red)
            assert torch.is_tensor(val) and val.shape == want.shape, (c, red, val.shape, want.shape)
            ((val * cot).sum() if val.dim() else val).backward()
            dev = float((np.abs(val.detach().cpu().numpy().astype(np.float64) - want) / np.abs(want)).max())
            print(f"{name}-{regime} {c} {red}: value off by {dev:.3e} of itself (bar {LOSS_BAR:.3e})")
            assert dev <= LOSS_BAR, (c, red)
            util.assert_close(f"d {c}({red}) / d rendering", x.grad.cpu().numpy(), want_g, rtol=1e-3, atol_scale=1e-4)


def test_huber_delta_is_honoured(device):
    from skelsplat_amd.keypoints import huber_loss
    ref = reference("op", "peak1")
    x = torch.from_numpy(ref["img"]).to(device)
    got = huber_loss(x, None, ref["gt_2d"].to(device), delta=2.0, reduction="none").cpu().numpy()
    want = kr.criterion_xy("huber", torch.from_numpy(ref["xy"]), ref["gt_2d"], delta=2.0).numpy()
    assert float((np.abs(got - want) / np.abs(want)).max()) <= LOSS_BAR
    assert not np.allclose(want, ref["huber", "none"][0])


def test_two_runs_are_bit_identical(device):
    from skelsplat_amd.keypoints import softargmax2d
    for name, regime in (("chunks", "peak002"), ("odd", "peak1")):
        ref = reference(name, regime)
        outs = []
        for _ in range(2):
            x = torch.from_numpy(ref["img"]).to(device).requires_grad_(True)
            xy = softargmax2d(x)
            (xy * ref["cot"].float().to(device)).sum().backward()
            outs.append((xy.detach().clone(), x.grad.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("name", ["odd", "chunks"])
def test_result_does_not_depend_on_the_batching(device, name):
    """The same planes (the same memory) as (V,C,H,W), as (V*C,H,W) and one plane at a time: the same bits, forward and backward.
    (`odd`: every plane but the first starts off 16-byte alignment.)"""
    from skelsplat_amd.keypoints import softargmax2d
    ref = reference(name, "peak002")
    V, C, H, W = ref["img"].shape
    cot = ref["cot"].float().to(device)
    base = torch.from_numpy(ref["img"]).to(device)

    def run(view, g):
        x = view.detach().requires_grad_(True)
        xy = softargmax2d(x)
        (xy * g).sum().backward()
        return xy.detach(), x.grad

    xy4, g4 = run(base, cot)
    xy3, g3 = run(base.view(V * C, H, W), cot.view(V * C, 2))
    assert torch.equal(xy4.view(-1, 2), xy3) and torch.equal(g4.view(V * C, H, W), g3)
    for p in range(V * C):
        xy1, g1 = run(base.view(V * C, H, W)[p], cot.view(V * C, 2)[p])
        assert xy1.shape == (2,)
        assert torch.equal(xy1, xy3[p]) and torch.equal(g1, g3[p]), p


_WIDE = {}


def wide_reference():
    """Float64 keypoints and image gradient of keypoint_cases.wide_image() under cotangent((1, 5)), computed once."""
    if not _WIDE:
        img = kc.wide_image()
        x = torch.from_numpy(img).double().requires_grad_(True)
        xy = kr.softargmax2d(x)
        cot = torch.from_numpy(kc.cotangent(img.shape[:2]))
        (g,) = torch.autograd.grad((xy * cot).sum(), x)
        _WIDE.update(img=img, xy=xy.detach().numpy(), cot=cot, g_xy=g.numpy())
    return _WIDE


def test_more_than_64_chunks_per_plane(device):
    """keypoint_cases.wide_image(): 68 chunks per plane, so four lanes of k_softargmax_merge take a second record each -- the walk
    `k += 64`, the maximum over both trips and the fp64 rescale of the later records.  test_keypoints_cpu.py shows that dropping
    those records moves every plane's keypoint by 25 px or more.  Forward and backward against float64, the all-zero plane and the
    plane with two equal maxima (one on each trip) at their closed forms, two runs and one plane at a time bit for bit."""
    from skelsplat_amd.keypoints import softargmax2d
    ref = wide_reference()
    V, C, H, W = kc.WIDE_SHAPE
    cot = ref["cot"].float().to(device)
    base = torch.from_numpy(ref["img"]).to(device)

    def run(view, g):
        x = view.detach().requires_grad_(True)
        xy = softargmax2d(x)
        (xy * g).sum().backward()
        return xy.detach(), x.grad

    xy, g = run(base, cot)
    got = xy.cpu().numpy()
    dev = coord_dev(got, ref["xy"], W, H)
    print(f"wide: coordinates off by {dev:.3e} of the extent (bar {COORD_BAR:.3e})")
    assert got.shape == (V, C, 2) and dev <= COORD_BAR
    util.assert_close("d softargmax2d / d image", g.cpu().numpy(), ref["g_xy"], rtol=1e-3, atol_scale=1e-4)
    np.testing.assert_allclose(got[0, kc.WIDE_ZERO_PLANE], [(W - 1) / 2, (H - 1) / 2], rtol=1e-6)
    centre = np.mean(kc.WIDE_PLANES[3][2], axis=0)
    assert coord_dev(got[0, 3], centre, W, H) <= COORD_BAR
    xy2, g2 = run(base, cot)
    assert torch.equal(xy, xy2) and torch.equal(g, g2)
    for p in range(C):          # the same memory: plane p starts (p * H * W) % 4 floats past a 16-byte boundary either way
        xy1, g1 = run(base.view(C, H, W)[p], cot.view(C, 2)[p])
        assert torch.equal(xy1, xy[0, p]) and torch.equal(g1, g[0, p]), p


@pytest.mark.parametrize("name", ["odd", "chunks"])
def test_backward_stores_at_every_phase_of_image_and_gradient(device, name):
    """sks_softargmax_bwd with `img` and `dL_dimg` at all 16 pairs of 4-byte phases.  The kernel stores the gradient 16 bytes at a
    time only where it is as aligned as the image, which keypoint_cases.bwd_stores_16_bytes works out from the two phases alone:
    4 of the 16 pairs; the other 12 take the element-wise stores.  ONE stats buffer, from one forward on the aligned image: given
    the stats every element's gradient is a function of that element alone, so whatever the grouping into head, 16-byte groups
    and tail, the interior equals the (0, 0) result bit for bit, holds no sentinel, and both guards stay untouched
    (tests/guarded.py)."""
    from skelsplat_amd import _lib, keypoints
    ref = reference(name, "peak002")
    V, C, H, W = ref["img"].shape
    planes, total = V * C, ref["img"].size
    size = guarded.buffer_floats(total)
    lib = _lib.load()
    flat = torch.from_numpy(ref["img"].reshape(-1)).to(device)
    _, stats = keypoints._fwd(flat.view(V, C, H, W), 100.0)
    cot = ref["cot"].float().to(device).reshape(planes, 2).contiguous()
    imgs = {}
    for p in guarded.PHASES:
        imgs[p] = torch.zeros(size, dtype=torch.float32, device=device)
        imgs[p][guarded.interior(p, total)] = flat
    sentinel = torch.full((size,), int(guarded.SENTINEL), dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    want, scalar = None, 0
    for pi in guarded.PHASES:
        for pg in guarded.PHASES:
            out = sentinel.clone()
            assert imgs[pi].data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
            with torch.cuda.device(device):
                rc = lib.sks_softargmax_bwd(planes, W, H, 100.0, imgs[pi].data_ptr() + 4 * (guarded.GUARD + pi), stats.data_ptr(),
                                            cot.data_ptr(), out.data_ptr() + 4 * (guarded.GUARD + pg), stream)
            _lib.check(rc, "sks_softargmax_bwd")
            bits = out.cpu().numpy()
            if want is None:            # (0, 0): held to float64 like every other gradient, then the yardstick of the other 15
                want = bits[guarded.interior(0, total)].copy()
                util.assert_close("d softargmax2d / d image", want.view(np.float32).reshape(ref["img"].shape), ref["g_xy"],
                                  rtol=1e-3, atol_scale=1e-4)
            guarded.check(f"{name} image phase {pi}, gradient phase {pg}", bits, pg, total, want)
            scalar += not kc.bwd_stores_16_bytes(pi, pg)
    assert scalar == 12


def test_non_default_stream_is_honoured(device):
    """The image is produced on a side stream BEHIND a long-running kernel (the library's bounded idle kernel); the op, enqueued
    on that stream right after, must see it -- on any other stream it would read the NaN the buffer held before."""
    from skelsplat_amd import _lib
    from skelsplat_amd.keypoints import softargmax2d
    ref = reference("pan", "peak1")
    src = torch.from_numpy(ref["img"]).to(device)
    cot = ref["cot"].float().to(device)
    x = torch.full_like(src, float("nan")).requires_grad_(True)
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        _lib.check(_lib.load().sks_prof_spin(5000.0, ctypes.c_void_p(side.cuda_stream)), "sks_prof_spin")
        with torch.no_grad():
            x.copy_(src)
        xy = softargmax2d(x)
        (g,) = torch.autograd.grad((xy * cot).sum(), x)
    side.synchronize()
    x2 = src.clone().requires_grad_(True)
    xy2 = softargmax2d(x2)
    (g2,) = torch.autograd.grad((xy2 * cot).sum(), x2)
    assert torch.equal(xy.detach(), xy2.detach()) and torch.equal(g, g2)
    assert coord_dev(xy.detach().cpu().numpy(), ref["xy"], *ref["img"].shape[:1:-1]) <= COORD_BAR


def test_cpu_and_fp16_tensors_raise(device):
    from skelsplat_amd import keypoints
    with pytest.raises(RuntimeError, match="ROCm device"):
        keypoints.softargmax2d(torch.zeros(3, 8, 8))
    with pytest.raises(RuntimeError, match="float32"):
        keypoints.softargmax2d(torch.zeros(3, 8, 8, device=device, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="float32"):
        keypoints.l2_loss(torch.zeros(3, 8, 8, device=device, dtype=torch.float64), None, torch.zeros(3, 2, device=device))
    with pytest.raises(RuntimeError):
        keypoints.softargmax2d(torch.zeros(3, 0, 8, device=device))


def softargmax2d_tensor_ops(x, beta=100.0):
    """The reference's formulation as plain tensor ops on the device (softmax, index grids, two weighted sums), in the dtype of x."""
    H, W = x.shape[-2:]
    p = torch.softmax(beta * x.reshape(*x.shape[:-2], H * W), dim=-1)
    rows = torch.linspace(0, 1, steps=H, device=x.device, dtype=x.dtype).view(-1, 1).repeat(1, W).view(1, H * W)
    cols = torch.linspace(0, 1, steps=W, device=x.device, dtype=x.dtype).view(1, -1).repeat(H, 1).view(1, H * W)
    return torch.stack([(p * cols).sum(-1) * (W - 1), (p * rows).sum(-1) * (H - 1)], dim=-1)


def l2_loss_grad_tensor_ops(gt_2d):
    """`loss_grad` of the l2 keypoint criterion from the tensor-op formula, float64 on the device."""
    def loss_grad(render, gt=None):
        with torch.enable_grad():
            x = render.detach().double().requires_grad_(True)
            loss = ((softargmax2d_tensor_ops(x) - gt_2d.double()) ** 2).mean(dim=(1, 2))
            (g,) = torch.autograd.grad(loss.sum(), x)
        return g.float(), loss.detach().float(), torch.ones_like(loss, dtype=torch.float32)
    return loss_grad


def test_keypoint_loss_grad_drives_the_loop(device):
    """keypoint_loss_grad("l2", ...) handed to a MultiViewLoop (a custom loss_grad: the tensor-op tail, no device tail): three
    accumulation groups of a 4-view 64 x 48 scene end at the parameters of the same loop driven by the tensor-op formula in
    float64 on the device -- which is first held to the float64 restatement here."""
    from skelsplat_amd.keypoints import keypoint_loss_grad
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    from skelsplat_amd.heatmaps import generate_heatmaps
    ref = reference("op", "peak1")
    got = softargmax2d_tensor_ops(torch.from_numpy(ref["img"]).to(device).double()).cpu().numpy()
    assert coord_dev(got, ref["xy"], ref["img"].shape[3], ref["img"].shape[2]) <= 1e-9

    W, H, V = 64, 48, 4
    sc = SyntheticScene("h36m", n_views=V, seed=5, W=W, H=H, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5, device=device)
    gt_2d = torch.tensor(sc.poses_2d, dtype=torch.float32, device=device)
    res = []
    for make in (lambda: keypoint_loss_grad("l2", gt_2d), lambda: l2_loss_grad_tensor_ops(gt_2d)):
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9,
                                                scaling_modifier=1.0, device=device)
        gm.training_setup()
        with torch.no_grad():   # finite opacity, tilted quaternions, anisotropic scales: every Jacobian carries signal
            gm._opacity.fill_(2.0)
            gm._rotation.add_(0.1 * torch.randn(gm._rotation.shape, generator=torch.Generator().manual_seed(0)).to(device))
            gm._scaling.add_(0.3 * torch.randn(gm._scaling.shape, generator=torch.Generator().manual_seed(1)).to(device))
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(), gt_2d, sc.cameras)
        loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", accumulation_steps=4, loss_grad=make())
        assert not loop.device_tail and not loop.sparse          # the loss_grad path (_local_view_grads)
        loop.run(12)                                             # three accumulation groups
        assert loop.last_losses is not None
        res.append([p.detach().cpu().clone() for p in (gm._xyz, gm._scaling, gm._rotation, gm._opacity)])
    moved = (res[1][0] - torch.tensor(sc.pose_3d_init).float()).norm(dim=1).mean().item()
    print(f"joints moved {moved:.4f} mm on average; largest xyz difference {(res[0][0] - res[1][0]).abs().max().item():.3e}")
    assert moved > 0.05, f"the optimisation did not move the joints ({moved} mm): the test is vacuous"
    for nm, a, b in zip(("xyz", "scaling", "rotation", "opacity"), res[0], res[1]):
        util.assert_close(nm, a, b, rtol=1e-4, atol_scale=1e-4)


def test_keypoint_loss_grad_picks_its_rows_by_image_size(device):
    """Cameras of two sizes: the loop calls loss_grad once per size; a dict {(H, W): detections} serves both batches."""
    from skelsplat_amd import keypoints
    a, b = reference("op", "peak1"), reference("pan", "peak1")
    gt = {tuple(r["img"].shape[2:]): r["gt_2d"].to(device) for r in (a, b)}
    fn = keypoints.keypoint_loss_grad("huber", gt)
    for r in (a, b):
        dL, loss, scale = fn(torch.from_numpy(r["img"]).to(device), None)
        want = kr.criterion_xy("huber", torch.from_numpy(r["xy"]), r["gt_2d"]).mean(dim=(1, 2)).numpy()
        assert float((np.abs(loss.cpu().numpy() - want) / want).max()) <= LOSS_BAR
        assert dL.shape == r["img"].shape and torch.equal(scale, torch.ones_like(loss))
        # 'mean' per view: the gradient of the SUM of the per-view means = V x the gradient of the mean over everything
        util.assert_close("dL", dL.cpu().numpy() / r["img"].shape[0], r["huber", "mean"][1], rtol=1e-3, atol_scale=1e-4)

    class Cam:
        def __init__(self, w, h):
            self.image_width, self.image_height = w, h
    rows = keypoints.detections_by_size([Cam(64, 48), Cam(80, 64), Cam(64, 48)], torch.arange(12.0, device=device).view(3, 2, 2))
    assert set(rows) == {(48, 64), (64, 80)} and rows[48, 64][:, 0, 0].tolist() == [0.0, 8.0] and rows[64, 80].shape == (1, 2, 2)


def test_full_size_plane_against_the_restatement(device):
    """1 x 17 x 1000 x 1002 (H36M's wider sensor): 62 chunks per plane and the row / column arithmetic at the real width.  Planes
    alternate between the two regimes; peaks sit in the first, middle and last rows."""
    from skelsplat_amd.keypoints import softargmax2d
    C, H, W = 17, 1000, 1002
    rng = np.random.default_rng(7)
    rows, cols = np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64)
    img = np.empty((1, C, H, W), dtype=np.float32)
    for c in range(C):
        cy = (3.3, H / 2 + 0.4, H - 2.6)[c % 3] if c < 6 else rng.uniform(0.1, 0.9) * (H - 1)
        cx, sigma = rng.uniform(0.05, 0.95) * (W - 1), rng.uniform(2.0, 6.0)
        amp = rng.uniform(0.9, 1.0) if c % 2 == 0 else rng.uniform(0.015, 0.02)
        img[0, c] = (amp * np.outer(np.exp(-(rows - cy) ** 2 / (2 * sigma ** 2)), np.exp(-(cols - cx) ** 2 / (2 * sigma ** 2)))).astype(np.float32)
    cot = torch.from_numpy(kc.cotangent((1, C)))
    x64 = torch.from_numpy(img).double().requires_grad_(True)
    xy64 = kr.softargmax2d(x64)
    (g64,) = torch.autograd.grad((xy64 * cot).sum(), x64)
    x = torch.from_numpy(img).to(device).requires_grad_(True)
    xy = softargmax2d(x)
    (xy * cot.float().to(device)).sum().backward()
    dev = coord_dev(xy.detach().cpu().numpy(), xy64.detach().numpy(), W, H)
    print(f"full size: coordinates off by {dev:.3e} of the extent (bar {COORD_BAR:.3e})")
    assert dev <= COORD_BAR
    util.assert_close("d softargmax2d / d image", x.grad.cpu().numpy(), g64.numpy(), rtol=1e-3, atol_scale=1e-4)
