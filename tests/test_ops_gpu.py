"""GPU parity of the smaller ops: fused masked-L2, fused SSIM, 3-NN mean distance, and the multi-view loop."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from tests import util
from tests.ssim_cases import ssim_torch

pytestmark = pytest.mark.gpu


SSIM_SHAPES = [(2, 3, 67, 45), (1, 17, 128, 160), (5, 5, 270, 480), (1, 2, 33, 200), (1, 1, 12, 16), (2, 1, 97, 131)]


@pytest.mark.parametrize("shape", SSIM_SHAPES)
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_fused_ssim_map_matches_conv2d_ssim(device, shape, padding):
    """The map-returning autograd function (fused_ssim/__init__.py:8-32) under an arbitrary upstream gradient."""
    from fused_ssim import FusedSSIMMap
    g = torch.Generator().manual_seed(1)
    img1 = torch.rand(shape, generator=g).to(device).requires_grad_(True)
    img2 = torch.rand(shape, generator=g).to(device)
    m = FusedSSIMMap.apply(0.01 ** 2, 0.03 ** 2, img1, img2, padding, True)
    wgt = torch.rand(m.shape, generator=g)
    (m * wgt.to(device)).sum().backward()
    ref1 = img1.detach().double().cpu().requires_grad_(True)
    mr = ssim_torch(ref1, img2.double().cpu())
    if padding == "valid":
        mr = mr[:, :, 5:-5, 5:-5]
    (mr * wgt.double()).sum().backward()
    util.assert_close("ssim_map", m.detach().cpu(), mr.detach(), rtol=2e-5, atol_scale=5e-6)
    util.assert_close("dL_dimg1", img1.grad.cpu(), ref1.grad, rtol=1e-3, atol_scale=1e-4)
    # a contiguous tensor at a 4-byte offset takes the scalar-load path and gives the same map
    n = int(np.prod(shape))
    f1, f2 = torch.rand(n + 1, generator=g).to(device), torch.rand(n + 1, generator=g).to(device)
    a, b = f1[1:].view(shape), f2[1:].view(shape)
    assert a.is_contiguous() and a.data_ptr() % 16 != 0
    m1 = FusedSSIMMap.apply(0.01 ** 2, 0.03 ** 2, a, b, "same", False)
    m2 = FusedSSIMMap.apply(0.01 ** 2, 0.03 ** 2, a.clone(), b.clone(), "same", False)
    assert torch.equal(m1, m2)


@pytest.mark.parametrize("shape", SSIM_SHAPES)
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_fused_ssim_matches_conv2d_ssim(device, shape, padding):
    from fused_ssim import fused_ssim
    g = torch.Generator().manual_seed(0)
    img1 = torch.rand(shape, generator=g).to(device).requires_grad_(True)
    img2 = torch.rand(shape, generator=g).to(device)
    val = fused_ssim(img1, img2, padding=padding)
    val.backward()
    ref1 = img1.detach().double().cpu().requires_grad_(True)
    m = ssim_torch(ref1, img2.double().cpu())
    if padding == "valid":
        m = m[:, :, 5:-5, 5:-5]
    ref = m.mean()
    ref.backward()
    # tests.py:82-91 of fused-ssim asserts torch.isclose at default rtol=1e-5 on value and gradient (fp32 vs fp32);
    # against an fp64 reference the fp32 kernel is held to 2e-5 relative on the value, 1e-4*max on the gradient
    assert abs(val.item() - ref.item()) <= 2e-5 * abs(ref.item())
    util.assert_close("dL_dimg1", img1.grad.cpu(), ref1.grad, rtol=1e-3, atol_scale=1e-4)
    # train=False returns the same value and keeps no state; the reduction scratch clears itself between calls
    for _ in range(3):
        assert abs(fused_ssim(img1.detach(), img2, padding=padding, train=False).item() - val.item()) <= 1e-7


def test_fused_ssim_wrapper_reproduces_the_reference_wrapper(device):
    """tests/golden/reference_ssim.npz: the reference's own fused_ssim/__init__.py executed over its own PyTorch SSIM
    (tests/golden/make_golden_ssim.py): constants, "same" / "valid", train / inference, the mean over the cropped map and
    the gradient that reaches img1 -- value 1e-5, gradient 1e-4 of its scale (the kernels keep fp32 sums in another order)."""
    from fused_ssim import fused_ssim, allowed_padding
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_ssim.npz"))
    assert list(allowed_padding) == G["allowed_padding"].tolist()
    for tag in ("a", "b", "c"):
        img2 = torch.tensor(G[tag + "_img2"], device=device)
        for padding in ("same", "valid"):
            for mode in ("train", "infer"):
                x = torch.tensor(G[tag + "_img1"], device=device).requires_grad_(True)
                val = fused_ssim(x, img2, padding=padding, train=mode == "train")
                key = f"{tag}_{padding}_{mode}"
                assert abs(val.item() - float(G[key + "_value"])) <= 1e-5 * abs(float(G[key + "_value"])), key
                if mode == "train":
                    (3.0 * val).backward()
                    util.assert_close(key, x.grad.cpu().numpy(), G[key + "_grad"], rtol=1e-3, atol_scale=1e-4)


@pytest.mark.parametrize("min_blocks", ["1", "40"], ids=["strips-of-8", "strips-of-2"])
def test_fused_ssim_long_strips(device, min_blocks, monkeypatch):
    """The kernels walk strips of tiles down the image and carry 10 filtered rows from tile to tile; small test images
    would always get one-tile strips (the launch wants >= 2 048 workgroups), so the strip length is forced here."""
    from fused_ssim import fused_ssim, FusedSSIMMap
    monkeypatch.setenv("SKS_SSIM_MIN_BLOCKS", min_blocks)
    g = torch.Generator().manual_seed(4)
    shape = (2, 3, 300, 136)   # 10 tile rows (the last one partial), 3 tile columns
    img1 = torch.rand(shape, generator=g).to(device).requires_grad_(True)
    img2 = torch.rand(shape, generator=g).to(device)
    m = FusedSSIMMap.apply(0.01 ** 2, 0.03 ** 2, img1, img2, "same", True)
    wgt = torch.rand(shape, generator=g)
    (m * wgt.to(device)).sum().backward()
    ref1 = img1.detach().double().cpu().requires_grad_(True)
    mr = ssim_torch(ref1, img2.double().cpu())
    (mr * wgt.double()).sum().backward()
    util.assert_close("ssim_map", m.detach().cpu(), mr.detach(), rtol=2e-5, atol_scale=5e-6)
    util.assert_close("dL_dimg1", img1.grad.cpu(), ref1.grad, rtol=1e-3, atol_scale=1e-4)
    # the mean form (fused sum + scalar-gradient backward), "valid" crop
    a = img1.detach().clone().requires_grad_(True)
    val = fused_ssim(a, img2, padding="valid")
    val.backward()
    b = img1.detach().double().cpu().requires_grad_(True)
    want = ssim_torch(b, img2.double().cpu())[:, :, 5:-5, 5:-5].mean()
    want.backward()
    assert abs(val.item() - want.item()) <= 2e-5 * abs(want.item())
    util.assert_close("dL_dimg1 (mean)", a.grad.cpu(), b.grad, rtol=1e-3, atol_scale=1e-4)
    # and strips of any length give the same bits as one-tile strips
    monkeypatch.setenv("SKS_SSIM_MIN_BLOCKS", "1000000")
    m1 = FusedSSIMMap.apply(0.01 ** 2, 0.03 ** 2, img1.detach(), img2, "same", False)
    assert torch.equal(m1, m.detach())


def test_fused_ssim_random_shapes(device, monkeypatch):
    """60 random (B, CH, H, W) including degenerate ones (one row, one column, W % 4 != 0, fewer than 11 rows), both
    paddings, random strip lengths: map, gradient and the fused mean against conv2d SSIM."""
    import random
    from skelsplat_amd import ops
    rnd = random.Random(1)
    for _ in range(60):
        B, CH = rnd.choice([1, 2, 3]), rnd.choice([1, 2, 5])
        H = rnd.choice([1, 2, 5, 9, 10, 11, 16, 31, 32, 33, 63, 64, 65, 100])
        W = rnd.choice([1, 2, 3, 4, 7, 8, 12, 16, 60, 63, 64, 65, 68, 128, 132, 200])
        monkeypatch.setenv("SKS_SSIM_MIN_BLOCKS", rnd.choice(["1", "3", "2048"]))
        pad = rnd.choice(["same", "valid"])
        a = torch.rand((B, CH, H, W), device=device, requires_grad=True)
        b = torch.rand((B, CH, H, W), device=device)
        m = ops.FusedSSIMMap.apply(1e-4, 9e-4, a, b, pad, True)
        ref1 = a.detach().double().cpu().requires_grad_(True)
        mr = ssim_torch(ref1, b.double().cpu())
        if pad == "valid":
            mr = mr[:, :, 5:-5, 5:-5]
        if mr.numel() == 0:
            assert m.numel() == 0
            continue
        w = torch.rand(mr.shape)
        (m * w.to(device)).sum().backward()
        (mr * w.double()).sum().backward()
        tag = f"{(B, CH, H, W)} {pad}"
        assert (m.detach().cpu().double() - mr.detach()).abs().max().item() < 2e-5, tag
        assert (a.grad.cpu().double() - ref1.grad).abs().max().item() <= 2e-4 * max(ref1.grad.abs().max().item(), 1e-9), tag
        assert abs(ops.fused_ssim(a.detach(), b, padding=pad, train=False).item() - mr.mean().item()) < 2e-5, tag


def test_fused_ssim_empty_valid_map_is_nan(device):
    from fused_ssim import fused_ssim
    a = torch.rand(1, 2, 9, 40, device=device)
    assert math.isnan(fused_ssim(a, a.clone(), padding="valid", train=False).item())   # 9 - 10 rows: nothing left
    assert abs(fused_ssim(a, a.clone(), padding="same", train=False).item() - 1.0) < 1e-6


@pytest.mark.parametrize("P", [1, 3, 4, 17, 19, 300, 2000])
def test_knn_matches_bruteforce(device, P):
    from simple_knn._C import distCUDA2
    pts = torch.randn(P, 3, generator=torch.Generator().manual_seed(P)) * 100
    got = distCUDA2(pts.to(device)).cpu().numpy()
    p = pts.numpy().astype(np.float32)
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(np.float32)
    np.fill_diagonal(d2, np.float32(np.finfo(np.float32).max))
    if P >= 4:
        part = np.sort(d2, axis=1)[:, :3]
        want = ((part[:, 0] + part[:, 1]) + part[:, 2]) / np.float32(3.0)
        np.testing.assert_allclose(got, want, rtol=2e-6)
    else:  # fewer than 3 neighbours: the reference leaves FLT_MAX entries in the sum (simple_knn.cu:155,183)
        assert np.all(got > 1e37)


@pytest.mark.parametrize("shape", [(1, 3, 7, 5), (4, 17, 100, 100), (2, 19, 54, 96)])
def test_masked_l2_matches_reference_semantics(device, shape):
    from skelsplat_amd.ops import masked_l2
    g = torch.Generator().manual_seed(1)
    render = (torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) > 0.7)).to(device)
    gt = (torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) > 0.6)).to(device)
    dL, S, N = masked_l2(render, gt)
    for v in range(shape[0]):
        r = render[v].double().cpu().requires_grad_(True)
        t = gt[v].double().cpu()
        mask = (t > 0) | (r > 0)
        loss = ((r - t) ** 2)[mask].mean()          # utils/loss_utils.py:88-97
        loss.backward()
        assert int(N[v].item()) == int(mask.sum())
        assert abs(S[v].item() / N[v].item() - loss.item()) <= 1e-6 * loss.item()
        util.assert_close("dL", (dL[v].double().cpu() / N[v].item()), r.grad, rtol=1e-5, atol_scale=1e-6)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_fused_l2_loss_gaussian_criterion(device, reduction):
    """The fused criterion a user registers in train.py's `losses` table equals utils/loss_utils.py:86-100 (restated in
    skelsplat_amd.loop.l2_loss_gaussian, which the CPU suite pins to the reference's own function), value and gradient."""
    from skelsplat_amd.ops import l2_loss_gaussian as fused
    g = torch.Generator().manual_seed(2)
    shape = (17, 90, 131)
    r0 = (torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) > 0.7)).to(device)
    gt = (torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) > 0.6)).to(device)
    r = r0.clone().requires_grad_(True)
    out = fused(r, gt, None, 1.0, reduction=reduction)
    rr = r0.double().cpu().requires_grad_(True)
    t = gt.double().cpu()
    mask = (t > 0) | (rr > 0)
    err = ((rr - t) ** 2)[mask]
    if reduction == "none":
        util.assert_close("loss vector", out.detach().cpu(), err.detach(), rtol=1e-6, atol_scale=1e-7)
        return
    loss = out[0] if reduction == "mean" else out
    assert reduction == "sum" or out[1] is None
    want = err.mean() if reduction == "mean" else err.sum()
    (3.0 * loss).backward()
    (3.0 * want).backward()
    assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item())
    util.assert_close("grad", r.grad.cpu(), rr.grad, rtol=1e-5, atol_scale=1e-6)


def _make_loop_scene(dev, W=160, H=128, V=4, seed=3):
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    from skelsplat_amd.heatmaps import generate_heatmaps
    sc = SyntheticScene("h36m", n_views=V, seed=seed, W=W, H=H, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5, device=dev)
    def model(device):
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9,
                                                scaling_modifier=1.0, device=device)
        gm.training_setup()
        return gm
    return sc, model


def test_loop_matches_reference_loop(device):
    """40 iterations (10 Adam steps) of the batched HIP loop vs the literal per-iteration reference loop on the
    PyTorch oracle: same joints within 0.5 mm (north-star MPJPE bar) -- in practice within 1e-2 mm."""
    from skelsplat_amd.loop import MultiViewLoop, mpjpe
    from skelsplat_amd.heatmaps import generate_heatmaps
    from tests.ref_loop import run_reference_loop
    import copy
    sc, model = _make_loop_scene(device)
    gm = model(device)
    hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                           torch.tensor(sc.poses_2d, device=device), sc.cameras)
    loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", accumulation_steps=4, lambda_consistency=1e-5)
    out = loop.run(40).cpu()
    # reference loop on CPU
    cams_cpu = [copy.copy(c).to("cpu") for c in sc.cameras]
    gm_ref = model("cpu")
    ref = run_reference_loop(gm_ref, cams_cpu, hm.cpu(), sc.W, sc.H, "h36m", 40)
    moved = (ref - torch.tensor(sc.pose_3d_init).float()).norm(dim=1).mean().item()
    diff = (out - ref).norm(dim=1).max().item()
    assert moved > 0.05, f"the optimisation did not move the joints ({moved} mm): test is vacuous"
    assert diff < 0.5, f"HIP loop and reference loop disagree by {diff} mm"
    assert diff < 0.02 * max(moved, 1.0), (diff, moved)
    # scaling / rotation parameters follow too (quirk Q7: last view's gradients)
    util.assert_close("scaling", gm._scaling.detach().cpu(), gm_ref._scaling.detach(), rtol=1e-3, atol_scale=1e-4)


def test_fused_loss_equals_tensor_op_loss_in_loop(device):
    from skelsplat_amd.loop import MultiViewLoop, masked_l2_grad_torch
    from skelsplat_amd.heatmaps import generate_heatmaps
    sc, model = _make_loop_scene(device, seed=5)
    outs = []
    for lg in (None, masked_l2_grad_torch):
        gm = model(device)
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                               torch.tensor(sc.poses_2d, device=device), sc.cameras)
        loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", loss_grad=lg)
        outs.append(loop.run(20).cpu())
    assert (outs[0] - outs[1]).norm(dim=1).max().item() < 1e-3


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_device_tail_loop_matches_tensor_op_tail(device, use_graph):
    """sks_loop_pack_grads + sks_loop_adam_step (device-side activation Jacobians, limb gradient, LR schedule, Adam)
    reproduce the tensor-op tail + torch.optim.Adam; also as one captured hipGraph per accumulation group."""
    from skelsplat_amd.loop import MultiViewLoop, masked_l2_grad_torch
    from skelsplat_amd.heatmaps import generate_heatmaps
    sc, model = _make_loop_scene(device, seed=7)
    res = []
    for mode in ("device", "torch"):
        gm = model(device)
        with torch.no_grad():   # finite opacity, tilted quaternions, anisotropic scales: every Jacobian carries signal
            gm._opacity.fill_(2.0)   # (with isotropic scales the rotation gradient is rounding noise, which Adam's
            #                           1/sqrt(v) normalisation turns into +-lr steps of arbitrary sign)
            gm._rotation.add_(0.1 * torch.randn(gm._rotation.shape, generator=torch.Generator().manual_seed(0)).to(device))
            gm._scaling.add_(0.3 * torch.randn(gm._scaling.shape, generator=torch.Generator().manual_seed(1)).to(device))
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                               torch.tensor(sc.poses_2d, device=device), sc.cameras)
        if mode == "device":
            loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", use_graph=use_graph)
            assert loop.device_tail and loop.use_graph == use_graph
        else:
            loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", loss_grad=masked_l2_grad_torch)
            assert not loop.device_tail
        loop.run(40)
        res.append([p.detach().cpu().clone() for p in (gm._xyz, gm._scaling, gm._rotation, gm._opacity)])
    moved = (res[1][0] - torch.tensor(sc.pose_3d_init).float()).norm(dim=1).mean().item()
    assert moved > 1.0
    assert (res[0][0] - res[1][0]).norm(dim=1).max().item() < 2e-3 * moved        # xyz within 0.2 % of the distance moved
    util.assert_close("scaling", res[0][1], res[1][1], rtol=1e-4, atol_scale=1e-4)
    util.assert_close("rotation", res[0][2], res[1][2], rtol=1e-4, atol_scale=1e-4)
    util.assert_close("opacity", res[0][3], res[1][3], rtol=1e-5, atol_scale=1e-5)


@pytest.mark.parametrize("dataset", ["h36m", "panoptic"])
def test_sparse_fused_loss_backward_equals_dense_path(device, dataset):
    """sks_geometry + sks_backward_fused_loss (no image, no dense gradient, per-tile heat-map statistics) give the
    same loss sums and the same gradients as sks_forward(clamp) -> sks_masked_l2 -> sks_backward."""
    from skelsplat_amd import rasterizer as R
    from skelsplat_amd.ops import masked_l2
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    from skelsplat_amd.heatmaps import generate_heatmaps
    W, H = 176, 144
    sc = SyntheticScene(dataset, n_views=3, seed=11, W=W, H=H, ring=2500.0, fx=1145.0 * (W / 1000) * 1.5, device=device)
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=4.2, scene_type=dataset,
                                            device=device)
    hm = generate_heatmaps(torch.tensor(sc.pose_3d_gt, device=device).float(), gm.get_scaling.detach() * 1.3,
                           gm._rotation.detach(), torch.tensor(sc.poses_2d, device=device), sc.cameras)
    P, C = sc.n_points, sc.n_joints
    with torch.no_grad():
        args = (gm._xyz.detach(), gm.get_features.reshape(P, C), gm.get_opacity.detach(), gm.get_scaling.detach(),
                gm.get_rotation.detach(), None)
    views = R.ViewBatch.from_cameras(sc.cameras)
    color, inv, radii, st = R.forward_views(views, *args, clamp01=True)
    dL, S, N = masked_l2(color, hm)
    gd = R.backward_views(st, *args, dL)
    stats = R.gt_tile_stats(hm)
    st2 = R.geometry_views(views, args[0], C, args[2], args[3], args[4], None)
    gs, sums = R.backward_fused_loss(st2, stats, *args)
    assert torch.equal(st2.radii, radii)
    assert torch.equal(sums[:, 1], N), (sums[:, 1], N)                       # mask counts are integers: exact
    assert ((sums[:, 0] - S).abs() <= 1e-5 * S.abs()).all(), (sums[:, 0], S)
    assert float(N.min()) > 1000 and float(S.min()) > 0
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        util.assert_close(k, gs[k].cpu(), gd[k].cpu(), rtol=1e-4, atol_scale=1e-5)
    # the same call with the heat-maps as separable factors (no plane read): the pseudo-GT it evaluates is bit for bit the
    # stored one, so gradients and mask counts are identical; the constants come from sks_heatmap_totals
    from skelsplat_amd.heatmaps import heatmap_factors
    fac = R.HeatmapFactors(3, C, W, H, device)
    heatmap_factors(torch.tensor(sc.pose_3d_gt, device=device).float(), gm.get_scaling.detach() * 1.3, gm._rotation.detach(),
                    torch.tensor(sc.poses_2d, device=device), sc.cameras, views=views, out=fac)
    for v in range(3):
        assert torch.equal(fac.planes(v), hm[v])
    fst = R.GtStats()
    fst.gt, fst.tile_S, fst.tile_N, fst.factors = None, None, None, fac
    fst.totals = fac.totals(views, torch.empty((3, 2), dtype=torch.float64, device=device))
    assert torch.equal(fst.totals[:, 1], stats.totals[:, 1])
    for _ in range(5):      # reproducible bit for bit: the blocks of a view are combined in fixed point, in any order
        assert torch.equal(fac.totals(views, torch.empty((3, 2), dtype=torch.float64, device=device)), fst.totals)
    assert ((fst.totals[:, 0] - stats.totals[:, 0]).abs() <= 1e-6 * stats.totals[:, 0].abs()).all()
    gf, sums_f = R.backward_fused_loss(st2, fst, *args)
    assert torch.equal(sums_f[:, 1], sums[:, 1]) and ((sums_f[:, 0] - sums[:, 0]).abs() <= 1e-6 * sums[:, 0].abs()).all()
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        assert torch.equal(gf[k], gs[k]), k


def test_sparse_loop_equals_dense_loop(device):
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    sc, model = _make_loop_scene(device, seed=9)
    outs = []
    for sparse in (True, False):
        gm = model(device)
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                               torch.tensor(sc.poses_2d, device=device), sc.cameras)
        loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", sparse=sparse, use_graph=sparse)
        assert loop.sparse == sparse
        loop.run(40)
        outs.append((gm._xyz.detach().cpu().clone(), gm._scaling.detach().cpu().clone()))
    moved = (outs[0][0] - torch.tensor(sc.pose_3d_init).float()).norm(dim=1).mean().item()
    assert moved > 1.0 and (outs[0][0] - outs[1][0]).norm(dim=1).max().item() < 2e-3 * moved
    util.assert_close("scaling", outs[0][1], outs[1][1], rtol=1e-4, atol_scale=1e-4)


# (The whole-scene MPJPE bar -- 500 iterations through the production path against the per-iteration loop -- is
#  tests/test_loop_golden.py::test_production_loop_follows_the_reference_trajectory[h36m_mid-True]: the same 112x96 scene
#  shape, but against the trajectory of the REFERENCE's own train.training() instead of the restated loop run here, which
#  took 90 s of CPU time per test run.)


def test_loop_with_mixed_image_sizes(device):
    """H36M mixes 1000x1000 and 1002x1000 cameras (quirk Q11): views are grouped by size, one launch sequence per group,
    and the result equals the literal per-iteration reference loop."""
    import copy
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    from tests.ref_loop import view_grads_ref
    a = SyntheticScene("h36m", n_views=4, seed=13, W=160, H=128, ring=2500.0, fx=1145.0 * 0.16 * 1.5, device=device)
    b = SyntheticScene("h36m", n_views=4, seed=13, W=162, H=128, ring=2500.0, fx=1145.0 * 0.16 * 1.5, device=device)
    cams = [a.cameras[0], b.cameras[1], a.cameras[2], b.cameras[3]]        # sizes 160, 162, 160, 162
    def model(dev):
        gm = GaussianModel().create_from_points(a.pose_3d_init, a.spatial_lr_scale, 17, scaling=3.9, device=dev)
        gm.training_setup()
        return gm
    outs = []
    for sparse in (True, False):
        gm = model(device)
        hms = [generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                                 torch.tensor(a.poses_2d[v:v + 1], device=device), [cams[v]])[0] for v in range(4)]
        loop = MultiViewLoop(gm, cams, hms, dataset="h36m", sparse=sparse)
        assert len(loop.size_groups) == 2
        if sparse:   # one launch sequence for all four views: per-view sizes + offsets into one flat heat-map buffer
            assert loop.views_all.mixed and loop.views_all.V == 4 and loop.fused_tail
            assert loop.stats_all.offsets is not None and loop.stats_all.gt.numel() == 17 * 128 * (160 + 162) * 2
        loop.run(24)
        outs.append(gm._xyz.detach().cpu().clone())
    # literal reference loop on the CPU oracle
    gm = model("cpu")
    cams_cpu = [copy.copy(c).to("cpu") for c in cams]
    hms_cpu = [h.cpu() for h in hms]
    acc = torch.zeros(4, 17, 3)
    for it in range(1, 25):
        gm.update_learning_rate(it)
        idx = (it - 1) % 4
        _, (gx, gs, gr, go) = view_grads_ref(gm, cams_cpu[idx], hms_cpu[idx], cams_cpu[idx].image_width, 128, "h36m", 1e-5)
        acc[idx] = gx
        gm._scaling.grad, gm._rotation.grad, gm._opacity.grad = gs, gr, go
        if it % 4 == 0:
            gm._xyz.grad = acc.mean(0)
            gm.optimizer.step()
            gm.optimizer.zero_grad(set_to_none=True)
    ref = gm._xyz.detach()
    moved = (ref - torch.tensor(a.pose_3d_init).float()).norm(dim=1).mean().item()
    assert moved > 1.0
    for o in outs:
        assert (o - ref).norm(dim=1).max().item() < 5e-3 * moved


@pytest.mark.parametrize("shape", [(2, 3, 48, 64), (1, 17, 50, 70), (2, 2, 33, 1030), (1, 5, 16, 4100)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gt_tile_stats(device, shape):
    """sks_gt_tile_stats: per (view, tile, channel) sum of gt^2 and count of gt > 0, and the per-view totals; ragged
    tiles, widths that are not multiples of 4, more than 64 / 256 tile columns."""
    from skelsplat_amd import rasterizer as R
    V, C, H, W = shape
    g = torch.Generator().manual_seed(3)
    gt = torch.rand(shape, generator=g)
    gt = torch.where(torch.rand(shape, generator=g) < 0.6, torch.zeros(()), gt).to(device)
    st = R.gt_tile_stats(gt, tiles=True)
    gy, gx = (H + 15) // 16, (W + 15) // 16
    pad = torch.zeros((V, C, gy * 16, gx * 16), dtype=torch.float64)
    pad[:, :, :H, :W] = gt.cpu().double()
    t = pad.reshape(V, C, gy, 16, gx, 16)
    S = (t * t).sum(dim=(3, 5)).permute(0, 2, 3, 1).reshape(V, gy * gx, C)
    N = (t > 0).double().sum(dim=(3, 5)).permute(0, 2, 3, 1).reshape(V, gy * gx, C)
    assert torch.equal(st.tile_N.cpu().double(), N)
    torch.testing.assert_close(st.tile_S.cpu().double(), S, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(st.totals.cpu()[:, 0], S.sum(dim=(1, 2)), rtol=1e-6, atol=1e-6)
    assert torch.equal(st.totals.cpu()[:, 1], N.sum(dim=(1, 2)))
    st2 = R.gt_tile_stats(gt, tiles=True)
    assert torch.equal(st2.tile_S, st.tile_S)   # fixed summation order
    st3 = R.gt_tile_stats(gt)                   # totals only
    assert st3.tile_S is None and torch.equal(st3.totals[:, 1], st.totals[:, 1])
    torch.testing.assert_close(st3.totals[:, 0], st.totals[:, 0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", [(2, 3, 48, 64), (1, 17, 50, 70), (2, 2, 33, 1030), (1, 5, 16, 4100)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gt_tile_stats_signed(device, shape):
    """test_gt_tile_stats' shapes with a fifth of the non-zero entries negative: the masked L2 of an all-zero render leaves a
    pixel with gt <= 0 out (utils/loss_utils.py:88-91), so a negative entry adds to neither sum -- per tile and in the totals."""
    from skelsplat_amd import rasterizer as R
    V, C, H, W = shape
    g = torch.Generator().manual_seed(3)
    gt = torch.rand(shape, generator=g)
    gt = torch.where(torch.rand(shape, generator=g) < 0.6, torch.zeros(()), gt)
    gt = torch.where(torch.rand(shape, generator=g) < 0.2, -gt, gt)
    assert int((gt < 0).sum()) > 100
    st = R.gt_tile_stats(gt.to(device), tiles=True)
    gy, gx = (H + 15) // 16, (W + 15) // 16
    pad = torch.zeros((V, C, gy * 16, gx * 16), dtype=torch.float64)
    pad[:, :, :H, :W] = gt.double()
    t = pad.reshape(V, C, gy, 16, gx, 16)
    S = (t * t * (t > 0)).sum(dim=(3, 5)).permute(0, 2, 3, 1).reshape(V, gy * gx, C)
    N = (t > 0).double().sum(dim=(3, 5)).permute(0, 2, 3, 1).reshape(V, gy * gx, C)
    assert torch.equal(st.tile_N.cpu().double(), N)
    torch.testing.assert_close(st.tile_S.cpu().double(), S, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(st.totals.cpu()[:, 0], S.sum(dim=(1, 2)), rtol=1e-6, atol=1e-6)
    assert torch.equal(st.totals.cpu()[:, 1], N.sum(dim=(1, 2)))
    assert float((S.sum(dim=(1, 2)) - (t * t).sum(dim=(1, 2, 3, 4, 5))).abs().min()) > 1.0      # (the plain sum of squares is another number)
    # the negative entries set to zero: the same bits, per tile and in the totals
    st0 = R.gt_tile_stats(gt.clamp_min(0.0).to(device), tiles=True)
    assert torch.equal(st0.tile_S, st.tile_S) and torch.equal(st0.tile_N, st.tile_N) and torch.equal(st0.totals[:, 1], st.totals[:, 1])
    torch.testing.assert_close(st0.totals[:, 0], st.totals[:, 0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("W,H", [(200, 160), (130, 77), (1030, 40)], ids=["200x160", "130x77", "1030x40"])
def test_heatmap_kernel_equals_formula(device, W, H):
    """sks_heatmaps writes exactly what the tensor-op formula of skelsplat_amd/heatmaps.py gives (which the CPU suite
    pins against scipy.ndimage.gaussian_filter): same fp32 operations, IEEE division."""
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    from skelsplat_amd import heatmaps as hmod
    sc = SyntheticScene("h36m", n_views=3, seed=4, W=W, H=H, device=device)
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scene_type="h36m", device=device)
    p2d = torch.tensor(sc.poses_2d, device=device)
    args = (gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(), p2d, sc.cameras)
    out = hmod.generate_heatmaps(*args)
    row, col, cmin, den = hmod.heatmap_factors(*args)
    ref = (row[:, :, :, None] * col[:, :, None, :] - cmin[:, :, None, None]) / den[:, :, None, None]
    assert out.shape == (3, 17, H, W) and torch.equal(out, ref)
    # and the factor shortcut for the plane minimum / maximum is exact
    hm = row[:, :, :, None] * col[:, :, None, :]
    assert torch.equal(hm.amin(dim=(2, 3)), cmin) and torch.equal(hm.amax(dim=(2, 3)) - cmin + 1e-8, den)
    assert float(out.max()) <= 1.0 and float(out.min()) >= 0.0


@pytest.mark.parametrize("ds,V,W,H", [("h36m", 3, 200, 160), ("panoptic", 5, 330, 177), ("h36m", 2, 1000, 1000)],
                         ids=["200x160", "330x177", "1000x1000"])
def test_heatmap_factor_kernel_equals_tensor_ops(device, ds, V, W, H):
    """sks_heatmap_factors against the tensor-op restatement in oracle/ (the one pinned to the reference's own
    generate_heatmaps by the CPU suite), with rotated, anisotropic Gaussians so that the (R J)^T Sigma^T (R J) operand order matters."""
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    from skelsplat_amd import heatmaps as hmod
    from skelsplat_amd import rasterizer as R
    sc = SyntheticScene(ds, n_views=V, seed=7, W=W, H=H, device=device)
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scene_type=ds, device=device)
    g = torch.Generator().manual_seed(3)
    J = sc.n_joints
    scaling = (gm.get_scaling.detach() * (0.5 + torch.rand((J, 3), generator=g).to(device))).contiguous()
    rot = torch.randn((J, 4), generator=g).to(device)
    p2d = torch.tensor(sc.poses_2d, device=device)
    p2d[0, 0] = torch.tensor([-7.5, 3.2])            # clamped to the image like the reference's impulse position
    p2d[-1, -1] = torch.tensor([W + 20.0, H - 0.5])
    args = (gm._xyz.detach(), scaling, rot, p2d, sc.cameras)
    row, col, cmin, den = hmod.heatmap_factors(*args, scaling_modifier=1.3)
    from oracle import heatmaps_ref
    row_t, col_t, cmin_t, den_t = heatmaps_ref.heatmap_factors(*args, scaling_modifier=1.3)
    for name, a, b in (("row", row, row_t), ("col", col, col_t), ("cmin", cmin, cmin_t), ("den", den, den_t)):
        util.assert_close(name, a.cpu(), b.cpu(), rtol=2e-5, atol_scale=1e-6)
    # the planes and their per-view totals in one pass == planes, then sks_gt_tile_stats over them
    totals = torch.empty((V, 2), dtype=torch.float64, device=device)
    out = hmod.generate_heatmaps(*args, scaling_modifier=1.3, totals=totals)
    assert torch.equal(out, hmod.generate_heatmaps(*args, scaling_modifier=1.3))
    st = R.gt_tile_stats(out)
    assert torch.equal(totals[:, 1], st.totals[:, 1])
    torch.testing.assert_close(totals[:, 0], st.totals[:, 0], rtol=1e-6, atol=0)


def test_heatmap_kernels_reproduce_the_reference_golden(device):
    """tests/golden/reference_heatmaps.npz is the output of the REFERENCE's own generate_heatmaps + normalize_heatmaps
    (utils/general_utils.py:175-304, run in the build container by tests/golden/make_heatmap_golden.py): the two HIP
    kernels reproduce it directly, including the reference's own 2D covariance (which is not the rasterizer's)."""
    import os
    import types
    from skelsplat_amd.heatmaps import generate_heatmaps
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_heatmaps.npz"))
    W, H = int(g["W"]), int(g["H"])
    t = lambda a: torch.tensor(a).to(device)
    cams = [types.SimpleNamespace(image_width=W, image_height=H, world_view_transform=t(g["world_view_transform"][v]),
                                  full_proj_transform=t(g["world_view_transform"][v]),   # (unused by the heat-maps)
                                  FoVx=float(g["fov"][v, 0]), FoVy=float(g["fov"][v, 1])) for v in range(2)]
    hm = generate_heatmaps(t(g["xyz"]), torch.exp(t(g["scaling_raw"])), t(g["rotation_raw"]), t(g["poses_2d"]), cams)
    want = torch.tensor(g["heatmaps"])
    assert hm.shape == want.shape
    assert (hm.cpu() - want).abs().max().item() < 5e-6, (hm.cpu() - want).abs().max().item()


@pytest.mark.parametrize("sparse", [True, False], ids=["sparse", "dense"])
def test_scene_streaming_reuses_graphs(device, sparse):
    """MultiViewLoop.new_scene re-initialises parameters, optimiser state, heat-maps and tile statistics in place, so a
    second frame replays the hipGraphs captured for the first one and ends exactly where a freshly built loop ends."""
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.scene import GaussianModel
    sc, model = _make_loop_scene(device, seed=21)
    rng = np.random.default_rng(0)
    pose2 = (np.asarray(sc.pose_3d_init) + rng.normal(0, 25.0, np.asarray(sc.pose_3d_init).shape)).astype(np.float32)
    p2d2 = (np.asarray(sc.poses_2d) + rng.normal(0, 2.0, np.asarray(sc.poses_2d).shape)).astype(np.float32)

    def fresh(points, p2d):
        gm = GaussianModel().create_from_points(points, sc.spatial_lr_scale, sc.n_joints, scaling=3.9, device=device)
        gm.training_setup()
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                               torch.tensor(p2d, device=device), sc.cameras)
        return gm, MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", sparse=sparse, use_graph=True)

    gmA, loopA = fresh(sc.pose_3d_init, sc.poses_2d)
    loopA.run(120, groups_per_graph=10)
    first = gmA._xyz.detach().clone()
    ptrs = (gmA._xyz.data_ptr(), loopA.size_groups[0][2].data_ptr())
    graph = loopA._multi[1]
    loopA.new_scene(pose2, poses_2d=p2d2)
    assert loopA.iteration == 0 and int(loopA.counters.sum()) == 0
    loopA.run(120, groups_per_graph=10)
    assert loopA._multi[1] is graph and ptrs == (gmA._xyz.data_ptr(), loopA.size_groups[0][2].data_ptr())
    gmB, loopB = fresh(pose2, p2d2)
    loopB.run(120, groups_per_graph=10)
    assert not torch.equal(first, gmA._xyz)
    for a, b in ((gmA._xyz, gmB._xyz), (gmA._scaling, gmB._scaling), (gmA._rotation, gmB._rotation), (gmA._opacity, gmB._opacity)):
        assert torch.equal(a.detach(), b.detach())


def test_run_that_captures_again_sees_the_callers_write(device):
    """run() with another `groups_per_graph` captures again, and the eager group that warms the capture is a real step: on the fused
    tail it must refresh the geometry from the parameters, which the caller has written since the last run -- nobody told the
    loop otherwise.  Graph run against eager step_group()s through the same write: the same bits."""
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    sc, model = _make_loop_scene(device)
    gma, gmb = model(device), model(device)
    hm = generate_heatmaps(gma._xyz.detach(), gma.get_scaling.detach(), gma._rotation.detach(),
                           torch.tensor(sc.poses_2d, device=device), sc.cameras)
    a = MultiViewLoop(gma, sc.cameras, hm, dataset="h36m", sparse=True, use_graph=True)
    b = MultiViewLoop(gmb, sc.cameras, hm, dataset="h36m", sparse=True, use_graph=False)
    assert a.fused_tail
    a.run(12, groups_per_graph=2)
    for _ in range(3):
        b.step_group()
    assert a._multi[0][1] == 2 and a.iteration == b.iteration == 12
    with torch.no_grad():
        gma._xyz.data += 3.0
        gmb._xyz.data += 3.0
    a.run(28, groups_per_graph=3)
    for _ in range(4):
        b.step_group()
    assert a._multi[0][1] == 3 and a.iteration == b.iteration == 28        # (captured again: one eager group, one replay of three)
    for pa, pb in ((gma._xyz, gmb._xyz), (gma._scaling, gmb._scaling), (gma._rotation, gmb._rotation), (gma._opacity, gmb._opacity)):
        assert torch.equal(pa.detach(), pb.detach())


def test_fused_step_tail_many_views(device):
    """The single-workgroup tail walks the views four at a time: 7 views of a 19-joint skeleton (two rounds, the second
    one partial) still equal the separate kernels bit for bit."""
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    sc = SyntheticScene("panoptic", n_views=7, seed=23, W=192, H=112, ring=2500.0, fx=1400.0 * 0.1 * 1.5, device=device)
    res = []
    for fused in (True, False):
        gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9,
                                                scene_type="panoptic", device=device)
        gm.training_setup()
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                               torch.tensor(sc.poses_2d, device=device), sc.cameras)
        loop = MultiViewLoop(gm, sc.cameras, hm, dataset="panoptic", accumulation_steps=7, sparse=True, use_graph=True,
                             fused_tail=fused)
        assert loop.fused_tail == fused and loop.P == 19
        loop.run(70, groups_per_graph=4)
        res.append([t.detach().clone() for t in (gm._xyz, gm._scaling, gm._rotation, gm._opacity, loop.last_losses[1])])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert (res[0][0].cpu() - torch.tensor(sc.pose_3d_init).float()).norm(dim=1).mean() > 0.5


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_fused_step_tail_equals_separate_kernels(device, use_graph):
    """sks_loop_fused_step (compositing backward + one single-workgroup tail: geometry backward, Adam, geometry of the
    updated parameters) gives bit-identical parameters and losses to the separate launches."""
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    sc, model = _make_loop_scene(device, seed=17)
    res = []
    for fused in (True, False):
        gm = model(device)
        with torch.no_grad():
            gm._scaling.add_(0.2 * torch.randn(gm._scaling.shape, generator=torch.Generator().manual_seed(1)).to(device))
            gm._rotation.add_(0.2 * torch.randn(gm._rotation.shape, generator=torch.Generator().manual_seed(2)).to(device))
            gm._opacity.fill_(2.0)
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                               torch.tensor(sc.poses_2d, device=device), sc.cameras)
        loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", sparse=True, use_graph=use_graph, fused_tail=fused)
        assert loop.fused_tail == fused
        loop.run(84, groups_per_graph=5)
        S, N = loop.last_losses
        res.append([t.detach().clone() for t in (gm._xyz, gm._scaling, gm._rotation, gm._opacity, S, N, loop.accumulated_grads)])
    for k, (a, b) in enumerate(zip(*res)):
        if k == 4:   # S starts from the heat-map totals, which each loop accumulates with double atomics (order varies)
            torch.testing.assert_close(a, b, rtol=1e-12, atol=0)
        else:
            assert torch.equal(a, b), k
    assert (res[0][0].cpu() - torch.tensor(sc.pose_3d_init).float()).norm(dim=1).mean() > 1.0


@pytest.mark.parametrize("kind", ["uniform", "clustered", "duplicates", "line"])
@pytest.mark.parametrize("P", [1, 3, 5, 17, 300, 5000, 40000])
def test_knn_grid_equals_allpairs(device, P, kind):
    """The uniform-grid search used for large clouds returns exactly the floats of the all-pairs sweep (both are exact
    3-NN searches evaluating each squared distance the same way), whatever the distribution."""
    from skelsplat_amd.ops import distCUDA2
    g = torch.Generator().manual_seed(P + len(kind))
    if kind == "uniform":
        pts = torch.rand(P, 3, generator=g) * 1000
    elif kind == "clustered":   # a few tight blobs far apart: most grid cells are empty, the search needs many shells
        centres = torch.rand(5, 3, generator=g) * 1e4
        pts = centres[torch.randint(0, 5, (P,), generator=g)] + torch.randn(P, 3, generator=g)
    elif kind == "duplicates":
        base = torch.rand(max(1, P // 4), 3, generator=g) * 100
        pts = base[torch.randint(0, base.shape[0], (P,), generator=g)]
    else:                        # degenerate extent in two axes
        pts = torch.zeros(P, 3)
        pts[:, 0] = torch.rand(P, generator=g) * 50
    pts = pts.to(device)
    a = distCUDA2(pts, method="allpairs")
    b = distCUDA2(pts, method="grid")
    assert torch.equal(a, b)
    if P > 2048:
        assert torch.equal(distCUDA2(pts), b)


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_knn_box_pass_takes_a_second_trip(device, kind):
    """k_knn_bbox runs at most 256 workgroups of 256 threads, so its grid-stride loop takes a second trip only for P > 65 536;
    here P = 70 001 and the smallest and the largest coordinate of every axis sit at indices >= 65 536, where only that trip
    reads them.  The grid search, the automatic choice and the all-pairs sweep agree bit for bit, and on 512 sampled rows (the
    extreme points among them) all equal the float32 brute force of test_knn_matches_bruteforce.  The cap of 160 cells per
    axis, reached above 8 million points, stays out of scope."""
    from skelsplat_amd.ops import distCUDA2
    P, first_trip = 70001, 256 * 256
    g = torch.Generator().manual_seed(P + len(kind))
    if kind == "uniform":
        pts = torch.rand(P, 3, generator=g) * 1000
    else:
        centres = torch.rand(5, 3, generator=g) * 1e4
        pts = centres[torch.randint(0, 5, (P,), generator=g)] + torch.randn(P, 3, generator=g)
    p = pts.numpy().astype(np.float32)
    ext = np.unique(np.concatenate([p.argmin(axis=0), p.argmax(axis=0)]))
    early = ext[ext < first_trip]
    free = np.setdiff1d(np.arange(first_trip, P), ext)[:early.size]
    p[np.concatenate([early, free])] = p[np.concatenate([free, early])]          # swap the early extremes behind the first trip
    ext = np.unique(np.concatenate([p.argmin(axis=0), p.argmax(axis=0)]))
    assert ext.min() >= first_trip and np.all(p[:first_trip].min(axis=0) > p.min(axis=0)) \
        and np.all(p[:first_trip].max(axis=0) < p.max(axis=0))
    dev_pts = torch.from_numpy(p).to(device)
    b = distCUDA2(dev_pts, method="grid")
    assert torch.equal(distCUDA2(dev_pts), b) and torch.equal(distCUDA2(dev_pts, method="allpairs"), b)
    rng = np.random.default_rng(len(kind))
    rows = np.concatenate([ext, rng.choice(np.setdiff1d(np.arange(P), ext), 512 - ext.size, replace=False)])
    d = p[rows, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(np.float32)
    d2[np.arange(rows.size), rows] = np.float32(np.finfo(np.float32).max)
    part = np.partition(d2, 3, axis=1)[:, :3]
    part.sort(axis=1)
    want = ((part[:, 0] + part[:, 1]) + part[:, 2]) / np.float32(3.0)
    np.testing.assert_allclose(b.cpu().numpy()[rows], want, rtol=2e-6)


# ------------------------------------------------------------------------------------------ view-sharded exchange
@pytest.fixture
def rccl_world1(device):
    """A torch.distributed process group of ONE rank on RCCL: MultiViewLoop then takes the exchange branch -- padded
    shard, all_gather_into_tensor, rank-major sks_loop_adam_step -- that 2..8 GPUs take."""
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29600 + os.getpid() % 1000)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
    try:
        yield dist
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["sparse", "dense", "sparse-hipgraph", "mixed-sizes"])
def test_exchange_branch_on_rccl_equals_unsharded_loop(device, rccl_world1, mode):
    """The production path of N > 1 GPUs at world size 1: the group runs geometry + fused backward into the padded shard,
    ONE all_gather_into_tensor over RCCL, and the optimiser kernel on the gathered (rank-major) buffer.  Bit-identical
    to the loop that never touches torch.distributed (shard_views=False)."""
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.scene import SyntheticScene
    sc, model = _make_loop_scene(device, seed=31)
    cams = sc.cameras
    if mode == "mixed-sizes":
        b = SyntheticScene("h36m", n_views=4, seed=31, W=162, H=128, ring=2500.0, fx=1145.0 * 0.16 * 1.5, device=device)
        cams = [b.cameras[0], sc.cameras[1], sc.cameras[2], b.cameras[3]]
    res = []
    for shard in (True, False):
        gm = model(device)
        with torch.no_grad():
            gm._opacity.fill_(2.0)
            gm._scaling.add_(0.2 * torch.randn(gm._scaling.shape, generator=torch.Generator().manual_seed(1)).to(device))
        hms = [generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                                 torch.tensor(sc.poses_2d[v:v + 1], device=device), [cams[v]])[0] for v in range(4)]
        hm = torch.stack(hms) if mode != "mixed-sizes" else hms
        loop = MultiViewLoop(gm, cams, hm, dataset="h36m", sparse=mode != "dense", shard_views=shard,
                             use_graph=mode == "sparse-hipgraph", graph_collectives=True, fused_tail=False)
        assert loop.exchange == shard and loop.world == 1 and loop.device_tail
        if shard:
            assert loop._allg.shape == (4, 17, 11) and loop._shard.shape == (4, 17, 11)
        assert loop.use_graph == (mode == "sparse-hipgraph")
        loop.run(32)
        S, N = loop.last_losses
        res.append([x.detach().clone() for x in (gm._xyz, gm._scaling, gm._rotation, gm._opacity, loop.accumulated_grads, N)])
    for k, (a, b_) in enumerate(zip(*res)):
        assert torch.equal(a, b_), k
    assert (res[0][0].cpu() - torch.tensor(sc.pose_3d_init).float()).norm(dim=1).mean() > 0.5


def test_direct_rccl_gather_equals_torch_distributed(device, rccl_world1):
    """skelsplat_amd.rccl_direct: ncclAllGather through a communicator of the library's own, enqueued on the CURRENT stream
    (torch.distributed's process group hands every collective to an internal stream), gives what
    dist.all_gather_into_tensor gives; one communicator per (group, device); opt-in: without SKS_RCCL_DIRECT=1 there is none."""
    import torch.distributed as dist
    from skelsplat_amd.rccl_direct import DirectGather
    assert os.environ.get("SKS_RCCL_DIRECT") is None and DirectGather.create(device) is None     # off unless asked for
    os.environ["SKS_RCCL_DIRECT"] = "1"
    try:
        dg = DirectGather.create(device)
        assert dg is not None and DirectGather.create(device) is dg
    finally:
        del os.environ["SKS_RCCL_DIRECT"]
    inp = torch.randn((4, 19, 11), device=device)
    a, b = torch.empty_like(inp), torch.full_like(inp, float("nan"))
    dist.all_gather_into_tensor(a, inp)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):      # on whatever stream is current: no hand-over to another one
        dg.all_gather_into_tensor(b, inp)
    side.synchronize()
    assert torch.equal(a, inp) and torch.equal(b, inp)
    with pytest.raises(ValueError):
        dg.all_gather_into_tensor(torch.empty(5, device=device), inp)
    # the weighted all-reduce (pre-multiplied sum): with one rank, out = weight * inp; the op of a weight is built once
    m, out = torch.randn((19, 3), device=device), torch.empty((19, 3), device=device)
    for w in (4.0 / 31.0, 1.0, 4.0 / 31.0):
        dg.all_reduce_weighted(out, m, w)
        torch.cuda.synchronize()
        assert torch.allclose(out, m * w, rtol=1e-6, atol=0)
    assert len(dg._ops) == 2
    with pytest.raises(ValueError):       # tensors of another device than the communicator's
        dg.all_gather_into_tensor(torch.empty(4), torch.empty(4))
    dg.destroy()
    assert DirectGather.create(device) is None


def test_adam_step_reads_the_gathered_rank_major_layout(device):
    """sks_loop_adam_step(shard_world = N) on the buffer all_gather_into_tensor leaves for N ranks (view v = row
    (v % N) * ceil(V / N) + v // N, pad rows ignored) == the view-major call, for uneven shards (7 views over 2, 3, 4 and
    8 ranks) and the many-view code path (31 views over 8)."""
    import ctypes
    from skelsplat_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream(device).cuda_stream
    g = torch.Generator(device=device).manual_seed(11)
    sched = (ctypes.c_double * 5)(2.0, 0.02, 0.0, 0.0, 4000.0)
    lrs = (ctypes.c_double * 3)(0.005, 0.001, 0.05)
    adam = (ctypes.c_double * 3)(0.9, 0.999, 1e-15)
    for V, P, worlds, limb in ((7, 17, (2, 3, 4, 8), (ctypes.c_int * 8)(12, 13, 15, 16, 5, 6, 2, 3)), (31, 19, (8,), None)):
        grads = torch.randn((V, P, 11), device=device, generator=g)
        init = [torch.randn(s, device=device, generator=g) for s in ((P, 3), (P, 3), (P, 4), (P, 1))]
        slots0 = torch.randn((V, P, 3), device=device, generator=g)
        mask, last = (1 << V) - 1 - 2, V - 2        # one view not rendered in this group: its slot keeps the old value

        def run(buf, world):
            prm = [x.clone() for x in init]
            slots = slots0.clone()
            m, vv = torch.zeros((P, 11), device=device), torch.zeros((P, 11), device=device)
            cnt = torch.zeros(2, dtype=torch.int32, device=device)
            for _ in range(3):
                _lib.check(lib.sks_loop_adam_step(V, P, buf.data_ptr(), slots.data_ptr(), mask, last, prm[0].data_ptr(),
                                                  prm[1].data_ptr(), prm[2].data_ptr(), prm[3].data_ptr(), m.data_ptr(),
                                                  vv.data_ptr(), cnt.data_ptr(), V, sched, lrs, adam, 1e-3, limb, world, stream),
                           "sks_loop_adam_step")
            return prm + [slots, m, vv, cnt]

        ref = run(grads, 1)
        for world in worlds:
            vmax = (V + world - 1) // world
            buf = torch.full((world * vmax, P, 11), float("nan"), device=device)    # pad rows must never be read
            for v in range(V):
                buf[(v % world) * vmax + v // world] = grads[v]
            for a, b in zip(ref, run(buf, world)):
                assert torch.equal(a, b), (V, world)
        assert not torch.equal(ref[0], init[0])


def test_adam_step_with_the_criterion_reads_the_sums_from_the_gathered_blocks(device):
    """sks_loop_adam_step_es(shard_world = N, loss_sums = NULL): every rank's block of the gathered buffer is its gradient rows
    (padded to an even float count) followed by its views' {S, N} doubles (sks_loop_shard_floats) -- the criterion's inputs cross in
    the gradients' all_gather.  Against the one-rank call (view-major rows, separate sums), for uneven shards: the same stopping
    iteration, cut inside a group, and bit for bit the same state; after the stop further launches change nothing."""
    import ctypes
    from skelsplat_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream(device).cuda_stream
    g = torch.Generator(device=device).manual_seed(5)
    sched = (ctypes.c_double * 5)(2e-3, 2e-4, 0.0, 0.0, 4000.0)    # (small steps: the limb term of the loss barely moves)
    lrs = (ctypes.c_double * 3)(0.005, 0.001, 0.05)
    adam = (ctypes.c_double * 3)(0.9, 0.999, 1e-15)
    limb = (ctypes.c_int * 8)(12, 13, 15, 16, 5, 6, 2, 3)
    V, P, acc, w, tol = 7, 17, 5, 3, 5e-4
    groups = 9
    grads = torch.randn((groups, V, P, 11), device=device, generator=g) * 1e-3
    # losses that settle: S / N converges geometrically, so the window test fires a few groups in, in the middle of a group
    N = torch.full((groups, V), 1000.0, dtype=torch.float64, device=device)
    it = torch.arange(groups * V, device=device, dtype=torch.float64).reshape(groups, V)
    S = N * (0.5 + 0.3 * torch.exp(-it / 2.5))
    init = [torch.randn(s_, device=device, generator=g) for s_ in ((P, 3), (P, 3), (P, 4), (P, 1))]

    def run(world):
        prm = [x.clone() for x in init]
        slots = torch.zeros((V, P, 3), device=device)
        m, vv = torch.zeros((P, 11), device=device), torch.zeros((P, 11), device=device)
        cnt = torch.zeros(2, dtype=torch.int32, device=device)
        es = torch.zeros(2 + 2 * w, dtype=torch.int32, device=device)
        flag = torch.zeros(1, dtype=torch.int32).pin_memory()
        vmax = (V + world - 1) // world
        nfl = int(lib.sks_loop_shard_floats(V, P, world))
        assert nfl % 2 == 0 and nfl >= vmax * P * 11 + 4 * vmax
        snap = None
        for k in range(groups):
            it0 = k * acc + 1
            views = [(it0 + j - 1) % V for j in range(acc)]
            mask = 0
            for v in views:
                mask |= 1 << v
            sums = torch.stack([S[k], N[k]], dim=1).contiguous()          # (V, 2): this group's sums, by view
            if world == 1:
                buf, sp = grads[k].contiguous(), sums.data_ptr()
            else:
                buf = torch.full((world * nfl,), float("nan"), device=device)
                for v in range(V):
                    r, l = v % world, v // world
                    buf[r * nfl + l * P * 11:r * nfl + (l + 1) * P * 11] = grads[k, v].reshape(-1)
                    buf[r * nfl + nfl - 4 * vmax:r * nfl + nfl].view(torch.float64).view(vmax, 2)[l] = sums[v]
                sp = None
            _lib.check(lib.sks_loop_adam_step_es(V, P, buf.data_ptr(), slots.data_ptr(), mask, views[-1], prm[0].data_ptr(),
                                                 prm[1].data_ptr(), prm[2].data_ptr(), prm[3].data_ptr(), m.data_ptr(), vv.data_ptr(),
                                                 cnt.data_ptr(), acc, sched, lrs, adam, 1e-3, limb, world, sp, es.data_ptr(), w, tol,
                                                 flag.data_ptr(), stream), "sks_loop_adam_step_es")
            torch.cuda.synchronize()
            if int(flag[0]) and snap is None:
                snap = [x.clone() for x in prm + [slots, m, vv, cnt]]
        assert snap is not None, "the criterion never fired"
        for a, b in zip(snap, prm + [slots, m, vv, cnt]):          # launches behind the stop did nothing
            assert torch.equal(a, b)
        assert int(es[1]) == int(flag[0]) == int(cnt[0])
        return int(flag[0]), snap

    stop1, ref = run(1)
    assert stop1 % acc != 0 and 2 * w <= stop1 < groups * acc, stop1      # the cut falls inside a group
    for world in (2, 3, 4, 8):
        stop, got = run(world)
        assert stop == stop1, (world, stop, stop1)
        for a, b in zip(ref, got):
            assert torch.equal(a, b), world


def test_early_stopping_cuts_the_group_like_the_reference(device):
    """training.early_stopping = opt_early_stopping (train.py:155, 182-233): the criterion sees every iteration's loss in
    order; when it fires inside a group, only the views up to that iteration refresh their slots, that view's scaling /
    rotation / opacity gradients win, the optimiser steps at once and the scene ends.  Against the literal per-iteration
    loop on the oracle with the reference's own criterion class semantics."""
    import copy
    from skelsplat_amd.loop import MultiViewLoop, OptEarlyStopping
    from skelsplat_amd.heatmaps import generate_heatmaps
    from tests.ref_loop import view_grads_ref
    sc, model = _make_loop_scene(device, seed=9)
    gm = model(device)
    hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                           torch.tensor(sc.poses_2d, device=device), sc.cameras)
    tol = 8e-4        # with the reference's window of 4 (= the views) this fires at iteration 30 of this scene: mid-group
    loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", early_stopping=OptEarlyStopping(window_size=4, repeat_tolerance=tol))
    assert loop._stopping and not loop.fused_tail and not loop.use_graph
    assert loop._es_device                        # the reference's criterion runs inside the optimiser kernel
    with pytest.raises(ValueError):               # ... any other callable is a host decision per group: no hipGraph
        MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", early_stopping=lambda loss: False, use_graph=True)
    loop.run(400)
    assert loop.stopped_at is not None and loop.iteration == loop.stopped_at < 400
    # literal loop
    gmr = model("cpu")
    cams_cpu = [copy.copy(c).to("cpu") for c in sc.cameras]
    hm_cpu = hm.cpu()
    crit = OptEarlyStopping(window_size=4, repeat_tolerance=tol)
    acc = torch.zeros(4, 17, 3)
    stopped = None
    for it in range(1, 401):
        gmr.update_learning_rate(it)
        idx = (it - 1) % 4
        loss, (gx, gs, gr, go) = view_grads_ref(gmr, cams_cpu[idx], hm_cpu[idx], sc.W, sc.H, "h36m", 1e-5)
        stop = crit(float(loss))
        acc[idx] = gx
        gmr._scaling.grad, gmr._rotation.grad, gmr._opacity.grad = gs, gr, go
        if it % 4 == 0 or stop:
            gmr._xyz.grad = acc.mean(0)
            gmr.optimizer.step()
            gmr.optimizer.zero_grad(set_to_none=True)
        if stop:
            stopped = it
            break
    assert stopped is not None and stopped % 4 != 0, stopped          # the cut falls inside a group
    assert stopped == loop.stopped_at, (stopped, loop.stopped_at)
    assert (gm._xyz.detach().cpu() - gmr._xyz.detach()).norm(dim=1).max().item() < 0.05
    util.assert_close("scaling", gm._scaling.detach().cpu(), gmr._scaling.detach(), rtol=1e-3, atol_scale=1e-4)
    # a loop that never stops is somewhere else by then
    gm2 = model(device)
    MultiViewLoop(gm2, sc.cameras, hm, dataset="h36m").run(stopped + 2)
    assert (gm2._xyz.detach() - gm._xyz.detach()).norm(dim=1).max().item() > 1e-3


@pytest.mark.parametrize("mode", ["eager", "hipgraph", "dense", "sharded-world1"])
def test_device_side_early_stopping_decides_like_the_host_criterion(device, mode, request):
    """sks_loop_adam_step_es against the host path (the same OptEarlyStopping class fed from a read-back of every group's sums,
    MultiViewLoop._early_stop_cut): the same stopping iteration and bit for bit the same parameters, moments and slots -- eager,
    inside hipGraphs (25 groups per graph: the groups replayed behind the stop must do nothing), on the dense path, and through
    the view-sharded exchange, where the sums ride in the gradients' all_gather."""
    from skelsplat_amd.loop import MultiViewLoop, OptEarlyStopping
    from skelsplat_amd.heatmaps import generate_heatmaps
    if mode == "sharded-world1":
        request.getfixturevalue("rccl_world1")
    sc, model = _make_loop_scene(device, seed=9)
    tol = 8e-4
    res = []
    for on_device in (True, False):
        gm = model(device)
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                               torch.tensor(sc.poses_2d, device=device), sc.cameras)
        crit = OptEarlyStopping(window_size=4, repeat_tolerance=tol)
        host_crit = OptEarlyStopping(window_size=4, repeat_tolerance=tol)
        loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", sparse=mode != "dense",
                             shard_views=mode == "sharded-world1", use_graph=on_device and mode == "hipgraph",
                             graph_collectives=True,
                             early_stopping=crit if on_device else (lambda loss: host_crit(loss)))
        assert loop._es_device == on_device and loop.exchange == (mode == "sharded-world1")
        if on_device and mode == "sharded-world1":
            assert loop._shard_flat is not None and loop._allg.numel() == loop._shard_flat.numel()
        loop.run(400)
        assert loop.stopped_at is not None and loop.iteration == loop.stopped_at and loop.stopped_at % 4 != 0
        assert int(loop.counters[0]) == loop.stopped_at          # the device's own iteration counter ended there too
        res.append((loop.stopped_at, [x.detach().clone() for x in (gm._xyz, gm._scaling, gm._rotation, gm._opacity, loop.exp_avg,
                                                                   loop.exp_avg_sq, loop.accumulated_grads, loop.counters)]))
        if on_device:       # a second scene through the same loop: state, flag and counters start over
            loop.new_scene(torch.tensor(sc.pose_3d_init, device=device, dtype=torch.float32), heatmaps=hm)
            assert loop.stopped_at is None and int(loop._es_state.abs().sum()) == 0
            loop.run(400)
            assert loop.stopped_at == res[0][0]
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for k, (a, b) in enumerate(zip(res[0][1], res[1][1])):
        assert torch.equal(a, b), k


def test_heatmap_dropout_zeroes_the_drawn_planes(device):
    """training.dropout (general_utils.py:267-283): three cameras from randint(4) and three joints from randint(J) get no
    impulse -> all-zero planes; the other planes are untouched and the fused totals see the zeros."""
    from skelsplat_amd.heatmaps import generate_heatmaps, draw_dropout
    sc, model = _make_loop_scene(device, seed=4)
    gm = model(device)
    p2d = torch.tensor(sc.poses_2d, device=device)
    args = (gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(), p2d, sc.cameras)
    base = generate_heatmaps(*args)
    torch.manual_seed(123)
    cams = torch.randint(4, (3,))
    joints = torch.randint(17, (3,))
    torch.manual_seed(123)
    mask = draw_dropout(4, 17)
    want = torch.zeros(4, 17, dtype=torch.bool)
    for c in cams.tolist():
        want[c, joints] = True
    assert torch.equal(mask, want) and mask.any()
    totals = torch.zeros((4, 2), dtype=torch.float64, device=device)
    hm = generate_heatmaps(*args, drop_mask=mask, totals=totals)
    m = mask.to(device)
    assert float(hm[m].abs().max()) == 0.0 and torch.equal(hm[~m], base[~m])
    torch.testing.assert_close(totals[:, 0], (hm.double() ** 2).sum(dim=(1, 2, 3)), rtol=1e-6, atol=0)   # (fp32 partial sums per thread)
    assert torch.equal(totals[:, 1], (hm > 0).sum(dim=(1, 2, 3)).double())


def test_heatmap_totals_are_reproducible_bit_for_bit(device):
    """The per-view loss constants (sum of gt^2, count of gt > 0) feed the reported loss and the early-stopping criterion:
    both ways of forming them -- on the way while sks_heatmaps writes the planes (what MultiViewLoop.new_scene takes), and from
    the factors alone (sks_heatmap_totals) -- combine their workgroups' sums in fixed point, so repeated runs agree exactly
    although the workgroups finish in a different order every time."""
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    from skelsplat_amd.heatmaps import generate_heatmaps
    sc = SyntheticScene("h36m", n_views=4, seed=3, device=device, W=1000, H=1000)
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, device=device)
    p2d = torch.tensor(sc.poses_2d, device=device)
    args = (gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(), p2d, sc.cameras)
    runs = []
    for _ in range(6):
        totals = torch.zeros((4, 2), dtype=torch.float64, device=device)
        hm = generate_heatmaps(*args, totals=totals)
        runs.append(totals.clone())
    for t in runs[1:]:
        assert torch.equal(t, runs[0])
    torch.testing.assert_close(runs[0][:, 0], (hm.double() ** 2).sum(dim=(1, 2, 3)), rtol=1e-6, atol=0)
    assert torch.equal(runs[0][:, 1], (hm > 0).sum(dim=(1, 2, 3)).double())


@pytest.mark.parametrize("mixed", [False, True], ids=["4x1000", "1002-1000-1000-1002"])
def test_full_size_h36m_loop_sparse_equals_dense(device, mixed):
    """BASELINE config 2 at full size, through the loop: 40 iterations of the sparse fused step (two launches per group,
    hipGraphs) end where the dense device path (full images, sks_masked_l2, dense backward) ends -- with four equal sensors
    and with H36M's real mix of 1002- and 1000-wide ones (one launch sequence in the sparse path, two in the dense one)."""
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    a = SyntheticScene("h36m", n_views=4, seed=0, device=device, W=1000, H=1000)
    b = SyntheticScene("h36m", n_views=4, seed=0, device=device, W=1002, H=1000)
    cams = [b.cameras[0], a.cameras[1], a.cameras[2], b.cameras[3]] if mixed else a.cameras
    res = []
    for kw in (dict(sparse=True, use_graph=True), dict(sparse=False)):
        gm = GaussianModel().create_from_points(a.pose_3d_init, a.spatial_lr_scale, 17, device=device)
        gm.training_setup()
        hms = [generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                                 torch.tensor(a.poses_2d[v:v + 1], device=device), [cams[v]])[0] for v in range(4)]
        loop = MultiViewLoop(gm, cams, hms if mixed else torch.stack(hms), dataset="h36m", **kw)
        assert (len(loop.size_groups) == 2) == mixed
        if kw["sparse"]:
            assert loop.fused_tail and (loop.views_all.mixed == mixed)
        loop.run(40)
        S, N = loop.last_losses
        res.append([x.detach().clone() for x in (gm._xyz, gm._scaling, gm._rotation, N, S)])
    moved = (res[0][0].cpu() - torch.tensor(a.pose_3d_init).float()).norm(dim=1).mean().item()
    assert moved > 0.5
    assert (res[0][0] - res[1][0]).norm(dim=1).max().item() < 2e-3 * moved
    util.assert_close("scaling", res[0][1].cpu(), res[1][1].cpu(), rtol=1e-4, atol_scale=1e-4)
    assert torch.equal(res[0][3], res[1][3])                                  # mask counts: integers, exact
    assert ((res[0][4] - res[1][4]).abs() <= 1e-5 * res[1][4].abs()).all()



# ------------------------------------------------------------------ frame batching: F frames in the two launches of one
@pytest.mark.parametrize("factored", [True, False], ids=["factors", "planes"])
@pytest.mark.parametrize("mode", ["same", "mixed", "graph5", "wide9", "panoptic7", "oneview", "twoviews"])
def test_frame_batch_equals_separate_loops(device, mode, factored):
    """FrameBatchLoop steps F independent frames per launch (sks_loop_fused_step(frames=F), one tail workgroup per frame);
    every frame must end EXACTLY where a MultiViewLoop running it alone ends: parameters, Adam moments, V-slot buffers,
    per-view losses, and the heat-maps generated for it.  `mixed`: two image sizes (H36M's 1000/1002 sensors, scaled);
    `graph5`: 5 views with 4-iteration groups (masks that rotate) inside hipGraphs; `wide9`: 9 views per frame.
    `factors` (the default): the batch never writes a heat-map plane -- the fused step evaluates the pseudo-GT from its
    separable factors and the loss constants come from sks_heatmap_totals -- and still equals the loops that read planes."""
    from skelsplat_amd.loop import MultiViewLoop, FrameBatchLoop
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    F = 3
    V = {"graph5": 5, "wide9": 9, "panoptic7": 7, "oneview": 1, "twoviews": 2}.get(mode, 4)   # wide9: > 8 views, LDS-parked slot walk
    ds = "panoptic" if mode == "panoptic7" else "h36m"            # panoptic7: 19 joints / channels (the CG = 20 kernels)
    sc, model = _make_loop_scene(device, V=V, seed=51)
    if ds == "panoptic":
        sc = SyntheticScene("panoptic", n_views=V, seed=51, W=192, H=112, ring=2500.0, fx=1400.0 * 0.1 * 1.5, device=device)

        def model(device):
            gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, sc.n_joints, scaling=3.9,
                                                    scene_type="panoptic", device=device)
            gm.training_setup()
            return gm
    cams = sc.cameras
    if mode == "mixed":
        b = SyntheticScene("h36m", n_views=V, seed=51, W=162, H=128, ring=2500.0, fx=1145.0 * 0.16 * 1.5, device=device)
        cams = [b.cameras[0], sc.cameras[1], sc.cameras[2], b.cameras[3]]
    rng = np.random.default_rng(5)
    base3, base2 = np.asarray(sc.pose_3d_init, np.float32), np.asarray(sc.poses_2d, np.float32)
    pts = np.stack([base3 + rng.normal(0, 30.0 * f, base3.shape) for f in range(F)]).astype(np.float32)
    p2d = np.stack([base2 + rng.normal(0, 3.0 * f, base2.shape) for f in range(F)]).astype(np.float32)
    drop = torch.zeros((F, V, sc.n_joints), dtype=torch.bool)
    drop[1, min(2, V - 1), [3, 9]] = True          # frame 1 loses two planes of one view (training.dropout)
    use_graph = mode == "graph5"
    iters = 44
    fb = FrameBatchLoop(model(device), cams, F, dataset=ds, use_graph=use_graph, factored=factored)
    assert (fb.hset is None) == factored
    fb.new_scenes(pts, poses_2d=p2d, drop_masks=drop)
    out = fb.run(iters, groups_per_graph=4).clone()
    assert tuple(out.shape) == (F, sc.n_joints, 3) and fb.iteration == iters
    assert int(fb.counters[:, 0].min()) == int(fb.counters[:, 0].max()) > 0
    for f in range(F):
        gm = model(device)
        hm0 = [torch.zeros((sc.n_joints, int(c.image_height), int(c.image_width)), device=device) for c in cams]
        loop = MultiViewLoop(gm, cams, hm0 if mode == "mixed" else torch.stack(hm0), dataset=ds, sparse=True,
                             use_graph=use_graph, fused_tail=True)
        assert loop.fused_tail
        from skelsplat_amd.heatmaps import generate_heatmaps
        # (new_scene draws its own dropout; give the planes explicitly instead)
        gm.reset_from_points(pts[f])
        for slots, vb, gt, stats, idx in loop.size_groups:
            generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                              torch.tensor(p2d[f][slots], device=device), [cams[k] for k in slots], out=gt, views=vb,
                              totals=stats.totals, drop_mask=drop[f][slots])
        if len(loop.size_groups) > 1:
            loop._merge_totals()
        for v in range(V):                                       # the batched generator wrote / describes the same planes
            mine = (fb.factors.planes(f * V + v, (int(cams[v].image_width), int(cams[v].image_height))) if factored
                    else fb.hset.planes[f * V + v])
            assert torch.equal(mine, loop.hset.planes[v]), (f, v)
        assert torch.equal(fb.stats_all.totals[f * V:(f + 1) * V, 1], loop.stats_all.totals[:, 1])     # counts: exact
        tS, rS = fb.stats_all.totals[f * V:(f + 1) * V, 0], loop.stats_all.totals[:, 0]
        assert ((tS - rS).abs() <= 1e-6 * rS.abs()).all()    # sums: fp32 partials of different lengths, fp64 across
        loop.run(iters, groups_per_graph=4)
        assert torch.equal(out[f], gm._xyz.detach()), f
        assert torch.equal(fb.scaling[f], gm._scaling.detach()) and torch.equal(fb.rotation[f], gm._rotation.detach())
        assert torch.equal(fb.opacity[f], gm._opacity.detach())
        assert torch.equal(fb.exp_avg[f], loop.exp_avg) and torch.equal(fb.exp_avg_sq[f], loop.exp_avg_sq)
        assert torch.equal(fb.accumulated_grads[f], loop.accumulated_grads)
        assert torch.equal(fb.counters[f], loop.counters)
        S, N = loop.last_losses
        # N (a pixel count) is exact; S starts from the heat-map totals sks_heatmaps accumulates with fp64 atomics, whose
        # order is not fixed: equal to the last few bits (nothing but the reported loss reads S)
        assert torch.equal(fb.last_losses[1][f], N)
        assert ((fb.last_losses[0][f] - S).abs() <= (1e-6 if factored else 1e-12) * S.abs()).all()
    assert not torch.equal(out[0], out[1])


def test_frame_batch_sequence_with_a_partial_last_batch(device):
    """optimize_sequence: 5 frames through batches of 2 (the last one padded) == the same frames through a batch of 5."""
    from skelsplat_amd.loop import FrameBatchLoop
    sc, model = _make_loop_scene(device, V=4, seed=52)
    rng = np.random.default_rng(6)
    base3, base2 = np.asarray(sc.pose_3d_init, np.float32), np.asarray(sc.poses_2d, np.float32)
    pts = np.stack([base3 + rng.normal(0, 20.0, base3.shape) for _ in range(5)]).astype(np.float32)
    p2d = np.stack([base2 + rng.normal(0, 2.0, base2.shape) for _ in range(5)]).astype(np.float32)
    a = FrameBatchLoop(model(device), sc.cameras, 2, dataset="h36m", use_graph=True).optimize_sequence(pts, p2d, iterations=24, groups_per_graph=3)
    fb = FrameBatchLoop(model(device), sc.cameras, 5, dataset="h36m")
    fb.new_scenes(pts, poses_2d=p2d)
    b = fb.run(24)
    assert tuple(a.shape) == (5, sc.n_joints, 3) and torch.equal(a, b)
    assert (a.cpu() - torch.tensor(pts)).norm(dim=2).mean().item() > 0.05


def test_frame_pipeline_on_streams_equals_one_batch(device):
    """FramePipeline: 7 frames through 2 loops of 2 frames on 2 HIP streams (two rounds, the last batch padded) == the same
    7 frames in one 7-frame batch -- bit for bit, whatever the interleaving of the streams' graph launches."""
    from skelsplat_amd.loop import FrameBatchLoop, FramePipeline
    sc, model = _make_loop_scene(device, V=4, seed=53)
    rng = np.random.default_rng(7)
    base3, base2 = np.asarray(sc.pose_3d_init, np.float32), np.asarray(sc.poses_2d, np.float32)
    pts = np.stack([base3 + rng.normal(0, 20.0, base3.shape) for _ in range(7)]).astype(np.float32)
    p2d = np.stack([base2 + rng.normal(0, 2.0, base2.shape) for _ in range(7)]).astype(np.float32)
    pipe = FramePipeline(model(device), sc.cameras, frames=2, streams=2, dataset="h36m")
    a = pipe.optimize_sequence(pts, p2d, iterations=32, groups_per_graph=3, interleave=8)
    torch.cuda.synchronize()
    fb = FrameBatchLoop(model(device), sc.cameras, 7, dataset="h36m")
    fb.new_scenes(pts, poses_2d=p2d)
    b = fb.run(32)
    assert tuple(a.shape) == (7, sc.n_joints, 3) and torch.equal(a, b)
    a2 = pipe.optimize_sequence(pts, p2d, iterations=32, groups_per_graph=3, interleave=8)   # graphs reused
    assert torch.equal(a2, b)


def test_frame_batch_refuses_what_it_cannot_do(device):
    from skelsplat_amd.loop import FrameBatchLoop
    sc, model = _make_loop_scene(device, V=4, seed=3)
    with pytest.raises(ValueError, match="exceeds"):
        FrameBatchLoop(model(device), sc.cameras, 17)
    fb = FrameBatchLoop(model(device), sc.cameras, 2)
    with pytest.raises(ValueError, match="points must be"):
        fb.new_scenes(np.zeros((3, 17, 3), np.float32), poses_2d=np.zeros((2, 4, 17, 2), np.float32))
    with pytest.raises(ValueError, match="poses_2d or heatmaps"):
        fb.new_scenes(np.zeros((2, 17, 3), np.float32))

# ------------------------------------------------------------------ two ranks, one GPU (gloo): the sharded branch at world 2
def _two_rank_worker(rank, world, port, mode, ret):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)   # RCCL refuses two ranks on one device
    from skelsplat_amd.loop import MultiViewLoop
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.scene import SyntheticScene
    sc, model = _make_loop_scene(dev, V=5, seed=41)          # 5 views over 2 ranks: shards of 3 and 2, one pad row
    cams = sc.cameras
    if mode == "mixed":
        b = SyntheticScene("h36m", n_views=5, seed=41, W=162, H=128, ring=2500.0, fx=1145.0 * 0.16 * 1.5, device=dev)
        cams = [b.cameras[0], sc.cameras[1], sc.cameras[2], b.cameras[3], sc.cameras[4]]
    gm = model(dev)
    with torch.no_grad():
        gm._opacity.fill_(2.0)
    hms = [generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                             torch.tensor(sc.poses_2d[v:v + 1], device=dev), [cams[v]])[0] for v in range(5)]
    es = "no_stopping"
    if mode == "early_stop":
        from skelsplat_amd.loop import OptEarlyStopping
        # (a tolerance the masked-L2 losses always meet: the criterion fires as soon as it has its two windows, at iteration 8 --
        # the third iteration of the second group --, and the ranks learn of it ES_SYNC_GROUPS groups into the run)
        es = OptEarlyStopping(window_size=4, repeat_tolerance=1.0)
    loop = MultiViewLoop(gm, cams, hms, dataset="h36m", accumulation_steps=5, sparse=mode != "dense", fused_tail=False,
                         early_stopping=es)
    assert loop.world == world and loop.exchange == (world > 1) and loop.device_tail
    if mode == "early_stop":
        assert loop._es_device
    if world > 1:
        assert loop.local_ids == [v for v in range(5) if v % 2 == rank]
        # (with the criterion on the device a rank's block also carries its views' {S, N}: a flat buffer, sks_loop_shard_floats)
        assert tuple(loop._allg.shape) == ((6, 17, 11) if mode != "early_stop" else (2 * loop._shard_flat.numel(),))
    if mode == "dropout":
        # training.dropout (general_utils.py:267-283): ONE draw of dropped (camera, joint) planes per scene.  The ranks'
        # default generators are deliberately out of step here; rank 0's draw must be the scene's on every rank
        torch.manual_seed(1234 + 77 * rank)
        loop.new_scene(torch.tensor(sc.pose_3d_init, device=dev, dtype=torch.float32), poses_2d=torch.tensor(sc.poses_2d, device=dev),
                       dropout=True)
        with torch.no_grad():
            gm._opacity.fill_(2.0)
        if world == 1:   # the draw did drop planes, and some of them belong to views the second rank owns at world 2
            dropped = [int((pl.reshape(pl.shape[0], -1).abs().amax(1) == 0).sum()) for pl in loop.hset.planes]
            assert sum(dropped) > 0 and dropped[1] + dropped[3] > 0, dropped
    loop.run(600 if mode == "early_stop" else 30)
    torch.cuda.synchronize()
    if mode == "early_stop":
        # the criterion fired in the middle of the run, inside a group; every rank enqueued the same number of groups (each holds
        # a collective: a rank that had stopped a group earlier than its peer would leave that peer hanging in its last all_gather)
        assert loop.stopped_at == 8 and loop.iteration == 8, loop.stopped_at
        assert int(loop.counters[0]) == loop.stopped_at
    if rank == 0:
        ret.put([x.detach().cpu().numpy() for x in (gm._xyz, gm._scaling, gm._rotation, gm._opacity, loop.accumulated_grads)]
                + [np.array([loop.stopped_at or 0, loop.iteration])])
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["sparse", "dense", "mixed", "dropout", "early_stop"])
def test_two_ranks_on_one_gpu_equal_one_rank(device, mode):
    """The view-sharded device path at world size 2 -- uneven shards (3 + 2 views, one zero pad row), all_gather, the
    rank-major optimiser kernel, every rank stepping identically -- as two processes sharing this GPU over gloo (RCCL
    does not allow two ranks on one device; the collective's transport is not what is under test).  Bit-identical to
    one process.  "early_stop": the reference's criterion on the device fires mid-run; the ranks look at its flag only behind a
    stream synchronisation every ES_SYNC_GROUPS groups, so both stop after the same number of collectives (no hang) and at
    the iteration the single process stops at."""
    import os
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = 29700 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, mode, ret)) for r in range(2)]
    for p in procs:
        p.start()
    two = ret.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    one_p = ctx.Process(target=_two_rank_worker, args=(0, 1, port + 1, mode, ret))
    one_p.start()
    one = ret.get(timeout=300)
    one_p.join(timeout=120)
    assert one_p.exitcode == 0
    for k, (a, b) in enumerate(zip(two, one)):
        assert np.array_equal(a, b), k


# ------------------------------------------------- BASELINE config 4's scene on the device path: four ranks, one GPU (gloo)
# (four, not config 4's eight: with the parent, eight ranks would be nine processes holding the one GPU at once; config 4's own
# partition over eight ranks is checked on the host, test_cpu.py::test_config4_partition_on_eight_ranks_equals_one_rank_and_the_reference_loop)
GPU_RANKS = 4


def _config4_gpu_worker(rank, world, port, mode, ret):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)   # RCCL refuses several ranks on one device
    from skelsplat_amd.loop import MultiViewLoop, OptEarlyStopping
    from skelsplat_amd.heatmaps import generate_heatmaps
    from skelsplat_amd.scene import SyntheticScene, GaussianModel
    sc = SyntheticScene("panoptic", n_views=31, seed=5, W=192, H=112, device=dev)
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, 19, scaling=4.2, scene_type="panoptic", device=dev)
    gm.training_setup()
    hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(), torch.tensor(sc.poses_2d, device=dev),
                           sc.cameras)
    es = OptEarlyStopping(window_size=4, repeat_tolerance=1.0) if mode == "early_stop" else "no_stopping"
    loop = MultiViewLoop(gm, sc.cameras, hm, dataset="panoptic", accumulation_steps=31, sparse=mode != "dense", early_stopping=es)
    assert loop.world == world and loop.exchange == (world > 1) and loop.device_tail
    n_local = len(loop.local_ids)
    if world > 1:
        assert loop.vmax == 8 and n_local == (7 if rank == 3 else 8)      # 8,8,8,7
    loop.run(93)          # three groups -- or, with the criterion, its stop at iteration 8 and the groups enqueued behind it
    torch.cuda.synchronize()
    if mode == "early_stop":
        assert loop.stopped_at == 8 and loop.iteration == 8 and int(loop.counters[0]) == 8, loop.stopped_at
    if world > 1:
        mine = [n_local, float(gm._xyz.detach().abs().sum()), loop.iteration]
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        assert sorted(g[0] for g in gathered) == [7, 8, 8, 8]
        assert all(g[1] == gathered[0][1] and g[2] == gathered[0][2] for g in gathered)     # every rank holds the same parameters
    if rank == 0:
        ret.put([x.detach().cpu().numpy() for x in (gm._xyz, gm._scaling, gm._rotation, gm._opacity, loop.accumulated_grads)]
                + [np.array([loop.stopped_at or 0, loop.iteration])])
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["sparse", "dense", "early_stop"])
def test_config4_views_on_four_ranks_on_one_gpu_equal_one_rank(device, mode):
    """BASELINE config 4's 31 Panoptic-shaped views over FOUR ranks, shards 8,8,8,7 (as config 4's 4,4,4,4,4,4,4,3: full shards
    and one zero pad row in the last), all_gather, the rank-major optimiser kernel (`shard_world = 4`), with the early-stopping
    sums in the gathered block -- through the DEVICE path (HIP kernels, device tail), as four processes sharing this GPU over
    gloo.  Bit-identical to one process; with the criterion every rank stops after the same number of collectives at the
    iteration the single process stops at.  (What no test can give here is the timing of eight GPUs.)"""
    import os
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = 29900 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_config4_gpu_worker, args=(r, GPU_RANKS, port, mode, ret)) for r in range(GPU_RANKS)]
    for p in procs:
        p.start()
    sharded = ret.get(timeout=600)
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0
    one_p = ctx.Process(target=_config4_gpu_worker, args=(0, 1, port + 1, mode, ret))
    one_p.start()
    one = ret.get(timeout=300)
    one_p.join(timeout=120)
    assert one_p.exitcode == 0
    for k, (a, b) in enumerate(zip(sharded, one)):
        assert np.array_equal(a, b), k


def _adam_groups(dev, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = {"xyz": (17, 3), "f_dc": (17, 1, 17), "f_rest": (17, 0, 17), "opacity": (17, 1), "scaling": (17, 3), "rotation": (17, 4),
              "big": (1000, 33)}
    lrs = {"xyz": 1.6e-1, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 2.5e-2, "scaling": 5e-3, "rotation": 1e-3, "big": 1e-2}
    return [{"params": [torch.nn.Parameter((torch.randn(s, generator=g) * 3).to(dev))], "lr": lrs[n], "name": n} for n, s in shapes.items()]


@pytest.mark.gpu
def test_one_launch_adam_is_torch_adam(device):
    """skelsplat_amd.optim.Adam (sks_adam_multi: every group in one launch) against torch.optim.Adam as the reference builds it
    (gaussian_model.py:218: lr = 0, eps = 1e-15, six groups, the xyz group's lr rewritten every iteration): 60 steps, a group
    that never gets a gradient, one that gets its first gradient late (its own step count), an empty tensor."""
    from skelsplat_amd.optim import Adam
    ga, gb = _adam_groups(device, 3), _adam_groups(device, 3)
    oa, ob = torch.optim.Adam(ga, lr=0.0, eps=1e-15), Adam(gb, lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(5)
    for it in range(60):
        for o in (oa, ob):
            for grp in o.param_groups:
                if grp["name"] == "xyz":
                    grp["lr"] = 1.6e-1 * (0.99 ** it)
        gen_state = gen.get_state()
        for o in (oa, ob):
            gen.set_state(gen_state)
            for grp in o.param_groups:
                p = grp["params"][0]
                if grp["name"] == "f_dc" or (grp["name"] == "rotation" and it < 7):
                    p.grad = None
                    continue
                scale = 1e-4 if grp["name"] == "opacity" else 10.0
                p.grad = (torch.randn(p.shape, generator=gen) * scale).to(device)
            o.step()
            o.zero_grad(set_to_none=True)
    # (the step counts are read straight from optimizer.state, without a state_dict() in between: they live there, as torch keeps them)
    for a, b in zip(oa.param_groups, ob.param_groups):
        pa, pb = a["params"][0], b["params"][0]
        tol = 2e-6 * float(pa.abs().max()) if pa.numel() else 0.0
        assert torch.allclose(pa, pb, rtol=2e-5, atol=tol), a["name"]
        if pa in oa.state:
            assert int(oa.state[pa]["step"]) == int(ob.state[pb]["step"]) == (53 if a["name"] == "rotation" else 60)
            assert torch.allclose(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"], rtol=2e-5, atol=1e-12)
        else:
            assert pb not in ob.state and a["name"] == "f_dc"
    # the state goes through state_dict() into a plain torch.optim.Adam and back: both continue alike
    gc = _adam_groups(device, 3)
    for src, dst in zip(gb, gc):
        dst["params"][0].data.copy_(src["params"][0].data)
    oc = torch.optim.Adam(gc, lr=0.0, eps=1e-15)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))     # (load_state_dict keeps tensors that already have the right dtype and device: no aliasing)
    for o in (ob, oc):
        for grp in o.param_groups:
            p = grp["params"][0]
            p.grad = torch.full_like(p, 0.5)
        o.step()
    for b, c in zip(ob.param_groups, oc.param_groups):
        pb, pc = b["params"][0], c["params"][0]
        assert torch.allclose(pb, pc, rtol=2e-5, atol=2e-6 * float(pb.abs().max()) if pb.numel() else 0.0), b["name"]


@pytest.mark.gpu
def test_one_launch_adam_state_moves_with_the_reference_parameter_surgery(device):
    """scene/gaussian_model.py:341-404 (replace_tensor_to_optimizer, _prune_optimizer, cat_tensors_to_optimizer) move a parameter's
    state dict to a NEW nn.Parameter: the step count (and with it the bias correction) must go along -- it lives in state["step"],
    not in a cache keyed by the old parameter's identity."""
    from skelsplat_amd.optim import Adam
    pa, pb = torch.nn.Parameter(torch.ones(7, 3, device=device)), torch.nn.Parameter(torch.ones(7, 3, device=device))
    oa = torch.optim.Adam([{"params": [pa], "lr": 1e-2, "name": "xyz"}], lr=0.0, eps=1e-15)
    ob = Adam([{"params": [pb], "lr": 1e-2, "name": "xyz"}], lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(0)

    def steps(n):
        for _ in range(n):
            g = torch.randn(oa.param_groups[0]["params"][0].shape, generator=gen).to(device)
            for o in (oa, ob):
                o.param_groups[0]["params"][0].grad = g.clone()
                o.step()
    steps(5)
    assert int(ob.state[pb]["step"]) == 5          # visible without a state_dict() in between
    for o in (oa, ob):     # _prune_optimizer (gaussian_model.py:357-376): keep rows 0..4, re-seat the state under a new Parameter
        grp = o.param_groups[0]
        old = grp["params"][0]
        st = o.state.get(old)
        mask = torch.arange(7, device=device) < 5
        st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][mask], st["exp_avg_sq"][mask]
        del o.state[old]
        grp["params"][0] = torch.nn.Parameter(old[mask].detach().clone().requires_grad_(True))
        o.state[grp["params"][0]] = st
    steps(4)
    qa, qb = oa.param_groups[0]["params"][0], ob.param_groups[0]["params"][0]
    assert int(oa.state[qa]["step"]) == int(ob.state[qb]["step"]) == 9
    assert torch.allclose(qa, qb, rtol=2e-5, atol=2e-6)


@pytest.mark.gpu
def test_one_launch_adam_refuses_what_its_kernel_does_not_do(device):
    """No fall-back: options the kernel does not implement are refused at construction, CPU / non-fp32 tensors at step()."""
    from skelsplat_amd.optim import Adam
    for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(NotImplementedError):
            Adam([torch.nn.Parameter(torch.ones(3, device=device))], lr=1e-2, **kw)
    for p in (torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(3, device=device, dtype=torch.float64))):
        o = Adam([p], lr=1e-2)
        p.grad = torch.ones_like(p)
        with pytest.raises(RuntimeError, match="ROCm"):
            o.step()
        assert torch.equal(p.detach().cpu(), torch.ones(3, dtype=p.dtype)) and len(o.state[p]) == 0     # nothing was touched


@pytest.mark.gpu
def test_chained_eager_steps_start_from_the_tails_geometry(device, monkeypatch):
    """The fused step's tail leaves the geometry of the UPDATED parameters behind.  run() chains its own eager groups on it (one
    geometry launch for the whole run), step_group(parameters_untouched=True) does on the caller's word; a plain step_group()
    recomputes it -- a write through `.data` between two steps is invisible from inside.  Bit for bit the same trajectory."""
    from skelsplat_amd import loop as L
    from skelsplat_amd.heatmaps import generate_heatmaps
    sc, model = _make_loop_scene(device, seed=9)
    calls = {"n": 0}
    real = L.R.geometry_views

    def counted(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)
    monkeypatch.setattr(L.R, "geometry_views", counted)
    loops = []
    for k in range(4):
        gm = model(device)
        hm = generate_heatmaps(gm._xyz.detach(), gm.get_scaling.detach(), gm._rotation.detach(),
                               torch.tensor(sc.poses_2d, device=device), sc.cameras)
        loops.append(L.MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", sparse=True, use_graph=k == 3))
    a, b, c, d = loops
    assert a.fused_tail and not a.use_graph and d.use_graph
    for k in range(6):                          # one captured graph per group: the chained ones are a second graph, without geometry
        d.step_group(parameters_untouched=k > 0)
    assert len(d._graphs) == 2
    n0 = calls["n"]
    a.run(24)                                   # 6 groups, chained
    assert calls["n"] - n0 == 1
    n0 = calls["n"]
    for _ in range(6):
        b.step_group()                          # on its own: geometry from the parameters every time
    assert calls["n"] - n0 == 6
    n0 = calls["n"]
    for k in range(6):
        c.step_group(parameters_untouched=k > 0)
    assert calls["n"] - n0 == 1
    for pa, pb, pc, pd in zip(*[(l.gm._xyz, l.gm._scaling, l.gm._rotation, l.gm._opacity) for l in loops]):
        assert torch.equal(pa, pb) and torch.equal(pa, pc) and torch.equal(pa, pd)
    # a write between steps: the plain call sees it, because it looks at nothing but the parameters
    with torch.no_grad():
        a.gm._xyz.data.add_(3.0), b.gm._xyz.data.add_(3.0)
    a.step_group(), b.step_group()
    assert torch.equal(a.gm._xyz, b.gm._xyz)
