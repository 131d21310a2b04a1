"""Frame batches whose frames are seen by different camera rigs (rigs.RigBank, sks_rig_select, the *_dv entry points through
FrameBatchLoop / FramePipeline): every frame ends bit for bit where a FrameBatchLoop(frames=1, cameras=its rig) running it
alone ends, whatever the other frames' rigs, through eager launches and captured graphs alike."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 4
ITERS = 60
GPG = 5             # groups per graph: run() takes one eager group, two replays of the 5-group graph, then single-group graphs
TOL = 1e-3


class Setup:
    """n rigs of 4 views (ring radius grows with the rig, so cameras_extent differs by far more than a rounding step), each
    with a pose of its own; H36M rigs mix 1000- and 1002-wide sensors (dataset_readers.py:68-80), Occlusion-Person is 1280x720."""

    def __init__(self, dev, dataset, n_rigs):
        from skelsplat_amd.scene import SyntheticScene, Camera, cameras_extent
        from skelsplat_amd.rigs import RigBank
        self.dev, self.dataset = dev, dataset
        self.scenes = [SyntheticScene(dataset, n_views=V, seed=30 + r, ring=4000.0 + 600.0 * r, device=dev) for r in range(n_rigs)]
        self.rigs = []
        for sc in self.scenes:
            cams = sc.cameras
            if dataset == "h36m":
                cams = [c if j % 2 == 0 else Camera(c.uid, c.R, c.T, c.K, c.image_width + 2, c.image_height, device=dev)
                        for j, c in enumerate(cams)]
            self.rigs.append(cams)
        self.J = self.scenes[0].n_joints
        self.extent = [cameras_extent(r) for r in self.rigs]
        self.bank = RigBank(self.rigs, dev)

    def model(self, r=0):
        """the template of one frame, with rig r's spatial scale (what a one-rig loop's schedule is made from)"""
        from skelsplat_amd.scene import GaussianModel
        gm = GaussianModel().create_from_points(self.scenes[r].pose_3d_init, self.extent[r], self.J, device=self.dev)
        gm.training_setup()
        return gm

    def frames(self, ids, seed=5):
        rng = np.random.default_rng(seed)
        pts = np.stack([self.scenes[r].pose_3d_init + rng.normal(0, 10.0 + 5.0 * f, (self.J, 3)) for f, r in enumerate(ids)])
        p2d = np.stack([self.scenes[r].poses_2d + rng.normal(0, 1.0 + 0.5 * f, (V, self.J, 2)) for f, r in enumerate(ids)])
        return pts.astype(np.float32), p2d.astype(np.float32)


def _es(on):
    from skelsplat_amd.loop import OptEarlyStopping
    return OptEarlyStopping(window_size=4, repeat_tolerance=TOL) if on else "no_stopping"


def _state(fb, f):
    return [fb.xyz[f], fb.scaling[f], fb.rotation[f], fb.opacity[f], fb.counters[f]]


def _alone(s, r, pt, p2d_f, es, factored, iters=ITERS, loops=None):
    """the frame alone on rig r: FrameBatchLoop(frames=1, cameras=that rig), eager"""
    from skelsplat_amd.loop import FrameBatchLoop
    key = (r, es, factored)
    if loops is None or key not in loops:
        one = FrameBatchLoop(s.model(r), s.rigs[r], 1, dataset=s.dataset, factored=factored, early_stopping=_es(es))
        if loops is not None:
            loops[key] = one
    else:
        one = loops[key]
    one.new_scenes(pt[None], poses_2d=p2d_f[None])
    one.run(iters)
    torch.cuda.synchronize()
    return [t.clone() for t in _state(one, 0)], one.stopped_at[0]


def _assert_frames(s, fb, ids, pts, p2d, es, factored, iters=ITERS, n=None):
    torch.cuda.synchronize()
    fb.check_rigs()
    loops = {}
    for f, r in enumerate(ids[:n]):
        want, stop = _alone(s, r, pts[f], p2d[f], es, factored, iters, loops)
        print(f"frame {f} rig {r}: stopped_at {fb.stopped_at[f]} (alone: {stop}), iteration {int(fb.counters[f, 0])}")
        for k, (a, b) in enumerate(zip(_state(fb, f), want)):
            assert torch.equal(a, b), (f, r, "xyz scaling rotation opacity counters".split()[k])
        assert fb.stopped_at[f] == stop, (f, fb.stopped_at[f], stop)


def test_selection_fills_the_batch_buffers(device):
    """sks_rig_select against the host restatement and against the objects a one-rig loop builds; device ids and host ids."""
    from skelsplat_amd.loop import FrameBatchLoop
    from skelsplat_amd.rasterizer import ViewBatch
    from skelsplat_amd.triangulation import device_projection_matrices
    s = Setup(device, "h36m", 3)
    for r, rig in enumerate(s.rigs):
        vb = ViewBatch.from_cameras(rig, allow_mixed=True)
        assert torch.equal(s.bank.viewmatrix_dev[r], vb.viewmatrix) and torch.equal(s.bank.projmatrix_dev[r], vb.projmatrix)
        assert s.bank.tan[r, :, 0].tolist() == list(vb.tanfovx) and s.bank.tan[r, :, 1].tolist() == list(vb.tanfovy)
        assert torch.equal(s.bank.proj_dev[r], device_projection_matrices(rig, device))
    F = 5
    fb = FrameBatchLoop(s.model(), rigs=s.bank, frames=F, dataset="h36m")
    for ids in ([2, 0, 1, 1, 2], torch.tensor([1, 1, 0, 2, 0], device=device)):
        fb._sel.select(ids)
        torch.cuda.synchronize()
        want = s.bank.select_host(ids.cpu() if torch.is_tensor(ids) else ids)
        assert torch.equal(fb.views_all.viewmatrix.cpu(), want["viewmatrix"])
        assert torch.equal(fb.views_all.projmatrix.cpu(), want["projmatrix"])
        tab = fb._sel.table.cpu()
        assert torch.equal(tab[0, :F * V].view(torch.float32), want["tanfovx"]) and torch.equal(tab[1, :F * V].view(torch.float32), want["tanfovy"])
        assert torch.equal(tab[2:, :F * V].t().contiguous(), want["wh"]) and int(tab[:, F * V:].abs().sum()) == 0
        assert torch.equal(fb._sel.proj.cpu(), want["proj"]) and torch.equal(fb._sel.sched.cpu(), want["sched_log"])
        fb.check_rigs()


@pytest.mark.parametrize("factored", [True, False], ids=["factors", "planes"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("es", [False, True], ids=["no_stopping", "opt_early_stopping"])
@pytest.mark.parametrize("dataset", ["h36m", "occlusion-person"])
def test_frames_of_different_rigs_end_like_their_own_loops(device, dataset, es, use_graph, factored):
    """F frames, F different rigs: each frame equals FrameBatchLoop(frames=1, cameras=its rig) running it alone."""
    from skelsplat_amd.loop import FrameBatchLoop
    F = 4
    s = Setup(device, dataset, F)
    for a in range(F):          # the per-frame schedule is exercised: the xyz learning rates differ well beyond rounding
        for b in range(a + 1, F):
            assert abs(s.extent[a] - s.extent[b]) > 1e-3 * s.extent[a]
    assert len({float(x) for x in s.bank.sched_log[:, 0]}) == F
    if dataset == "h36m":
        assert s.bank.sizes == [(1000, 1000), (1002, 1000)] * 2
    else:
        assert s.bank.sizes == [(1280, 720)] * V
    ids = [2, 0, 3, 1]
    pts, p2d = s.frames(ids)
    fb = FrameBatchLoop(s.model(), rigs=s.bank, frames=F, dataset=dataset, use_graph=use_graph, factored=factored,
                        early_stopping=_es(es))
    fb.new_scenes(pts, poses_2d=p2d, rig_ids=ids)
    fb.run(ITERS, groups_per_graph=GPG)
    _assert_frames(s, fb, ids, pts, p2d, es, factored)


@pytest.mark.parametrize("es", [False, True], ids=["no_stopping", "opt_early_stopping"])
def test_equal_ids_reproduce_the_cameras_loop(device, es):
    from skelsplat_amd.loop import FrameBatchLoop
    F, r = 4, 1
    s = Setup(device, "h36m", 3)
    pts, p2d = s.frames([r] * F)
    kw = dict(dataset="h36m", use_graph=True, early_stopping=_es(es))
    fb = FrameBatchLoop(s.model(), rigs=s.bank, frames=F, **kw)
    fb.new_scenes(pts, poses_2d=p2d, rig_ids=[r] * F)
    fb.run(ITERS, groups_per_graph=GPG)
    ref = FrameBatchLoop(s.model(r), s.rigs[r], F, **kw)
    ref.new_scenes(pts, poses_2d=p2d)
    ref.run(ITERS, groups_per_graph=GPG)
    torch.cuda.synchronize()
    for name in ("xyz", "scaling", "rotation", "opacity", "counters", "exp_avg", "exp_avg_sq", "accumulated_grads", "_sums"):
        assert torch.equal(getattr(fb, name), getattr(ref, name)), name
    assert fb.stopped_at == ref.stopped_at


def test_two_batches_of_different_rigs_through_one_captured_graph(device):
    from skelsplat_amd.loop import FrameBatchLoop
    F = 4
    s = Setup(device, "h36m", 4)
    fb = FrameBatchLoop(s.model(), rigs=s.bank, frames=F, dataset="h36m", use_graph=True)
    ids1, ids2 = [0, 1, 2, 3], torch.tensor([3, 3, 0, 2], device=device)
    pts, p2d = s.frames(ids1, seed=6)
    fb.new_scenes(pts, poses_2d=p2d, rig_ids=ids1)
    fb.run(ITERS, groups_per_graph=GPG)
    multi, single = fb._multi[1], fb._graph[1]
    _assert_frames(s, fb, ids1, pts, p2d, False, True)
    pts, p2d = s.frames(ids2.tolist(), seed=7)
    fb.new_scenes(pts, poses_2d=p2d, rig_ids=ids2)
    fb.run(ITERS, groups_per_graph=GPG)
    assert fb._multi[1] is multi and fb._graph[1] is single       # replayed as they were: nothing was captured again
    _assert_frames(s, fb, ids2.tolist(), pts, p2d, False, True)


def test_initial_joints_are_triangulated_with_each_frames_own_matrices(device):
    from skelsplat_amd.loop import FrameBatchLoop
    from skelsplat_amd.triangulation import triangulate_sequence
    F = 4
    s = Setup(device, "occlusion-person", 3)
    ids = [2, 0, 1, 2]
    _, p2d = s.frames(ids)
    p2d = torch.tensor(p2d, device=device)
    fb = FrameBatchLoop(s.model(), rigs=s.bank, frames=F, dataset="occlusion-person")
    fb.new_scenes(None, poses_2d=p2d, rig_ids=ids)
    torch.cuda.synchronize()
    for f, r in enumerate(ids):
        want = triangulate_sequence(s.bank.proj_dev[r], p2d[f])
        assert torch.equal(fb.xyz[f], want), f
        assert torch.isfinite(want).all() and float((want.cpu() - torch.tensor(s.scenes[r].pose_3d_gt)).norm(dim=1).max()) < 100.0
    with pytest.raises(ValueError, match="factored=False"):
        fb.new_scenes(None, heatmaps=[[None] * V] * F, rig_ids=ids)
    planes = FrameBatchLoop(s.model(), rigs=s.bank, frames=F, dataset="occlusion-person", factored=False)
    with pytest.raises(ValueError, match="ready heatmaps do not carry the detections"):
        planes.new_scenes(None, heatmaps=[[None] * V] * F, rig_ids=ids)


@pytest.mark.parametrize("es", [False, True], ids=["no_stopping", "opt_early_stopping"])
def test_pipeline_sequence_with_interleaved_rigs(device, es):
    """N = 40 frames, 3 rigs interleaved, 2 streams of 16 frames (the last batch is short: its filler repeats the last frame
    and its rig): every frame equals its single-frame run."""
    from skelsplat_amd.loop import FramePipeline
    N, iters = 40, 40
    s = Setup(device, "h36m", 3)
    ids = [(f * 2 + f // 5) % 3 for f in range(N)]
    assert len(set(ids[32:])) > 1 and len(set(ids)) == 3
    pts, p2d = s.frames(ids)
    pipe = FramePipeline(s.model(), rigs=s.bank, frames=16, streams=2, dataset="h36m", early_stopping=_es(es))
    out = pipe.optimize_sequence(pts, p2d, iterations=iters, groups_per_graph=GPG, interleave=20, rig_ids=np.asarray(ids))
    torch.cuda.synchronize()
    pipe.check_rigs()
    out2 = pipe.optimize_sequence(pts, p2d, iterations=iters, groups_per_graph=GPG, interleave=20,
                                  rig_ids=torch.tensor(ids, device=device))
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    loops = {}
    for f, r in enumerate(ids):
        want, stop = _alone(s, r, pts[f], p2d[f], es, True, iters, loops)
        assert torch.equal(out[f], want[0]), (f, r)
        if es:
            assert int(pipe.stopped_at[f]) == (stop or 0), (f, int(pipe.stopped_at[f]), stop)


def test_refusals_and_an_id_outside_the_bank_on_the_device(device):
    from skelsplat_amd.loop import FrameBatchLoop, FramePipeline
    F = 4
    s = Setup(device, "occlusion-person", 3)
    pts, p2d = s.frames([0, 1, 2, 0])
    plain = FrameBatchLoop(s.model(), s.rigs[0], F, dataset="occlusion-person")
    with pytest.raises(ValueError, match="rig_ids needs a rig bank"):
        plain.new_scenes(pts, poses_2d=p2d, rig_ids=[0, 1, 2, 0])
    with pytest.raises(ValueError, match="rig_ids needs a rig bank"):
        plain.optimize_sequence(pts, p2d, iterations=4, rig_ids=[0, 1, 2, 0])
    with pytest.raises(ValueError, match="rig_ids needs a rig bank"):
        FramePipeline(s.model(), s.rigs[0], frames=2, streams=2, dataset="occlusion-person").optimize_sequence(
            pts, p2d, iterations=4, rig_ids=[0, 1, 2, 0])
    with pytest.raises(ValueError, match="either cameras="):
        FrameBatchLoop(s.model(), s.rigs[0], F, rigs=s.bank)
    fb = FrameBatchLoop(s.model(), rigs=s.bank, frames=F, dataset="occlusion-person")
    with pytest.raises(ValueError, match="outside the bank"):
        fb.new_scenes(pts, poses_2d=p2d, rig_ids=[0, 1, 3, 0])
    with pytest.raises(ValueError, match=r"must be \(4,\)"):
        fb.new_scenes(pts, poses_2d=p2d, rig_ids=[0, 1])
    # ids on the device are checked by the kernel: frame 2 names rig 7 of 3 -- nothing is written for it (it keeps rig 1, which
    # the batch before gave its slot), the other frames get their rigs, and the error is reported
    fb.new_scenes(pts, poses_2d=p2d, rig_ids=[0, 0, 1, 0])
    ids = [2, 1, 7, 0]
    pts, p2d = s.frames([2, 1, 1, 0])
    fb.new_scenes(pts, poses_2d=p2d, rig_ids=torch.tensor(ids, device=device))
    fb.run(ITERS)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="frame 2 of a batch named a rig outside the bank"):
        fb.check_rigs()
    fb.check_rigs()         # (reported once)
    _assert_frames(s, fb, [2, 1, 1, 0], pts, p2d, False, True)
