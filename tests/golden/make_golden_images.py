"""Generates tests/golden/reference_images.npz: the REFERENCE's own debug pictures (train.py:279-304, `debug.save_images`).

Run in the build container:  python tests/golden/make_golden_images.py

`train.training()` runs exactly as tests/golden/make_golden_loop.py runs it for `h36m_small` (4 views, 64 x 48, the synthetic
scene, the stand-ins of tests/golden/_ref_env.py) -- with `debug.save_images=True`, a handful of iterations and a temporary
output directory.  The reference then writes heatmaps/heatmap_{i}.png (train.py:113-114), images/render_1_{i}.png after
iteration 1's render (:143-144) and images/render_{i}.png at the end (:236-237).  Recorded: the decoded files, the (C,H,W)
tensor each picture was made from (the heat-maps generate_heatmaps returned; the image save_images' own render call returned),
the scene's inputs, and the Gaussians' raw parameters at the two save_images calls.

The reference's `save_heatmaps` is also called directly on a few hand-made tensors (`hand_*`): C = 15 / 17 / 19, odd sizes, a
0 .. 255 integer ramp (the input most sensitive to the truncation), negative values.  Flat and NaN inputs stay out: the reference
is undefined there (a NaN cast to uint8).

PIL decodes the files here and nowhere else."""
import logging
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_env as env   # noqa: E402

SPEC = dict(cfg="h36m", dataset="h36m", V=4, W=64, H=48, iters=8, fx=1145.0 * 0.064 * 1.5, ring=2500.0)


def hand_made():
    """name -> (C,H,W) float32."""
    rng = np.random.default_rng(5)
    ramp = np.arange(256, dtype=np.int64).reshape(16, 16)
    out = {
        # sums to the integers 0 .. 255 exactly: (s / 255) * 255 is s again only if the divide is correctly rounded -- one ulp
        # less and the truncation gives s - 1
        "ramp17": np.stack([(ramp + c) // 17 for c in range(17)]).astype(np.float32),
        "blobs15": np.maximum(rng.normal(0.0, 1.0, (15, 9, 13)), 0.0).astype(np.float32) ** 2,
        "dense19": rng.uniform(0.0, 1.0, (19, 7, 5)).astype(np.float32),
        "negative17": rng.normal(-3.0, 2.0, (17, 11, 18)).astype(np.float32),
        "single1": rng.uniform(-1.0, 4.0, (1, 3, 5)).astype(np.float32),
    }
    assert (out["ramp17"].sum(axis=0) == ramp).all()
    return out


def decode(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "L", im.mode
    return np.asarray(im).copy()


def run(out):
    import train as ref_train                      # /root/reference/train.py
    from scene.dataset_readers import CameraInfo, getNerfppNorm
    from utils.camera_utils import cameraList_from_camInfos
    from utils.graphics_utils import BasicPointCloud, focal2fov
    from skelsplat_amd.scene import SyntheticScene     # inputs only (stored in the fixture)
    assert ref_train.__file__.startswith(env.REF)
    spec = SPEC
    cfg = env.load_config(spec["cfg"], **{"debug.save_images": True, "debug.save_iterations": [],
                                          "optimization.iterations": spec["iters"]})
    sc = SyntheticScene(spec["dataset"], n_views=spec["V"], seed=0, W=spec["W"], H=spec["H"], ring=spec["ring"], fx=spec["fx"])
    cams = sc.cameras
    infos = [CameraInfo(uid=i, R=c.R, T=c.T, FovY=focal2fov(c.K[1, 1], c.image_height), FovX=focal2fov(c.K[0, 0], c.image_width),
                        K=c.K, depth_params=None, image_path="", image_name="", depth_path="", width=c.image_width,
                        height=c.image_height, heatmap=None) for i, c in enumerate(cams)]
    n_joints = sc.n_joints
    rec = dict(saving=None, renders={}, params={})

    class Scene:
        """scene/__init__.py:25-99 without the ply / json files (as in make_golden_loop.py)."""

        def __init__(self, dataset, model, gaussians, initial_guess_3d, cameras, scene_name, output_dir):
            self.gaussians, self.scene_name = gaussians, scene_name
            self.scene_type = dataset.data_root.split("/")[-1]
            self.cameras_extent = getNerfppNorm(cameras)["radius"]
            self.train_cameras = {1.0: cameraList_from_camInfos(cameras, 1.0, model, False)}
            pcd = BasicPointCloud(points=np.asarray(initial_guess_3d, np.float32).reshape(-1, 3), colors=None, normals=None)
            gaussians.create_from_pcd(pcd, cameras, self.cameras_extent, model.opacity_on, model.scaling, n_joints,
                                      model.scaling_modifier, self.scene_type)
            rec["spatial_lr_scale"] = float(self.cameras_extent)
            rec["gm"] = gaussians

        def getTrainCameras(self, scale=1.0):
            return self.train_cameras[scale]

        def save_h36m(self, iteration, scene_name):
            pass

    real_heat = ref_train.generate_heatmaps

    def heat(*a, **k):
        hm = real_heat(*a, **k)
        rec["heatmaps"] = hm
        return hm

    real_render = dict(ref_train.render_functions)

    def make_render(fn):
        def render(cam, *a, **k):
            pkg = fn(cam, *a, **k)
            if rec["saving"] is not None:       # a call of save_images' own
                rec["renders"].setdefault(rec["saving"], []).append(pkg["render"].detach().clone().numpy())
            return pkg
        return render

    real_save = ref_train.save_images

    def save_images(train_cameras, gaussians, pipe, model, output_dir, name="image"):
        rec["saving"] = name
        rec["params"][name] = [p.detach().clone().numpy() for p in (gaussians._xyz, gaussians._scaling, gaussians._rotation,
                                                                    gaussians._opacity)]
        rec["features"] = gaussians.get_features.detach().clone().numpy()
        try:
            return real_save(train_cameras, gaussians, pipe, model, output_dir, name=name)
        finally:
            rec["saving"] = None

    p2d = torch.tensor(sc.poses_2d, dtype=torch.float32)
    loader = [(0, (sc.pose_3d_init, sc.pose_3d_gt, p2d, infos, "S1_Directions_0"))]
    ref_train.Scene = Scene
    ref_train.generate_heatmaps = heat
    ref_train.save_images = save_images
    for k, fn in real_render.items():
        ref_train.render_functions[k] = make_render(fn)
    V = spec["V"]
    try:
        with env.no_gpu(), tempfile.TemporaryDirectory() as tmp:
            ref_train.training(cfg.dataset, cfg.model, cfg.optimization, cfg.pipeline, cfg.debug, cfg.training, loader, tmp,
                               logging.getLogger("ref"))
            png = {name: np.stack([decode(os.path.join(tmp, sub, f"{name}_{i}.png")) for i in range(V)])
                   for sub, name in (("heatmaps", "heatmap"), ("images", "render_1"), ("images", "render"))}
            hand = hand_made()
            for name, planes in hand.items():
                ref_train.save_heatmaps(1, {"0": torch.tensor(planes)}, os.path.join(tmp, "hand"), name=name)
                out[f"hand_{name}_planes"] = planes
                out[f"hand_{name}_png"] = decode(os.path.join(tmp, "hand", "heatmaps", f"{name}_0.png"))
    finally:
        ref_train.render_functions.update(real_render)
        ref_train.generate_heatmaps = real_heat
        ref_train.save_images = real_save
    hm = rec["heatmaps"]
    assert sorted(rec["renders"]) == ["render", "render_1"] and all(len(v) == V for v in rec["renders"].values())
    o = cfg.optimization
    out.update({
        "hand_names": np.array(sorted(hand)),
        "dataset": np.array(spec["dataset"]), "iterations": np.int64(spec["iters"]),
        "antialiasing": np.bool_(bool(cfg.pipeline.antialiasing)),
        "accumulation_steps": np.int64(cfg.training.accumulation_steps),
        "lambda_consistency": np.float64(cfg.training.lambda_consistency),
        "pose_3d_init": np.asarray(sc.pose_3d_init), "pose_3d_gt": np.asarray(sc.pose_3d_gt), "poses_2d": np.asarray(sc.poses_2d),
        "cam_R": np.stack([c.R for c in cams]), "cam_T": np.stack([c.T for c in cams]), "cam_K": np.stack([c.K for c in cams]),
        "cam_WH": np.array([[c.image_width, c.image_height] for c in cams]),
        "spatial_lr_scale": np.float64(rec["spatial_lr_scale"]),
        "model": np.array([cfg.model.scaling, cfg.model.scaling_modifier, float(cfg.model.opacity_on)]),
        "opt": np.array([o.position_lr_init, o.position_lr_final, o.position_lr_delay_mult, o.position_lr_max_steps,
                         o.feature_lr, o.opacity_lr, o.scaling_lr, o.rotation_lr]),
        "features": rec["features"].reshape(rec["features"].shape[0], -1).astype(np.float32),
        "heatmap_planes": np.stack([hm[str(v)].numpy() for v in range(V)]).astype(np.float32),
        "heatmap_png": png["heatmap"],
    })
    for name in ("render_1", "render"):
        out[name + "_planes"] = np.stack(rec["renders"][name]).astype(np.float32)
        out[name + "_png"] = png[name]
        for key, a in zip(("xyz", "scaling", "rotation", "opacity"), rec["params"][name]):
            out[f"{name}_{key}"] = a.astype(np.float32)
    assert not (out["render_1_xyz"] == out["render_xyz"]).all()      # the optimiser stepped between the two pictures
    for k in ("heatmap", "render_1", "render"):
        assert out[k + "_png"].shape == (V, spec["H"], spec["W"]) and out[k + "_png"].dtype == np.uint8
        assert out[k + "_planes"].shape[0] == V and out[k + "_planes"].shape[2:] == (spec["H"], spec["W"])
        print(k, "planes", out[k + "_planes"].shape, "max byte per view", out[k + "_png"].reshape(V, -1).max(axis=1))


def main():
    env.install([])
    out = {}
    run(out)
    path = os.path.join(HERE, "reference_images.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
