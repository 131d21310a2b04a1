"""Generates tests/golden/reference_keypoint.npz by running the REFERENCE's own `softargmax2d` and its four keypoint
criteria (utils/loss_utils.py:41-64, 76-83, 131-150, 215-223; imported from /root/reference in the build container) in fp32 on
the CPU, values and autograd gradients with respect to the image, over the cases of tests/keypoint_cases.py.
Run:  python tests/golden/make_golden_keypoint.py

The images are rebuilt from seeds by tests/keypoint_cases.py (they are too large to commit); per case `<name>_<regime>` the
file holds
  checksum        float64 sums of the image the outputs were made from
  gt_2d           (V, J, 2) float32 detections: the float64 keypoints minus keypoint_cases.RESIDUALS
  xy              the reference's softargmax2d, (V, C, 2) float32
  idx             flat indices into the image at which gradients are recorded (keypoint_cases.sample_index)
  g_xy            d sum(xy * cotangent) / d image at idx
  <crit>_<red>    the reference's return value for reduction = mean / sum / none
  g_<crit>        d <crit>_mean / d image at idx   (the 'sum' gradient is the 'mean' one times the element count, or equal to it
                  for l2_sqrt, and is not recorded)
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def main():
    for n in ("tensordict", "cupy", "cupyx", "cupyx.scipy", "cupyx.scipy.ndimage", "plyfile", "cv2"):
        _stub(n)
    sys.modules["tensordict"].TensorDict = dict
    sys.modules["cupyx.scipy.ndimage"].gaussian_filter = None
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = None
    sys.path.insert(0, REF)
    from utils import loss_utils
    sys.path.append(ROOT)
    from tests import keypoint_cases as kc
    from tests import keypoint_ref as kr

    crits = {"l2": loss_utils.l2_loss, "l2_sqrt": loss_utils.l2_loss_sqrt, "huber": loss_utils.huber_loss,
             "cauchy": loss_utils.cauchy_loss}
    out = {}
    for name, regime in kc.CASES:
        key = f"{name}_{regime}"
        img = kc.make_image(name, regime)
        gt_2d = kc.detections(kr.softargmax2d(torch.from_numpy(img)).numpy())
        idx = kc.sample_index(img)
        out[key + "_checksum"], out[key + "_gt_2d"], out[key + "_idx"] = kc.checksum(img), gt_2d, idx

        def grad_of(fn):
            x = torch.from_numpy(img).clone().requires_grad_(True)
            val = fn(x)
            val.backward()
            return val.detach().numpy(), x.grad.numpy().ravel()[idx]

        cot = torch.from_numpy(kc.cotangent(img.shape[:2])).float()
        xy = loss_utils.softargmax2d(torch.from_numpy(img))
        assert xy.dtype == torch.float32
        out[key + "_xy"] = xy.numpy()
        _, out[key + "_g_xy"] = grad_of(lambda x: (loss_utils.softargmax2d(x) * cot).sum())
        g2 = torch.from_numpy(gt_2d)
        for cname, fn in crits.items():
            for red in ("mean", "sum", "none"):
                with torch.no_grad():
                    out[f"{key}_{cname}_{red}"] = fn(torch.from_numpy(img), None, g2, reduction=red).numpy()
            val, out[f"{key}_g_{cname}"] = grad_of(lambda x: fn(x, None, g2, reduction="mean"))
            assert np.array_equal(val, out[f"{key}_{cname}_mean"])
    path = os.path.join(HERE, "reference_keypoint.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
