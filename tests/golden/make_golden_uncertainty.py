"""Generates tests/golden/reference_uncertainty.npz by running the REFERENCE's own code on seeded inputs: the covariance its
model reports for a set of Gaussians (scene/gaussian_model.py GaussianModel.get_covariance -> utils/general_utils.py
build_scaling_rotation / strip_symmetric, then unpack_covariance, :144-165), through the unmodified tests/golden/_ref_env.py,
and what utils/analize_error_confidence_correlation.py's `percent_inside_sigmas` and `percent_inside_sigmas_per_joint` make of
those covariances (the script is loaded by path; matplotlib's Agg backend, its `__main__` guard keeps the plots from running).
Run:  python tests/golden/make_golden_uncertainty.py

The file holds arrays and short names only:
  xyz (N,P,3), scaling_raw (N,P,3), rotation_raw (N,P,4), gt (N,P,3) float32     the seeded inputs, N = 37 frames of P = 17
      joints (629 Gaussians): standard deviations of 5-80 mm with ratios up to 4 inside a joint, un-normalised quaternions, and
      the ground truth at a Mahalanobis distance drawn uniformly from [0.05, 4] in a random direction
  modifiers (2,) float32                             1.0 and 1.3
  cov_m<i> (N,P,3,3) float32                         unpack_covariance(get_covariance(modifiers[i])): float32, as the reference
                                                     computes it
  ks (3,) int64                                      1, 2, 3
  overall_m<i> (3,), per_joint_m<i> (P,3) float64    the two functions' fractions, from the float32 covariances widened to
                                                     float64 (what the script's JSON round trip hands them)
  joint_names (P,)                                   the script's own names (:193)"""
import importlib.util
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_env                                                         # noqa: E402

OUT = os.path.join(HERE, "reference_uncertainty.npz")
N, P = 37, 17
MODIFIERS = (1.0, 1.3)
KS = (1, 2, 3)
JOINTS = ['root', 'lhip', 'lknee', 'lfoot', 'rhip', 'rknee', 'rfoot', 'spine', 'thorax', 'neck', 'head', 'rshoulder', 'relbow',
          'rhand', 'lshoulder', 'lelbow', 'lhand']


def inputs(seed=20261024):
    """(the seed: one whose sample keeps every joint's d2 more than 1 500 units of 2^-24 sum_k (|delta|_1 / sigma_k)^2 from the
    thresholds 1, 4, 9 under both modifiers -- tests/test_uncertainty_cpu.py asserts the distance on the stored arrays)"""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0.0, 600.0, (N, P, 3)).astype(np.float32)
    base = rng.uniform(np.log(5.0), np.log(20.0), (N, P, 1))
    scaling_raw = (base + rng.uniform(0.0, np.log(4.0), (N, P, 3))).astype(np.float32)
    q = rng.normal(0.0, 1.0, (N, P, 4))
    rotation_raw = (q / np.linalg.norm(q, axis=-1, keepdims=True) * rng.uniform(0.3, 3.0, (N, P, 1))).astype(np.float32)
    # the ground truth: xyz + R S (m u), |u| = 1, m uniform in [0.05, 4] -- in float64 from the float32 parameters, modifier 1
    s = np.exp(scaling_raw.astype(np.float64))
    qn = rotation_raw.astype(np.float64)
    qn /= np.linalg.norm(qn, axis=-1, keepdims=True)
    r, x, y, z = (qn[..., i] for i in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(N, P, 3, 3)
    u = rng.normal(0.0, 1.0, (N, P, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    m = rng.uniform(0.05, 4.0, (N, P, 1))
    gt = (xyz.astype(np.float64) + np.einsum("npab,npb->npa", R, s * u * m)).astype(np.float32)
    return xyz, scaling_raw, rotation_raw, gt


def main():
    _ref_env.install([])
    spec = importlib.util.spec_from_file_location("ref_analize_error_confidence",
                                                  os.path.join(_ref_env.REF, "utils", "analize_error_confidence_correlation.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    xyz, scaling_raw, rotation_raw, gt = inputs()
    out = dict(xyz=xyz, scaling_raw=scaling_raw, rotation_raw=rotation_raw, gt=gt, modifiers=np.array(MODIFIERS, np.float32),
               ks=np.array(KS, np.int64), joint_names=np.array(JOINTS))
    with _ref_env.no_gpu():
        from scene.gaussian_model import GaussianModel
        from utils.general_utils import unpack_covariance
        gm = GaussianModel(1)
        gm._scaling = torch.from_numpy(scaling_raw.reshape(-1, 3))
        gm._rotation = torch.from_numpy(rotation_raw.reshape(-1, 4))
        for i, mod in enumerate(MODIFIERS):
            cov = unpack_covariance(gm.get_covariance(float(np.float32(mod)))).numpy()
            assert cov.dtype == np.float32 and cov.shape == (N * P, 3, 3) and np.isfinite(cov).all()
            cov64 = cov.astype(np.float64)
            overall = script.percent_inside_sigmas(xyz.reshape(-1, 3).astype(np.float64), cov64,
                                                   gt.reshape(-1, 3).astype(np.float64), ks=KS)
            per_joint = script.percent_inside_sigmas_per_joint(xyz.astype(np.float64), cov64.reshape(N, P, 3, 3),
                                                               gt.astype(np.float64), JOINTS, ks=KS)
            out[f"cov_m{i}"] = cov.reshape(N, P, 3, 3)
            out[f"overall_m{i}"] = np.array([overall[k] for k in KS], np.float64)
            out[f"per_joint_m{i}"] = np.array([[per_joint[j][k] for k in KS] for j in JOINTS], np.float64)
            print("modifier", mod, "overall", out[f"overall_m{i}"])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
