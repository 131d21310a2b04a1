"""Generates tests/golden/reference_fuse.npz by running the REFERENCE's own `compute_reprojection_error` and
`compute_weighted_average_pose` (dataset_tools/h36m/compute_initial_guess.py:23-116, everything float64, and
dataset_tools/panoptic/compute_initial_guess_panoptic.py:23-117, whose line 67 rounds u - x to float32; both loaded by path from
/root/reference in the build container -- their `__main__` guards keep the dataset code from running) on seeded synthetic inputs.
Run:  python tests/golden/make_golden_fuse.py

Per case `<name>` = v<V>j<J>n<N> the file holds, in THIS project's layout (frames first):
  proj      (V,3,4) float64 K [R|t]: cameras on a ring looking at the subject, focal lengths 1 000-1 500 px, images up to 2 048 px
  p3d       (N,V,J,3) per-view candidates, millimetres, |X| <= 1e4: truth + per-view noise of 20-60 mm
  p2d       (N,V,J,2) detections: projected truth + noise, redrawn until EVERY |u_ic - x_c| >= MIN_ERR px (asserted below on the
            stored values: it bounds the cancellation in u - x, and with it the tests' tolerance, on every case)
  err64, fused64    the H36M script's ebar (N,V,J) and fused poses (N,J,3)
  err32, fused32    the Panoptic script's (ebar is float32 there)
Half of the cases store p3d / p2d as float32, half as float64.  The reference is ALWAYS handed float64 arrays, the float32 ones
widened exactly: with float32 candidates AND float32 weights np.average would run the final average itself in float32, which is
an accident of the input dtype and not one of the two variants this fixture pins (the average in float64)."""
import importlib.util
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_fuse.npz")
MIN_ERR = 0.5
# (N, V, J, stored dtype)
CASES = ((3, 4, 17, np.float64), (2, 5, 19, np.float32), (2, 2, 5, np.float64), (1, 1, 3, np.float32),
         (2, 31, 19, np.float32), (1, 33, 2, np.float64))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ring(V, rng):
    """V cameras on a ring around the subject: (proj (V,3,4), centre of the subject)."""
    centre = np.array([150.0, -250.0, 950.0])
    P = np.zeros((V, 3, 4))
    for v in range(V):
        a = 2 * np.pi * (v + rng.uniform(-0.2, 0.2)) / V
        eye = centre + np.array([np.cos(a), np.sin(a), 0.0]) * rng.uniform(3800.0, 5200.0) + [0.0, 0.0, rng.uniform(-300.0, 900.0)]
        z = centre + rng.normal(0, 60.0, 3) - eye
        z /= np.linalg.norm(z)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])                       # world -> camera
        t = -R @ eye
        f = rng.uniform(1000.0, 1500.0)
        W, H = rng.uniform(1000.0, 2048.0, 2)
        K = np.array([[f, 0.0, W / 2], [0.0, f * rng.uniform(0.99, 1.01), H / 2], [0.0, 0.0, 1.0]])
        P[v] = K @ np.hstack([R, t[:, None]])
    return P, centre


def _pixels(P, X):
    """P (V,3,4), X (..,3) -> (V,..,2)."""
    h = np.einsum("vkm,...m->v...k", P, np.concatenate([X, np.ones(X.shape[:-1] + (1,))], -1))
    return h[..., :2] / h[..., 2:3]


def make_case(N, V, J, dtype, seed):
    rng = np.random.default_rng(seed)
    P, centre = _ring(V, rng)
    truth = centre + rng.uniform(-800.0, 800.0, (N, J, 3))
    sigma = rng.uniform(20.0, 60.0, V)
    p3d = (truth[:, None] + rng.normal(0, 1.0, (N, V, J, 3)) * sigma[None, :, None, None]).astype(dtype)
    assert np.abs(p3d).max() <= 1e4
    u_truth = np.moveaxis(_pixels(P, truth), 0, 1)                                   # (N,V,J,2)
    u = np.stack([np.moveaxis(_pixels(P, p3d[:, i].astype(np.float64)), 0, 1) for i in range(V)], 1)      # (N,Vi,Vc,J,2)
    p2d = (u_truth + rng.normal(0, 3.0, u_truth.shape)).astype(dtype)
    for _ in range(200):
        e = np.linalg.norm(u - p2d.astype(np.float64)[:, None], axis=-1)             # (N,Vi,Vc,J)
        bad = (e < 1.25 * MIN_ERR).any(axis=1)                                       # (N,Vc,J)
        if not bad.any():
            break
        p2d[bad] = (u_truth[bad] + rng.normal(0, 3.0, (int(bad.sum()), 2))).astype(dtype)
    e = np.linalg.norm(u - p2d.astype(np.float64)[:, None], axis=-1)
    assert e.min() >= MIN_ERR, e.min()
    return P, p3d, p2d


def main():
    sys.path.insert(0, os.path.join(REF, "dataset_tools", "h36m"))
    h36m = _load("ref_initial_guess_h36m", "dataset_tools/h36m/compute_initial_guess.py")
    panoptic = _load("ref_initial_guess_panoptic", "dataset_tools/panoptic/compute_initial_guess_panoptic.py")
    out = {"min_err": np.float64(MIN_ERR)}
    names = []
    for k, (N, V, J, dtype) in enumerate(CASES):
        name = f"v{V}j{J}n{N}"
        names.append(name)
        P, p3d, p2d = make_case(N, V, J, dtype, seed=1000 + k)
        # the reference's layout is views first; float32 inputs widened exactly (see the docstring)
        world = np.ascontiguousarray(np.moveaxis(p3d.astype(np.float64), 0, 1))
        det = np.ascontiguousarray(np.moveaxis(p2d.astype(np.float64), 0, 1))
        plist = [P[v] for v in range(V)]
        out.update({f"{name}_proj": P, f"{name}_p3d": p3d, f"{name}_p2d": p2d})
        for tag, mod, edt in (("64", h36m, np.float64), ("32", panoptic, np.float32)):
            err = mod.compute_reprojection_error(world, det, plist)
            fused = mod.compute_weighted_average_pose(world, det, plist)
            assert err.shape == (N, V, J) and err.dtype == edt and fused.shape == (N, J, 3) and fused.dtype == np.float64
            assert np.isfinite(err).all() and np.isfinite(fused).all()
            out[f"{name}_err{tag}"], out[f"{name}_fused{tag}"] = err, fused
        print(name, p3d.dtype, "min e", float(out[f"{name}_err64"].min()),
              "variants differ by", float(np.abs(out[f"{name}_fused64"] - out[f"{name}_fused32"]).max()))
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
