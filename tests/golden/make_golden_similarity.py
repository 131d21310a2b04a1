"""Generates tests/golden/reference_similarity.npz by running the REFERENCE's own `pairwise_cosine_similarity`,
`compute_scaling_weights` and `identify_consistent_views` (utils/similarity_utils.py:9-27, 159-187, 68-79; loaded by path from
/root/reference in the build container, MPLBACKEND=Agg: the module imports matplotlib.pyplot at its top) on seeded gradients.
Run:  python tests/golden/make_golden_similarity.py

Per case `<name>` = v4j17 / v4j19 the file holds
  grads       (4,J,3) float32, magnitudes log-uniform in 1e-6 .. 1e-2; view 2 of joints 0-2 is ZERO, view 3 of joints 3-5 OPPOSES
              view 0 exactly, the rest are a common direction plus noise (so that `select` keeps some views and drops others)
  similarity  (J,4,4) float32   pairwise_cosine_similarity(grads)
  scale       (4,J)   float32   compute_scaling_weights(similarity) -- the reference divides by 3, which is V - 1 here
  select      (J,4)   bool      identify_consistent_views(similarity, threshold)
and once
  threshold   float32 0.5
  same_grads  (4,N,3) float32: four IDENTICAL rows per joint, random directions -- the joints where the reference's mean
              similarity rounds above 1 and its weight_function returns 0 -- with same_similarity / same_scale as above.
Four views only: the reference's divisor is the literal 3."""
import importlib.util
import os

os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_similarity.npz")
THRESHOLD = 0.5


def _load():
    spec = importlib.util.spec_from_file_location("ref_similarity_utils", os.path.join(REF, "utils", "similarity_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_grads(J, seed):
    rng = np.random.default_rng(seed)
    common = rng.normal(size=(1, J, 3))
    common /= np.linalg.norm(common, axis=-1, keepdims=True)
    d = common + rng.normal(scale=rng.uniform(0.05, 1.5, size=(1, J, 1)), size=(4, J, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    g = d * 10.0 ** rng.uniform(-6.0, -2.0, size=(4, J, 1))
    g = g.astype(np.float32)
    g[2, 0:3] = 0.0
    g[3, 3:6] = -g[0, 3:6]
    return g


def main():
    ref = _load()
    out = {"threshold": np.float32(THRESHOLD)}
    names = []
    for J, seed in ((17, 4170), (19, 4190)):
        name = f"v4j{J}"
        names.append(name)
        g = make_grads(J, seed)
        t = torch.from_numpy(g)
        sim = ref.pairwise_cosine_similarity(t)
        scale = ref.compute_scaling_weights(sim)
        sel = ref.identify_consistent_views(sim, threshold=THRESHOLD)
        assert sim.shape == (J, 4, 4) and sim.dtype == torch.float32 and scale.shape == (4, J) and sel.shape == (J, 4)
        out.update({f"{name}_grads": g, f"{name}_similarity": sim.numpy(), f"{name}_scale": scale.numpy(),
                    f"{name}_select": sel.numpy()})
        print(name, "kept per joint", sel.sum(1).tolist())
    rng = np.random.default_rng(361)
    d = rng.normal(size=(2000, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    # (unit length: below about 1e-1 the 1e-8 added to the norm already keeps every cosine under 1)
    g = np.broadcast_to(d.astype(np.float32)[None], (4, 2000, 3)).copy()
    sim = ref.pairwise_cosine_similarity(torch.from_numpy(g))
    scale = ref.compute_scaling_weights(sim).numpy()
    zero = np.flatnonzero((scale == 0).all(0))
    print("identical views: the reference's weight is 0 for", int((scale == 0).any(0).sum()), "of 2000 directions")
    keep = np.concatenate([zero[:8], np.flatnonzero((scale != 0).all(0))[:8]])
    assert len(zero) >= 8
    out.update({"same_grads": g[:, keep], "same_similarity": sim.numpy()[keep], "same_scale": scale[:, keep]})
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
