"""oracle/sks_oracle.c held to the REFERENCE's own rasterizer sources compiled for the host (oracle/ref_build.py, oracle/ref.py).

The oracle is this project's restatement of forward.cu / backward.cu / rasterizer_impl.cu / auxiliary.h; what it is compared
with here is those files themselves, run one block at a time on one thread with exp() routed to the oracle's expf.  Forward:
every artefact bit for bit (np.array_equal) -- a misread convention (a glm product's order, the clamp of t, the low-pass, the
radius, getRect's rounding, the sort key, the alpha gates, the T stop) moves bits.  Backward: the reference sums in fp32 in
thread order, the oracle in double: the project's standing tolerance (rtol 1e-3, atol 1e-5 x max),
`extreme` cases at the computed rounding allowance (util.assert_close_bound).

Known deviations, stated where they apply and nowhere else:
  * dL_dsh is not compared: the reference's SH backward runs over the feature buffer as vec3 coefficients and reads flags its
    forward never wrote; the true dL/dfeature, dL_dcolors, is compared.
  * the background handed to the reference is zero-padded to NUM_CHANNELS floats (its backward reads bg_color[ch] for every
    channel, backward.cu:613-614) -- the oracle pads the same way.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import ref_cases


_ref = ref_cases.compiled_reference


HAND = ref_cases.hand_cases()


def check_forward(rc, o, r):
    for k in ref_cases.FORWARD_EXACT:
        assert o[k].shape == r[k].shape and o[k].dtype == r[k].dtype, (rc.name, k, o[k].shape, r[k].shape)
        assert np.array_equal(o[k], r[k]), f"{rc.name}: {k} differs from the compiled reference in {(o[k] != r[k]).sum()} places"
    assert o["R"] == r["R"]
    vis = r["radii"] > 0
    for k in ref_cases.GEOM_EXACT:
        if k == "cov3D" and rc.precomp:     # (handed in: the reference leaves its own cov3D array unwritten)
            continue
        assert np.array_equal(o[k][vis], r[k][vis]), f"{rc.name}: {k} of the visible Gaussians"
    assert np.array_equal(o["point_offsets"], r["point_offsets"]), f"{rc.name}: point_offsets"


@functools.lru_cache(maxsize=None)
def _hand(name):
    ref = _ref()
    rc = HAND[name]()
    o, r = rc.forward(orc), rc.forward(ref)
    return rc, o, r


@pytest.mark.parametrize("name", list(HAND))
def test_forward_is_the_references_bit_for_bit(name):
    rc, o, r = _hand(name)
    check_forward(rc, o, r)
    assert (r["radii"] > 0).any() and r["n_contrib"].max() > 0, "the case draws nothing"


@pytest.mark.parametrize("name", list(HAND))
def test_backward_is_the_references_within_the_standing_tolerance(name):
    rc, o, r = _hand(name)
    check_forward(rc, o, r)
    ratios = ref_cases.grad_ratios(rc, rc.backward(_ref(), r), rc.backward(orc, o))
    print(f"{rc.name}: observed / allowed " + ", ".join(f"{k[3:]} {v:.3f}" for k, v in ratios.items()))
    assert ratios["dL_dmeans3D"] > 0 and ratios["dL_dcolors"] >= 0


def test_the_hand_cases_reach_what_they_are_for():
    """Each special case really is one: two compositing rounds with a partial second one, culling both ways, one Gaussian."""
    rc, o, r = _hand("tile-of-300")
    lengths = r["ranges"][:, 1].astype(np.int64) - r["ranges"][:, 0]
    assert lengths.max() > 256 and lengths.max() % 256 != 0, lengths
    assert r["n_contrib"].max() > 256, "the second round composites nothing"
    rc, o, r = _hand("culled")
    assert not orc.mark_visible(rc.means, rc.cam)[[0, 2]].any() and orc.mark_visible(rc.means, rc.cam)[1]
    assert (r["radii"][:3] == 0).all() and (r["radii"][3:] > 0).any()
    rc, o, r = _hand("P=1")
    assert rc.P == 1 and r["radii"][0] > 0 and r["R"] >= 1
    rc, o, r = _hand("70x36")
    assert rc.W % 16 and rc.H % 16
    rc, o, r = _hand("clamped-t")
    limx, limy = 1.3 * rc.cam.tanfovx, 1.3 * rc.cam.tanfovy
    pv = rc.means.astype(np.float64) @ rc.cam.view.reshape(4, 4)[:3, :3] + rc.cam.view.reshape(4, 4)[3, :3]
    outside = (np.abs(pv[:, 0] / pv[:, 2]) > limx) | (np.abs(pv[:, 1] / pv[:, 2]) > limy)
    assert (outside & (r["radii"] > 0)).any(), "no visible Gaussian has its t.x / t.y clamped"
    assert {HAND[n]().C for n in ("seed0-plain", "seed4-plain", "seed5-plain")} == {17, 19, 15}


@pytest.mark.parametrize("name", ["seed0-plain", "culled", "seed4-plain", "seed5-plain"])
def test_mark_visible_is_the_references(name):
    ref = _ref()
    rc = HAND[name]()
    got = ref.mark_visible(rc.means, rc.cam, channels=rc.C)
    assert np.array_equal(orc.mark_visible(rc.means, rc.cam), got)
    assert np.array_equal(got, rc.forward(ref)["radii"] > 0) or name == "culled"


# forty seeds of each generator of tests/fuzz_cases.py that feeds the rasterizer, `extreme` included (the one-call generator's
# every third seed has 33-71 channels, which no rasterizer build has: left out)
FUZZ = {"binned": [s for s in range(5000, 5060) if s % 5][:40], "extreme": list(range(20000, 20200, 5)),
        "one-call": [s for s in range(700, 760) if s % 3], "fused-loss": list(range(300, 340))}


@pytest.mark.parametrize("generator,seed", [(g, s) for g, seeds in FUZZ.items() for s in seeds])
def test_fuzz_generators_forward_exact_backward_in_tolerance(generator, seed):
    """One view of the scene the generator draws for the seed: forward bit for bit, backward as above.  Prints the observed /
    allowed ratio per gradient."""
    ref = _ref()
    rc = ref_cases.fuzz_cases(generator, seed)
    assert rc is not None, "the seed's scene has a channel count no rasterizer build has"
    o, r = rc.forward(orc), rc.forward(ref)
    check_forward(rc, o, r)
    ratios = ref_cases.grad_ratios(rc, rc.backward(ref, r), rc.backward(orc, o, bounds=rc.extreme))
    print(f"{generator} seed {seed}: observed / allowed " + ", ".join(f"{k[3:]} {v:.3f}" for k, v in ratios.items()))


def test_the_fuzz_selection_is_forty_seeds_of_each_generator():
    assert {g: len(s) for g, s in FUZZ.items()} == {"binned": 40, "extreme": 40, "one-call": 40, "fused-loss": 40}


def test_launch_rewrite_touches_launches_only():
    """The one textual change the recipe makes to the reference's sources, on text of our own."""
    from oracle import ref_build
    text = ("a <<= 3; std::cerr << x << y;\n\tkernelA << <(P + 255) / 256, 256 >> > (\n\t\tP, q);\n"
            "\tkernelB<NUM_CHANNELS> << <grid, block >> >(r);\nif (a < b && c >> 2 > (d)) {}\n")
    out, n = ref_build.rewrite_launches(text)
    assert n == 2
    assert "ref_shim::launch(kernelA, (P + 255) / 256, 256, \n\t\tP, q);" in out
    assert "ref_shim::launch(kernelB<NUM_CHANNELS>, grid, block, r);" in out
    assert "a <<= 3; std::cerr << x << y;" in out and "if (a < b && c >> 2 > (d)) {}" in out
