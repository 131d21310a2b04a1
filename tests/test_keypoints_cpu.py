"""CPU tests of the keypoint readout: the float64 restatement (tests/keypoint_ref.py) against the reference's own fp32
results (tests/golden/reference_keypoint.npz, made by tests/golden/make_golden_keypoint.py), the reference's quirks, and the
host-side argument checks of the three sks_softargmax_* entry points.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import keypoint_cases as kc
from tests import keypoint_ref as kr
from tests import util

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_keypoint.npz"))


@pytest.fixture(scope="module")
def restated():
    """Per case: image, float64 keypoints and the float64 gradients at the fixture's sample points (computed once)."""
    out = {}
    for name, regime in kc.CASES:
        key = f"{name}_{regime}"
        img = kc.make_image(name, regime)
        gt = torch.from_numpy(GOLD[key + "_gt_2d"])
        idx = torch.from_numpy(GOLD[key + "_idx"].astype(np.int64))

        def grad_of(fn):
            x = torch.from_numpy(img).double().requires_grad_(True)
            fn(x).backward()
            return x.grad.reshape(-1)[idx].numpy()

        cot = torch.from_numpy(kc.cotangent(img.shape[:2]))
        grads = {"xy": grad_of(lambda x: (kr.softargmax2d(x) * cot).sum())}
        for c in kr.CRITERIA:
            grads[c] = grad_of(lambda x: kr.criterion(c, x, gt, "mean"))
        out[key] = (img, kr.softargmax2d(torch.from_numpy(img)).numpy(), grads)
    return out


def test_fixture_was_made_from_these_images(restated):
    for key, (img, _, _) in restated.items():
        np.testing.assert_allclose(kc.checksum(img), GOLD[key + "_checksum"], rtol=1e-9, err_msg=key)
        assert np.array_equal(kc.sample_index(img), GOLD[key + "_idx"]), key


def test_restatement_agrees_with_the_reference_fixture(restated):
    """The largest deviation of the reference's fp32 CPU results from the float64 restatement, over the whole case set:
    coordinates relative to W - 1 / H - 1, losses relative to the value.  These ARE the figures keypoint_ref pins (and the GPU
    bar is DEVICE_FACTOR times them), so they are held from both sides."""
    dev_coord = dev_loss = 0.0
    for key, (img, xy64, _) in restated.items():
        H, W = img.shape[2:]
        d = np.abs(GOLD[key + "_xy"].astype(np.float64) - xy64)
        dc = max(d[..., 0].max() / max(W - 1, 1), d[..., 1].max() / max(H - 1, 1))
        dl = 0.0
        gt = torch.from_numpy(GOLD[key + "_gt_2d"])
        for c in kr.CRITERIA:
            for red in ("mean", "sum", "none"):
                want = kr.criterion(c, torch.from_numpy(img), gt, red).numpy()
                got = GOLD[f"{key}_{c}_{red}"].astype(np.float64)
                assert got.shape == want.shape, (key, c, red)
                dl = max(dl, float((np.abs(got - want) / np.abs(want)).max()))
        print(f"{key}: reference fp32 vs float64 restatement: coordinates {dc:.3e}, losses {dl:.3e}")
        dev_coord, dev_loss = max(dev_coord, dc), max(dev_loss, dl)
    print(f"measured: coordinates {dev_coord:.4e} (pinned {kr.REF_FP32_DEV_COORD}), losses {dev_loss:.4e} (pinned {kr.REF_FP32_DEV_LOSS})")
    assert 0.9 * kr.REF_FP32_DEV_COORD <= dev_coord <= kr.REF_FP32_DEV_COORD
    assert 0.9 * kr.REF_FP32_DEV_LOSS <= dev_loss <= kr.REF_FP32_DEV_LOSS


def test_restatement_gradients_are_the_references(restated):
    """Gradients with respect to the image at the fixture's sample points.  softargmax2d's own gradient: the project's standing
    rtol = 1e-3, atol_scale = 1e-4.  A criterion's gradient is linear in dL/dxy, and the reference's dL/dxy is taken at ITS
    keypoints, which lie `delta_px` (measured here, from the fixture) off: relative to the largest slope over
    keypoint_cases.RESIDUALS that moves dL/dxy by at most delta_px x curvature / largest slope <= 2 delta_px (cauchy: 2 / 1;
    huber 2 / 1.8; l2 and l2_sqrt 2 / 8), which is added to the absolute part."""
    for key, (img, xy64, grads) in restated.items():
        delta_px = float(np.abs(GOLD[key + "_xy"].astype(np.float64) - xy64).max())
        util.assert_close(key + " g_xy", GOLD[key + "_g_xy"], grads["xy"], rtol=1e-3, atol_scale=1e-4)
        for c in kr.CRITERIA:
            util.assert_close(f"{key} g_{c}", GOLD[f"{key}_g_{c}"], grads[c], rtol=1e-3, atol_scale=1e-4 + 2.0 * delta_px)


def test_reference_quirks_are_pinned():
    """What the fixture records of the reference's arithmetic as written: huber's outer branch is |delta - error| - 0.5 delta
    (a unit below the textbook delta (error - 0.5 delta) at delta = 1), and l2_sqrt is ONE root over the sum of all joints and
    both coordinates, a scalar under every reduction."""
    outer = 0
    for name, regime in kc.CASES:
        key = f"{name}_{regime}"
        err = np.abs(GOLD[key + "_xy"] - GOLD[key + "_gt_2d"]).astype(np.float64)
        hub = GOLD[key + "_huber_none"].astype(np.float64)
        assert hub.shape == err.shape
        big = err > 1.0
        outer += int(big.sum())
        np.testing.assert_allclose(hub[big], err[big] - 1.5, atol=1e-5, err_msg=key)
        np.testing.assert_allclose(hub[~big], err[~big] ** 2, atol=1e-5, err_msg=key)
        assert np.all(np.abs(hub[big] - (err[big] - 0.5)) > 0.99)                      # not the textbook branch
        assert np.all(np.abs(err - 1.0) > 1e-3), key                                   # no residual sits on the branch point
        for red in ("mean", "sum", "none"):
            v = GOLD[f"{key}_l2_sqrt_{red}"]
            assert v.shape == () and v > 0.0, (key, red)
            np.testing.assert_allclose(v, np.sqrt(GOLD[key + "_l2_sum"]), rtol=1e-5, err_msg=key)
        assert GOLD[key + "_l2_none"].shape == err.shape and GOLD[key + "_cauchy_none"].shape == err.shape
    assert outer > 50      # both branches are exercised
    # restated the same way
    r = torch.tensor([[3.0, 0.5]], dtype=torch.float64)
    np.testing.assert_allclose(kr.criterion_xy("huber", r, torch.zeros(1, 2)).numpy(), [[1.5, 0.25]])
    np.testing.assert_allclose(kr.criterion_xy("l2_sqrt", r, torch.zeros(1, 2)).numpy(), np.sqrt(9.25))


def test_uniform_plane_reads_out_the_exact_centre(restated):
    """An all-zero plane: the softmax is uniform and the keypoint is ((W - 1) / 2, (H - 1) / 2)."""
    for name, planes in kc.ZERO_PLANES.items():
        for regime in kc.REGIMES:
            img, xy64, _ = restated[f"{name}_{regime}"]
            H, W = img.shape[2:]
            for v, c in planes:
                assert not img[v, c].any()
                np.testing.assert_allclose(xy64[v, c], [(W - 1) / 2, (H - 1) / 2], rtol=1e-13)
                np.testing.assert_allclose(GOLD[f"{name}_{regime}_xy"][v, c], [(W - 1) / 2, (H - 1) / 2], rtol=1e-5)


def test_entry_points_report_bad_arguments():
    """Host-side checks: planes, W, H < 1 and a scratch buffer that is too small come back as an error string, before
    anything is enqueued or a pointer is read."""
    from skelsplat_amd import _lib
    lib = _lib.load()
    assert lib.sks_softargmax_scratch_bytes(17, 1000, 1000) == 17 * 62 * 32        # 62 chunks of 16384 elements, 4 doubles each
    assert lib.sks_softargmax_scratch_bytes(6, 53, 37) == 6 * 32
    assert lib.sks_softargmax_scratch_bytes(1, 1, 1) == 32
    for bad in ((0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, 0), (2, -3, 8)):
        assert lib.sks_softargmax_scratch_bytes(*bad) == 0
        assert b"at least 1" in lib.sks_last_error()
        with pytest.raises(RuntimeError, match="at least 1"):
            _lib.check(lib.sks_softargmax_fwd(*bad, 100.0, None, None, None, None, 1 << 20, None), "sks_softargmax_fwd")
        with pytest.raises(RuntimeError, match="at least 1"):
            _lib.check(lib.sks_softargmax_bwd(*bad, 100.0, None, None, None, None, None), "sks_softargmax_bwd")
    need = lib.sks_softargmax_scratch_bytes(4, 80, 64)
    with pytest.raises(RuntimeError, match="scratch"):
        _lib.check(lib.sks_softargmax_fwd(4, 80, 64, 100.0, None, None, None, None, need - 1, None), "sks_softargmax_fwd")
    with pytest.raises(RuntimeError, match="missing pointer"):
        _lib.check(lib.sks_softargmax_fwd(4, 80, 64, 100.0, None, None, None, None, need, None), "sks_softargmax_fwd")
    with pytest.raises(RuntimeError, match="too large"):
        _lib.check(lib.sks_softargmax_bwd(1, 65536, 65536, 100.0, None, None, None, None, None), "sks_softargmax_bwd")


def _keypoint_of_first(flat, W, count, beta=100.0):
    """Float64 [E col, E row] under softmax(beta x) over the FIRST `count` elements of a plane of width W."""
    z = beta * flat[:count].astype(np.float64)
    e = np.exp(z - z.max())
    k = np.arange(count)
    return np.array([(e * (k % W)).sum(), (e * (k // W)).sum()]) / e.sum()


def test_wide_image_reaches_the_second_trip_of_the_merge():
    """keypoint_cases.wide_image(), on the reference alone: more than 64 chunks per plane, every plane's maximum in the chunk its
    table states, and a merge that ignored the chunks from 64 on -- a wave's second trip -- would move every keypoint by more than
    100 bars (at least 25 px against a bar of about 0.1 px)."""
    from skelsplat_amd import _lib
    COORD_BAR = kr.DEVICE_FACTOR * kr.REF_FP32_DEV_COORD                                 # test_keypoints_gpu.py's, of the extent
    V, C, H, W = kc.WIDE_SHAPE
    n = H * W
    nchunks = _lib.load().sks_softargmax_scratch_bytes(V * C, W, H) // (V * C * 32)      # 4 doubles per (plane, chunk)
    assert nchunks == -(-n // kc.SA_CHUNK) == 68 > kc.MERGE_LANES
    assert n % 4 == 3 and [(c * n) % 4 for c in range(C)] == [0, 3, 2, 1, 0]
    assert 1046 * W >= kc.MERGE_LANES * kc.SA_CHUNK > 1045 * W
    img = kc.wide_image()
    assert img.shape == kc.WIDE_SHAPE and img.dtype == np.float32
    flat = img.reshape(C, n)
    for c, (_, _, centres, chunks) in kc.WIDE_PLANES.items():
        at = np.flatnonzero(flat[c] == flat[c].max())
        assert (at // kc.SA_CHUNK).tolist() == chunks, c
        assert at.tolist() == sorted(round(cy) * W + round(cx) for cx, cy in centres), c
    assert len(kc.WIDE_PLANES[3][3]) == 2                                # plane 3: exactly two equal maximal floats
    assert not flat[kc.WIDE_ZERO_PLANE].any()
    xy64 = kr.softargmax2d(torch.from_numpy(img)).numpy()[0]
    np.testing.assert_allclose(xy64[kc.WIDE_ZERO_PLANE], [(W - 1) / 2, (H - 1) / 2], rtol=1e-13)
    np.testing.assert_allclose(xy64[3], np.mean(kc.WIDE_PLANES[3][2], axis=0), rtol=1e-9)
    for c in range(C):
        np.testing.assert_allclose(_keypoint_of_first(flat[c], W, n), xy64[c], rtol=1e-12)
        cut = _keypoint_of_first(flat[c], W, kc.MERGE_LANES * kc.SA_CHUNK)
        moved = np.abs(cut - xy64[c])
        print(f"plane {c}: without chunks 64.. the keypoint moves by ({moved[0]:.1f}, {moved[1]:.1f}) px; "
              f"the bar is ({COORD_BAR * (W - 1):.3f}, {COORD_BAR * (H - 1):.3f}) px")
        assert max(moved[0] / (W - 1), moved[1] / (H - 1)) > 100 * COORD_BAR, c
        assert moved.max() >= 25.0, c


def test_backward_store_branch_and_what_a_slip_in_it_looks_like():
    """Host arithmetic and numpy only.  k_softargmax_bwd stores 16 bytes at a time for the 4 of the 16 (image phase, gradient phase)
    pairs where the phases agree and element by element for the other 12 (keypoint_cases.bwd_stores_16_bytes); and the checks
    test_keypoints_gpu.py applies to its guarded gradient buffers fail when a range is written one element off, in either
    direction, or keeps a sentinel."""
    from tests import guarded
    pairs = [(i, g) for i in guarded.PHASES for g in guarded.PHASES]
    assert sum(not kc.bwd_stores_16_bytes(i, g) for i, g in pairs) == 12
    # the rule, spelled out per chunk for the two images the GPU test uses
    for name in ("odd", "chunks"):
        V, C, H, W = kc.SHAPES[name]
        n = H * W
        for i, g in pairs:
            for p in range(V * C):
                for begin in range(0, n, kc.SA_CHUNK):
                    head = min(min(kc.SA_CHUNK, n - begin), (4 - (i + p * n + begin)) % 4)
                    assert ((g + p * n + begin + head) % 4 == 0) == kc.bwd_stores_16_bytes(i, g)
    n = 6 * 37 * 53
    want = (np.arange(n, dtype=np.float32) + 1.0).view(np.int32)
    for phase in guarded.PHASES:
        buf = np.full(guarded.buffer_floats(n), guarded.SENTINEL, dtype=np.int32)
        buf[guarded.interior(phase, n)] = want
        guarded.check("in place", buf, phase, n, want)
        for shift, text in ((1, "guard after"), (-1, "guard before")):
            off = np.full(guarded.buffer_floats(n), guarded.SENTINEL, dtype=np.int32)
            off[guarded.GUARD + phase + shift:guarded.GUARD + phase + shift + n] = want
            with pytest.raises(AssertionError, match=text):
                guarded.check("one off", off, phase, n, want)
        one = buf.copy()                                     # one group's elements written one further on, inside the range
        one[guarded.GUARD + phase + 401:guarded.GUARD + phase + 405] = want[400:404]
        one[guarded.GUARD + phase + 400] = guarded.SENTINEL
        with pytest.raises(AssertionError, match="never written"):
            guarded.check("group one off", one, phase, n, want)


def test_losses_holds_the_reference_keys_that_exist():
    from skelsplat_amd import keypoints, ops
    assert set(keypoints.losses) == {"l2", "l2_sqrt", "huber", "cauchy", "l2_gaussian"}
    assert keypoints.losses["l2_gaussian"] is ops.l2_loss_gaussian
    with pytest.raises(RuntimeError, match="ROCm device"):
        keypoints.softargmax2d(torch.zeros(2, 3, 4))
    with pytest.raises(KeyError):
        keypoints.keypoint_loss_grad("l1_l2", torch.zeros(1, 1, 2))
