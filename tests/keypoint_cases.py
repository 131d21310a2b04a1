"""TEST INFRASTRUCTURE -- the seeded heat-map planes of the keypoint tests, shared by the fixture generator
(tests/golden/make_golden_keypoint.py), the CPU tests and the GPU tests.  numpy only.

The planes are too large to commit (the largest case is 4.5 MB), so they are REBUILT from seeds: every plane is a sum of
separable Gaussian blobs evaluated in float64 and rounded to float32.  The fixture records what cannot be rebuilt --
the detections, the reference's outputs -- and a float64 checksum of every image it was made from.

Shapes are (V, C, H, W), the smallest at which the kernels of csrc/sks_keypoint.hip can go wrong (SA_CHUNK = 16384
elements per workgroup, 16-byte groups):
  one     (1,1,1,1)       the reference multiplies by h - 1 = w - 1 = 0
  row7    (1,1,1,7)       h - 1 = 0; shorter than two 16-byte groups
  odd     (2,3,37,53)     H * W odd: every plane but the first starts off 16-byte alignment (all three offsets occur), every
                          plane is shorter than one chunk; plane (1,2) is ALL ZERO (uniform softmax, keypoint = exact centre)
  chunks  (1,17,251,263)  five chunks per plane, the last of 477 elements; the maximum lies in the first (plane 0), a middle
                          (plane 1) and the last chunk (plane 2); planes 3 and 4 have TWO EQUAL maxima in different chunks
  pan     (4,19,64,80)    Panoptic's channel count, four views
  op      (2,15,48,64)    Occlusion-Person's; plane (0,7) is all zero
Each in two regimes: `peak1` (peak 0.9 .. 1.0: at beta = 100 the background's weights underflow) and `peak002` (peak
0.015 .. 0.02: the background dominates and the keypoint is pulled towards the image centre, as in the reference).

Beside the case set, and not part of the fixture: wide_image(), (1,5,1097,1003), 68 chunks per plane -- the one shape at which a
lane of the merge kernel takes a second chunk record.
"""
import numpy as np

SHAPES = {"one": (1, 1, 1, 1), "row7": (1, 1, 1, 7), "odd": (2, 3, 37, 53), "chunks": (1, 17, 251, 263),
          "pan": (4, 19, 64, 80), "op": (2, 15, 48, 64)}
REGIMES = {"peak1": (0.9, 1.0), "peak002": (0.015, 0.02)}
CASES = [(name, regime) for name in SHAPES for regime in REGIMES]
ZERO_PLANES = {"odd": [(1, 2)], "op": [(0, 7)]}
# (view, channel) -> [(cx, cy), ...] of the `chunks` case; integer centres make the two maxima of planes 3 and 4 equal floats
PLACED = {(0, 0): [(40.3, 5.3)], (0, 1): [(101.7, 125.4)], (0, 2): [(100.3, 250.0)],
          (0, 3): [(40.0, 20.0), (200.0, 230.0)], (0, 4): [(130.0, 60.0), (131.0, 190.0)]}
# residual |keypoint - detection| in pixels, cycled over joints and coordinates: both branches of huber (delta = 1), none
# within 1e-3 px of delta, and never all zero (l2_sqrt's gradient is 0 / 0 there)
RESIDUALS = (0.3, -0.6, 1.7, -2.5, 0.05, 4.0, -0.9, 1.2)


def make_image(name, regime):
    """The (V, C, H, W) float32 image of a case."""
    V, C, H, W = SHAPES[name]
    lo, hi = REGIMES[regime]
    rng = np.random.default_rng([sorted(SHAPES).index(name), sorted(REGIMES).index(regime), 20240])
    img = np.zeros((V, C, H, W), dtype=np.float32)
    cols, rows = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    for v in range(V):
        for c in range(C):
            cx, cy = rng.uniform(0.15, 0.85) * (W - 1), rng.uniform(0.15, 0.85) * (H - 1)
            sigma, amp = rng.uniform(1.5, 4.0), rng.uniform(lo, hi)
            if (v, c) in ZERO_PLANES.get(name, ()):
                continue
            centres = PLACED.get((v, c), [(cx, cy)]) if name == "chunks" else [(cx, cy)]
            plane = np.zeros((H, W))
            for bx, by in centres:
                plane += amp * np.outer(np.exp(-(rows - by) ** 2 / (2 * sigma ** 2)), np.exp(-(cols - bx) ** 2 / (2 * sigma ** 2)))
            img[v, c] = plane.astype(np.float32)
    return img


# ---- more than 64 chunks per plane: k_softargmax_merge's second trip ---------------------------------------------------------
# One wave merges a plane's chunk records, lane L taking chunks L, L + 64, ...: only a plane of more than 64 chunks makes a lane
# take a second one.  wide_image() is NOT an entry of SHAPES / CASES: those are bound to the golden fixture and to the measured
# REF_FP32_DEV_* constants.  SA_CHUNK restates csrc/sks_keypoint.hip's constant; tests/test_keypoints_cpu.py holds it to the
# library's own sks_softargmax_scratch_bytes.
SA_CHUNK = 16384
MERGE_LANES = 64
WIDE_SHAPE = (1, 5, 1097, 1003)     # H * W = 1 100 291: 68 chunks; H * W % 4 == 3, so the planes start at phases 0, 3, 2, 1, 0;
#                                     rows from 1046 on lie wholly in chunks 64 and above
# plane -> (amplitude, sigma, [(cx, cy), ...], chunk(s) of the maximum); plane 4 is all zero (uniform softmax, the exact centre)
WIDE_PLANES = {0: (0.95, 3.0, [(700.3, 1080.4)], [66]),                 # peak1: the maximum on the second trip
               1: (0.018, 2.5, [(200.7, 300.2)], [18]),                 # peak002: maximum on the first trip, background everywhere
               2: (0.017, 3.5, [(500.6, 1075.3)], [65]),                # peak002: the maximum on the second trip
               3: (0.93, 3.0, [(100.0, 50.0), (900.0, 1085.0)], [3, 66])}    # two equal maxima, one on each trip
WIDE_ZERO_PLANE = 4


def wide_image():
    """The WIDE_SHAPE float32 image: sums of blobs evaluated in float64 and rounded to float32, like make_image."""
    V, C, H, W = WIDE_SHAPE
    img = np.zeros(WIDE_SHAPE, dtype=np.float32)
    cols, rows = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    for c, (amp, sigma, centres, _) in WIDE_PLANES.items():
        plane = np.zeros((H, W))
        for bx, by in centres:
            plane += amp * np.outer(np.exp(-(rows - by) ** 2 / (2 * sigma ** 2)), np.exp(-(cols - bx) ** 2 / (2 * sigma ** 2)))
        img[0, c] = plane.astype(np.float32)
    return img


def bwd_stores_16_bytes(img_phase, grad_phase):
    """k_softargmax_bwd's `vec_store` for base pointers img_phase / grad_phase floats past a 16-byte boundary.  A chunk of plane p
    starts at the same element offset e from both bases; its scalar head takes (4 - (img_phase + e)) % 4 elements, so the first
    group's gradient lies (grad_phase + e + (4 - (img_phase + e)) % 4) % 4 = (grad_phase - img_phase) % 4 floats past a boundary,
    whatever the plane and the chunk: 16-byte stores where the two phases agree, element by element for the other 12 of the 16
    pairs."""
    return (grad_phase - img_phase) % 4 == 0


def checksum(img):
    """Two float64 sums that move when any element or its position does."""
    x = img.astype(np.float64).ravel()
    return np.array([x.sum(), (x * (1.0 + (np.arange(x.size) % 1009))).sum()])


def cotangent(shape):
    """The fixed upstream gradient of softargmax2d's (V, C, 2) output (float64; the tests cast it)."""
    k = np.arange(int(np.prod(shape)) * 2, dtype=np.float64).reshape(*shape, 2)
    return np.cos(0.7 * k) + 0.25 * np.sin(0.13 * k * k)


def detections(xy64):
    """gt_2d for float64 keypoints xy64 (V, J, 2): the keypoints minus RESIDUALS, cycled; float32."""
    r = np.resize(np.array(RESIDUALS), xy64.shape)
    return (xy64 - r).astype(np.float32)


def sample_index(img, strided=16, window=2):
    """Flat indices into `img` at which the fixture records gradients: everything for small images, else per plane
    `strided` evenly spaced elements and the (2 window + 1)^2 neighbourhood of the plane's (first) maximum."""
    V, C, H, W = img.shape
    n = H * W
    if img.size <= 4096:
        return np.arange(img.size, dtype=np.int32)
    out = []
    for p in range(V * C):
        plane = img.reshape(V * C, n)[p]
        r0, c0 = divmod(int(plane.argmax()), W)
        rr, cc = np.meshgrid(np.clip(np.arange(r0 - window, r0 + window + 1), 0, H - 1),
                             np.clip(np.arange(c0 - window, c0 + window + 1), 0, W - 1), indexing="ij")
        idx = np.unique(np.concatenate([np.arange(strided) * (n // strided), (rr * W + cc).ravel()]))
        out.append(idx + p * n)
    return np.concatenate(out).astype(np.int32)
