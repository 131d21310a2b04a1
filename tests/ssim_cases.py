"""Seeded fused-SSIM test inputs shared by the CPU (oracle) and GPU (parity) tests, and the float64 conv2d SSIM.

Input classes (make(name, shape)): what each one reaches is listed in CLASSES.  Shapes are the smallest at which the
kernels' mechanisms exist: a tile is 64 x 32 outputs, a strip hands 10 filtered rows from tile to tile, the 16-byte path
needs W % 4 == 0.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

TAPS32 = np.array([0.001028380123898387, 0.0075987582094967365, 0.036000773310661316, 0.10936068743467331,
                   0.21300552785396576, 0.26601171493530273, 0.21300552785396576, 0.10936068743467331,
                   0.036000773310661316, 0.0075987582094967365, 0.001028380123898387], dtype=np.float32)   # ssim.cu:9-19


def ssim_window(ch, like, taps=None):
    """The reference's 11 x 11 window (utils/loss_utils.py:253-262); with `taps` the exact outer product of those taps
    in float64 instead (what a separable filter with these taps sums, in another order)."""
    if taps is None:
        g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
        g = (g / g.sum()).unsqueeze(1)
        w2 = g.mm(g.t()).float()
    else:
        t = torch.as_tensor(np.asarray(taps, dtype=np.float64))
        w2 = torch.outer(t, t)
    return w2[None, None].expand(ch, 1, 11, 11).contiguous().to(like)


def ssim_moments(img1, img2, taps=None):
    """mu1, mu2, E[x^2], E[y^2], E[xy] under the window, zero padding."""
    ch = img1.size(-3)
    win = ssim_window(ch, img1, taps)
    conv = lambda x: F.conv2d(x, win, padding=5, groups=ch)
    return conv(img1), conv(img2), conv(img1 * img1), conv(img2 * img2), conv(img1 * img2)


def ssim_torch(img1, img2, C1=0.01 ** 2, C2=0.03 ** 2, taps=None):
    """The reference's own SSIM oracle (utils/loss_utils.py:253-300 == submodules/fused-ssim/tests/test.py:24-54)."""
    mu1, mu2, e11, e22, e12 = ssim_moments(img1, img2, taps)
    s1 = e11 - mu1.pow(2)
    s2 = e22 - mu2.pow(2)
    s12 = e12 - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1.pow(2) + mu2.pow(2) + C1) * (s1 + s2 + C2))


# ---- shapes ------------------------------------------------------------------------------------------------------
SHAPE_VEC = (1, 2, 75, 132)      # 3 tile rows (the last one partial), 3 tile columns, 16-byte path
SHAPE_SCALAR = (2, 1, 97, 131)   # W % 4 != 0: scalar path
SHAPE_SHORT = (1, 1, 12, 16)     # fewer rows than the filter has taps beside it
SHAPE_TINY = (1, 1, 5, 7)        # "valid" is empty
SHAPE_TALL = (1, 3, 300, 136)    # 10 tile rows: strips of 8, 2 and 1 under SKS_SSIM_MIN_BLOCKS 1, 40, 1000000
MAIN_SHAPES = [SHAPE_VEC, SHAPE_SCALAR]
ALL_SHAPES = [SHAPE_VEC, SHAPE_SCALAR, SHAPE_SHORT, SHAPE_TINY, SHAPE_TALL]
MIN_BLOCKS = ["1", "40", "1000000"]


class Case:
    def __init__(self, name, img1, img2, C1=0.01 ** 2, C2=0.03 ** 2):
        self.name, self.C1, self.C2 = name, C1, C2
        self.img1 = np.ascontiguousarray(img1, dtype=np.float32)
        self.img2 = np.ascontiguousarray(img2, dtype=np.float32)
        self.shape = self.img1.shape


def _rng(name, shape, seed):
    return np.random.default_rng([seed, sum(name.encode()), *shape])


def _blobs(rng, shape, shift, clip=True, normalise=False, per_plane=None):
    """Gaussian blobs per plane; `shift` moves every centre by a fraction of a pixel.  clip: exactly 0 outside 3 sigma
    (and below 2^-16); otherwise exp() runs down through the denormals to 0."""
    B, CH, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros(shape, np.float64)
    for p in range(B * CH):
        n = per_plane or (2 + p % 2)
        for _ in range(n):
            cy, cx = rng.uniform(0, H - 1), rng.uniform(0, W - 1)
            sig, amp = rng.uniform(1.5, 3.5), rng.uniform(0.3, 1.0)
            r2 = (yy - cy - shift[0]) ** 2 + (xx - cx - shift[1]) ** 2
            h = amp * np.exp(-r2 / (2 * sig * sig))
            if clip:
                h[r2 > (3 * sig) ** 2] = 0.0
            out[p // CH, p % CH] += h
        if normalise:
            out[p // CH, p % CH] /= out[p // CH, p % CH].sum()
    out = out.astype(np.float32)
    if clip:
        out[out < 2.0 ** -16] = 0.0
    return out


def _noise(name, shape, seed):
    r = _rng(name, shape, seed)
    return Case(name, r.random(shape, np.float32), r.random(shape, np.float32))


def _flat(levels, noisy):
    def gen(name, shape, seed):
        r = _rng(name, shape, seed)
        B, CH, H, W = shape
        a = np.empty(shape, np.float32)
        for p in range(B * CH):
            a[p // CH, p % CH] = levels[p % len(levels)]
        b = a + np.float32(1e-3) * r.random(shape, np.float32) if noisy else a.copy()
        return Case(name, a, b)
    return gen


def _heatmaps(scale=1.0, **consts):
    def gen(name, shape, seed):
        a = _blobs(_rng(name, shape, seed), shape, (0.0, 0.0))
        b = _blobs(_rng(name, shape, seed), shape, (0.3, -0.45))
        return Case(name, a * np.float32(scale), b * np.float32(scale), **consts)
    return gen


def _tails(name, shape, seed):
    a = _blobs(_rng(name, shape, seed), shape, (0.0, 0.0), clip=False, normalise=True, per_plane=1)
    b = _blobs(_rng(name, shape, seed), shape, (0.3, -0.45), clip=False, normalise=True, per_plane=1)
    return Case(name, a, b)


SEAM_X = [0, 63, 64, -1]
SEAM_Y = [0, 31, 32, 41, 42, -1]


def _seams(name, shape, seed):
    """One impulse per plane (clipped to the image); the batch grows to 12 planes: every y of SEAM_Y with two of the x of
    SEAM_X, every x three times (the two passes are separate mechanisms: halo columns and swizzle, carried rows)."""
    _, _, H, W = shape
    n = 2 * len(SEAM_Y)
    a, b = np.zeros((n, 1, H, W), np.float32), np.zeros((n, 1, H, W), np.float32)
    for p in range(n):
        y = SEAM_Y[p % len(SEAM_Y)]
        x = SEAM_X[(p % len(SEAM_Y) + 2 * (p // len(SEAM_Y))) % len(SEAM_X)]
        x, y = min(x, W - 1) % W, min(y, H - 1) % H
        a[p, 0, y, x] = 1.0
        b[p, 0, y, x] = 0.75
        b[p, 0, (y + 3) % H, (x + 2) % W] = 0.5
    return Case(name, a, b)


def _checker(shifted):
    def gen(name, shape, seed):
        _, _, H, W = shape
        yy, xx = np.mgrid[0:H, 0:W]
        board = (((yy // 8) + (xx // 8)) % 2).astype(np.float32)
        a = np.broadcast_to(board, shape).copy()
        b = np.broadcast_to(np.float32(1) - board if shifted else board, shape).copy()
        return Case(name, a, b)
    return gen


def _signed(name, shape, seed):
    r = _rng(name, shape, seed)
    return Case(name, r.uniform(-1, 1, shape).astype(np.float32), r.uniform(-1, 1, shape).astype(np.float32))


def _nonfinite(name, shape, seed):
    c = _noise(name, shape, seed)
    B, CH, H, W = shape
    c.img1[0, 0, H // 3, W // 3] = np.nan
    c.img2[B - 1, CH - 1, (2 * H) // 3, (2 * W) // 3] = np.inf
    return c


# name -> generator.  What each class reaches:
CLASSES = {
    "noise": _noise,                                        # control: variance 1/12 everywhere, nothing cancels
    "flat-same-lo": _flat([0.0, 2.0 ** -16], False),        # E[x^2] - mu^2 cancels, B -> C2, map -> 1, gradient is rounding
    "flat-same-hi": _flat([0.7, 1.0], False),
    "flat-noisy-lo": _flat([0.0, 2.0 ** -16], True),
    "flat-noisy-hi": _flat([0.7, 1.0], True),
    "heatmaps": _heatmaps(),                                # the project's pair: zeros with blobs, nearly identical images
    "tails": _tails,                                        # numerators below 2^-100: the flagged class
    "seams": _seams,                                        # the map is the footprint: halo columns, carried rows, swizzle
    "checker-same": _checker(False),                        # step edges across every tile border
    "checker-shift": _checker(True),                        # ... D < 0, negative map
    "signed": _signed,                                      # negative mu, Cn < 0
    "blobs255": _heatmaps(scale=255.0),                     # denominators up to ~2^50
    "nonfinite": _nonfinite,                                # one nan, one +inf
    "constants": _heatmaps(C1=2.0 ** -12, C2=2.0 ** -12),   # constants are arguments
}
MAY_BE_FLAGGED = ("tails", "nonfinite")
EVERY_SHAPE = ("seams", "checker-same", "checker-shift")

_CACHE = {}


def make(name, shape, seed=0):
    key = (name, tuple(shape), seed)
    if key not in _CACHE:
        _CACHE[key] = CLASSES[name](name, tuple(shape), seed)
    return _CACHE[key]


def case_list():
    """(class, shape): every class on the two main shapes, the seams and the checkerboards on all of them."""
    out = []
    for name in CLASSES:
        for shape in (ALL_SHAPES if name in EVERY_SHAPE else MAIN_SHAPES):
            out.append((name, shape))
    return out


def case_id(v):
    return v if isinstance(v, str) else "x".join(str(s) for s in v)
