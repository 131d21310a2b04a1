"""The CPU restatement of the preview's fixed sequence (include/skelsplat_hip.h, csrc/sks_preview.hip), in numpy: what the GPU
tests compare the kernels with bit for bit, and what tests/test_preview_cpu.py holds to the reference's own pictures
(tests/golden/reference_images.npz).

One view (C,H,W) float32 ->
  1. s = p[0]; s += p[1]; ...; s += p[C-1]            every addition rounded to float32, channels in ascending order
  2. lo = min(s), hi = max(s)                           NaN if any pixel is NaN (numpy's min / max propagate it, as torch's do)
  3. t = ((s - lo) / (hi - lo)) * 255                   float32, one rounding per operation
  4. q = trunc(t) where 0 <= t <= 255, else 0           (a NaN t fails the comparison)
"""
import numpy as np


def channel_sum(planes):
    """(C,H,W) float32 -> (H,W) float32, the sequential sum."""
    p = np.asarray(planes)
    assert p.dtype == np.float32 and p.ndim == 3 and p.shape[0] >= 1
    s = p[0].copy()
    with np.errstate(all="ignore"):
        for c in range(1, p.shape[0]):
            s = (s + p[c]).astype(np.float32)
    return s


def quantise(s, lo=None, hi=None):
    """Steps 2 - 4 on a sum plane -> ((H,W) uint8, (lo, hi) float32)."""
    s = np.asarray(s)
    assert s.dtype == np.float32
    with np.errstate(all="ignore"):
        lo = np.float32(s.min() if lo is None else lo)
        hi = np.float32(s.max() if hi is None else hi)
        t = ((s - lo) / np.float32(hi - lo)).astype(np.float32) * np.float32(255.0)
        assert t.dtype == np.float32
        ok = (t >= 0) & (t <= 255)
        q = np.where(ok, np.trunc(np.where(ok, t, 0)), 0).astype(np.uint8)
    return q, np.array([lo, hi], dtype=np.float32)


def preview(planes):
    """(C,H,W) float32 -> ((H,W) uint8, (2,) float32 {lo, hi})."""
    return quantise(channel_sum(planes))


def preview_views(planes):
    """(V,C,H,W) -> ((V,H,W) uint8, (V,2) float32)."""
    out = [preview(p) for p in planes]
    return np.stack([q for q, _ in out]), np.stack([m for _, m in out])


def heatmap_planes(row, col, cmin, den, w=None, h=None):
    """One view's (J,h,w) planes from its factors row (J,H), col (J,W), cmin, den (J,): the float32 expression sks_heatmaps
    stores, (row[y] * col[x] - cmin) / den, one rounding per operation."""
    row, col, cmin, den = (np.asarray(a, dtype=np.float32) for a in (row, col, cmin, den))
    h, w = h or row.shape[1], w or col.shape[1]
    prod = (row[:, :h, None] * col[:, None, :w]).astype(np.float32)
    return ((prod - cmin[:, None, None]).astype(np.float32) / den[:, None, None]).astype(np.float32)
