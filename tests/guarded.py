"""TEST INFRASTRUCTURE -- output ranges between guards, for kernels that are handed a pointer at any 4-byte phase.  numpy only.

A kernel's output range of `n` floats is placed `GUARD + phase` floats into a buffer that is filled with SENTINEL, a quiet-NaN
bit pattern with a payload no arithmetic of the kernels produces (theirs are the default NaN or a propagated input, and the
inputs hold no NaN).  Everything is compared as int32.  check() holds what an exactly-once write means: the interior equals
the expected bits (so it holds no sentinel either), and the GUARD floats before and after it are untouched.
tests/test_keypoints_gpu.py and tests/test_masked_l2_gpu.py run the kernels into such buffers; tests/test_keypoints_cpu.py and
tests/test_masked_l2_cpu.py show on numpy writes that a range written one element off, or short of one 16-byte group, fails.
"""
import numpy as np

SENTINEL = np.int32(0x7FC5A5A5)
GUARD = 64                      # floats before and after the range; a multiple of 4, so the range starts at `phase`
PHASES = (0, 1, 2, 3)


def buffer_floats(n):
    """Floats of a buffer that takes a range of n floats at any phase between its guards (a multiple of 4)."""
    return GUARD + 4 + n + GUARD + (-n) % 4


def interior(phase, n):
    return slice(GUARD + phase, GUARD + phase + n)


def check(name, bits, phase, n, want_bits):
    """bits: the whole buffer as int32 after the kernel ran; want_bits: the n expected floats as int32."""
    bits, want_bits = np.asarray(bits), np.asarray(want_bits)
    assert bits.dtype == np.int32 and want_bits.dtype == np.int32 and want_bits.shape == (n,), name
    assert bits.shape == (buffer_floats(n),), name
    lo, hi = GUARD + phase, GUARD + phase + n
    assert np.all(bits[:lo] == SENTINEL), f"{name}: the guard before the range was written"
    assert np.all(bits[hi:] == SENTINEL), f"{name}: the guard after the range was written"
    inner = bits[lo:hi]
    left = int(np.count_nonzero(inner == SENTINEL))
    assert left == 0, f"{name}: {left} elements of the range were never written"
    bad = np.flatnonzero(inner != want_bits)
    assert bad.size == 0, f"{name}: {bad.size} elements differ, the first at {int(bad[0])}"
