"""TEST INFRASTRUCTURE -- the seeded cases of the masked-L2 tests (k_masked_l2, csrc/sks_ops.hip), shared by
tests/test_masked_l2_cpu.py and tests/test_masked_l2_gpu.py.  numpy only; nothing here loads the HIP library.

The kernel runs `blocks` workgroups of `threads` threads per view (sks_masked_l2_launch gives both); thread t of the
stride = blocks x threads walks the view's n4 = n // 4 16-byte groups in two loops,
    unrolled   while t + 3 stride < n4:  groups t, t + stride, t + 2 stride, t + 3 stride (non-temporal stores), t += 4 stride
    remainder  while t < n4:             group t, t += stride
and workgroup 0 takes the n % 4 elements after the last group one by one.  regime() works the loops' trip counts out of
(blocks, threads, n); REGIMES states what every case is there for, and the CPU test holds the two together, so a retuned launch
shape cannot silently empty a case.

A case is (V, n per view): the arrays are (V, n) float32, used as (V, 1, 1, n) through ops.masked_l2 or flat through the C ABI.
With n % 4 != 0 view v starts v * n % 4 floats past a 16-byte boundary: the kernel's 16-byte groups are relative to the VIEW.
"""
import numpy as np

U = 2.0 ** -24                 # the unit the allowances are counted in
S_BAR_U = 8.0                  # |S - S64| <= S_BAR_U x U x S64 (the count is in reference())
LOSS_BAR_U = 10.0              # the fused criterion's float: S_BAR_U, plus the division (fp64: nothing), plus the cast to float (1)

CASES = {"tail": (2, 3),
         "one_block": (3, 4 * 700 + 2),
         "few_blocks": (2, 4 * (1024 * 37 + 5) + 1),
         "remainder": (2, 4 * (2 * 262144 + 77) + 3),
         "edge0": (1, 3145728),
         "edge1": (1, 3145732),
         "main": (2, 3151731),
         "main2": (1, 4 * (7 * 262144 + 300) + 1)}

# what regime() must give with the library's launch shape: workgroups per view, threads that take at least one unrolled trip,
# the largest trip count of the unrolled and of the remainder loop over the threads, elements of the scalar tail
REGIMES = {"tail": dict(blocks=1, unrolled_threads=0, unrolled_trips=0, remainder_trips=0, tail=3),
           "one_block": dict(blocks=1, unrolled_threads=0, unrolled_trips=0, remainder_trips=1, tail=2),
           "few_blocks": dict(blocks=38, unrolled_threads=0, unrolled_trips=0, remainder_trips=1, tail=1),
           "remainder": dict(blocks=256, unrolled_threads=0, unrolled_trips=0, remainder_trips=3, tail=3),
           "edge0": dict(blocks=256, unrolled_threads=0, unrolled_trips=0, remainder_trips=3, tail=0),
           "edge1": dict(blocks=256, unrolled_threads=1, unrolled_trips=1, remainder_trips=3, tail=0),
           "main": dict(blocks=256, unrolled_threads=1500, unrolled_trips=1, remainder_trips=3, tail=3),
           "main2": dict(blocks=256, unrolled_threads=262144, unrolled_trips=2, remainder_trips=3, tail=1)}
# the cases whose gradient is also written at every 4-byte phase of the three base pointers (test_masked_l2_gpu.py)
PHASE_CASES = ("main", "remainder", "one_block")
# (render, gt, dL) phases: the four where all three agree, four where dL alone differs, two where all three differ
PHASE_TRIPLES = ((0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 0, 1), (1, 1, 3), (2, 2, 0), (3, 3, 2), (0, 1, 2), (3, 2, 0))


def regime(blocks, threads, n):
    """The loops' trip counts for a view of n elements launched as (blocks, threads): a dict like REGIMES' entries."""
    n4, stride = n // 4, blocks * threads
    t = np.arange(stride, dtype=np.int64)
    unrolled = np.maximum(0, -((t + 3 * stride - n4) // (4 * stride)))         # ceil((n4 - 3 stride - t) / (4 stride)), at least 0
    after = t + 4 * stride * unrolled
    remainder = np.maximum(0, -((after - n4) // stride))
    # every group is taken exactly once: thread t's groups are t, t + stride, ..., and their count is the sum of its trips
    assert int((4 * unrolled + remainder).sum()) == n4 and np.all(after + stride * remainder >= n4)
    return dict(blocks=blocks, unrolled_threads=int(np.count_nonzero(unrolled)), unrolled_trips=int(unrolled.max()),
                remainder_trips=int(remainder.max()), tail=n - 4 * n4)


def make_inputs(name):
    """(render, gt), (V, n) float32: render uniform in [-0.5, 1.5] with 40 % exact zeros -- an unclamped render has entries below 0
    and above 1 --, gt uniform in [-0.25, 1.0] with 50 % exact zeros; non-zero magnitudes are at least 1e-3, so no square
    underflows.  The zeros are +0.0."""
    V, n = CASES[name]
    rng = np.random.default_rng([sorted(CASES).index(name), 8086])

    def draw(lo, hi, zeros):
        x = rng.uniform(lo, hi, (V, n)).astype(np.float32)
        x = np.where(np.abs(x) < 1e-3, np.float32(1e-3), x)
        return np.where(rng.random((V, n)) < zeros, np.float32(0.0), x).astype(np.float32)

    return draw(-0.5, 1.5, 0.4), draw(-0.25, 1.0, 0.5)


def reference(render, gt):
    """What the kernel is held to, per view: N (exact), S64 (float64) and dL (float32, compared as int32).

    N    the count of (gt > 0) | (render > 0).
    S64  the float64 sum of (double(r) - double(g))^2 over the mask; the kernel's S lies within S_BAR_U x 2^-24 x S64.  Counted,
         not measured, in units of u = 2^-24 relative to a 16-byte group's sum: e = fl(a - b) carried into e^2 is 2u; the FMA
         chain of four on non-negative partial sums bounded by the group's sum is 4u; the group sums are added in fp64 (n x 2^-53:
         nothing).  6u per group, hence at most 6u of the total; 8u are allowed.  One dropped group of `main` moves S by ~21u.
    dL   float32 where(mask, 2 * (r - g), +0.0): the kernel's 2 * e is exact, and r - g is -0 for no pair of floats under
         round-to-nearest unless r is -0, which the inputs do not hold."""
    mask = (gt > 0) | (render > 0)
    d = render.astype(np.float64) - gt.astype(np.float64)
    S64 = np.where(mask, d * d, 0.0).sum(axis=1)
    dL = np.where(mask, np.float32(2.0) * (render - gt), np.float32(0.0)).astype(np.float32)
    return mask.sum(axis=1), S64, dL


def restated(render, gt):
    """The kernel's arithmetic, restated for one view (1-D arrays): (N, S, dL, worst group deviation in units of U).
    Per 16-byte group -- relative to the view's start -- e = fl(a - b) on the mask, the four e^2 through a chain of fp32 FMAs
    from 0, every group's float into a float64 sum; the tail elements as groups of one.  (fma(e, e, acc) is formed as the
    float64 e * e + acc, exact in all but a vanishing share of the cases, rounded to float.)"""
    n = render.size
    n4 = n // 4
    mask = (gt > 0) | (render > 0)
    e = np.where(mask, render - gt, np.float32(0.0)).astype(np.float32)
    sq = e.astype(np.float64) ** 2
    grp = sq[:4 * n4].reshape(n4, 4)
    acc = np.zeros(n4, dtype=np.float32)
    for k in range(4):
        acc = (grp[:, k] + acc.astype(np.float64)).astype(np.float32)
    sums = np.concatenate([acc.astype(np.float64), sq[4 * n4:].astype(np.float32).astype(np.float64)])
    d = render.astype(np.float64) - gt.astype(np.float64)
    ex = np.where(mask, d * d, 0.0)
    exact = np.concatenate([ex[:4 * n4].reshape(n4, 4).sum(axis=1), ex[4 * n4:]])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.where(exact > 0, np.abs(sums - exact) / (U * exact), 0.0).max() if exact.size else 0.0
    return int(mask.sum()), float(sums.sum()), (np.float32(2.0) * e).astype(np.float32), float(worst)


def s_deviation_u(S, S64):
    """|S - S64| in units of 2^-24 x S64 (0 for an empty mask, where both are 0)."""
    S, S64 = np.asarray(S, dtype=np.float64), np.asarray(S64, dtype=np.float64)
    assert np.all((S64 > 0) | (S == 0))
    return np.where(S64 > 0, np.abs(S - S64) / (U * np.where(S64 > 0, S64, 1.0)), 0.0)
