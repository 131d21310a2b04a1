"""CPU tests of the masked-L2 cases (tests/masked_l2_cases.py): every case reaches the loop trips of k_masked_l2 it is there for
-- from the library's own launch shape, sks_masked_l2_launch, a host-only query --, the kernel's arithmetic restated in numpy
stays inside the counted allowance on every case, and the slips the GPU tests exist to catch do fail their checks while the
sums the training loops look at do not move.  No GPU."""
import numpy as np
import pytest

from tests import guarded
from tests import masked_l2_cases as mc


@pytest.fixture(scope="module")
def launch():
    from skelsplat_amd import _lib
    return _lib.masked_l2_launch


@pytest.mark.parametrize("name", list(mc.CASES))
def test_every_case_reaches_its_regime(launch, name):
    V, n = mc.CASES[name]
    blocks, threads = launch(n)
    assert threads == 1024 and 1 <= blocks <= 256
    got = mc.regime(blocks, threads, n)
    print(f"{name}: V {V}, n {n}: {got}")
    assert got == mc.REGIMES[name]


def test_the_cases_are_the_ones_the_kernel_can_go_wrong_at(launch):
    blocks, threads = launch(mc.CASES["main"][1])
    stride = blocks * threads
    assert mc.CASES["edge0"][1] // 4 == 3 * stride and mc.CASES["edge1"][1] // 4 == 3 * stride + 1
    V, n = mc.CASES["main"]
    assert V == 2 and n % 2 == 1 and n % 4 == 3                       # view 1 starts three floats past a 16-byte boundary
    assert mc.CASES["one_block"][1] % 4 == 2 and mc.CASES["one_block"][0] == 3      # views at phases 0, 2, 0
    assert max(V * n for V, n in mc.CASES.values()) <= 7_400_000      # the largest array of the suite's masked-L2 tests
    assert launch(0) == (0, 0) and launch(1) == (1, 1024) and launch(4 * 1024 + 4) == (2, 1024)
    # the phase triples: all four where the three pointers agree, at least four where dL alone differs
    same = [t for t in mc.PHASE_TRIPLES if t[0] == t[1] == t[2]]
    dl = [t for t in mc.PHASE_TRIPLES if t[0] == t[1] != t[2]]
    assert sorted(same) == [(p, p, p) for p in guarded.PHASES] and len(dl) >= 4


def test_inputs_are_what_the_cases_state():
    r, g = mc.make_inputs("remainder")
    assert r.dtype == g.dtype == np.float32 and r.shape == g.shape == mc.CASES["remainder"]
    assert -0.5 <= r.min() < -0.4 and 1.4 < r.max() <= 1.5 and -0.25 <= g.min() < -0.2 and 0.9 < g.max() <= 1.0
    assert abs((r == 0).mean() - 0.4) < 0.01 and abs((g == 0).mean() - 0.5) < 0.01
    assert not np.signbit(r[r == 0]).any() and not np.signbit(g[g == 0]).any()
    assert np.abs(r[r != 0]).min() >= np.float32(1e-3) and np.abs(g[g != 0]).min() >= np.float32(1e-3)
    N, S64, dL = mc.reference(r, g)
    # P(render > 0) = 0.6 x 0.75, P(gt > 0) = 0.5 x 0.8: 67 % of the elements are in the mask, 33 % are not
    assert 0.66 * r.shape[1] < N.min() and N.max() < 0.68 * r.shape[1]
    assert not np.signbit(dL[dL == 0]).any()
    r2, g2 = mc.make_inputs("remainder")
    assert np.array_equal(r, r2) and np.array_equal(g, g2)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_restated_arithmetic_stays_within_the_allowance(name):
    """The kernel's arithmetic in numpy against the float64 reference: N and the gradient's bits equal, every 16-byte group within
    the counted 6u of its own sum, the view's S within S_BAR_U = 8u of S64."""
    r, g = mc.make_inputs(name)
    N, S64, dL = mc.reference(r, g)
    for v in range(r.shape[0]):
        n_, S, d, worst = mc.restated(r[v], g[v])
        dev = float(mc.s_deviation_u(S, S64[v]))
        print(f"{name} view {v}: restated S off by {dev:.2e} u, worst single group {worst:.2f} u")
        assert n_ == N[v]
        assert np.array_equal(d.view(np.int32), dL[v].view(np.int32))
        assert worst <= 6.0 and dev <= mc.S_BAR_U


def test_a_dropped_group_fails_the_bits_and_moves_neither_sum():
    """The slip the loop tests cannot see: one 16-byte group of dL left unwritten (or written as zeros) in `main`.  N and S come
    from the loads, so they stay inside their bars; the bit comparison and the guard check fail.  Had the LOADS skipped the group
    too, S would move by ~21u, past the bar of 8."""
    r, g = mc.make_inputs("main")
    N, S64, dL = mc.reference(r, g)
    n = r.shape[1]
    n_, S, d, _ = mc.restated(r[1], g[1])
    k = 3 * 256 * 1024 + 17                      # a group of the single unrolled trip's fourth store
    assert d[4 * k:4 * k + 4].any()
    slipped = d.copy()
    slipped[4 * k:4 * k + 4] = 0.0
    assert n_ == N[1] and mc.s_deviation_u(S, S64[1]) <= mc.S_BAR_U
    assert not np.array_equal(slipped.view(np.int32), dL[1].view(np.int32))
    for phase in guarded.PHASES:
        buf = np.full(guarded.buffer_floats(n), guarded.SENTINEL, dtype=np.int32)
        buf[guarded.interior(phase, n)] = d.view(np.int32)
        guarded.check("whole", buf, phase, n, dL[1].view(np.int32))
        buf[guarded.GUARD + phase + 4 * k:guarded.GUARD + phase + 4 * k + 4] = guarded.SENTINEL      # never written
        with pytest.raises(AssertionError, match="4 elements of the range were never written"):
            guarded.check("dropped", buf, phase, n, dL[1].view(np.int32))
        buf[guarded.interior(phase, n)] = d.view(np.int32)
        buf[guarded.GUARD + phase + 4 * k - 4:guarded.GUARD + phase + 4 * k] = d[4 * k:4 * k + 4].view(np.int32)   # misplaced
        buf[guarded.GUARD + phase + 4 * k:guarded.GUARD + phase + 4 * k + 4] = guarded.SENTINEL
        with pytest.raises(AssertionError):
            guarded.check("misplaced", buf, phase, n, dL[1].view(np.int32))
    # the loads skipping the group as well: S leaves its bar
    d64 = r[1, 4 * k:4 * k + 4].astype(np.float64) - g[1, 4 * k:4 * k + 4].astype(np.float64)
    m = (g[1, 4 * k:4 * k + 4] > 0) | (r[1, 4 * k:4 * k + 4] > 0)
    lost = float((d64 * d64)[m].sum())
    mean_group = S64[1] / (n // 4)
    print(f"a mean group of main is {mean_group / (mc.U * S64[1]):.1f} u of S, this one {lost / (mc.U * S64[1]):.1f} u")
    assert mean_group / (mc.U * S64[1]) > 2 * mc.S_BAR_U
