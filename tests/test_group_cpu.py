"""The schedule of an accumulation group (skelsplat_amd/_group.py) against a literal walk of the reference's loop
(train.py:136-138, 212): for it in 1..N: view = (it - 1) % V; the optimiser steps when it % accumulation_steps == 0."""
import ctypes

import pytest

from skelsplat_amd._group import next_group

VIEWS = (1, 2, 3, 4, 5, 8, 31, 64)
ACC_STEPS = (1, 2, 3, 4, 5, 8, 31, 62)


def _walk(start, N, acc, V):
    """The groups the reference's loop forms over iterations start + 1 .. N: [(views in iteration order, stepping iteration)]."""
    groups, views = [], []
    for it in range(start + 1, N + 1):
        views.append((it - 1) % V)
        if it % acc == 0:
            groups.append((tuple(views), it))
            views = []
    assert not views
    return groups


@pytest.mark.parametrize("V", VIEWS)
def test_schedule_is_the_reference_loop(V):
    """Views, mask, last view, count and end iteration, group for group, from iteration 0 and from every iteration inside the
    first two groups; far enough that every view has been rendered (V = 64: bit 63 of the mask, intact as a C unsigned long long)."""
    for acc in ACC_STEPS:
        for start in range(2 * acc + 1):
            N = -(-(start + max(4 * acc, V)) // acc) * acc
            it, seen = start, 0
            for views, end in _walk(start, N, acc, V):
                g = next_group(it, acc, V)
                mask = 0
                for v in views:
                    mask |= 1 << v
                assert (g.views, g.mask, g.last_view, g.n_iters, g.end) == (views, mask, views[-1], len(views), end), (acc, start, it)
                assert g.key == (mask, views[-1], len(views))
                assert ctypes.c_ulonglong(g.mask).value == g.mask
                seen |= g.mask
                it = g.end
            assert it == N and seen == (1 << V) - 1
            if V == 64:
                assert seen >> 63 == 1


@pytest.mark.parametrize("V", VIEWS)
def test_full_group_key_does_not_depend_on_the_iteration(V):
    """What the graph run relies on: when accumulation_steps is a multiple of V and the iteration a multiple of accumulation_steps,
    the next group is all views, accumulation_steps iterations, whatever the iteration -- one key for every group of a graph."""
    hit = 0
    for acc in ACC_STEPS + (V, 2 * V):
        for it in range(0, 3 * acc + 1):
            if acc % V == 0 and it % acc == 0:
                assert next_group(it, acc, V).key == ((1 << V) - 1, (acc - 1) % V, acc), (acc, it)
                hit += 1
    assert hit >= 8


def test_cut_group_is_the_first_iterations():
    """Early stopping at the k-th iteration of a group (from 0): the first k + 1 iterations, the mask of those views, view k last."""
    for V, acc, start in ((4, 4, 0), (4, 4, 5), (3, 5, 7), (64, 62, 62), (5, 8, 0)):
        g = next_group(start, acc, V)
        for k in range(g.n_iters):
            c = g.cut(k)
            views = tuple((it - 1) % V for it in range(start + 1, start + k + 2))
            assert (c.views, c.last_view, c.n_iters, c.end) == (views, views[-1], k + 1, start + k + 1)
            assert c.mask == sum(1 << v for v in set(views))
        assert g.cut(g.n_iters - 1) == g
