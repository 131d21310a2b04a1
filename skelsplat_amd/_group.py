"""The schedule of an accumulation group (reference: train.py:136-138, 212): iteration `it` renders view (it - 1) % V, and the
optimiser steps at every multiple of `acc_steps`.  Plain integers: no torch, no device."""
from functools import lru_cache
from typing import NamedTuple


class Group(NamedTuple):
    views: tuple        # the views of the group's iterations, in iteration order
    mask: int           # bit v: view v's slot is refreshed
    last_view: int      # its scaling / rotation / opacity gradients win (quirk Q7)
    n_iters: int
    key: tuple          # (mask, last_view, n_iters): what the kernels, and a captured graph, know of a group
    end: int            # the iteration the optimiser steps at

    def cut(self, k):
        """The group that early stopping ends at its k-th iteration (from 0): its first k + 1 iterations, view k last."""
        return Group(*_of(self.views[:k + 1]), self.end - self.n_iters + k + 1)


def _of(views):
    mask = 0
    for v in views:
        mask |= 1 << v
    return views, mask, views[-1], len(views), (mask, views[-1], len(views))


@lru_cache(maxsize=4096)
def _from(first_view, n_iters, V):      # (a loop asks for the same few groups over and over, once per step on a host-bound path)
    return _of(tuple((first_view + k) % V for k in range(n_iters)))


def next_group(iteration, acc_steps, V):
    """The group behind `iteration` (taken at face value; 0: nothing has run): up to the next multiple of `acc_steps`."""
    n = acc_steps - iteration % acc_steps
    return Group(*_from(iteration % V, n, V), iteration + n)
