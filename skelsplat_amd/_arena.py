"""The capacity check of the binned path's arena (forward_views, `check_capacity`): how large a shape's arena is by default, where a
call's pair counts go, who looks at them when, and what follows.  Host bookkeeping over a few ints in host memory: a call draws
one ticket in front of its launch (`begin`) and hands it back behind it (`finish`).  Shapes are (device, V, P, C, W, H)."""
import time

import torch

_BIN_CAP_HINT = {}     # shape -> arena capacity learned from a sizing call or an overflow
_BIN_CAP_SEEN = set()  # shapes whose arena a synchronous call has sized already ("auto" goes lazy after that)
_BIN_PROBE = {}        # shape -> _Probes: the lazy tickets of the shape
_SYNC_PROBE = {}       # shape -> (pinned int32 tensor, its numpy view): the counts of the synchronous check
_BIN_ZOMBIES = []      # lazy tickets behind an overflowed one (the GPU may still write them: kept alive, never looked at again)
_PROBES_IN_FLIGHT = 1024     # calls of one shape the host may be ahead of the GPU by (36 bytes of pinned memory each)


def default_capacity(shape_key):     # the caller gave none: what the shape has learned, else 16 pairs per Gaussian
    return _BIN_CAP_HINT.get(shape_key, max(4096, 16 * shape_key[2]))


def with_headroom(cap, need):     # behind an "auto" shape's sizing call: later calls go unchecked until the call after them
    return max(cap, int(need * 1.5) + 1024)


def grown(need):     # behind an overflow: the arena of the redone call / of the calls to come
    return int(need * 1.25) + 1024


def _pinned(n):
    return torch.empty((n,), dtype=torch.int32).pin_memory()


class _Ticket:
    """One call's part in the check.  `cap`: the capacity it runs with.  `host`: what goes into `num_rendered_dev` and what
    ForwardState.num_rendered_dev shows -- V + 1 int32 of host memory the device can write (`view`: the same through numpy) -- or
    None: then a device tensor of the caller's if `device` (nobody looks, or the check reads it back), else nothing at all."""
    __slots__ = ("key", "cap", "host", "view", "device", "sync", "headroom")

    def __init__(self, key, cap, host=None, view=None, device=False, sync=False, headroom=False):
        self.key, self.cap, self.host, self.view, self.device, self.sync, self.headroom = key, cap, host, view, device, sync, headroom


class _Probes:
    __slots__ = ("pending", "free")

    def __init__(self):
        self.pending, self.free = [], []      # lazy tickets nobody has looked at yet, oldest first / looked at: to be reused


def begin(shape_key, cap, mode, capturing, alloc=_pinned):
    """The ticket of a binned forward about to be launched.  `cap`: the caller's capacity, None = the shape's default; `mode`: its
    check_capacity; `capturing`: its stream is being captured into a hipGraph; `alloc(n)`: n int32 the device can write."""
    headroom = mode == "auto" and cap is None
    cap = default_capacity(shape_key) if cap is None else int(cap)
    if mode == "lazy" or (mode == "auto" and shape_key in _BIN_CAP_SEEN):
        return _lazy_probe(shape_key, cap, capturing, alloc)
    if mode is True and not capturing:
        return _Ticket(shape_key, cap, *_sync_counts(shape_key, alloc), sync=True)
    return _Ticket(shape_key, cap, device=True, sync=bool(mode), headroom=headroom)


def finish(ticket, counts=None):
    """Behind the launch: the pairs per view the call needed, or None = not looked at (a lazy ticket: a later `begin` of the shape
    does; an unchecked one: nobody).  `counts`: the caller's tensor of a `device` ticket (read back: a host synchronisation).  A
    measured need marks the shape sized and may move its default; the caller redoes a call that needed more than `ticket.cap`."""
    if not ticket.sync:
        return None
    need = _wait_counts(ticket) if ticket.view is not None else int(counts[:ticket.key[1]].max().item())
    _BIN_CAP_SEEN.add(ticket.key)
    if need > ticket.cap:
        _BIN_CAP_HINT[ticket.key] = grown(need)
    elif ticket.headroom:
        _BIN_CAP_HINT[ticket.key] = with_headroom(ticket.cap, need)
    return need


def _sync_counts(shape_key, alloc=_pinned):
    hit = _SYNC_PROBE.get(shape_key)
    if hit is None:
        host = alloc(shape_key[1] + 1)
        hit = _SYNC_PROBE[shape_key] = (host, host.numpy())
    hit[1][:] = -1      # "not written yet" (_wait_counts)
    return hit


def _wait_counts(ticket):
    """check_capacity=True: the pair counts of the call just enqueued.  The reference reads them back with a blocking copy between
    its scan and its duplication kernels (rasterizer_impl.cu:283-288).  Here k_bin_scan stores them straight into pinned host
    memory ~30 us into the launch sequence and the host spins on THAT -- not on the stream: it has the counts long before the
    forward's compositor is through (0.4 ms on the stress scene), returns, and the caller's next launches queue up behind the
    running forward.  The check stays synchronous and exact (an arena that was too small is grown and the forward redone before
    anything is returned); what it no longer costs is the idle GPU between two calls (bench.py stress: default mode vs "auto")."""
    (dev_index, V, *_), view = ticket.key, ticket.view
    t0 = time.perf_counter()
    while int(view[:V].min()) < 0:
        if time.perf_counter() - t0 > 0.2:      # (counts that never arrive: wait for the stream, look once more)
            torch.cuda.current_stream(dev_index).synchronize()
            if int(view[:V].min()) < 0:
                raise RuntimeError("skelsplat_amd: the binned forward's pair counts did not reach the host")
            break
    return int(view[:V].max())


def _lazy_probe(shape_key, cap, capturing, alloc=_pinned):
    """The lazy capacity check: never synchronises.  A probed call hands sks_forward a pinned int32 buffer as `num_rendered_dev`;
    k_bin_scan stores the call's pair counts there (device-visible host memory: a V-int store, no copy launch, no event).  Called
    in front of every lazy call of the shape: looks at the tickets of EARLIER calls that the GPU has been through by now (they
    complete in call order; -1 = not written yet), raises if one of them needed more pairs than its arena held -- that image
    missed entries; the arena has been grown for the calls to come --, and returns this call's ticket: EVERY eager call is
    probed (the host runs hundreds of microseconds ahead of the GPU on this path, so up to _PROBES_IN_FLIGHT tickets wait to be
    looked at; waiting for the previous call's counts, as an earlier version did, stalled every step); without a buffer only
    inside a capture.  The gradients of an overflowed call are NaN (k_geom_bwd_binned)."""
    V = shape_key[1]
    st = _BIN_PROBE.get(shape_key)
    if st is None:
        st = _BIN_PROBE[shape_key] = _Probes()
    pending = st.pending
    while pending and int(pending[0].view[:V].min()) >= 0:
        seen = pending.pop(0)
        pneed = int(seen.view[:V].max())
        st.free.append(seen)
        if pneed > seen.cap:
            _BIN_CAP_HINT[shape_key] = grown(pneed)
            _BIN_ZOMBIES.extend(pending)
            del _BIN_PROBE[shape_key]
            raise RuntimeError(f"skelsplat_amd: a previous binned forward of this shape needed {pneed} (Gaussian, tile) pairs "
                               f"per view but its arena held {seen.cap}: that image missed entries.  The arena has been grown; "
                               "call again (check_capacity=True checks every call synchronously).")
    if capturing:
        return _Ticket(shape_key, cap)
    if len(pending) >= _PROBES_IN_FLIGHT:     # (never reached by a loop that synchronises now and then: every call is probed)
        torch.cuda.synchronize()
        return _lazy_probe(shape_key, cap, capturing, alloc)
    if st.free:
        ticket = st.free.pop()
        ticket.cap = cap
    else:
        host = alloc(V + 1)
        ticket = _Ticket(shape_key, cap, host, host.numpy())
    ticket.view[:V] = -1
    pending.append(ticket)
    return ticket
