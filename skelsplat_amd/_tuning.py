"""The forward's fill configuration: the candidates, what has been measured per shape and per kind of caller, and the timing and
picking the tuners share (rasterizer.tune_forward / Workspace.tune issue the calls).  No result bit depends on any of it."""
import torch

from . import _lib

PLAIN_STORES = 0x100     # a tuner candidate's bit 8: plain stores instead of non-temporal ones (SKS_NO_NT_STORES)
# What the tuners try by default: passes per fill block, non-temporal stores -- the kind that streams past the 256 MB Infinity Cache
# at the rate HBM takes writes, whatever buffer it writes.  Plain stores (TUNE_CANDIDATES_WITH_PLAIN, on request) may sit in that
# cache when a call rewrites the same ~cache-sized outputs step after step: the kernel then retires before its bytes are in HBM
# (H36M forward 46 -> 38-41 us) and they drain under whatever runs next -- a cache-assisted figure, not an HBM rate, and 40 %
# slower on outputs beyond the cache's size; round 5 took such candidates at equal step time, which moved the reported kernel
# fraction by 0.15 without moving the step.
TUNE_CANDIDATES = (0, 3, 4, 5)
TUNE_CANDIDATES_WITH_PLAIN = TUNE_CANDIDATES + (PLAIN_STORES | 3, PLAIN_STORES | 4, PLAIN_STORES | 5)
TUNE_CANDIDATES_FRESH = TUNE_CANDIDATES  # outputs in fresh memory every call (the autograd path)
_FILL_BITS = (0xff << 8) | 16            # flag bits a candidate occupies: passes per fill block, SKS_NO_NT_STORES
_FILL_TUNE = {}          # (device, V, P, C, W, H, "workspace" | "fresh") -> flag bits: what forward_views ORs in when the caller sets none
_MEASURING = [False]     # tune_forward is timing candidates: forward_views leaves the flags as given
_FILL_TUNE_LOG = {}      # same key -> {candidate name: median microseconds} of the measurement behind the pick
TUNE_WARM = 12     # untimed calls in front of a tuner's measurement (_time_candidates)


def _tune_flag_bits(c):
    return ((int(c) & 0xff) << 8) | (_lib.SKS_NO_NT_STORES if int(c) & PLAIN_STORES else 0)


def tune_name(c):
    """A tuner candidate in words ("default (2 passes, non-temporal)", "4 passes, plain stores")."""
    if not c:
        return "default (2 passes, non-temporal stores)"
    return f"{int(c) & 0xff or 2} passes, {'plain' if int(c) & PLAIN_STORES else 'non-temporal'} stores"


def _time_candidates(set_bits, step_fn, candidates, reps, rounds, dev_index, warm=None):
    """Interleaved round-robin timing of `step_fn` under every candidate; {candidate: [microseconds per call, one per round]}.
    `warm` untimed calls first: the measurement is host wall time over device synchronisations, and a process's first calls (cold
    Python paths, clocks still ramping) are host-bound at several times the step's GPU time."""
    import time
    set_bits(_tune_flag_bits(candidates[0]))
    for _ in range(TUNE_WARM if warm is None else warm):
        step_fn()
    times = {c: [] for c in candidates}
    for _ in range(rounds):
        for c in candidates:
            set_bits(_tune_flag_bits(c))
            for _ in range(2):
                step_fn()
            torch.cuda.synchronize(dev_index)
            t0 = time.perf_counter()
            for _ in range(reps):
                step_fn()
            torch.cuda.synchronize(dev_index)
            times[c].append(1e6 * (time.perf_counter() - t0) / reps)
    return times


def _pick(times, candidates, set_bits=None, step_fn=None, reps=8, dev_index=None, confirm=True):
    """The candidate to keep, judged by each one's LEAST disturbed round (a host hiccup only ever adds time).  The library's default
    (the first candidate) stays unless another beats it by more than 2 % -- and, when the caller's step can be re-run, beats it
    again in a confirmation measurement (three more interleaved rounds of just the two): a pick made from one noisy process state
    (round 6 saw a cold bench process read 80 / 85 / 76 / 76 us for a 66 us step and choose five passes: 11 % slower) does not survive
    that.  Returns (best, {candidate: least-disturbed microseconds})."""
    low = {c: min(v) for c, v in times.items()}
    best = min(low, key=low.get)
    if best != candidates[0] and low[best] > 0.98 * low[candidates[0]]:
        best = candidates[0]
    if best != candidates[0] and step_fn is not None and confirm:
        again = _time_candidates(set_bits, step_fn, (candidates[0], best), reps, 3, dev_index, warm=0)
        if min(again[best]) > 0.98 * min(again[candidates[0]]):
            best = candidates[0]
    return best, low


def fill_tuning():
    """What has been measured so far: {(device, V, P, C, W, H, kind): (pick in words, {candidate: median us})}."""
    names = {_tune_flag_bits(c): tune_name(c) for c in TUNE_CANDIDATES_WITH_PLAIN}
    return {k: (names.get(v, hex(v)), _FILL_TUNE_LOG.get(k, {})) for k, v in _FILL_TUNE.items()}
