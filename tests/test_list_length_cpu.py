"""The list-length cases (tests/list_length_cases.py) are what they say, without a device: every case's claims about its tile
lists hold on the oracle; the set claims every row of the binned path's sorter table, both sides of every threshold; the library
answers the list-regime query on the host; and the compiled reference (oracle/_ref, where the channel count has a build) agrees
with the oracle on every case -- forward bit for bit, backward at the standing tolerance."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import geometry_cases as G, list_length_cases as LC, ref_cases
from skelsplat_amd import _lib


def test_list_regime_answers_without_a_device():
    r = _lib.list_regime()
    assert set(r) == set(_lib.LIST_REGIME_FIELDS)
    assert 0 < r["wave_sort"] <= 64 < r["wave_k"] < r["sort_lds"] and r["wave_k"] % 64 == 0
    assert r["sort_lds"] & (r["sort_lds"] - 1) == 0, "the LDS network's capacity is a power of two"
    assert r["long_list"] > 0 and r["classes"] > 1 and r["band_threads"] % 64 == 0
    assert r["wave_k"] < 1 << (r["classes"] - 1) or r["classes"] == 8
    out = (_lib._i * _lib.LIST_REGIME_INTS)(*([-1] * _lib.LIST_REGIME_INTS))
    assert _lib.load().sks_list_regime(out) == 0 and list(out)[len(r):] == [0] * (_lib.LIST_REGIME_INTS - len(r))
    assert _lib.load().sks_list_regime(None) != 0 and b"out must be provided" in _lib.load().sks_last_error()


def test_the_set_covers_every_regime():
    """Every row of the table in tests/list_length_cases.py, both sides of each threshold and both sides of the long-tile count,
    is claimed by a case (and test_case_is_what_it_says holds every claim to the oracle)."""
    r = LC.regime()
    ws, wk, lds, ll = r["wave_sort"], r["wave_k"], r["sort_lds"], r["long_list"]
    rows = set()
    for name in LC.names():
        rows |= LC.claimed_rows(LC.get(name))
    need = {"load", "wave", "wave-whole", "wave-partial", "lds", "lds-pow2", "lds-padded", "global", "remembered", "walk"}
    need |= {f"wave-k{k}" for k in range(2, wk // 64 + 1)}
    need |= {f"len={n}" for t in (ws, wk, lds) for n in (t, t + 1)}
    need |= {f"nlong={ll}", f"nlong={ll + 1}"}
    need |= {f"class-{k}" for k in range(r["classes"])}
    need |= {f"ties-{x}" for x in ("wave", "lds", "global")}
    need |= {f"saturate-{h}-{x}" for h in ("upper", "lower") for x in ("lds", "global")}
    assert need <= rows, sorted(need - rows)
    # the long ladder scene in every channel form, and more than 2**11 entries far beyond the LDS network's capacity
    assert {n.split("-")[0] for n in LC.names()} >= {"onehot17", "dense17", "dense32", "extras", "nofeat"}
    assert max(LC.ladder_lengths()) > lds + lds // 4
    assert LC.rows_of(ws) == {"load"} and "wave" in LC.rows_of(ws + 1) and "lds" in LC.rows_of(wk + 1) and LC.rows_of(lds + 1) == {"global"}


@functools.lru_cache(maxsize=None)
def _forward(name):
    c = LC.get(name)
    return c, G.oracle_forward(c, 0)


@pytest.mark.parametrize("name", LC.names())
def test_case_is_what_it_says(name):
    c, o = _forward(name)
    G.check_claims(c)
    got = LC.check_lists(c, o)
    print(f"{name}: {got}")
    assert G.host_bytes(c) <= 64 << 20


@pytest.mark.parametrize("make", list(LC.clamp_cases().values()) + [LC.one_call_case], ids=list(LC.clamp_cases()) + ["one-call"])
def test_the_further_scenes_are_what_they_say(make):
    c = make()
    G.check_claims(c)
    o = G.oracle_forward(c, 0)
    LC.check_lists(c, o)
    if c.clamp:
        assert (o["color"] > 1).mean() > 0.02 and (o["color"] < 0).mean() > 0.02, "the clamp does not bite on both sides"


@pytest.mark.parametrize("seed", range(600, 640))
def test_fuzz_cases_keep_their_claims(seed):
    c = LC.fuzz_case(seed)
    LC.check_lists(c, G.oracle_forward(c, 0))


# ------------------------------------------------------------------------------------------------------------
# the compiled reference
# ------------------------------------------------------------------------------------------------------------
def _ref_case(c):
    dLc, dLi = G.draw_dL(c)
    c.dL_color, c.dL_inv = dLc, dLi if dLi is not None else np.zeros((c.V, 1, c.H, c.W), np.float32)
    return ref_cases.RefCase(c.name, c, bg=c.bg, use_inv=dLi is not None, extreme=c.bound)


@pytest.mark.parametrize("name", LC.names())
def test_the_compiled_reference_agrees_with_the_oracle(name):
    """Forward bit for bit (ranges and point_list: the reference's one stable radix sort against the order the oracle states),
    backward within the standing tolerance.  A case of a channel count the reference has no build of is left to the oracle."""
    from oracle import ref as ref_mod
    c, o = _forward(name)
    if c.C not in ref_mod.CHANNELS:
        assert name.startswith("dense32"), f"{name}: C = {c.C} has no build of the reference"
        return
    ref = ref_cases.compiled_reference()
    rc = _ref_case(c)
    r = rc.forward(ref)
    for k in ref_cases.FORWARD_EXACT:
        assert np.array_equal(o[k], r[k]), f"{name}: {k} differs from the compiled reference in {(o[k] != r[k]).sum()} places"
    assert o["R"] == r["R"]
    ratios = ref_cases.grad_ratios(rc, rc.backward(ref, r), rc.backward(orc, o, bounds=rc.extreme))
    print(f"{name}: observed / allowed " + ", ".join(f"{k[3:]} {v:.3f}" for k, v in ratios.items()))
