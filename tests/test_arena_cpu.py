"""The binned arena's capacity check (skelsplat_amd/_arena.py) without a GPU: the rules are host bookkeeping over a few ints in
host memory.  The tests hand the module plain int32 host tensors through its allocator argument and write "the GPU's" pair counts
into them by hand (-1 = not written yet)."""
import pytest
import torch

from skelsplat_amd import _arena as A

V, P = 3, 500


def alloc(n):
    return torch.empty((n,), dtype=torch.int32)


@pytest.fixture
def key():
    """A shape of its own, and no trace of it afterwards (the module's state is per shape and lives as long as the process)."""
    k = ("cpu-test", V, P, 17, 64, 48)
    yield k
    A._BIN_CAP_HINT.pop(k, None), A._BIN_CAP_SEEN.discard(k), A._BIN_PROBE.pop(k, None), A._SYNC_PROBE.pop(k, None)
    A._BIN_ZOMBIES[:] = [t for t in A._BIN_ZOMBIES if t.key != k]


def gpu_writes(ticket, counts):
    ticket.host[:V] = torch.tensor(counts, dtype=torch.int32)


def test_default_capacity_is_the_hint_or_sixteen_pairs_per_gaussian(key):
    assert A.default_capacity(key) == max(4096, 16 * P) == 8000
    assert A.default_capacity(key[:2] + (10,) + key[3:]) == 4096
    A._BIN_CAP_HINT[key] = 123
    assert A.default_capacity(key) == 123
    assert A.begin(key, None, False, False, alloc).cap == 123 and A.begin(key, 77, False, False, alloc).cap == 77


def test_synchronous_counts_are_preset_and_finish_returns_the_largest_view(key):
    t = A.begin(key, None, True, False, alloc)
    assert t.host.shape == (V + 1,) and t.host.tolist() == [-1] * (V + 1) and not t.device
    gpu_writes(t, [5, 900, 7])
    t.host[V] = 10 ** 6      # (the slot behind the views is not a count)
    assert A.finish(t) == 900 and key in A._BIN_CAP_SEEN
    assert key not in A._BIN_CAP_HINT      # check_capacity=True leaves a clean call's arena as it is
    t2 = A.begin(key, None, True, False, alloc)
    assert t2.host is t.host and t2.host.tolist() == [-1] * (V + 1)      # the shape's buffer, preset again
    gpu_writes(t2, [1, 2, 9000])      # more than the default's 8000: the caller redoes with grown(need)
    assert A.finish(t2) == 9000 > t2.cap and A._BIN_CAP_HINT[key] == A.grown(9000) == int(9000 * 1.25) + 1024


def test_unchecked_and_captured_synchronous_calls_leave_the_counts_to_the_callers_device_tensor(key):
    t = A.begin(key, None, False, False, alloc)
    assert t.host is None and t.device and A.finish(t, torch.tensor([9, 9, 9, 9])) is None and key not in A._BIN_CAP_SEEN
    t = A.begin(key, None, True, True, alloc)
    assert t.host is None and t.device and A.finish(t, torch.tensor([3, 11, 4, 0], dtype=torch.int32)) == 11


@pytest.mark.parametrize("given", [None, 5000])
def test_auto_sizes_the_shape_synchronously_once_and_is_lazy_afterwards(key, given):
    t = A.begin(key, given, "auto", False, alloc)
    assert key not in A._BIN_CAP_SEEN and key not in A._BIN_PROBE      # no probe: this call is looked at here and now
    assert t.host is None and t.device      # (the sizing call reads back a tensor of the caller's)
    assert A.finish(t, torch.tensor([100, 4000, 2, 10 ** 6], dtype=torch.int32)) == 4000 and key in A._BIN_CAP_SEEN
    if given is None:
        assert t.cap == 8000 and A._BIN_CAP_HINT[key] == max(8000, int(4000 * 1.5) + 1024) == 8000
    else:
        assert t.cap == 5000 and key not in A._BIN_CAP_HINT      # the caller sized the arena: the shape learns nothing
    t2 = A.begin(key, given, "auto", False, alloc)
    assert A.finish(t2) is None and A._BIN_PROBE[key].pending == [t2] and t2.host.tolist()[:V] == [-1] * V


def test_auto_headroom_exceeds_a_default_that_was_nearly_full(key):
    t = A.begin(key, None, "auto", False, alloc)
    assert A.finish(t, torch.tensor([7000, 1, 1, 0], dtype=torch.int32)) == 7000
    assert A._BIN_CAP_HINT[key] == A.with_headroom(8000, 7000) == int(7000 * 1.5) + 1024 == 11524
    assert A.begin(key, None, "auto", False, alloc).cap == 11524


def test_lazy_probes_are_harvested_oldest_first_only_once_written_and_never_waited_for(key):
    t1, t2, t3 = (A.begin(key, 1000, "lazy", False, alloc) for _ in range(3))
    assert len({t.host.data_ptr() for t in (t1, t2, t3)}) == 3 and A._BIN_PROBE[key].pending == [t1, t2, t3]
    gpu_writes(t1, [1, 2, 3])
    gpu_writes(t2, [4, 5, 6])
    t4 = A.begin(key, 1000, "lazy", False, alloc)      # returns at once: t3's counts are still -1
    st = A._BIN_PROBE[key]
    assert st.pending == [t3, t4] and t4 is t2 and st.free == [t1]      # t1, then t2 looked at; the last one's buffer reused
    assert t4.host.tolist()[:V] == [-1] * V
    t5 = A.begin(key, 1000, "lazy", False, alloc)      # t3 blocks t4 and itself: nothing harvested, the free buffer reused
    assert st.pending == [t3, t4, t5] and t5 is t1 and st.free == []
    gpu_writes(t4, [1, 1, 1])      # (calls complete in order: a written t4 behind an unwritten t3 is not looked at either)
    A.begin(key, 1000, "lazy", False, alloc)
    assert st.pending[:3] == [t3, t4, t5] and len(st.pending) == 4
    gpu_writes(t3, [0, 0, 0])      # a partly written ticket is not harvested
    t3.host[1] = -1
    A.begin(key, 1000, "lazy", False, alloc)
    assert st.pending[0] is t3 and len(st.pending) == 5


def test_lazy_overflow_raises_grows_the_hint_and_forgets_the_shapes_probes(key):
    t1 = A.begin(key, 16, "lazy", False, alloc)
    t2 = A.begin(key, 16, "lazy", False, alloc)
    t3 = A.begin(key, 16, "lazy", False, alloc)
    gpu_writes(t1, [3, 16, 2])      # exactly full is not an overflow
    gpu_writes(t2, [3, 640, 2])
    with pytest.raises(RuntimeError, match="missed entries"):
        A.begin(key, 16, "lazy", False, alloc)
    assert A._BIN_CAP_HINT[key] == int(640 * 1.25) + 1024 == 1824
    assert key not in A._BIN_PROBE and [t for t in A._BIN_ZOMBIES if t.key == key] == [t3]
    t5 = A.begin(key, None, "lazy", False, alloc)      # starts clean, with the grown default
    assert t5.cap == 1824 and A._BIN_PROBE[key].pending == [t5] and A._BIN_PROBE[key].free == []
    assert t5.host.data_ptr() not in {t.host.data_ptr() for t in (t1, t2, t3)}
    gpu_writes(t3, [9999, 9999, 9999])      # a zombie's counts are never looked at again
    gpu_writes(t5, [1, 1, 1])
    A.begin(key, None, "lazy", False, alloc)


def test_the_capacity_a_lazy_ticket_is_judged_by_is_its_own_calls(key):
    t1 = A.begin(key, 100, "lazy", False, alloc)
    gpu_writes(t1, [50, 50, 50])
    t2 = A.begin(key, 40, "lazy", False, alloc)      # harvests t1 (clean at 100) and reuses it with this call's capacity
    assert t2 is t1 and t2.cap == 40
    gpu_writes(t2, [50, 50, 50])
    with pytest.raises(RuntimeError, match="needed 50 .* held 40"):
        A.begin(key, 100, "lazy", False, alloc)


def test_inside_a_capture_a_lazy_call_gets_no_probe_but_harvests_what_has_arrived(key):
    t1 = A.begin(key, 1000, "lazy", False, alloc)
    t2 = A.begin(key, 1000, "lazy", False, alloc)
    gpu_writes(t1, [1, 2, 3])
    tc = A.begin(key, 1000, "lazy", True, alloc)
    assert tc.host is None and not tc.device and A.finish(tc) is None
    assert A._BIN_PROBE[key].pending == [t2] and A._BIN_PROBE[key].free == [t1]
    gpu_writes(t2, [1, 2000, 3])
    A._BIN_CAP_SEEN.add(key)      # ("auto" on a sized shape is lazy)
    with pytest.raises(RuntimeError, match="missed entries"):
        A.begin(key, 1000, "auto", True, alloc)


def test_the_new_modules_import_the_library_table_and_the_shared_base_only():
    """One direction of imports: rasterizer.py imports these modules, none of them imports it (at any level of its code)."""
    import ast
    import os
    pkg = os.path.dirname(A.__file__)
    for name in ("_arena", "_base", "_tuning", "sparse"):
        tree = ast.parse(open(os.path.join(pkg, name + ".py")).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level:
                names = [node.module] if node.module else [a.name for a in node.names]
                assert set(names) <= {"_lib", "_base"}, (name, names)
            elif isinstance(node, (ast.Import, ast.ImportFrom)):
                mods = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module]
                assert not any(m.startswith("skelsplat_amd") for m in mods), (name, mods)
