"""The device link table (rt_linktable_*, link_kernels.hip) against the dict
model of tests/link_helpers.py: tables of 8, 64 and 4096 slots, batches of 0,
1, 63, 64, 65, 255, 256 and 257 items, probe chains built on purpose (2, 3 and
a wave's worth of ids on one home slot, a chain that wraps past the last
slot), ids that agree in the hashed bytes only and in the others only, all-zero
and all-0xFF ids, duplicates within and across batches, removal in the middle
of a chain, re-insertion, the reclaim forced on the 8-slot table, and a full
table."""
import numpy as np
import pytest

import link_helpers as lh

pytestmark = pytest.mark.gpu

BATCHES = (0, 1, 63, 64, 65, 255, 256, 257)


def _ids(rng, n):
    return [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(n)]


class Pair:
    """A device table and its model, driven together and compared at every step."""

    def __init__(self, max_links):
        import reticulum_amd as rt
        self.tab = rt.LinkTable(max_links, device=0)
        self.model = lh.TableModel(max_links)
        assert self.tab.capacity == self.model.capacity

    def insert(self, ids, values):
        want = self.model.insert(ids, values)
        got = self.tab.insert(ids, values).cpu().tolist() if ids else []
        assert got == want
        return got

    def remove(self, ids):
        want = self.model.remove(ids)
        got = self.tab.remove(ids).cpu().tolist() if ids else []
        assert got == want
        return got

    def check(self, ids):
        if not ids:
            return
        values, found = self.tab.lookup(ids)
        want_v, want_f = self.model.lookup(ids)
        assert found.cpu().tolist() == want_f and values.cpu().tolist() == want_v
        assert len(self.tab) == len(self.model)


@pytest.mark.parametrize("n", BATCHES)
def test_insert_lookup_remove_at_batch_edges(n):
    import reticulum_amd as rt
    rng = np.random.Generator(np.random.PCG64(300 + n))
    p = Pair(2048)
    ids, others = _ids(rng, n), _ids(rng, n)
    if n == 0:
        tab = rt.LinkTable(4, device=0)
        import torch
        e8, e32 = torch.empty((0, 16), dtype=torch.uint8, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda")
        assert tab.insert(e8, e32).numel() == 0 and tab.remove(e8).numel() == 0
        assert tab.lookup(e8)[0].numel() == 0 and len(tab) == 0
        return
    assert p.insert(ids, list(range(100, 100 + n))) == [lh.OK] * n
    p.check(ids)                         # whole waves of hits
    p.check(others)                      # whole waves of misses
    p.check([x for pair in zip(ids, others) for x in pair])
    # across batches: every id again is a duplicate and keeps its first value
    assert p.insert(ids, [7] * n) == [lh.DUPLICATE] * n
    p.check(ids)
    # remove every other one, then all: the second time those are missing
    p.remove(ids[::2])
    p.check(ids)
    got = p.remove(ids)
    assert got.count(lh.OK) == n // 2
    p.check(ids + others)
    # the removed ids can be entered again, with new values
    assert p.insert(ids, list(range(5000, 5000 + n))) == [lh.OK] * n
    p.check(ids)


@pytest.mark.parametrize("max_links", [4, 32, 2048])
@pytest.mark.parametrize("chain", [2, 3, 64])
def test_chains_on_one_home_slot(max_links, chain):
    cap = lh.capacity(max_links)
    chain = min(chain, max_links)
    rng = np.random.Generator(np.random.PCG64(cap + chain))
    # the last slot is the home: every chain of two or more wraps past it
    for home in (1, cap - 1):
        p = Pair(max_links)
        ids = lh.ids_for_home(rng, cap, home, chain)
        assert p.insert(ids, list(range(chain))) == [lh.OK] * chain
        p.check(ids)
        # remove in the middle of the chain: its tail is still found
        mid = ids[len(ids) // 2 - (1 if chain == 2 else 0)]
        assert p.remove([mid]) == [lh.OK]
        p.check(ids)
        absent = lh.ids_for_home(rng, cap, home, 3)
        p.check(absent)
        # re-insert with a new value; the others keep theirs
        assert p.insert([mid], [900]) == [lh.OK]
        p.check(ids + absent)


def test_ids_that_agree_in_part_and_extreme_ids():
    rng = np.random.Generator(np.random.PCG64(16))
    p = Pair(32)
    cap = 64
    # equal in the hashed bytes (home and tag, bytes 0..7), different only in the others
    same_hash = lh.ids_for_home(rng, cap, 5, 4, tag=b"\xAA\xBB\xCC\xDD")
    same_hash = [same_hash[0][:8] + x[8:] for x in same_hash]
    # and the reverse: bytes 8..15 equal, the hashed bytes different
    same_tail = [x[:8] + same_hash[0][8:] for x in _ids(rng, 4)]
    special = [bytes(16), b"\xFF" * 16, bytes(15) + b"\x01", b"\xFF" * 15 + b"\xFE"]
    ids = same_hash + same_tail + special
    assert len(set(ids)) == len(ids)
    assert p.insert(ids[::2], list(range(0, len(ids), 2))) == [lh.OK] * (len(ids) // 2)
    p.check(ids)                          # the odd ones are misses next to near-equal hits
    assert p.insert(ids, list(range(50, 50 + len(ids)))) == [lh.DUPLICATE, lh.OK] * (len(ids) // 2)
    p.check(ids)
    assert p.remove([bytes(16), b"\xFF" * 16]) == [lh.OK, lh.OK]
    p.check(ids)


@pytest.mark.parametrize("n", [65, 257, 1024])
def test_duplicates_inside_one_batch_lowest_index_wins(n):
    """The copies of an id sit on lanes of different waves and workgroups; the
    value that stays is that of the lowest index, every time."""
    rng = np.random.Generator(np.random.PCG64(n))
    base = _ids(rng, 5)
    for rep in range(3):
        p = Pair(2048)
        pick = rng.integers(0, 5, n)
        pick[n - 1] = pick[0]            # first and last item: first wave and last workgroup
        ids = [base[k] for k in pick]
        values = list(range(1000 * rep, 1000 * rep + n))
        got = p.insert(ids, values)
        assert got.count(lh.OK) == len(set(ids))
        p.check(base)
        # removal alike: the lowest index of each id reports it
        got = p.remove(ids)
        assert got.count(lh.OK) == len(set(ids)) and got[0] == lh.OK
        p.check(base)


def test_churn_on_the_8_slot_table_forces_the_reclaim():
    """4 live links at most, 40 rounds of removing two and entering two new
    ones: 80 removals leave their mark in 8 slots, so the table is rebuilt many
    times over, and nobody notices."""
    rng = np.random.Generator(np.random.PCG64(8))
    p = Pair(4)
    live = _ids(rng, 4)
    assert p.insert(live, [0, 1, 2, 3]) == [lh.OK] * 4
    gone = []
    for r in range(40):
        out, live = live[:2], live[2:]
        assert p.remove(out) == [lh.OK, lh.OK]
        gone += out
        new = _ids(rng, 2)
        assert p.insert(new, [10 * r, 10 * r + 1]) == [lh.OK, lh.OK]
        live += new
        p.check(live + gone[-6:])
    # a table of nothing but removed entries: every probe ends, with a miss
    assert p.remove(live) == [lh.OK] * 4
    p.check(live + gone[:8])
    assert len(p.tab) == 0


def test_insert_into_a_full_table():
    rng = np.random.Generator(np.random.PCG64(88))
    p = Pair(4)
    ids = _ids(rng, 8)
    assert p.insert(ids[:5], [1, 2, 3, 4, 5]) == [lh.OK] * 5       # past max_links, still room
    assert p.insert(ids[5:], [6, 7, 8]) == [lh.OK] * 3
    more = _ids(rng, 65)
    # known ids are duplicates even now; new ones find no slot; the call returns
    assert p.insert(more + ids[:2], [9] * 67) == [lh.FULL] * 65 + [lh.DUPLICATE] * 2
    p.check(ids + more)
    assert len(p.tab) == 8
    # room again after a removal
    assert p.remove([ids[3]]) == [lh.OK]
    assert p.insert(more[:1], [77]) == [lh.OK]
    p.check(ids + more)


def test_host_forms_agree_with_the_device_forms():
    from reticulum_amd import _native
    rng = np.random.Generator(np.random.PCG64(4))
    lib, ctx = _native.load(), _native.context(0)
    tab = lib.rt_linktable_create(ctx, 32)
    assert tab and lib.rt_linktable_capacity(tab) == 64
    n = 65
    ids = np.frombuffer(b"".join(_ids(rng, n - 1)) + bytes(16), dtype=np.uint8).copy()
    ids[16 * 64:16 * 65] = ids[0:16]                     # the last item repeats the first
    values = np.arange(n, dtype=np.uint32)
    status = np.full(n, -1, dtype=np.int32)
    _native.check(lib.rt_linktable_insert_host(tab, ids.ctypes.data, values.ctypes.data, status.ctypes.data, n))
    assert status.tolist() == [0] * 64 + [1]
    out, found = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    _native.check(lib.rt_linktable_lookup_host(tab, ids.ctypes.data, out.ctypes.data, found.ctypes.data, n))
    assert found.tolist() == [1] * n and out.tolist() == list(range(64)) + [0]
    _native.check(lib.rt_linktable_remove_host(tab, ids.ctypes.data, status.ctypes.data, n))
    assert status.tolist() == [0] * 64 + [3]
    _native.check(lib.rt_linktable_lookup_host(tab, ids.ctypes.data, out.ctypes.data, found.ctypes.data, n))
    assert not found.any() and (out == 0xFFFFFFFF).all()
    assert lib.rt_linktable_insert_host(tab, None, values.ctypes.data, status.ctypes.data, 1) == _native.RT_E_INVAL
    lib.rt_linktable_destroy(tab)
