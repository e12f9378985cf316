"""The device packet hash list and rt_packet_filter (filter_kernels.hip)
against the set model of tests/filter_helpers.py.  Records are forged with
chosen packet_hash bytes; lists of 8 to 4096 hashes; batches of 0, 1, 63, 64,
65, 255, 256, 257 and 1025 packets.  After every step the statuses, the ok
bytes, the rest of the records, the membership of every hash used so far and
the three counts are compared with the model."""
import numpy as np
import pytest

import filter_helpers as fh

pytestmark = pytest.mark.gpu

BATCHES = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
OWN = bytes(range(100, 116))
FOREIGN = bytes(range(200, 216))
PAIRS = ((0, 1), (0, 63), (63, 64), (255, 256), (0, 1024))


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def _hashes(rng, n):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


class Pair:
    """A device list and its model, driven together and compared at every step."""

    def __init__(self, max_hashes):
        import reticulum_amd as rt
        self.lst = rt.PacketHashlist(max_hashes, device=0)
        self.model = fh.ListModel(max_hashes, OWN)
        assert self.lst.capacity == self.model.capacity
        self.own = _t(np.frombuffer(OWN, np.uint8))
        self.known = []

    def filter(self, packets, transit=(), transit_tab=None, stream=None):
        import torch
        want = self.model.filter(packets, transit)
        self.known += [p["packet_hash"] for p in packets]
        before = fh.records(packets)
        fields = _t(before) if packets else torch.empty((0, 96), dtype=torch.uint8, device="cuda:0")
        got = self.lst.filter(fields, self.own, transit=transit_tab, stream=stream)
        if stream is not None:
            stream.synchronize()
        assert got.cpu().tolist() == want
        after = fields.cpu().numpy()
        # a dropped packet's ok is cleared; the rest of every record stays as unpacked
        assert after[:, 0].tolist() == [1 if s == fh.PASS else 0 for s in want]
        assert (after[:, 1:] == before[:, 1:]).all()
        return want

    def check(self, more=()):
        hs = list(dict.fromkeys(self.known + list(more)))
        if hs:
            assert self.lst.contains(hs).cpu().tolist() == self.model.contains(hs)
        assert self.lst.counts() == self.model.counts()


def _mixed(rng, n, pool):
    """n packets of every kind the rules tell apart, hashes drawn from `pool`
    so that some come twice; fields follow from the hash as on the wire."""
    kinds = {}
    out = []
    for _ in range(n):
        h = pool[int(rng.integers(0, len(pool)))]
        if h not in kinds:
            kinds[h] = (int(rng.integers(0, 4)), int(rng.integers(0, 4)),
                        int(rng.choice([0x00, 0x00, 0x00, 0x01, 0x03, 0x05, 0x08, 0x0E, 0xFA, 0xFF, 0x09])),
                        rng.integers(0, 256, 16, dtype=np.uint8).tobytes())
        ptype, dtype, ctx, dest = kinds[h]
        header = int(rng.integers(0, 3))
        out.append(fh.packet(h, ptype, dtype, ctx, int(rng.integers(0, 3)), fh.HEADER_2 if header else fh.HEADER_1,
                             OWN if header < 2 else FOREIGN, dest, ok=int(rng.integers(0, 8) != 0)))
    return out


@pytest.mark.parametrize("n", BATCHES)
def test_mixed_batches_at_batch_edges(n):
    rng = np.random.Generator(np.random.PCG64(1377 + n))
    p = Pair(4096)
    pool = _hashes(rng, max(1, (2 * n) // 3))
    first = _mixed(rng, n, pool)
    got = p.filter(first)
    p.check()
    if n >= 255:
        assert set(got) == {fh.PASS, fh.NO_PACKET, fh.OTHER_TRANSPORT, fh.BAD_ANNOUNCE, fh.HOPS, fh.DUPLICATE}
    # the same packets again: what was remembered is a duplicate now
    p.filter(first)
    p.check()
    p.filter(_mixed(rng, n, pool + _hashes(rng, n)))
    p.check(_hashes(rng, 5))


@pytest.mark.parametrize("max_hashes", [8, 32, 2048])
@pytest.mark.parametrize("chain", [2, 3, 64])
def test_chains_on_one_home_slot(max_hashes, chain):
    cap = fh.capacity(max_hashes)
    chain = min(chain, max_hashes)
    rng = np.random.Generator(np.random.PCG64(cap + chain))
    # the last slot is the home: every chain of two or more wraps past it
    for home in (1, cap - 1):
        p = Pair(max_hashes)
        hs = fh.hashes_for_home(rng, cap, home, chain)
        assert p.filter([fh.packet(h) for h in hs]) == [fh.PASS] * chain
        p.check()
        assert p.filter([fh.packet(h) for h in hs]) == [fh.DUPLICATE] * chain
        # remove in the middle of the chain: its tail is still found
        mid = hs[len(hs) // 2 - (1 if chain == 2 else 0)]
        assert p.lst.remove([mid, mid]).cpu().tolist() == p.model.remove([mid, mid]) == [fh.OK, fh.MISSING]
        absent = fh.hashes_for_home(rng, cap, home, 3)
        p.check(absent)
        want = [fh.PASS if h == mid else fh.DUPLICATE for h in hs]
        assert p.filter([fh.packet(h) for h in hs]) == want
        p.check(absent)


def test_equal_tags_and_extreme_hashes():
    rng = np.random.Generator(np.random.PCG64(32))
    p = Pair(32)
    # equal in home and tag (bytes 0..7), different only in bytes 8..31
    same = fh.hashes_for_home(rng, 64, 5, 6, tag=b"\xAA\xBB\xCC\xDD")
    same = [same[0][:8] + x[8:] for x in same]
    # different only in the last byte, and only in bytes 24..31 (the second half of the compare)
    near = [same[0][:31] + bytes([same[0][31] ^ 1]), same[0][:24] + same[1][24:]]
    special = [bytes(32), b"\xFF" * 32, bytes(31) + b"\x01", b"\xFF" * 31 + b"\xFE"]
    hs = same + near + special
    assert len(set(hs)) == len(hs)
    assert p.filter([fh.packet(h) for h in hs[::2]]) == [fh.PASS] * (len(hs) // 2)
    p.check(hs)                                  # the odd ones are misses next to near-equal hits
    assert p.filter([fh.packet(h) for h in hs]) == [fh.DUPLICATE, fh.PASS] * (len(hs) // 2)
    p.check()
    assert p.lst.remove([bytes(32), b"\xFF" * 32]).cpu().tolist() == p.model.remove([bytes(32), b"\xFF" * 32])
    p.check()


def _with_copies(rng, n, h, at, **kind):
    """n packets of distinct hashes, with hash h at the indices `at`."""
    fill = _hashes(rng, n)
    return [fh.packet(h if i in at else fill[i], **kind) for i in range(n)]


@pytest.mark.parametrize("variant", ["plain", "lower_copy_for_another_transport", "lrproof", "in_transit",
                                     "single_announce", "keepalive"])
def test_one_hash_twice_in_a_batch(variant):
    import reticulum_amd as rt
    rng = np.random.Generator(np.random.PCG64(len(variant)))
    dest = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
    kind = {"lrproof": dict(packet_type=fh.PROOF, destination_type=fh.LINK, context=fh.LRPROOF),
            "in_transit": dict(destination_type=fh.LINK, destination_hash=dest),
            "single_announce": dict(packet_type=fh.ANNOUNCE),
            "keepalive": dict(destination_type=fh.LINK, context=fh.KEEPALIVE)}.get(variant, {})
    transit, tab = (), None
    if variant == "in_transit":
        tab = rt.LinkTable(8, device=0)
        assert tab.insert([dest], [0]).cpu().tolist() == [0]
        transit = {dest}
    p = Pair(4096)
    for lo, hi in PAIRS + ((0, 299),):
        h = _hashes(rng, 1)[0]
        n = hi + 1
        at = set(range(300)) if hi == 299 else {lo, hi}
        packets = _with_copies(rng, n, h, at, **kind)
        if variant == "in_transit":                  # only the copies belong to the carried link
            for i in range(n):
                if i not in at:
                    packets[i]["destination_hash"] = bytes(16)
        if variant == "lower_copy_for_another_transport":
            packets[lo].update(header_type=fh.HEADER_2, transport_id=FOREIGN)
        got = p.filter(packets, transit, tab)
        copies = [got[i] for i in sorted(at)]
        if variant == "plain":
            assert copies == [fh.PASS] + [fh.DUPLICATE] * (len(at) - 1)
        elif variant == "lower_copy_for_another_transport":
            assert copies == [fh.OTHER_TRANSPORT, fh.PASS] + [fh.DUPLICATE] * (len(at) - 2)
        else:
            assert copies == [fh.PASS] * len(at)
        p.check()
        assert p.model.contains([h]) == [0 if variant in ("lrproof", "in_transit") else 1]
    # the whole of it again, in one batch per pair: remembered hashes are duplicates now
    p.filter(_with_copies(rng, 257, p.known[0], {3, 256}, **kind), transit, tab)
    p.check()


@pytest.mark.parametrize("n", [65, 257])
def test_many_copies_inside_one_batch_lowest_index_wins(n):
    """Five hashes with a dozen copies or more each, shuffled over one wave
    plus a lane (65) and one workgroup plus a lane (257): each hash enters
    once, and the filter passes the lowest index of each, every time."""
    rng = np.random.Generator(np.random.PCG64(n))
    d = 5
    base = _hashes(rng, d)
    for rep in range(3):
        pick = np.arange(n) % d
        rng.shuffle(pick)
        pick[n - 1] = pick[0]            # first and last item: first wave and last workgroup
        hs = [base[k] for k in pick]
        assert len(set(hs)) == d
        # through hashlist_add
        p = Pair(4096)
        p.lst.add(hs)
        p.model.add(hs)
        assert p.lst.counts() == p.model.counts() == (d, 0, 0)
        assert p.lst.contains(base).cpu().tolist() == p.model.contains(base) == [1] * d
        # through packet_filter (Pair.filter holds the statuses and the ok bytes to the model's)
        p = Pair(4096)
        want = p.filter([fh.packet(h) for h in hs])
        assert want == [fh.PASS if hs.index(h) == i else fh.DUPLICATE for i, h in enumerate(hs)]
        p.check()
        assert p.model.counts() == (d, 0, 0)


def test_previous_generation_only():
    rng = np.random.Generator(np.random.PCG64(656))
    p = Pair(8)
    hs = _hashes(rng, 5)
    ann = dict(packet_type=fh.ANNOUNCE)
    kinds = [{}, ann, dict(destination_type=fh.LINK), dict(packet_type=fh.ANNOUNCE, destination_type=fh.LINK),
             dict(context=fh.RESOURCE)]
    first = [fh.packet(h, **k) for h, k in zip(hs, kinds)]
    assert p.filter(first) == [fh.PASS] * 5
    p.lst.cull()
    assert p.model.cull()
    p.check()
    assert p.model.contains(hs) == [2] * 5
    # DATA: dropped, not moved.  SINGLE announce: passes, moved.  A rule-3 packet: entered without a lookup.
    assert p.filter(first + first) == [fh.DUPLICATE, fh.PASS, fh.DUPLICATE, fh.BAD_ANNOUNCE, fh.PASS] * 2
    p.check()
    assert p.model.contains(hs) == [2, 1, 2, 2, 1] and p.model.counts() == (2, 5, 0)


def test_packets_that_never_consult_the_list_are_remembered():
    rng = np.random.Generator(np.random.PCG64(1388))
    p = Pair(64)
    kinds = [dict(context=c, destination_type=fh.LINK) for c in sorted(fh.ALWAYS)] + \
            [dict(destination_type=fh.PLAIN), dict(destination_type=fh.GROUP, hops=0)]
    hs = _hashes(rng, len(kinds))
    packets = [fh.packet(h, **k) for h, k in zip(hs, kinds)]
    # each one three times in a batch: all pass, each hash is entered once
    assert p.filter(packets * 3) == [fh.PASS] * (3 * len(kinds))
    p.check()
    assert p.model.counts() == (len(kinds), 0, 0)
    # the same hashes as ordinary packets are duplicates: they were remembered
    assert p.filter([fh.packet(h) for h in hs]) == [fh.DUPLICATE] * len(kinds)
    # dropped by the hop rule and the announce rule: not remembered; ok == 0 records: not looked at
    more = _hashes(rng, 4)
    drops = [fh.packet(more[0], destination_type=fh.PLAIN, hops=1), fh.packet(more[1], destination_type=fh.GROUP, hops=2),
             fh.packet(more[2], packet_type=fh.ANNOUNCE, destination_type=fh.PLAIN), fh.packet(more[3], ok=0),
             fh.packet(hs[0], ok=0)]
    assert p.filter(drops) == [fh.HOPS, fh.HOPS, fh.BAD_ANNOUNCE, fh.NO_PACKET, fh.NO_PACKET]
    p.check()
    assert p.model.contains(more) == [0] * 4


def test_cull_at_its_threshold_and_forgetting():
    rng = np.random.Generator(np.random.PCG64(657))
    p = Pair(8)
    hs = _hashes(rng, 12)
    one = lambda h: [fh.packet(h)]          # noqa: E731
    assert p.filter([fh.packet(h) for h in hs[:4]]) == [fh.PASS] * 4
    p.lst.cull()                             # exactly max_hashes // 2: nothing happens
    assert not p.model.cull()
    p.check()
    assert p.filter(one(hs[4])) == [fh.PASS]
    p.lst.cull()                             # one above: it rotates
    assert p.model.cull()
    p.check()
    assert p.model.counts() == (0, 5, 0)
    assert p.filter(one(hs[0])) == [fh.DUPLICATE]
    p.lst.cull()                             # an empty current generation stays
    assert not p.model.cull()
    assert p.filter([fh.packet(h) for h in hs[5:10]]) == [fh.PASS] * 5
    assert p.filter(one(hs[0])) == [fh.DUPLICATE]
    p.lst.cull()                             # the second rotation forgets hs[0..4]
    assert p.model.cull()
    p.check()
    assert p.filter([fh.packet(h) for h in hs[:2]] + one(hs[5])) == [fh.PASS, fh.PASS, fh.DUPLICATE]
    p.check()


def test_full_generation_passes_counts_overflow_and_resumes_after_the_cull():
    rng = np.random.Generator(np.random.PCG64(88))
    p = Pair(8)
    hs = _hashes(rng, 8)
    assert p.filter([fh.packet(h) for h in hs]) == [fh.PASS] * 8
    p.check()
    # full: new packets pass and are not remembered, each adds one to the overflow count, copies included
    more = _hashes(rng, 65)
    batch = [fh.packet(h) for h in more] + [fh.packet(more[0]), fh.packet(hs[0]), fh.packet(more[1], context=fh.CHANNEL)]
    assert p.filter(batch) == [fh.PASS] * 65 + [fh.PASS, fh.DUPLICATE, fh.PASS]
    p.check()
    assert p.model.counts() == (8, 0, 67)
    p.lst.add(more[:3])
    p.model.add(more[:3])
    p.check()
    p.lst.cull()
    assert p.model.cull()
    assert p.filter([fh.packet(h) for h in more[:6]] * 2) == [fh.PASS] * 6 + [fh.DUPLICATE] * 6
    p.check()
    assert p.model.counts() == (6, 8, 70)
    # a batch with more new hashes than room: all pass, the room is used up, which of them entered is open
    last = _hashes(rng, 70)
    got = p.lst.filter(_t(fh.records([fh.packet(h) for h in last])), p.own)
    assert got.cpu().tolist() == [fh.PASS] * 70
    assert p.lst.counts() == (8, 8, 70 + 68) and int((p.lst.contains(last) == 1).sum()) == 2
    # removal makes room again
    assert p.lst.remove(hs[:1] + more[:1]).cpu().tolist() == [fh.MISSING, fh.OK]
    assert p.lst.filter(_t(fh.records([fh.packet(hs[0])])), p.own).cpu().tolist() == [fh.DUPLICATE]
    assert p.lst.counts() == (7, 8, 138)


def test_a_call_on_another_stream_sees_the_one_before():
    import torch
    rng = np.random.Generator(np.random.PCG64(5))
    p = Pair(4096)
    hs = _hashes(rng, 1025)
    side = torch.cuda.Stream(device="cuda:0")
    for k in range(3):
        part = [fh.packet(h) for h in hs[k * 300:(k + 1) * 300 + 100]]
        p.filter(part, stream=side if k % 2 == 0 else None)      # overlaps the part before by 100
    torch.cuda.synchronize()
    p.check()
    assert p.model.counts() == (1000, 0, 0)


def test_add_reloads_a_saved_list_and_host_forms_agree():
    from reticulum_amd import _native
    rng = np.random.Generator(np.random.PCG64(242))
    p = Pair(2048)
    saved = _hashes(rng, 1025)
    p.lst.add(saved + saved[:65])                 # copies inside the batch enter once
    p.model.add(saved)
    p.check(saved)
    assert p.filter([fh.packet(h) for h in saved[:257]]) == [fh.DUPLICATE] * 257
    lib = _native.load()
    n = 65
    extra = _hashes(rng, n - 1)
    flat = np.frombuffer(b"".join(extra + extra[:1]), dtype=np.uint8).copy()      # the last repeats the first
    _native.check(lib.rt_hashlist_add_host(p.lst.handle, flat.ctypes.data, n))
    p.model.add(extra)
    found = np.zeros(n, dtype=np.uint8)
    _native.check(lib.rt_hashlist_contains_host(p.lst.handle, flat.ctypes.data, n, found.ctypes.data))
    assert found.tolist() == [1] * n
    status = np.full(n, -1, dtype=np.int32)
    _native.check(lib.rt_hashlist_remove_host(p.lst.handle, flat.ctypes.data, n, status.ctypes.data))
    assert status.tolist() == p.model.remove(extra + extra[:1]) == [fh.OK] * 64 + [fh.MISSING]
    p.check(extra)
    assert lib.rt_hashlist_add_host(p.lst.handle, None, 1) == _native.RT_E_INVAL


def test_device_argument_errors():
    import torch
    from reticulum_amd import device
    p = Pair(8)
    fields = torch.zeros((4, 96), dtype=torch.uint8, device="cuda:0")
    status = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError):
        device.packet_filter(p.lst.handle, fields, p.own[:15], status)
    with pytest.raises(ValueError):
        device.packet_filter(p.lst.handle, fields, p.own, status[:3])
    with pytest.raises(ValueError):
        device.packet_filter(p.lst.handle, fields[:, :95], p.own, status)
    with pytest.raises(ValueError):
        device.hashlist_contains(p.lst.handle, fields[:, :32].contiguous(), status)
