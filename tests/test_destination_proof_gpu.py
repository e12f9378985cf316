"""DestinationReceipts and rt_destination_proof_settle (dproof_kernels.hip)
against the model of tests/destination_proof_helpers.py, which
test_destination_proof.py ties to the reference, and against the fixture's own
verdicts.

Packets are laid out in one device buffer that ends with the last packet and
unpacked by rt_packet_unpack.  Both outputs have guard rows behind them and a
sentinel fill, and the work lists lie inside a larger buffer whose bytes around
them are compared with what they held before the call.  The model's signatures
are cached, so the batches are made of few distinct proofs."""
import functools

import numpy as np
import pytest

import destination_proof_helpers as dp
import link_helpers as lh

pytestmark = pytest.mark.gpu

GUARD = 3
SENTINEL = -77
FILL = 0xA5
PAD = 64                    # bytes kept around the work lists
SIZES = (0, 1, 63, 64, 65, 256, 257)
BIG = 1 << 20


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _world():
    """Two recipients and 64 packet hashes, receipt k under recipient k & 1."""
    rng = np.random.Generator(np.random.PCG64(2349))
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(2)]
    hashes = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(64)]
    elsewhere = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
    return seeds, hashes, elsewhere


def _key(k):
    return dp.public_key(_world()[0][k & 1])


def _proof(k, implicit, **kw):
    """The honest proof of receipt k."""
    seeds, hashes, _ = _world()
    return dp.proof_packet(hashes[k], seeds[k & 1], implicit, **kw)


def _stray(k):
    """An implicit proof of receipt k addressed to no receipt."""
    return _proof(k, True, address=_world()[2])


def _bad(raw):
    b = bytearray(raw)
    b[-1] ^= 0x10           # in S
    return bytes(b)


NOT_PROOF = bytes([lh.SINGLE << 2 | lh.DATA, 0]) + bytes(16) + bytes([0]) + bytes(40)


class Pair:
    """The receipts on the device and in the model, kept in step."""

    def __init__(self, max_receipts, scan_trials=None):
        import reticulum_amd as rt
        self.dev = rt.DestinationReceipts(max_receipts, scan_trials=scan_trials, device=0)
        self.model = dp.Receipts(max_receipts)
        self.trials = self.dev.scan_trials
        assert self.trials == (4 * max_receipts if scan_trials is None else scan_trials)

    def add(self, hashes, ids, keys=None):
        got = self.dev.add(hashes, ids, keys=keys).cpu().numpy().tolist()
        assert got == self.model.add(hashes, ids, keys)
        assert len(self.dev) == len(self.model)
        return got

    def add_world(self, ids, keyed=True):
        _, hashes, _ = _world()
        ids = list(ids)
        return self.add([hashes[k] for k in ids], ids, [_key(k) for k in ids] if keyed else None)

    def remove(self, hashes):
        assert self.dev.remove(hashes).cpu().numpy().tolist() == self.model.remove(hashes)
        assert len(self.dev) == len(self.model)


def _unpack(raws):
    import torch
    from reticulum_amd import device
    n = len(raws)
    lens = np.array([len(r) for r in raws], np.int32)
    offs = 1 + np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]) if n else np.zeros(0, np.int64)
    flat = np.full(int(offs[-1] + lens[-1]) if n else 1, 0x5C, np.uint8)
    for r, o in zip(raws, offs):
        flat[o:o + len(r)] = np.frombuffer(r, np.uint8)
    pkt, off = _dev(flat), _dev(offs.astype(np.int64))
    fields = torch.empty((n, 96), dtype=torch.uint8, device="cuda:0")
    if n:
        device.packet_unpack(pkt, off, _dev(lens), fields)
    return pkt, off, fields


def _settle(pair, raws, links=None, n_links=0, state=None):
    """One call over ``raws``, held to the model: statuses, receipt ids, the
    guard rows, the bytes around the work lists and len().  ``state`` gives the
    buffers of an earlier call to run into again.  Returns (results, state)."""
    import torch
    from reticulum_amd import device
    n = len(raws)
    pkt, off, fields = _unpack(raws)
    if state is None:
        status = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
        receipt = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
        held = torch.full((PAD + pair.dev.work_bytes(n) + PAD,), FILL, dtype=torch.uint8, device="cuda:0")
        state = (status, receipt, held)
    status, receipt, held = state
    need = pair.dev.work_bytes(n)
    pair.dev.work = held[PAD:PAD + need]
    link = None if links is None else _dev(np.asarray(links, np.int32))
    device.destination_proof_settle(pkt, off, fields, pair.dev, status[:n], receipt[:n], link=link, n_links=n_links)
    want = dp.settle([dp.unpack(r) for r in raws], pair.model, pair.trials, links=links, n_links=n_links)
    got = list(zip(status.cpu().numpy().tolist(), receipt.cpu().numpy().tolist()))
    assert got[n:] == [(SENTINEL, SENTINEL)] * GUARD
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got[:n], want)) if g != w]
    assert not wrong, wrong[:8]
    around = held.cpu().numpy()
    assert (around[:PAD] == FILL).all() and (around[PAD + need:] == FILL).all()
    assert len(pair.dev) == len(pair.model)
    return want, state


# ----------------------------------------------------------------- fixture --

def test_fixture_verdicts():
    vec = dp.vectors()
    for one_call in (True, False):
        for b in vec["batches"]:
            pair = Pair(16)
            hashes = [bytes.fromhex(h) for h, _ in b["receipts"]]
            for i, (h, (_, k)) in enumerate(zip(hashes, b["receipts"])):
                key = None if k is None else [bytes.fromhex(vec["identities"][k]["public"])]
                assert pair.add([h], [i], key) == [lh.OK]
            raws = [bytes.fromhex(r) for r in b["raws"]]
            got = _settle(pair, raws)[0] if one_call else [_settle(pair, [r])[0][0] for r in raws]
            assert [hashes[rid].hex() if st == dp.DELIVERED else None for st, rid in got] == b["delivered"], b["note"]
            assert len(pair.dev) == len(b["left"])
            if not one_call:
                break                                   # the per-packet form once: the batch form is the stage's own


def test_host_form_on_the_fixture():
    import reticulum_amd as rt
    vec = dp.vectors()
    (b,) = [b for b in vec["batches"] if "from_deliver" in b]
    r = rt.DestinationReceipts(8, device=0)
    hashes = [bytes.fromhex(h) for h, _ in b["receipts"]]
    r.add(hashes, list(range(len(hashes))), keys=[bytes.fromhex(vec["identities"][k]["public"]) for _, k in b["receipts"]])
    status, receipt = rt.settle_destination_proofs_batch([bytes.fromhex(x) for x in b["raws"]], r)
    assert status.tolist() == [dp.DELIVERED] * 4 and receipt.tolist() == [0, 1, 2, 3] and len(r) == 0
    status, receipt = rt.settle_destination_proofs_batch([], r)
    assert status.shape == receipt.shape == (0,)


# ------------------------------------------------------------- batch edges --

def _filler(i):
    return (NOT_PROOF, _proof(0, False) + b"\x00", _proof(1, True, context=0xFF), _proof(2, True)[:-1])[i % 4]


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes_and_candidate_counts(n):
    R = 8
    # no candidate at all; then every record a candidate, copies of 2 R proofs and R bad ones
    pair = Pair(R)
    pair.add_world(range(R))
    want, _ = _settle(pair, [_filler(i) for i in range(n)])
    assert all(st in (dp.NOT_PROOF, dp.BAD_LENGTH) for st, _ in want) and len(pair.dev) == R
    kinds = [lambda k: _proof(k, False), lambda k: _bad(_proof(k, False)), lambda k: _proof(k, True)]
    want, _ = _settle(pair, [kinds[(i // R) % 3](i % R) for i in range(n)])
    assert sum(st == dp.DELIVERED for st, _ in want) == min(n, R)
    # one candidate alone, on the first and the last lane of a wave and of a workgroup; 64 and 65 of them
    spots = sorted({p for p in (0, 63, 64, 255, 256) if p < n})
    for at in spots:
        pair = Pair(R)
        pair.add_world(range(R))
        raws = [_filler(i) for i in range(n)]
        raws[at] = _proof(at % R, bool(at & 1))
        want, _ = _settle(pair, raws)
        assert want[at] == (dp.DELIVERED, at % R) and len(pair.dev) == R - 1
    for count in (64, 65):
        if count <= n:
            pair = Pair(R)
            pair.add_world(range(R))
            step = n // count
            raws = [_filler(i) for i in range(n)]
            for j in range(count):
                raws[n - 1 - j * step] = _proof(j % R, bool(j & 1))
            want, _ = _settle(pair, raws)
            assert sum(st == dp.DELIVERED for st, _ in want) == R and len(pair.dev) == 0


# ---------------------------------------------------------------- the table --

def test_two_hashes_equal_in_16_bytes():
    seeds, hashes, _ = _world()
    twin = hashes[0][:16] + hashes[1][16:]
    pair = Pair(8)
    assert pair.add([hashes[0], twin, hashes[2]], [0, 1, 2], [_key(0), _key(1), _key(2)]) == \
        [lh.OK, lh.DUPLICATE, lh.OK]
    assert pair.dev.hashes[0].cpu().numpy().tobytes() == hashes[0]          # the earlier entry stays as it was
    assert pair.dev.keys[0].cpu().numpy().tobytes() == _key(0)
    assert pair.dev.keyed.cpu().numpy().tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
    want, _ = _settle(pair, [dp.proof_packet(twin, seeds[1], False), dp.proof_packet(twin, seeds[1], True),
                             dp.proof_packet(twin, seeds[0], False), _proof(0, False), _proof(2, True)])
    assert want == [(dp.NO_RECEIPT, -1)] * 3 + [(dp.DELIVERED, 0), (dp.DELIVERED, 2)]


def test_chain_on_one_home_slot_with_a_removal_inside():
    rng = np.random.Generator(np.random.PCG64(16))
    seeds, _, _ = _world()
    pair = Pair(8)
    heads = lh.ids_for_home(rng, pair.dev.table.capacity, 5, 5)
    hashes = [h + rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for h in heads]
    pair.add(hashes, list(range(5)), [_key(k) for k in range(5)])
    pair.remove([hashes[1]])
    proofs = [dp.proof_packet(h, seeds[k & 1], bool(k & 1)) for k, h in enumerate(hashes)]
    want, _ = _settle(pair, [proofs[4], proofs[1], proofs[3]])
    assert want == [(dp.DELIVERED, 4), (dp.NO_RECEIPT, -1), (dp.DELIVERED, 3)]
    pair.add([hashes[1]], [6], [_key(1)])                   # into a slot a removal left
    want, _ = _settle(pair, [proofs[1], proofs[2], proofs[0], proofs[0]])
    assert want == [(dp.DELIVERED, 6), (dp.DELIVERED, 2), (dp.DELIVERED, 0), (dp.NO_RECEIPT, -1)]
    assert len(pair.dev) == 0


def test_full_table_and_receipts_without_a_key():
    R = 8
    pair = Pair(R)
    pair.add_world([0, 1, 2, 3, 4])
    pair.add_world([5, 6, 7], keyed=False)
    assert pair.dev.keyed.cpu().numpy().tolist() == [1] * 5 + [0] * 3
    raws = [_proof(5, False), _proof(6, True), _stray(7), _stray(4), _proof(0, True), _proof(1, False),
            _bad(_proof(2, False)), _proof(2, False), _proof(3, True)]
    want, _ = _settle(pair, raws)
    assert want == [(dp.NO_RECEIPT, -1)] * 3 + [(dp.DELIVERED, 4), (dp.DELIVERED, 0), (dp.DELIVERED, 1),
                                                (dp.BAD_SIGNATURE, -1), (dp.DELIVERED, 2), (dp.DELIVERED, 3)]
    assert len(pair.dev) == 3
    # only receipts without a key are left: L = 0, every stray NO_RECEIPT whatever the budget
    want, _ = _settle(pair, [_stray(5), _proof(6, True), _stray(0)])
    assert want == [(dp.NO_RECEIPT, -1)] * 3 and len(pair.dev) == 3


# ------------------------------------------------------------------- copies --

@pytest.mark.parametrize("copies", [2, 300])
def test_one_proof_many_times(copies):
    for implicit in (False, True):
        pair = Pair(8)
        pair.add_world(range(3))
        want, _ = _settle(pair, [_proof(1, implicit)] * copies)
        assert want == [(dp.DELIVERED, 1)] + [(dp.NO_RECEIPT, -1)] * (copies - 1) and len(pair.dev) == 2


def test_a_bad_copy_below_a_good_one():
    pair = Pair(8)
    pair.add_world(range(4))
    raws = [_bad(_proof(0, False)), _proof(0, False), _bad(_proof(0, False)),
            _bad(_proof(1, True)), _proof(1, True), _bad(_proof(1, True))]
    want, _ = _settle(pair, raws)
    assert want == [(dp.BAD_SIGNATURE, -1), (dp.DELIVERED, 0), (dp.NO_RECEIPT, -1),
                    (dp.NO_RECEIPT, -1), (dp.DELIVERED, 1), (dp.NO_RECEIPT, -1)]


def test_a_stray_below_and_above_the_addressed_proof():
    pair = Pair(8)
    pair.add_world(range(4))
    raws = [_stray(0), _proof(0, True), _proof(1, True), _stray(1), _stray(2), _proof(2, False), _proof(3, False),
            _stray(3)]
    want, _ = _settle(pair, raws)
    assert want == [(dp.DELIVERED, 0), (dp.NO_RECEIPT, -1), (dp.DELIVERED, 1), (dp.NO_RECEIPT, -1),
                    (dp.DELIVERED, 2), (dp.NO_RECEIPT, -1), (dp.DELIVERED, 3), (dp.NO_RECEIPT, -1)]
    assert len(pair.dev) == 0


# --------------------------------------------------------------- the budget --

@pytest.mark.parametrize("L", [1, 5])
def test_scan_budget_whole_frames_only(L):
    for trials, fit in ((0, 0), (L - 1, 0), (L, 1), (2 * L - 1, 1), (2 * L, 2), (3 * L, 3), (BIG, 4)):
        pair = Pair(8, scan_trials=trials)
        pair.add_world(range(L))
        pair.add_world([6, 7], keyed=False)                 # not counted in L
        # four strays (the third an addressed proof with a bad signature) among proofs that need no scan
        raws = [NOT_PROOF, _stray(L - 1), _proof(0, False) + b"\x00", _stray(0), _bad(_proof(0, True)), _stray(7)]
        want, _ = _settle(pair, raws)
        strays = [want[k][0] for k in (1, 3, 4, 5)]
        assert strays[fit:] == [dp.DEFERRED] * (4 - fit), (trials, want)
        assert dp.DEFERRED not in strays[:fit]
        if fit >= 1:
            assert want[1] == (dp.DELIVERED, L - 1)


def test_an_addressed_proof_costs_no_budget():
    pair = Pair(8, scan_trials=0)
    pair.add_world(range(8))
    want, _ = _settle(pair, [_proof(k, bool(k & 1)) for k in range(8)] + [_stray(0)])
    # the stray is judged against the receipts outstanding at the start of the call: L = 8
    assert want == [(dp.DELIVERED, k) for k in range(8)] + [(dp.DEFERRED, -1)]
    assert len(pair.dev) == 0


# ------------------------------------------------------- links, second call --

def test_on_link_rule():
    pair = Pair(8)
    pair.add_world(range(4))
    on = lambda k, implicit: _proof(k, implicit, dtype=lh.LINK)        # noqa: E731
    raws = [on(0, False), on(1, True), on(2, False), on(3, True), _proof(0, False)]
    # link: in the table and active; in the table, past n_links; not in the table; active; (SINGLE: not asked)
    want, _ = _settle(pair, raws, links=[0, 5, -1, 2, 1], n_links=3)
    assert want == [(dp.ON_LINK, -1), (dp.DELIVERED, 1), (dp.DELIVERED, 2), (dp.ON_LINK, -1), (dp.DELIVERED, 0)]
    want, _ = _settle(pair, [on(3, True)])                              # no link column: no link is active
    assert want == [(dp.DELIVERED, 3)]


def test_a_second_call_into_the_same_buffers():
    pair = Pair(8)
    pair.add_world(range(6))
    first = [_proof(0, False), _stray(1), NOT_PROOF, _bad(_proof(2, False)), _proof(3, True)]
    want, state = _settle(pair, first)
    assert [st for st, _ in want] == [dp.DELIVERED, dp.DELIVERED, dp.NOT_PROOF, dp.BAD_SIGNATURE, dp.DELIVERED]
    assert len(pair.dev) == 3
    second = [_stray(0), _proof(2, False), _proof(1, True), _proof(4, True)[:-1], _stray(5)]
    want, _ = _settle(pair, second, state=state)
    assert want == [(dp.NO_RECEIPT, -1), (dp.DELIVERED, 2), (dp.NO_RECEIPT, -1), (dp.BAD_LENGTH, -1),
                    (dp.DELIVERED, 5)]
    assert len(pair.dev) == 1
    # the object's own work lists grow with the read and are kept between calls
    mine = Pair(8)
    mine.add_world(range(2))
    from reticulum_amd import device
    import torch
    for raws in ([_proof(0, True)], [_proof(1, False)] * 300):
        pkt, off, fields = _unpack(raws)
        st = torch.empty(len(raws), dtype=torch.int32, device="cuda:0")
        rc = torch.empty_like(st)
        device.destination_proof_settle(pkt, off, fields, mine.dev, st, rc)
        assert st.cpu().numpy().tolist()[0] == dp.DELIVERED and mine.dev.work.numel() >= mine.dev.work_bytes(len(raws))
    assert len(mine.dev) == 0
