"""rt_link_prove, the receipt table and rt_proof_settle (proof_kernels.hip)
against the model of tests/proof_helpers.py, which test_proof.py ties to the
reference, and against the fixture's own proof packets.

Packets are laid out in one device buffer that ends with the last packet and
unpacked by rt_packet_unpack; route and link come from the model, the token
status is the test's to choose.  Every output has guard rows behind it and the
proof rows a sentinel fill: rows the call must not write, the 13 bytes behind
every proof included, are compared with what they held before the call."""
import functools

import numpy as np
import pytest

import link_helpers as lh
import proof_helpers as ph
from oracle import ctoken

pytestmark = pytest.mark.gpu

GUARD = 3
SENTINEL = -77
FILL = 0xA5
ROW = 128
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
FLAGS = (ph.PROVE_ALL, ph.HAS_CHANNEL, ph.PROVE_ALL | ph.HAS_CHANNEL, 0, ph.PROVE_ALL)
N_LINKS = len(FLAGS)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rows(rows):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1).copy()


@functools.lru_cache(maxsize=None)
def _world():
    rng = np.random.Generator(np.random.PCG64(378))
    ids = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(N_LINKS)]
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(N_LINKS)]
    return ids, seeds, {i: k for k, i in enumerate(ids)}


def _signers(shared, peer_seeds=None):
    """(device signers, model signers); ``shared``: one seed row for all links."""
    import reticulum_amd as rt
    _, seeds, _ = _world()
    own = seeds[:1] if shared else seeds
    peers = [ph.public_key(s) for s in (peer_seeds or seeds)]
    dev = rt.LinkSigners(_rows(own), _rows(peers), list(FLAGS), device=0)
    assert dev.publics.cpu().numpy().tobytes() == b"".join(ph.public_key(s) for s in own)
    return dev, ph.Signers(own, peers, FLAGS)


def _unpack(raws):
    """(pkt, off, fields) on the device: the packets end to end, one byte in."""
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


def _link_packet(k, ptype, context, data):
    return bytes([lh.LINK << 2 | ptype, 0]) + _world()[0][k] + bytes([context]) + data


# --------------------------------------------------------------- link_prove --

# (link, packet type, context, token status): what the flags of FLAGS prove ...
PROVED = ((0, lh.DATA, lh.NONE, 0), (1, lh.DATA, lh.CHANNEL, 0), (2, lh.DATA, lh.NONE, 0), (2, lh.DATA, lh.CHANNEL, 2),
          (4, lh.DATA, lh.NONE, 0), (1, lh.DATA, lh.CHANNEL, 1))
# ... and what they do not; the last four are given link -1, link n_links, ok = 0 and route LINK_PLAIN
UNPROVED = ((3, lh.DATA, lh.NONE, 0), (0, lh.DATA, lh.NONE, 2), (0, lh.DATA, lh.CHANNEL, 0), (1, lh.DATA, lh.NONE, 0),
            (2, lh.DATA, lh.KEEPALIVE, 0), (2, lh.PROOF, lh.CHANNEL, 0), (2, lh.PROOF, lh.NONE, 0),
            (4, lh.DATA, lh.REQUEST, 0), (0, lh.DATA, lh.NONE, 0), (2, lh.DATA, lh.CHANNEL, 0), (4, lh.DATA, lh.NONE, 0),
            (0, lh.DATA, lh.NONE, 0))


def _records(pattern):
    """One record per flag of ``pattern`` (True: a packet the links prove).
    Eight payloads per kind, so that the model signs each hash once."""
    recs = []
    for i, p in enumerate(pattern):
        kinds = PROVED if p else UNPROVED
        j = i % len(kinds)
        k, ptype, context, tstat = kinds[j]
        raw = _link_packet(k, ptype, context, bytes([j, i % 8, int(p)]) * 11)
        twist = j - (len(UNPROVED) - 4) if not p else -1
        recs.append((raw, tstat, twist))
    return recs


def _prove(recs, shared, state=None):
    """Runs link_prove over the records into ``state``'s buffers (new ones
    where None) and holds the outcome to the model.  Returns the buffers."""
    import torch
    from reticulum_amd import device
    n = len(recs)
    signers, model = _signers(shared)
    _, _, table = _world()
    pkt, off, fields = _unpack([r[0] for r in recs])
    unpacked = [ph.unpack(r[0]) for r in recs]
    routes, links = [], []
    for (raw, tstat, twist), f in zip(recs, unpacked):
        route, link = ph.link_of(f, table)
        if twist == 0:
            link = -1
        elif twist == 1:
            link = N_LINKS
        elif twist == 3:
            route = lh.LINK_PLAIN
        routes.append(route)
        links.append(link)
    for i, r in enumerate(recs):
        if r[2] == 2:
            fields[i, 0] = 0
            unpacked[i] = None
    want = [ph.prove(f, routes[i], links[i], recs[i][1], model) for i, f in enumerate(unpacked)]
    if state is None:
        state = (torch.full((n + GUARD, ROW), FILL, dtype=torch.uint8, device="cuda:0"),
                 torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0"))
    proofs, proof_len = state
    before = proofs.cpu().numpy().copy()
    device.link_prove(fields, _dev(np.array(routes, np.uint8)), _dev(np.array(links, np.int32)),
                      _dev(np.array([r[1] for r in recs], np.int32)), signers, proofs[:n], proof_len[:n])
    torch.cuda.synchronize()
    rows, ln = proofs.cpu().numpy(), proof_len.cpu().numpy()
    assert (ln[n:] == SENTINEL).all()
    assert ln[:n].tolist() == [ph.PROOF_LEN if w is not None else 0 for w in want]
    expect = before.copy()
    for i, w in enumerate(want):
        if w is not None:
            expect[i, :ph.PROOF_LEN] = np.frombuffer(w, np.uint8)
    bad = np.nonzero((rows != expect).any(axis=1))[0]
    assert bad.size == 0, f"rows {bad[:8].tolist()} differ (proved: {[want[i] is not None for i in bad[:8]]})"
    return state, want


def _patterns(n):
    yield "none", [False] * n
    yield "all", [True] * n
    yield "every second", [bool(i & 1) for i in range(n)]
    for at in sorted({0, n - 1, 63, 64, n - 64} & set(range(n))):
        yield f"one at {at}", [i == at for i in range(n)]
    if n > 128:
        yield "whole waves", [bool((i >> 6) & 1) for i in range(n)]
        yield "whole waves, the others", [not (i >> 6) & 1 for i in range(n)]


@pytest.mark.parametrize("n", SIZES)
def test_link_prove_matches_the_model(n):
    for k, (name, pattern) in enumerate(_patterns(n)):
        _, want = _prove(_records(pattern), shared=bool(k & 1))
        assert sum(w is not None for w in want) == sum(pattern), name


def test_link_prove_twice_into_the_same_buffers():
    n = 130
    first = [bool(i % 3) for i in range(n)]
    state, _ = _prove(_records(first), shared=False)
    # rows the second call does not prove keep the first call's proofs
    state, want = _prove(_records([not p for p in first]), shared=False, state=state)
    rows = state[0].cpu().numpy()
    assert all((rows[i, 0] == 0x0F) == (first[i] or want[i] is not None) for i in range(n))


def test_link_prove_writes_the_reference_s_proofs():
    """Every case recorded from Link.receive: case c is given signer row c,
    with the seed and the flags its link had."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    vec = ph.vectors()
    links, cases = vec["links"], vec["proved"]
    table = {bytes.fromhex(l["link_id"]): k for k, l in enumerate(links)}
    raws = [bytes.fromhex(c["raw"]) for c in cases]
    n = len(raws)
    routes, tstat = [], []
    for c, raw in zip(cases, raws):
        f = ph.unpack(raw)
        route, link = ph.link_of(f, table)
        assert link == c["link"]
        routes.append(route)
        tstat.append(ctoken.decrypt(bytes.fromhex(links[link]["derived_key"]), f["data"])[0]
                     if route == lh.LINK_DECRYPT else 1)
    signers = rt.LinkSigners(_rows([bytes.fromhex(links[c["link"]]["seed"]) for c in cases]), _rows([bytes(32)] * n),
                             [c["flags"] for c in cases], device=0)
    _, _, fields = _unpack(raws)
    proofs = torch.full((n, ph.PROOF_LEN), FILL, dtype=torch.uint8, device="cuda:0")      # rows of exactly 115 bytes
    proof_len = torch.empty(n, dtype=torch.int32, device="cuda:0")
    device.link_prove(fields, _dev(np.array(routes, np.uint8)), _dev(np.arange(n, dtype=np.int32)),
                      _dev(np.array(tstat, np.int32)), signers, proofs, proof_len)
    torch.cuda.synchronize()
    rows, ln = proofs.cpu().numpy(), proof_len.cpu().tolist()
    for i, c in enumerate(cases):
        if c["proof"] is None:
            assert ln[i] == 0 and (rows[i] == FILL).all(), c["note"]
        else:
            assert ln[i] == ph.PROOF_LEN and rows[i].tobytes().hex() == c["proof"], c["note"]
    assert sum(ln) == 18 * ph.PROOF_LEN


def test_link_prove_argument_checks():
    import torch
    from reticulum_amd import device
    signers, _ = _signers(False)
    _, _, fields = _unpack([_link_packet(0, lh.DATA, lh.NONE, bytes(70))])
    route, link = _dev(np.array([3], np.uint8)), _dev(np.array([0], np.int32))
    status, ln = _dev(np.array([0], np.int32)), torch.empty(1, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="115"):
        device.link_prove(fields, route, link, status, signers, torch.empty((1, 114), dtype=torch.uint8, device="cuda:0"),
                          ln)
    with pytest.raises(ValueError):
        device.link_prove(fields, route, link.to(torch.int64), status, signers,
                          torch.empty((1, 128), dtype=torch.uint8, device="cuda:0"), ln)


# ------------------------------------------------------------ ReceiptTable --

def _hashes(rng, n):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


def test_receipts_hold_the_first_of_two_hashes_that_share_16_bytes():
    import torch
    import reticulum_amd as rt
    rng = np.random.Generator(np.random.PCG64(434))
    a, c = _hashes(rng, 2)
    b = a[:16] + c[16:]
    t = rt.ReceiptTable(8, device=0)
    assert t.add([a, b, c], [5, 6, 7]).cpu().tolist() == [lh.OK, lh.DUPLICATE, lh.OK]
    assert t.add([b], [2]).cpu().tolist() == [lh.DUPLICATE] and len(t) == 2
    rows = t.hashes.cpu().numpy()
    assert rows[5].tobytes() == a and rows[7].tobytes() == c and not rows[[0, 1, 2, 3, 4, 6]].any()
    values, found = t.table.lookup([a[:16], c[:16]])
    assert values.cpu().tolist() == [5, 7] and found.cpu().tolist() == [True, True]
    assert t.remove([b]).cpu().tolist() == [lh.OK] and len(t) == 1       # removal goes by the table's 16 bytes
    assert t.add([b], [6]).cpu().tolist() == [lh.OK]
    assert t.hashes[6].cpu().numpy().tobytes() == b
    with pytest.raises(ValueError):
        t.add([a], [8])
    torch.cuda.synchronize()


def test_receipts_in_a_chain_on_one_home_slot_and_a_full_table():
    import reticulum_amd as rt
    rng = np.random.Generator(np.random.PCG64(569))
    t = rt.ReceiptTable(8, device=0)
    assert t.table.capacity == 16
    heads = lh.ids_for_home(rng, 16, 5, 6)
    chain = [h + rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for h in heads]
    assert t.add(chain, list(range(6))).cpu().tolist() == [lh.OK] * 6
    assert t.remove([chain[2]]).cpu().tolist() == [lh.OK]
    assert t.remove([chain[2]]).cpu().tolist() == [lh.MISSING] and len(t) == 5
    values, found = t.table.lookup(heads)
    assert values.cpu().tolist() == [0, 1, -1, 3, 4, 5] and found.cpu().tolist() == [True, True, False, True, True, True]
    # what lies behind the removed entry still settles
    seed = _world()[1][0]
    import torch
    from reticulum_amd import device
    signers, model = _signers(False)
    raws = [ph.proof_packet(_world()[0][0], chain[k], seed) for k in (5, 2, 3)]
    pkt, off, fields = _unpack(raws)
    status = torch.empty(3, dtype=torch.int32, device="cuda:0")
    receipt = torch.empty(3, dtype=torch.int32, device="cuda:0")
    device.proof_settle(pkt, off, fields, _dev(np.zeros(3, np.int32)), signers, t, status, receipt)
    assert status.cpu().tolist() == [ph.DELIVERED, ph.NO_RECEIPT, ph.DELIVERED]
    assert receipt.cpu().tolist() == [5, -1, 3] and len(t) == 3
    # a full table: 16 slots, three entries, fifteen more hashes
    more = _hashes(rng, 15)
    st = t.add(more, [i % 8 for i in range(15)]).cpu().tolist()
    assert sorted(st) == [lh.OK] * 13 + [lh.FULL] * 2 and len(t) == 16


# ------------------------------------------------------------ proof_settle --

def _settle(raws, signers, model, table, receipts, links=None, clear_ok=()):
    """proof_settle on the device against the model; both tables move on."""
    import torch
    from reticulum_amd import device
    n = len(raws)
    _, _, link_table = _world()
    pkt, off, fields = _unpack(raws)
    unpacked = [ph.unpack(r) for r in raws]
    for i in clear_ok:
        fields[i, 0] = 0
        unpacked[i] = None
    if links is None:
        links = [ph.link_of(f, link_table)[1] for f in unpacked]
    want = ph.settle(unpacked, links, model, receipts)
    status = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    receipt = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    device.proof_settle(pkt, off, fields, _dev(np.array(links, np.int32)), signers, table, status[:n], receipt[:n])
    torch.cuda.synchronize()
    st, rc = status.cpu().numpy(), receipt.cpu().numpy()
    assert (st[n:] == SENTINEL).all() and (rc[n:] == SENTINEL).all()
    assert st[:n].tolist() == [w[0] for w in want]
    assert rc[:n].tolist() == [w[1] for w in want]
    assert all((s == ph.DELIVERED) == (r >= 0) for s, r in zip(st[:n], rc[:n]))
    assert len(table) == len(receipts)
    return st[:n].tolist(), rc[:n].tolist()


def _tables(hashes, max_receipts=64, ids=None):
    import reticulum_amd as rt
    ids = list(range(len(hashes))) if ids is None else ids
    table, model = rt.ReceiptTable(max_receipts, device=0), ph.Receipts(max_receipts)
    assert table.add(hashes, ids).cpu().tolist() == model.add(hashes, ids) == [lh.OK] * len(hashes)
    return table, model


def _proof(k, h, signer=None, context=lh.NONE, dtype=lh.LINK, ptype=lh.PROOF, tail=b""):
    seeds = _world()[1]
    sig = ph.sign(seeds[k if signer is None else signer], h)
    return bytes([dtype << 2 | ptype, 0]) + _world()[0][k] + bytes([context]) + h + sig + tail


def test_settle_every_fixture_case():
    import reticulum_amd as rt
    vec = ph.vectors()
    links = vec["links"]
    publics = [bytes.fromhex(l["public"]) for l in links[:4]]
    link_table = {bytes.fromhex(l["link_id"]): k for k, l in enumerate(links[:4])}
    signers = rt.LinkSigners(_rows([bytes(32)]), _rows(publics), [0] * 4, device=0)
    model = ph.Signers([bytes(32)], publics, [0] * 4)
    seen = set()
    for b in vec["settled"]:
        hashes = [bytes.fromhex(h) for h, _ in b["receipts"]]
        table, receipts = _tables(hashes, 16)
        raws = [bytes.fromhex(r) for r in b["raws"]]
        links_of = [ph.link_of(ph.unpack(r), link_table)[1] for r in raws]
        st, rc = _settle(raws, signers, model, table, receipts, links=links_of)
        seen |= set(st)
        for j, want in enumerate(b["delivered"]):
            if j not in b.get("caller", []):
                assert (hashes[rc[j]].hex() if rc[j] >= 0 else None) == want, (b["note"], j)
    assert seen == set(range(7))


@functools.lru_cache(maxsize=None)
def _settle_pool():
    """Proofs of every verdict for 24 receipts held by links 0..2."""
    rng = np.random.Generator(np.random.PCG64(2334))
    hashes = _hashes(rng, 24)
    other = _hashes(rng, 4)
    good = [_proof(i % 3, h, tail=bytes(i % 5)) for i, h in enumerate(hashes)]
    rest = []
    for i in range(4):
        h = hashes[i]
        rest += [_proof(0, other[i]),                                       # NO_RECEIPT
                 _proof(1, h, signer=3),                                    # BAD_SIGNATURE
                 _proof(2, h[:16] + other[i][16:]),                         # NO_RECEIPT: 16 bytes agree
                 _proof(0, h)[:19 + 95 - 30 * i],                           # SHORT
                 _proof(0, h, ptype=lh.DATA),                               # NOT_PROOF
                 _proof(0, h, context=ph.LRPROOF), _proof(0, h, context=lh.RESOURCE_PRF),
                 _proof(0, h, dtype=lh.SINGLE),                             # NOT_LINK
                 bytes([lh.LINK << 2 | lh.PROOF, 0]) + other[i][:16] + bytes([0]) + h + bytes(64)]  # NO_LINK
    return hashes, good, rest


@pytest.mark.parametrize("n", SIZES)
def test_settle_matches_the_model(n):
    hashes, good, rest = _settle_pool()
    signers, model = _signers(False)
    for every in (1, 2, 5):
        # every `every`-th packet a proof that would settle, several of them the same proof
        raws = [good[(i // every) % 17] if i % every == 0 else rest[i % len(rest)] for i in range(n)]
        table, receipts = _tables(hashes)
        st, _ = _settle(raws, signers, model, table, receipts, clear_ok=[i for i in range(n) if i % 29 == 7])
        assert st.count(ph.DELIVERED) == min(17, len({r for i, r in enumerate(raws) if i % every == 0 and i % 29 != 7}))


@pytest.mark.parametrize("candidates", [0, 1, 64, 65, 130])
def test_settle_candidate_counts(candidates):
    n = 130
    hashes, good, rest = _settle_pool()
    signers, model = _signers(False)
    rng = np.random.Generator(np.random.PCG64(candidates))
    at = set(rng.permutation(n)[:candidates].tolist())
    # candidates: receipts' own proofs and proofs with a bad signature, which reach the verify pass too
    raws = [(good[i % 24] if i % 3 else _proof(1, hashes[i % 24], signer=4)) if i in at else
            rest[(i % 4) * 9 + (0, 3, 4, 7, 8)[i % 5]] for i in range(n)]
    table, receipts = _tables(hashes)
    st, _ = _settle(raws, signers, model, table, receipts)
    assert sum(s in (ph.DELIVERED, ph.BAD_SIGNATURE) or (s == ph.NO_RECEIPT and i in at) for i, s in enumerate(st)) \
        == candidates


@pytest.mark.parametrize("copies", [2, 300])
def test_settle_delivers_the_lowest_index_of_one_proof(copies):
    hashes, good, rest = _settle_pool()
    signers, model = _signers(False)
    table, receipts = _tables(hashes)
    raws = [rest[3]] + [good[4]] * copies
    st, rc = _settle(raws, signers, model, table, receipts)
    assert st == [ph.SHORT, ph.DELIVERED] + [ph.NO_RECEIPT] * (copies - 1) and rc[1] == 4 and len(table) == 23
    st, _ = _settle(raws, signers, model, table, receipts)
    assert st == [ph.SHORT] + [ph.NO_RECEIPT] * copies and len(table) == 23


def test_settle_bad_copies_do_not_block_a_good_one():
    hashes, good, rest = _settle_pool()
    signers, model = _signers(False)
    table, receipts = _tables(hashes)
    h = hashes[7]                                # link 1's
    bad = bytearray(_proof(1, h))
    bad[19 + 70] ^= 4
    wrong_link = _proof(0, h, signer=1)          # link 1's signature arriving under link 0
    twin = _proof(2, h[:16] + hashes[8][16:])    # agrees with the receipt in 16 bytes only
    raws = [bytes(bad)] * 70 + [wrong_link, twin, _proof(1, h), bytes(bad), _proof(1, h)]
    st, rc = _settle(raws, signers, model, table, receipts)
    # behind the delivered proof the receipt is gone, for a bad signature too
    assert st == [ph.BAD_SIGNATURE] * 71 + [ph.NO_RECEIPT, ph.DELIVERED, ph.NO_RECEIPT, ph.NO_RECEIPT]
    assert rc[72] == 7


def test_settle_verifies_under_the_link_the_proof_arrived_on():
    """The reference takes the key of packet.link, whichever link the proved
    packet went out on (Transport.py:2327-2332, Packet.py:428-441)."""
    hashes, good, rest = _settle_pool()
    peer_seeds = list(_world()[1])
    peer_seeds[3] = peer_seeds[0]                # links 0 and 3 have one peer key
    signers, model = _signers(False, peer_seeds=tuple(peer_seeds))
    table, receipts = _tables(hashes)
    raws = [_proof(3, hashes[0], signer=0), _proof(4, hashes[3], signer=0), _proof(4, hashes[3], signer=4)]
    st, rc = _settle(raws, signers, model, table, receipts)
    assert st == [ph.DELIVERED, ph.BAD_SIGNATURE, ph.DELIVERED] and rc == [0, -1, 3]
