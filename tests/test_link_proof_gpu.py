"""device.link_establish: the link request proof stage alone, against the
model of tests/link_proof_helpers.py (which test_link_proof.py ties to the
reference) and the fixture's bytes.

Every call is checked in full (_check): status, slot and MTU per record with
the sentinel behind the outputs, the link table, the key set (a token made on
the host under the model's derived key decrypts under key_idx = slot; rows that
were not assigned still open their old tokens), the signers' rows, the pending
rows' state, hops, rebalanced and mtu, and the hash list."""
import numpy as np
import pytest

import ed25519_ref as ed
import link_proof_helpers as lp
from link_accept_helpers import x25519
from oracle import ctoken

pytestmark = pytest.mark.gpu

N_KEYS = 16


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def vec():
    return lp.vectors()


class Dest:
    """A destination identity that answers link requests, on the host."""

    def __init__(self, rng):
        self.seed = _rb(rng, 32)
        self.public = ed.public_key(self.seed)

    def proof(self, rng, link, mtu=None, hops=0, forge=False, data_len=None, peer_pub=None):
        """The raw LRPROOF a responder sends for ``link`` (an lp.Pending)."""
        pub = peer_pub or x25519(_rb(rng, 32), (9).to_bytes(32, "little"))
        sg = lp.signalling(mtu) if mtu is not None else b""
        data = ed.sign(self.seed, link.link_id + pub + self.public + sg, self.public) + pub + sg
        if forge:
            data = bytes([data[0] ^ 1]) + data[1:]
        if data_len is not None:
            data = (data + b"\x20" + bytes(7))[:data_len]      # (a 97th byte with the right mode bits)
        return bytes([0x0F, hops]) + link.link_id + b"\xff" + data


class World:
    """A key set with known keys, a link table, signers, a hash list, the
    pending links, and their models."""

    def __init__(self, rng, n_keys=N_KEYS, max_links=64, max_pending=32):
        import reticulum_amd as rt
        self.rng = rng
        self.keys = [_rb(rng, 64) for _ in range(n_keys)]
        self.ks = rt.KeySet(np.frombuffer(b"".join(self.keys), np.uint8).reshape(n_keys, 64), device=0)
        self.tab, self.table = rt.LinkTable(max_links, device=0), {}
        self.seeds = [_rb(rng, 32) for _ in range(n_keys)]
        self.peers = [_rb(rng, 32) for _ in range(n_keys)]
        self.flags = [0] * n_keys
        self.signers = rt.LinkSigners(self.seeds, self.peers, self.flags, device=0)
        self.publics = [self.signers.publics[k].cpu().numpy().tobytes() for k in range(n_keys)]
        self.seen, self.hashes = rt.PacketHashlist(4096, device=0), set()
        self.pending, self.model = rt.link.PendingLinks(max_pending, device=0), {}

    def open(self, dest, slot, expected_hops=1, flags=0, link=None):
        link = link or lp.Pending(_rb(self.rng, 16), _rb(self.rng, 32), dest.public, _rb(self.rng, 32), flags, slot,
                                  expected_hops)
        st = self.pending.add([link.link_id], [link.prv], [link.dest_public], [link.sig_seed], [link.flags],
                              [link.slot], [link.expected_hops])
        assert st.tolist() == [0]
        if link.rebalanced:                             # (a state the stage itself leaves; add() starts a link fresh)
            self.pending.rebalanced[self.pending.row_of(link.link_id)] = 1
        self.model[link.link_id] = link
        return link


def stage(w, raws, seen=True, signers=True):
    import torch
    from reticulum_amd import device
    n = len(raws)
    off = np.zeros(n, np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])[:-1]
    pkt = _t(np.frombuffer(b"".join(raws) + b"\x00", np.uint8))
    fields = torch.empty((n, 96), dtype=torch.uint8, device="cuda:0")
    device.packet_unpack(pkt, _t(off), _t(np.array([len(r) for r in raws], np.int32)), fields)
    # one buffer for the three outputs, a sentinel row between and behind them
    buf = torch.full((6, max(n, 1)), -7, dtype=torch.int32, device="cuda:0")
    device.link_establish(w.ks, w.tab, w.pending, pkt, _t(off), fields, buf[0, :n], buf[2, :n], buf[4, :n],
                          signers=w.signers if signers else None, seen=w.seen if seen else None)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[1::2] == -7).all() and (got[:, n:] == -7).all()
    return dict(status=got[0, :n], slot=got[2, :n], mtu=got[4, :n])


def run(w, raws, **kw):
    """The stage and the model over one batch, compared in full."""
    before = dict(w.table)
    want = lp.run(raws, w.model, w.table, n_keys=len(w.keys), n_links=len(w.peers), table_room=w.tab.capacity)
    got = stage(w, raws, **kw)
    _check(w, raws, got, want, before, kw.get("seen", True), kw.get("signers", True))
    return want


def _check(w, raws, got, want, before, seen, signers):
    assert got["status"].tolist() == [r[0] for r in want]
    assert got["slot"].tolist() == [r[1] for r in want]
    assert got["mtu"].tolist() == [r[2] for r in want]
    for raw, r in zip(raws, want):
        if r[0] == lp.ACTIVATED:
            link = w.model[lp.unpack(raw)[3]]
            w.keys[r[1]] = link.derived_key
            if signers:
                w.peers[r[1]], w.flags[r[1]] = link.dest_public, link.flags & 3
                w.seeds[r[1]], w.publics[r[1]] = link.sig_seed, ed.public_key(link.sig_seed)
        if seen and r[3]:
            w.hashes.add(lp.packet_hash(raw))
    # the link table: every id the model holds, and the pending ids that did not come up
    ids = list(w.table) + [k for k in w.model if k not in w.table]
    if ids:
        values, found = w.tab.lookup(ids)
        assert values.cpu().tolist() == [w.table.get(k, -1) for k in ids]
        assert found.cpu().tolist() == [k in w.table for k in ids]
    assert len(w.tab) == len(w.table) == len(before) + sum(r[0] == lp.ACTIVATED for r in want)
    # the key set: every row opens a token made under the key the model holds for it
    rng = np.random.Generator(np.random.PCG64(len(raws)))
    pts = [_rb(rng, int(rng.integers(0, 40))) for _ in w.keys]
    toks = [ctoken.encrypt(k, _rb(rng, 16), p) for k, p in zip(w.keys, pts)]
    back, status = w.ks.decrypt_batch(toks, key_idx=np.arange(len(w.keys), dtype=np.uint32))
    assert (status == 0).all() and back.to_list() == pts
    # the signers
    s = w.signers
    assert s.peer_publics.cpu().numpy().tobytes() == b"".join(w.peers)
    assert s.flags.cpu().tolist() == w.flags
    assert s.seeds.cpu().numpy().tobytes() == b"".join(w.seeds)
    assert s.publics.cpu().numpy().tobytes() == b"".join(w.publics)
    # the pending rows
    if w.model:
        ids = list(w.model)
        hops, reb, mtu = w.pending.hops(ids)
        assert w.pending.state(ids).tolist() == [w.model[k].state for k in ids]
        assert hops.tolist() == [w.model[k].expected_hops for k in ids]
        assert reb.tolist() == [int(w.model[k].rebalanced) for k in ids]
        assert mtu.tolist() == [w.model[k].mtu for k in ids]
    # the hash list: what the model remembered and nothing else of this batch
    hs = [lp.packet_hash(r) for r in raws if len(r) >= 19]
    if hs:
        assert w.seen.contains(hs).cpu().tolist() == [int(h in w.hashes) for h in hs]
    assert len(w.seen) == len(w.hashes)


def _fixture_world(vec, cases, seed):
    w = World(np.random.Generator(np.random.PCG64(seed)), max_pending=max(len(cases), 1))
    for k, c in enumerate(cases):
        w.open(None, k % N_KEYS, link=lp.fixture_link(vec, c, slot=k % N_KEYS, flags=k & 3))
    return w


def test_every_fixture_case_one_per_launch(vec):
    """Each case on a world of its own state, its packets one per launch: the
    reference's own sequence, and its bytes (the derived key included)."""
    w = World(np.random.Generator(np.random.PCG64(1)), max_pending=64)
    for k, c in enumerate(vec["cases"]):
        link = w.open(None, k % N_KEYS, link=lp.fixture_link(vec, c, slot=k % N_KEYS, flags=k & 3))
        for p in c["packets"]:
            want = run(w, [p["raw"]])
            assert want[0][0] == lp.STATUS[p["expect"]], c["note"]
            assert link.state == lp.STATE[p["after"]["status"]], c["note"]
            if p["after"]["active"]:
                assert w.keys[link.slot] == p["after"]["derived_key"], c["note"]
        if link.state == lp.ACTIVE:                      # the slot is free for the next case
            assert w.tab.remove([link.link_id]).cpu().tolist() == [0]
            del w.table[link.link_id]
        assert w.pending.remove([link.link_id]).tolist() == [0]
        del w.model[link.link_id]


def test_every_fixture_case_in_one_launch(vec):
    """All cases' packets in one batch, in order: the sequences decided inside
    the call as the reference decides them one after another."""
    cases = vec["cases"]
    w = World(np.random.Generator(np.random.PCG64(2)), n_keys=64, max_links=128, max_pending=64)
    for k, c in enumerate(cases):
        w.open(None, k, link=lp.fixture_link(vec, c, slot=k, flags=k & 3))
    raws = [p["raw"] for c in cases for p in c["packets"]]
    want = run(w, raws)
    assert [r[0] for r in want] == [lp.STATUS[p["expect"]] for c in cases for p in c["packets"]]
    # a second call on the same state: nothing is PENDING that was decided, nothing new comes up
    again = run(w, raws)
    assert not any(r[0] == lp.ACTIVATED for r in again)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_batch_edges(n):
    """Proofs on the first and last lane of a wave and a workgroup, and a batch
    of the same size with none at all."""
    rng = np.random.Generator(np.random.PCG64(100 + n))
    w, d = World(rng), Dest(rng)
    at = sorted({i for i in (0, 63, 64, 255, 256, n - 1) if 0 <= i < n})
    other = lambda: bytes([0x0C, 0]) + _rb(rng, 16) + b"\x00" + _rb(rng, int(rng.integers(1, 90)))   # noqa: E731
    raws = [other() for _ in range(n)]
    if n:
        run(w, raws)
    for k, i in enumerate(at):
        raws[i] = d.proof(rng, w.open(d, k, flags=k & 3), mtu=(None, 1196)[k & 1])
    want = run(w, raws)
    assert sum(r[0] == lp.ACTIVATED for r in want) == len(at)


def test_copies_of_one_proof():
    """2 and 300 copies: the lowest index activates, the rest find the link gone."""
    rng = np.random.Generator(np.random.PCG64(7))
    w, d = World(rng), Dest(rng)
    for k, copies in enumerate((2, 300)):
        raw = d.proof(rng, w.open(d, k), mtu=500)
        want = run(w, [raw] * copies)
        assert [r[0] for r in want] == [lp.ACTIVATED] + [lp.NOT_PENDING] * (copies - 1)


def test_order_inside_a_batch():
    rng = np.random.Generator(np.random.PCG64(8))
    w, d = World(rng), Dest(rng)
    # a forged copy below a genuine one: the link is dead; above it: the link is up
    link = w.open(d, 0)
    assert [r[0] for r in run(w, [d.proof(rng, link, forge=True), d.proof(rng, link)])] == \
        [lp.BAD_SIGNATURE, lp.NOT_PENDING]
    link = w.open(d, 1)
    assert [r[0] for r in run(w, [d.proof(rng, link), d.proof(rng, link, forge=True)])] == \
        [lp.ACTIVATED, lp.NOT_PENDING]
    # a bad length below a genuine one: the link is up
    link = w.open(d, 2)
    assert [r[0] for r in run(w, [d.proof(rng, link, data_len=97), d.proof(rng, link, mtu=400)])] == \
        [lp.BAD_SIZE, lp.ACTIVATED]
    # a hop-mismatched genuine proof below a hop-matched forged one: rebalanced and up
    link = w.open(d, 3)
    assert [r[0] for r in run(w, [d.proof(rng, link, hops=4), d.proof(rng, link, forge=True)])] == \
        [lp.ACTIVATED, lp.NOT_PENDING]
    assert link.rebalanced and link.expected_hops == 5
    # and a hop-mismatched forged one below a genuine one
    link = w.open(d, 4)
    assert [r[0] for r in run(w, [d.proof(rng, link, hops=4, forge=True), d.proof(rng, link)])] == \
        [lp.HOPS, lp.ACTIVATED]


def test_no_room():
    rng = np.random.Generator(np.random.PCG64(9))
    # m + 1 proofs for a link table with m slots: which of them finds none depends on the scheduling
    w, d = World(rng, max_links=2), Dest(rng)
    m = w.tab.capacity
    links = [w.open(d, k) for k in range(m + 1)]
    got = stage(w, [d.proof(rng, l) for l in links])
    assert sorted(got["status"].tolist()) == [lp.ACTIVATED] * m + [lp.NO_SLOT] and len(w.tab) == m
    states = w.pending.state([l.link_id for l in links]).tolist()
    assert [s == lp.ACTIVE for s in states] == [st == lp.ACTIVATED for st in got["status"].tolist()]
    assert sorted(states) == [lp.PENDING] + [lp.ACTIVE] * m
    # a slot not below n_keys; the link comes up once it has one
    w = World(rng)
    link = w.open(d, N_KEYS)
    raw = d.proof(rng, link)
    assert [r[0] for r in run(w, [raw, raw])] == [lp.NO_SLOT, lp.NOT_PENDING]
    assert link.state == lp.PENDING


def test_two_destinations_and_no_signers_no_list():
    rng = np.random.Generator(np.random.PCG64(10))
    w, d0, d1 = World(rng), Dest(rng), Dest(rng)
    l0, l1 = w.open(d0, 3, flags=1), w.open(d1, 9, flags=2)
    want = run(w, [d1.proof(rng, l0), d0.proof(rng, l0, mtu=1196), d1.proof(rng, l1)])
    assert [r[0] for r in want] == [lp.BAD_SIGNATURE, lp.NOT_PENDING, lp.ACTIVATED]
    l2 = w.open(d0, 5)
    assert run(w, [d0.proof(rng, l2)], seen=False, signers=False)[0][0] == lp.ACTIVATED


def test_pending_add_remove_against_a_dict():
    import reticulum_amd as rt
    rng = np.random.Generator(np.random.PCG64(11))
    p, model = rt.link.PendingLinks(8, device=0), {}
    ids = [_rb(rng, 16) for _ in range(12)]
    # chains: ids that share their first four bytes land in one chain of the table
    ids += [ids[0][:4] + _rb(rng, 12) for _ in range(3)]

    def add(batch):
        st = p.add(batch, [bytes([k]) * 32 for k in range(len(batch))], [bytes(32)] * len(batch),
                   [bytes([k + 1]) * 32 for k in range(len(batch))], [0] * len(batch), list(range(len(batch))),
                   [1] * len(batch))
        want = []
        for i in batch:
            want.append(1 if i in model else 2 if len(model) >= 8 else 0)
            if want[-1] == 0:
                model[i] = True
        assert st.tolist() == want

    def remove(batch):
        st = p.remove(batch)
        assert st.tolist() == [0 if model.pop(i, None) else 3 for i in batch]

    add([ids[0], ids[12], ids[0], ids[13]])
    add(ids[1:9])
    remove([ids[12], ids[12], ids[11]])
    add([ids[14], ids[9]])
    remove(ids[:4])
    add(ids[9:12])
    values, found = p.table.lookup(ids)
    assert found.cpu().tolist() == [i in model for i in ids] and len(p) == len(p.table) == len(model)
    rows = values.cpu().tolist()
    assert [rows[k] for k, i in enumerate(ids) if i in model] == [p.row_of(i) for i in ids if i in model]
    assert p.state([i for i in ids if i in model]).tolist() == [0] * len(model)
