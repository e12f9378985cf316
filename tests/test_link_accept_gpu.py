"""device.link_accept: the link request stage alone, against the model of
tests/link_accept_helpers.py (which test_link_accept.py ties to the reference)
with the fixture's ephemeral keys.

Every call is checked in full (_check): status, slot, link id, MTU, the
118-byte packet with the sentinel bytes behind it and whole sentinel rows where
nothing was accepted, the link table, the key set (a token made on the host
under the model's derived key decrypts under key_idx = slot; rows that were not
assigned still open their old tokens) and the signers' rows."""
import numpy as np
import pytest

import link_accept_helpers as la
from oracle import ctoken

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
N_KEYS = 16


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def env():
    import reticulum_amd as rt
    vec = la.vectors()
    model = la.fixture_dests(vec)
    dests = rt.LinkDestinations([d.hash for d in model], [d.seed for d in model], [d.flags for d in model], device=0)
    assert dests.publics.cpu().numpy().tobytes() == b"".join(d.public for d in model)
    return dict(vec=vec, model=model, dests=dests, tid=_t(np.frombuffer(vec["transport_id"], np.uint8)))


class World:
    """A key set with known keys, a link table, signers, and their models."""

    def __init__(self, rng, n_keys=N_KEYS, max_links=64, shared_seed=None):
        import reticulum_amd as rt
        self.keys = [_rb(rng, 64) for _ in range(n_keys)]
        self.ks = rt.KeySet(np.frombuffer(b"".join(self.keys), np.uint8).reshape(n_keys, 64), device=0)
        self.tab = rt.LinkTable(max_links, device=0)
        self.table = {}
        self.seeds = [shared_seed] if shared_seed else [_rb(rng, 32) for _ in range(n_keys)]
        self.peers = [_rb(rng, 32) for _ in range(n_keys)]
        self.flags = [0] * n_keys
        self.signers = rt.LinkSigners(self.seeds, self.peers, self.flags, device=0)
        self.publics = [self.signers.publics[k].cpu().numpy().tobytes() for k in range(len(self.seeds))]


def request(rng, dest, mtu=None, header2=None, keys=None):
    keys = _rb(rng, 64) if keys is None else keys
    data = keys + (la.signalling(mtu) if mtu is not None else b"")
    flags = la.LINKREQUEST
    if header2 is None:
        return bytes([flags, 0]) + dest.hash + b"\x00" + data
    return bytes([flags | 0x50, 2]) + header2 + dest.hash + b"\x00" + data


def other_packet(rng):
    return bytes([la.LINK << 2, 0]) + _rb(rng, 16) + b"\x00" + _rb(rng, int(rng.integers(1, 90)))


def stage(env, w, raws, slots, eph, nh_mtu=500, signers=True):
    import torch
    from reticulum_amd import device
    n = len(raws)
    off = np.zeros(n, np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])[:-1]
    pkt = _t(np.frombuffer(b"".join(raws) + b"\x00", np.uint8))
    fields = torch.empty((n, 96), dtype=torch.uint8, device="cuda:0")
    device.packet_unpack(pkt, _t(off), _t(np.array([len(r) for r in raws], np.int32)), fields)
    i32 = lambda: torch.full((n,), -7, dtype=torch.int32, device="cuda:0")     # noqa: E731
    out = dict(status=i32(), slot=i32(), mtu=i32(), plen=i32(),
               link_id=torch.full((n, 16), SENTINEL, dtype=torch.uint8, device="cuda:0"),
               proofs=torch.full((n, 128), SENTINEL, dtype=torch.uint8, device="cuda:0"))
    m = len(slots)
    device.link_accept(w.ks, w.tab, env["dests"], env["tid"], pkt, _t(off), fields, _t(np.array(slots, np.int32)),
                       _t(np.frombuffer(b"".join(eph), np.uint8).reshape(m, 32)) if m else
                       torch.empty((0, 32), dtype=torch.uint8, device="cuda:0"),
                       out["status"], out["slot"], out["link_id"], out["mtu"], out["proofs"], out["plen"],
                       nh_mtu=nh_mtu, signers=w.signers if signers else None)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run(env, w, raws, slots, eph, nh_mtu=500, rng=None):
    """The stage and the model over one batch, compared in full; the model's records."""
    before = dict(w.table)
    want = la.accept(raws, env["model"], env["vec"]["transport_id"], nh_mtu, slots, eph, w.table, len(w.keys),
                     len(w.peers))
    got = stage(env, w, raws, slots, eph, nh_mtu)
    _check(env, w, got, want, before, rng or np.random.Generator(np.random.PCG64(len(raws))))
    return want


def _check(env, w, got, want, before, rng):
    n = len(want)
    assert got["status"].tolist() == [r["status"] for r in want]
    assert got["slot"].tolist() == [r["slot"] for r in want]
    for i, r in enumerate(want):
        valid = r["status"] in (la.ACCEPTED, la.DUPLICATE, la.NO_SLOT)
        assert got["link_id"][i].tobytes() == (r["link_id"] if valid else bytes(16)), i
        assert got["mtu"][i] == (r["mtu"] if valid else 0), i
        row = got["proofs"][i].tobytes()
        if r["status"] == la.ACCEPTED:
            assert got["plen"][i] == la.LRPROOF_LEN and row[:118] == r["lrproof"], i
            assert row[118:] == bytes([SENTINEL]) * 10, i
            w.keys[r["slot"]] = r["derived_key"]
            w.peers[r["slot"]] = r["peer_sig_pub"]
            w.flags[r["slot"]] = r["dest"].flags & 3
            if len(w.seeds) > 1:
                w.seeds[r["slot"]], w.publics[r["slot"]] = r["dest"].seed, r["dest"].public
        else:
            assert got["plen"][i] == 0 and row == bytes([SENTINEL]) * 128, i
    # the link table: every id the model holds, old and new, and nothing of the others
    ids = list(w.table) + [r["link_id"] for r in want if r["link_id"] is not None and r["link_id"] not in w.table]
    if ids:
        values, found = w.tab.lookup(ids)
        assert values.cpu().tolist() == [w.table.get(k, -1) for k in ids]
        assert found.cpu().tolist() == [k in w.table for k in ids]
    assert len(w.tab) == len(w.table) and len(w.table) == len(before) + sum(r["status"] == la.ACCEPTED for r in want)
    # the key set: every row opens a token made under the key the model holds for it
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
    assert n == len(got["status"])


def _eph(env, raws, nh_mtu, rng, known=None):
    """One ephemeral row per valid request of the batch: the fixture's where it has one."""
    out = []
    for raw in raws:
        if la.decide(raw, env["model"], env["vec"]["transport_id"], nh_mtu)[0] == la.ACCEPTED:
            out.append((known or {}).get(raw) or _rb(rng, 32))
    return out


def test_every_fixture_case_in_one_launch_per_nh_mtu(env):
    rng = np.random.Generator(np.random.PCG64(1))
    cases = env["vec"]["cases"]
    known = {c["raw"]: c["ephemeral"] for c in cases if "ephemeral" in c}
    seen = 0
    for nh in sorted({c["nh_mtu"] for c in cases}, key=lambda v: -1 if v is None else v):
        group = [c for c in cases if c["nh_mtu"] == nh]
        raws = [c["raw"] for c in group]
        w = World(rng, n_keys=32)
        eph = _eph(env, raws, nh, rng, known)
        want = run(env, w, raws, list(range(31, 31 - len(eph), -1)), eph, nh_mtu=nh, rng=rng)
        for c, r in zip(group, want):
            # a HEADER_2 copy of a request in the same batch is its duplicate; every other case as the reference
            assert r["status"] == la.STATUS[c["expect"]] or (r["status"] == la.DUPLICATE and c["raw"][0] & 0x40)
            if r["status"] == la.ACCEPTED:
                assert (r["link_id"], r["mtu"], r["derived_key"], r["lrproof"]) == \
                    (c["link_id"], c["mtu"], c["derived_key"], c["lrproof"]), c["note"]
                seen += 1
    assert seen >= 26


def test_every_fixture_case_in_a_launch_of_its_own(env):
    rng = np.random.Generator(np.random.PCG64(2))
    w = World(rng, n_keys=4, max_links=128)
    for k, c in enumerate(env["vec"]["cases"]):
        if c["raw"][0] & 0x40 and c["reached"] == "accepted":
            w.tab.remove(list(w.table))                    # its HEADER_1 form came before it
            w.table.clear()
        got = stage(env, w, [c["raw"]], [k % 4], [c.get("ephemeral", bytes(32))], nh_mtu=c["nh_mtu"])
        assert got["status"].tolist() == [la.STATUS[c["expect"]]], c["note"]
        if c["reached"] == "accepted":
            assert got["proofs"][0].tobytes() == c["lrproof"] + bytes([SENTINEL]) * 10, c["note"]
            assert got["link_id"][0].tobytes() == c["link_id"] and got["mtu"][0] == c["mtu"], c["note"]
            assert got["slot"].tolist() == [k % 4]
            w.table[c["link_id"]] = k % 4
            tok = ctoken.encrypt(c["derived_key"], _rb(rng, 16), b"under the reference's key")
            back, status = w.ks.decrypt_batch([tok], key_idx=np.array([k % 4], np.uint32))
            assert status.tolist() == [0] and back.to_list() == [b"under the reference's key"], c["note"]
        else:
            assert got["slot"].tolist() == [-1] and got["plen"].tolist() == [0]
            assert got["proofs"][0].tobytes() == bytes([SENTINEL]) * 128


@pytest.mark.parametrize("n,where", [
    (0, []), (1, []), (1, [0]), (63, []), (63, [62]), (63, [0, 7, 62]), (64, [0, 63]), (64, range(64)),
    (65, [63, 64]), (65, []), (257, [0, 63, 64, 127, 128, 255, 256]), (257, [255]), (257, [256])])
def test_batch_edges(env, n, where):
    """None, one, some or all of the records are requests; requests on the
    first and last lane of a wave and of a workgroup of 256."""
    where = list(where)
    rng = np.random.Generator(np.random.PCG64(100 + n + len(where)))
    w = World(rng)
    raws = [request(rng, env["model"][i % 2], mtu=(None, 700)[i % 2]) if i in where else other_packet(rng)
            for i in range(n)]
    slots = [int(s) for s in rng.permutation(N_KEYS)[:len(where)]] if len(where) <= N_KEYS else None
    if slots is None:                   # all of a wave: more requests than the 16 keys, the rest get no slot
        slots = [int(s) for s in rng.permutation(N_KEYS)] + [N_KEYS] * (len(where) - N_KEYS)
    want = run(env, w, raws, slots, [_rb(rng, 32) for _ in slots], rng=rng)
    assert sum(r["status"] == la.ACCEPTED for r in want) == min(len(where), N_KEYS)
    assert sum(r["status"] == la.NO_SLOT for r in want) == max(len(where) - N_KEYS, 0)


@pytest.mark.parametrize("copies", [2, 300])
def test_one_request_many_times(env, copies):
    rng = np.random.Generator(np.random.PCG64(copies))
    w = World(rng)
    dup, other = request(rng, env["model"][0], mtu=500), request(rng, env["model"][1])
    raws = [other_packet(rng)] + [dup] * copies + [other]
    slots = list(range(N_KEYS)) + [3] * (copies + 1 - N_KEYS) if copies + 1 > N_KEYS else list(range(copies + 1))
    want = run(env, w, raws, slots, [_rb(rng, 32) for _ in slots], rng=rng)
    assert [r["status"] for r in want[1:-1]] == [la.ACCEPTED] + [la.DUPLICATE] * (copies - 1)
    assert want[1]["slot"] == 0 and want[-1]["status"] == la.ACCEPTED and want[-1]["slot"] == slots[copies]
    assert len(w.table) == 2            # exactly one slot consumed by all the copies


def test_present_id_no_slot_left_bad_slot_and_full_table(env):
    rng = np.random.Generator(np.random.PCG64(7))
    w = World(rng)
    a, b, c, d = (request(rng, env["model"][k % 2], mtu=600 + k) for k in range(4))
    first = run(env, w, [a], [9], [_rb(rng, 32)], rng=rng)
    assert first[0]["status"] == la.ACCEPTED
    # a is in the table now; three slots for four valid requests, one of them not below n_keys
    want = run(env, w, [a, b, other_packet(rng), c, d], [1, N_KEYS, 2], [_rb(rng, 32) for _ in range(3)], rng=rng)
    assert [r["status"] for r in want] == [la.DUPLICATE, la.NO_SLOT, la.NOT_REQUEST, la.ACCEPTED, la.NO_SLOT]
    assert want[3]["slot"] == 2 and set(w.table) == {first[0]["link_id"], want[3]["link_id"]}
    # a second call with fresh slots works beside the first calls' links
    want = run(env, w, [d, b], [5, 6], [_rb(rng, 32) for _ in range(2)], rng=rng)
    assert [r["slot"] for r in want] == [5, 6] and len(w.table) == 4
    # a table without a free slot
    full = World(rng, max_links=1)
    filler = [_rb(rng, 16) for _ in range(full.tab.capacity)]
    assert full.tab.insert(filler, list(range(len(filler)))).cpu().tolist() == [0] * len(filler)
    full.table.update(zip(filler, range(len(filler))))
    got = stage(env, full, [b], [4], [_rb(rng, 32)])
    assert got["status"].tolist() == [la.NO_SLOT] and got["slot"].tolist() == [-1] and len(full.tab) == len(filler)
    assert got["proofs"][0].tobytes() == bytes([SENTINEL]) * 128


def test_signers_with_one_shared_seed_row_and_without_signers(env):
    import reticulum_amd as rt
    rng = np.random.Generator(np.random.PCG64(8))
    one = la.Dest(env["model"][0].hash, env["model"][0].seed, env["model"][0].flags)
    w = World(rng, shared_seed=one.seed)
    e1 = dict(env, model=[one], dests=rt.LinkDestinations([one.hash], [one.seed], [one.flags], device=0))
    want = run(e1, w, [request(rng, one), request(rng, one, mtu=9000)], [3, 4], [_rb(rng, 32) for _ in range(2)],
               rng=rng)
    assert [r["status"] for r in want] == [la.ACCEPTED] * 2 and w.seeds == [one.seed]
    with pytest.raises(ValueError, match="one shared seed row"):
        stage(env, w, [request(rng, one)], [5], [_rb(rng, 32)])
    # signers of one link are one shared row too: its seed would never be written
    lone = World(rng, n_keys=1)
    with pytest.raises(ValueError, match="one shared seed row"):
        stage(env, lone, [request(rng, one)], [0], [_rb(rng, 32)])
    want = run(e1, lone, [request(rng, one)], [0], [_rb(rng, 32)], rng=rng)
    assert want[0]["status"] == la.ACCEPTED
    # a destination hash given twice could never reach its second row
    with pytest.raises(ValueError, match="distinct"):
        rt.LinkDestinations([one.hash, one.hash], [one.seed, one.seed], [one.flags] * 2, device=0)
    got = stage(env, w, [request(rng, env["model"][1])], [5], [_rb(rng, 32)], signers=False)
    assert got["status"].tolist() == [la.ACCEPTED] and got["slot"].tolist() == [5]


def test_keyset_rows_from_an_exchange(env):
    from reticulum_amd import device
    rng = np.random.Generator(np.random.PCG64(9))
    w = World(rng)
    n = 70
    prv, pub, salt = ([_rb(rng, k) for _ in range(n)] for k in (32, 32, 16))
    rows = [int(r) for r in rng.permutation(N_KEYS)] + [N_KEYS + k for k in range(n - N_KEYS)]
    mask = [int(i % 3 != 1) for i in range(n)]
    as_rows = lambda b, k: _t(np.frombuffer(b"".join(b), np.uint8).reshape(n, k))       # noqa: E731
    device.keyset_set_rows_x25519(w.ks, as_rows(prv, 32), as_rows(pub, 32), as_rows(salt, 16),
                                  _t(np.array(rows, np.int32)), mask=_t(np.array(mask, np.uint8)))
    for i in range(n):
        if mask[i] and rows[i] < N_KEYS:
            w.keys[rows[i]] = la.hkdf(64, la.x25519(prv[i], pub[i][:31] + bytes([pub[i][31] & 0x7F])), salt[i])
    toks = [ctoken.encrypt(k, _rb(rng, 16), b"row %d" % j) for j, k in enumerate(w.keys)]
    back, status = w.ks.decrypt_batch(toks, key_idx=np.arange(N_KEYS, dtype=np.uint32))
    assert (status == 0).all() and back.to_list() == [b"row %d" % j for j in range(N_KEYS)]


def test_host_form(env):
    import reticulum_amd as rt
    rng = np.random.Generator(np.random.PCG64(10))
    w = World(rng)
    c = next(c for c in env["vec"]["cases"] if c["reached"] == "accepted" and c["nh_mtu"] == 1196)
    res = rt.accept_requests_batch([other_packet(rng), c["raw"]], w.ks, w.tab, env["dests"],
                                   env["vec"]["transport_id"], [7], [c["ephemeral"]], nh_mtu=1196, signers=w.signers)
    assert res[0] == {"status": la.NOT_REQUEST, "slot": -1, "link_id": None, "mtu": None, "lrproof": None}
    assert res[1] == {"status": la.ACCEPTED, "slot": 7, "link_id": c["link_id"], "mtu": c["mtu"],
                      "lrproof": c["lrproof"]}
    assert rt.accept_requests_batch([], w.ks, w.tab, env["dests"], env["vec"]["transport_id"], [], []) == []
