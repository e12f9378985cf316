"""pipeline.inbound(accept=...): link requests answered inside the read.

One framed stream with access codes holds an announce, DATA and PROOF packets
on links that exist, and link requests of every fate: accepted ones, each
followed (one also preceded) in the same read by DATA packets on the new link
that are encrypted under the model's key; one replayed; one to a destination
that accepts none; one with a forged access code.  The read runs with the
access-code check, the packet hash list, the link table and the signers, and is
held to the model of tests/link_accept_helpers.py (which test_link_accept.py
ties to the reference) and, for the packet proofs of the new links, of
tests/proof_helpers.py.  A stream without a request gives, with ``accept``,
exactly what it gives without."""
import numpy as np
import pytest

import announce_helpers as ah
import ifac_helpers as ih
import link_accept_helpers as la
import link_helpers as lh
import proof_helpers as ph
from oracle import ctoken
from oracle import wire as ow

pytestmark = pytest.mark.gpu

ISZ = 16
N_KEYS = 16
SLOTS = [5, 6, 7, 8, 9]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _request(rng, dest, mtu=None):
    data = _rb(rng, 64) + (la.signalling(mtu) if mtu is not None else b"")
    return bytes([la.LINKREQUEST, 0]) + dest.hash + b"\x00" + data


def _data(link_id, key, context, pt, rng):
    return bytes([lh.LINK << 2 | lh.DATA, 0]) + link_id + bytes([context]) + ctoken.encrypt(key, _rb(rng, 16), pt)


@pytest.fixture(scope="module")
def case():
    vec = la.vectors()
    rng = np.random.Generator(np.random.PCG64(2127))
    dests = la.fixture_dests(vec)            # 0: PROVE_ALL, 1: HAS_CHANNEL, 2: accepts no requests
    keys = [_rb(rng, 64) for _ in range(N_KEYS)]
    old_ids = [_rb(rng, 16), _rb(rng, 16)]
    eph = [_rb(rng, 32) for _ in SLOTS]
    req = {name: _request(rng, dests[d], mtu) for name, d, mtu in
           (("A", 0, 700), ("B", 1, None), ("C", 2, 500), ("D", 0, 500), ("E", 1, 500), ("F", 1, 9000))}
    # what the requests that get through become, in stream order: A, B, D, F take slots 5, 6, 7, 8
    born = {}
    for k, name in enumerate("ABDF"):
        st, (dest, link_id, mtu, peer_pub, peer_sig) = la.decide(req[name], dests, vec["transport_id"], 1196)
        key, proof = la.establish(dest, link_id, mtu, peer_pub, eph[k])
        born[name] = dict(slot=SLOTS[k], link_id=link_id, mtu=mtu, key=key, lrproof=proof, dest=dest, peer=peer_sig)
    assert born["A"]["mtu"] == 700 and born["B"]["mtu"] == 500 and born["F"]["mtu"] == 1196
    a = ah.Announcer(rng)
    frames = [
        ("old data", _data(old_ids[0], keys[0], lh.NONE, b"on a link that exists", rng)),
        ("announce", ah.raw_packet(*a.data(b"app", False), False, 0)),
        ("request A", req["A"]),
        ("data A", _data(born["A"]["link_id"], born["A"]["key"], lh.NONE, b"first packet on link A", rng)),
        ("old proof", bytes([lh.LINK << 2 | lh.PROOF, 0]) + old_ids[1] + b"\x00" + _rb(rng, 96)),
        ("replay A", req["A"]),
        ("request B", req["B"]),
        ("channel B", _data(born["B"]["link_id"], born["B"]["key"], lh.CHANNEL, b"channel data on link B", rng)),
        ("data B", _data(born["B"]["link_id"], born["B"]["key"], lh.NONE, b"plain data on link B", rng)),
        ("request C", req["C"]),
        ("data D early", _data(born["D"]["link_id"], born["D"]["key"], lh.NONE, b"ahead of its request", rng)),
        ("request D", req["D"]),
        ("forged E", req["E"]),
        ("request F", req["F"]),
        ("data F wrong key", _data(born["F"]["link_id"], keys[3], lh.NONE, b"under another key", rng)),
        ("old data 2", _data(old_ids[0], keys[0], lh.NONE, b"and one more", rng)),
    ]
    return dict(vec=vec, dests=dests, keys=keys, old_ids=old_ids, eph=eph, born=born, frames=frames,
                ifac_key=_rb(rng, 64), seeds=[_rb(rng, 32) for _ in range(N_KEYS)],
                peers=[_rb(rng, 32) for _ in range(N_KEYS)])


def _wire(c, frames):
    out = []
    for name, raw in frames:
        code = ih.code(c["ifac_key"], raw, ISZ)
        if name.startswith("forged"):
            code = bytes([code[0] ^ 0x80]) + code[1:]
        out.append(ow.hdlc_frame(ow.ifac_mask(raw, code, c["ifac_key"])))
    return b"".join(out)


def _world(c):
    import reticulum_amd as rt
    ks = rt.KeySet(np.frombuffer(b"".join(c["keys"]), np.uint8).reshape(N_KEYS, 64), device=0)
    tab = rt.LinkTable(32, device=0)
    assert tab.insert(c["old_ids"], [0, 1]).cpu().tolist() == [lh.OK] * 2
    flags = [ph.PROVE_ALL] + [0] * (N_KEYS - 1)
    signers = rt.LinkSigners(c["seeds"], c["peers"], flags, device=0)
    d = c["dests"]
    dests = rt.LinkDestinations([x.hash for x in d], [x.seed for x in d], [x.flags for x in d], device=0)
    return ks, tab, signers, dests


def _read(c, frames, world, accept, n_pairs=None):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    ks, tab, signers, dests = world
    buf = torch.frombuffer(bytearray(_wire(c, frames)), dtype=torch.uint8).to("cuda:0")
    kw = dict(check_ifac=True, links=tab, signers=signers, announces=True, seen=rt.PacketHashlist(1024, device=0),
              transport_identity=_t(np.frombuffer(c["vec"]["transport_id"], np.uint8)))
    if accept:
        kw["accept"] = dict(destinations=dests, slots=_t(np.array(SLOTS, np.int32)), nh_mtu=1196,
                            ephemeral_privates=_t(np.frombuffer(b"".join(c["eph"]), np.uint8).reshape(len(SLOTS), 32)))
    res = pipeline.inbound(ks, buf, _t(np.frombuffer(c["ifac_key"], np.uint8)), ISZ, n_pairs or 2 * len(frames), **kw)
    torch.cuda.synchronize()
    return res


def test_requests_answered_inside_the_read(case):
    import torch
    c = case
    world = _world(c)
    ks, tab, signers, _ = world
    frames, born = c["frames"], c["born"]
    n = len(frames)
    res = _read(c, frames, world, accept=True)
    assert int(res["n_frames"]) == n
    names = [f[0] for f in frames]
    at = {name: i for i, name in enumerate(names)}
    want = {"request A": la.ACCEPTED, "replay A": la.NOT_REQUEST, "request B": la.ACCEPTED,
            "request C": la.NOT_ACCEPTING, "request D": la.ACCEPTED, "forged E": la.NOT_REQUEST,
            "request F": la.ACCEPTED}
    st = res["linkreq_status"].cpu().numpy()
    assert st.dtype == np.int32 and st.shape == (2 * n,)
    assert st[:n].tolist() == [want.get(name, la.NOT_REQUEST) for name in names]
    assert (st[n:] == la.NOT_REQUEST).all()
    # the replay was dropped by the packet filter and the forged one by the access-code check: neither took a slot
    assert res["filter_status"].cpu()[at["replay A"]] == 5 and res["ifac_status"].cpu()[at["forged E"]] == 2
    slot = res["accepted_link"].cpu().numpy()
    by_request = {"request " + k: v for k, v in born.items()}
    assert slot.tolist() == [by_request[name]["slot"] if name in by_request else -1 for name in names] + [-1] * n
    ids, mtu = res["link_id"].cpu().numpy(), res["link_mtu"].cpu().numpy()
    rows, plen = res["lr_proofs"].cpu().numpy(), res["lr_proof_len"].cpu().numpy()
    assert rows.shape == (2 * n, 128) and ids.shape == (2 * n, 16)
    for i, name in enumerate(names):
        b = by_request.get(name)
        if b is None:
            assert plen[i] == 0 and mtu[i] == 0 and not ids[i].any(), name
            continue
        assert ids[i].tobytes() == b["link_id"] and mtu[i] == b["mtu"], name
        assert plen[i] == la.LRPROOF_LEN and rows[i, :118].tobytes() == b["lrproof"], name
    assert not plen[n:].any()
    # the read's own packets on the new links: dispatched to the new slot and opened under the new key
    link, status = res["link"].cpu().numpy(), res["status"].cpu().numpy()
    pt, pt_off, pt_len = res["pt"].cpu().numpy(), res["pt_off"].cpu().numpy(), res["pt_len"].cpu().numpy()
    for name, who, text in (("data A", "A", b"first packet on link A"), ("channel B", "B", b"channel data on link B"),
                            ("data B", "B", b"plain data on link B"), ("data D early", "D", b"ahead of its request"),
                            ("old data", None, b"on a link that exists"), ("old data 2", None, b"and one more")):
        i = at[name]
        assert link[i] == (born[who]["slot"] if who else 0) and status[i] == 0, name
        assert pt[pt_off[i]:pt_off[i] + pt_len[i]].tobytes() == text, name
    assert link[at["data F wrong key"]] == born["F"]["slot"] and status[at["data F wrong key"]] == 2     # BAD_HMAC
    # and proved where the destination proves: A's link proves all, B's has a channel
    proofs, proof_len = res["proofs"].cpu().numpy(), res["proof_len"].cpu().numpy()
    proved = {"old data": (c["old_ids"][0], c["seeds"][0]), "old data 2": (c["old_ids"][0], c["seeds"][0]),
              "data A": (born["A"]["link_id"], c["dests"][0].seed), "data D early": (born["D"]["link_id"],
                                                                                   c["dests"][0].seed),
              "channel B": (born["B"]["link_id"], c["dests"][1].seed)}
    for i, (name, raw) in enumerate(frames):
        if name in proved:
            link_id, seed = proved[name]
            assert proof_len[i] == ph.PROOF_LEN, name
            assert proofs[i, :115].tobytes() == ph.proof_packet(link_id, ow.unpack(raw)["packet_hash"], seed), name
        else:
            assert proof_len[i] == 0, name
    # when the call returns: table, signers
    values, found = tab.lookup([b["link_id"] for b in born.values()])
    assert values.cpu().tolist() == [b["slot"] for b in born.values()] and found.all()
    assert len(tab) == 2 + len(born)
    for b in born.values():
        assert signers.peer_publics[b["slot"]].cpu().numpy().tobytes() == b["peer"]
        assert int(signers.flags[b["slot"]]) == b["dest"].flags & 3
        assert signers.seeds[b["slot"]].cpu().numpy().tobytes() == b["dest"].seed
        assert signers.publics[b["slot"]].cpu().numpy().tobytes() == b["dest"].public
    assert signers.peer_publics[9].cpu().numpy().tobytes() == c["peers"][9]          # a slot nobody took
    assert torch.equal(signers.flags.cpu()[:5], torch.tensor([ph.PROVE_ALL, 0, 0, 0, 0], dtype=torch.uint8))


def test_a_read_without_requests_is_the_read_without_accept(case):
    import torch
    c = case
    frames = [f for f in c["frames"] if "request" not in f[0] and "replay" not in f[0] and "forged" not in f[0]]
    n = len(frames)
    off = _read(c, frames, _world(c), accept=False)
    world = _world(c)
    on = _read(c, frames, world, accept=True)
    assert set(on) == set(off) | {"linkreq_status", "accepted_link", "link_id", "link_mtu", "lr_proofs", "lr_proof_len"}
    assert int(on["n_frames"]) == n == int(off["n_frames"])
    for k in off:
        a, b = on[k].cpu(), off[k].cpu()
        if k in ("n_frames", "frame_status", "counts"):
            assert torch.equal(a, b), k
        elif k == "pt":
            for i in range(n):
                lo, ln = int(on["pt_off"][i]), int(on["pt_len"][i])
                assert torch.equal(a[lo:lo + ln], b[lo:lo + ln]), (k, i)
        elif k == "proofs":
            for i in range(n):
                assert torch.equal(a[i, :int(on["proof_len"][i])], b[i, :int(off["proof_len"][i])]), (k, i)
        elif k == "frame_len":
            assert torch.equal(a[:int(on["counts"][0])], b[:int(off["counts"][0])]), k
        else:
            assert torch.equal(a[:n], b[:n]), k
    assert (on["linkreq_status"].cpu() == la.NOT_REQUEST).all() and (on["accepted_link"].cpu() == -1).all()
    assert not on["lr_proof_len"].cpu().any() and len(world[1]) == 2


def test_accept_argument_errors(case):
    import torch
    from reticulum_amd import pipeline
    c = case
    ks, tab, signers, dests = _world(c)
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    acc = dict(destinations=dests, slots=_t(np.array(SLOTS, np.int32)),
               ephemeral_privates=torch.zeros((len(SLOTS), 32), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError, match="accept needs links"):
        pipeline.inbound(ks, buf, None, 0, 4, accept=acc, links=tab)
    with pytest.raises(ValueError, match="one row per slot"):
        pipeline.inbound(ks, buf, None, 0, 4, links=tab, transport_identity=buf[:16],
                         accept=dict(acc, ephemeral_privates=acc["ephemeral_privates"][:2]))
