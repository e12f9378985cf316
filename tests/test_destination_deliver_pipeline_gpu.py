"""pipeline.inbound(deliver=...): packets for the node's SINGLE destinations
opened and proved inside the read.

One framed stream with access codes interleaves DATA packets on two links,
SINGLE packets to several destinations (opened by the newest ratchet, by a
later one, by the identity's key, by nothing), an announce, a link request to
one of the same destinations (``accept`` and ``deliver`` together) with a packet
on the new link behind it, junk, a replayed SINGLE packet and one with a forged
access code.  The read runs with the access-code check, with and without the
packet hash list, aligned and unaligned, and is held to the model of
tests/destination_deliver_helpers.py; every column that exists without
``deliver`` is bit-identical with and without it, but for ``status``, ``pt_len``
and ``pt_off`` of the frames the stage opens or rejects."""
import numpy as np
import pytest

import announce_helpers as ah
import destination_deliver_helpers as dd
import ifac_helpers as ih
import link_accept_helpers as la
import link_helpers as lh
from oracle import ctoken
from oracle import wire as ow

pytestmark = pytest.mark.gpu

ISZ = 16
N_KEYS = 8
SLOTS = [4, 5]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _link_data(link_id, key, pt, rng):
    return bytes([lh.LINK << 2 | lh.DATA, 0]) + link_id + b"\x00" + ctoken.encrypt(key, _rb(rng, 16), pt)


@pytest.fixture(scope="module")
def case():
    rng = np.random.Generator(np.random.PCG64(2202))
    model = [dd.make_dest(rng, 0, dd.F_PROVE_ALL), dd.make_dest(rng, 2, dd.F_PROVE_ALL), dd.make_dest(rng, 5, 0),
             dd.make_dest(rng, 1, dd.F_PROVE_ALL | dd.F_ENFORCE)]
    accepting = [la.Dest(m.hash, m.seed, la.F_ACCEPTS) for m in model]
    tid = _rb(rng, 16)
    keys = [_rb(rng, 64) for _ in range(N_KEYS)]
    old_ids = [_rb(rng, 16), _rb(rng, 16)]
    eph = [_rb(rng, 32) for _ in SLOTS]
    pool = [_rb(rng, 32) for _ in range(4)]

    def single(k, rank, text):
        return dd.packet(dd.seal(model[k], rank, text, pool[int(rng.integers(4))], _rb(rng, 16)), model[k].hash)

    request = bytes([la.LINKREQUEST, 0]) + model[1].hash + b"\x00" + _rb(rng, 64) + la.signalling(500)
    st, (dest, link_id, mtu, peer_pub, peer_sig) = la.decide(request, accepting, tid, 500)
    new_key, lrproof = la.establish(dest, link_id, mtu, peer_pub, eph[0])
    a = ah.Announcer(rng)
    replayed = single(1, 0, b"sent twice")
    frames = [
        ("link 0", _link_data(old_ids[0], keys[0], b"on link 0", rng)),
        ("single 0 identity", single(0, None, b"to destination 0")),
        ("single 1 newest", single(1, 0, b"newest ratchet")),
        ("announce", ah.raw_packet(*a.data(b"app", False), False, 0)),
        ("link 1", _link_data(old_ids[1], keys[1], b"on link 1", rng)),
        ("single 1 older", single(1, 1, b"older ratchet")),
        ("request", request),
        ("single 2 last", single(2, 4, b"the last of five")),
        ("data on the new link", _link_data(link_id, new_key, b"first packet on the new link", rng)),
        ("replayed", replayed),
        ("junk", bytes([lh.LINK << 2 | lh.DATA, 0]) + _rb(rng, 16) + b"\x00" + _rb(rng, 70)),
        ("single 3 enforced identity", single(3, None, b"never opened")),
        ("replay", replayed),
        ("forged single", single(0, None, b"forged access code")),
        ("single 2 identity", single(2, None, b"after five ratchets")),
        ("group to single", dd.packet(dd.seal(model[0], None, b"wrong type", pool[0], _rb(rng, 16)), model[0].hash,
                                      dtype=dd.GROUP)),
        ("link 0 again", _link_data(old_ids[0], keys[0], b"and one more", rng)),
        ("single 3 ratchet", single(3, 0, b"enforced, by its ratchet")),
    ]
    return dict(rng=rng, model=model, accepting=accepting, tid=tid, keys=keys, old_ids=old_ids, eph=eph,
                frames=frames, ifac_key=_rb(rng, 64), link_id=link_id, lrproof=lrproof)


def _wire(c, frames):
    out = []
    for name, raw in frames:
        code = ih.code(c["ifac_key"], raw, ISZ)
        if name.startswith("forged"):
            code = bytes([code[0] ^ 0x80]) + code[1:]
        out.append(ow.hdlc_frame(ow.ifac_mask(raw, code, c["ifac_key"])))
    return b"".join(out)


def _read(c, deliver, seen, aligned):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    frames, m = c["frames"], c["model"]
    ks = rt.KeySet(np.frombuffer(b"".join(c["keys"]), np.uint8).reshape(N_KEYS, 64), device=0)
    tab = rt.LinkTable(32, device=0)
    assert tab.insert(c["old_ids"], [0, 1]).cpu().tolist() == [lh.OK] * 2
    acc = c["accepting"]
    kw = dict(check_ifac=True, links=tab, announces=True, aligned=aligned,
              transport_identity=_t(np.frombuffer(c["tid"], np.uint8)))
    kw["accept"] = dict(destinations=rt.LinkDestinations([x.hash for x in acc], [x.seed for x in acc],
                                                         [x.flags for x in acc], device=0),
                        slots=_t(np.array(SLOTS, np.int32)), nh_mtu=500,
                        ephemeral_privates=_t(np.frombuffer(b"".join(c["eph"]), np.uint8).reshape(len(SLOTS), 32)))
    if seen:
        kw["seen"] = rt.PacketHashlist(1024, device=0)
    if deliver:
        kw["deliver"] = rt.SingleDestinations([x.hash for x in m], [x.prv for x in m], [x.identity_hash for x in m],
                                              [x.seed for x in m], [x.flags for x in m], [x.ratchets for x in m],
                                              max_frames=2 * len(frames), retry_trials=32, device=0)
    buf = torch.frombuffer(bytearray(_wire(c, frames)), dtype=torch.uint8).to("cuda:0")
    res = pipeline.inbound(ks, buf, _t(np.frombuffer(c["ifac_key"], np.uint8)), ISZ, 2 * len(frames), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("seen", [True, False])
@pytest.mark.parametrize("aligned", [True, False])
def test_single_packets_inside_the_read(case, seen, aligned):
    import torch
    c = case
    frames, model = c["frames"], c["model"]
    n = len(frames)
    names = [f[0] for f in frames]
    at = {name: i for i, name in enumerate(names)}
    on, off = _read(c, True, seen, aligned), _read(c, False, seen, aligned)
    assert int(on["n_frames"]) == n == int(off["n_frames"])
    assert set(on) == set(off) | {"deliver_status", "destination", "ratchet", "dest_proofs", "dest_proof_len"}
    # the model over the frames that reach the stage: the forged one never does, nor the replay behind the list
    dropped = {at["forged single"]} | ({at["replay"]} if seen else set())
    raws = [raw for i, (_, raw) in enumerate(frames) if i not in dropped]
    budget = dd.second_pass_pairs(raws, model)
    assert budget <= 32
    want = iter(dd.deliver(raws, model, 32))
    nothing = {"status": dd.NOT_DATA, "dest": -1, "ratchet": -1, "plaintext": None, "proof": None}
    want = [nothing if i in dropped else next(want) for i in range(n)]
    assert on["ifac_status"][at["forged single"]] == 2
    if seen:
        assert on["filter_status"][at["replay"]] == 5
    st, dest, ratchet = (on[k].numpy() for k in ("deliver_status", "destination", "ratchet"))
    assert st.dtype == np.int32 and st.shape == (2 * n,)
    plen, rows = on["dest_proof_len"].numpy(), on["dest_proofs"].numpy()
    pt, pt_off, pt_len, status = (on[k].numpy() for k in ("pt", "pt_off", "pt_len", "status"))
    for i, w in enumerate(want):
        name = names[i]
        assert (st[i], dest[i], ratchet[i]) == (w["status"], w["dest"], w["ratchet"]), name
        assert st[i] != dd.DEFERRED
        if w["status"] == dd.DELIVERED:
            assert status[i] == 0 and pt[pt_off[i]:pt_off[i] + pt_len[i]].tobytes() == w["plaintext"], name
        if w["proof"] is not None:
            assert plen[i] == 83 and rows[i, :83].tobytes() == w["proof"], name
        else:
            assert plen[i] == 0, name
    assert (st[n:] == dd.NOT_DATA).all() and not plen[n:].any()
    expect = {"single 0 identity": (dd.DELIVERED, -1), "single 1 newest": (dd.DELIVERED, 0),
              "single 1 older": (dd.DELIVERED, 1), "single 2 last": (dd.DELIVERED, 4),
              "single 2 identity": (dd.DELIVERED, -1), "single 3 enforced identity": (dd.NOT_OPENED, -1),
              "single 3 ratchet": (dd.DELIVERED, 0), "replayed": (dd.DELIVERED, 0),
              "replay": (dd.NOT_DATA if seen else dd.DELIVERED, -1 if seen else 0), "forged single": (dd.NOT_DATA, -1)}
    for name, (s, r) in expect.items():
        assert (st[at[name]], ratchet[at[name]]) == (s, r), name
    assert plen[at["single 2 last"]] == 0                       # destination 2 proves nothing
    # accept and deliver together: the request to destination 1 is answered, the packet behind it opened
    i = at["request"]
    assert on["linkreq_status"][i] == la.ACCEPTED and on["accepted_link"][i] == SLOTS[0]
    assert on["lr_proofs"][i, :118].numpy().tobytes() == c["lrproof"] and st[i] == dd.NOT_DATA
    i = at["data on the new link"]
    assert on["link"][i] == SLOTS[0] and status[i] == 0 and st[i] == dd.NOT_DATA
    assert pt[pt_off[i]:pt_off[i] + pt_len[i]].tobytes() == b"first packet on the new link"
    # every column that exists without deliver is bit-identical, but for what the stage opens or rejects
    opened = torch.from_numpy(np.isin(st[:n], (dd.DELIVERED, dd.NOT_OPENED)))
    assert opened.sum() == sum(w["status"] in (dd.DELIVERED, dd.NOT_OPENED) for w in want)
    for k in off:
        a, b = on[k], off[k]
        if k in ("n_frames", "frame_status", "counts"):
            assert torch.equal(a, b), k
        elif k == "pt":
            for i in range(n):
                if not opened[i]:
                    lo, ln = int(off["pt_off"][i]), int(off["pt_len"][i])
                    assert torch.equal(a[lo:lo + ln], b[lo:lo + ln]), (k, i)
        elif k == "lr_proofs":
            for i in range(n):
                assert torch.equal(a[i, :int(on["lr_proof_len"][i])], b[i, :int(off["lr_proof_len"][i])]), (k, i)
        elif k == "frame_len":
            assert torch.equal(a[:int(on["counts"][0])], b[:int(off["counts"][0])]), k
        elif k in ("status", "pt_len", "pt_off"):
            assert torch.equal(a[:n][~opened], b[:n][~opened]), k
            assert torch.equal(a[n:], b[n:]) or k == "pt_off", k
        else:
            assert torch.equal(a[:n], b[:n]), k


def test_deliver_argument_errors(case):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    m = case["model"]
    d = rt.SingleDestinations([x.hash for x in m], [x.prv for x in m], [x.identity_hash for x in m],
                              [x.seed for x in m], [x.flags for x in m], max_frames=4, retry_trials=0, device=0)
    ks = rt.KeySet(np.zeros((1, 64), np.uint8), device=0)
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="deliver needs links"):
        pipeline.inbound(ks, buf, None, 0, 4, deliver=d)
    with pytest.raises(ValueError, match="deliver needs links"):
        pipeline.inbound(ks, buf, None, 0, 8, deliver=d, links=rt.LinkTable(4, device=0))
    with pytest.raises(ValueError, match="distinct"):
        rt.SingleDestinations([m[0].hash, m[0].hash], [m[0].prv] * 2, [m[0].identity_hash] * 2, [m[0].seed] * 2,
                              [0, 0], device=0)
