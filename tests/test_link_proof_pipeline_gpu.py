"""pipeline.inbound(establish=...): link request proofs validated inside the read.

One framed stream with access codes holds LRPROOFs of several fates, DATA on
the new links behind and ahead of their proofs, a forged access code and a
replayed proof; the read runs with the access-code check, the packet hash
list, the link table and the signers, and is held to the model of
tests/link_proof_helpers.py.  Two nodes' worth of state in one process
complete a handshake device to device; and a read without any LRPROOF gives,
with ``establish``, exactly what it gives without."""
import numpy as np
import pytest

import ed25519_ref as ed
import ifac_helpers as ih
import link_helpers as lh
import link_proof_helpers as lp
import proof_helpers as ph
from oracle import ctoken
from oracle import wire as ow
from test_link_proof_gpu import Dest, _rb, _t

pytestmark = pytest.mark.gpu

ISZ = 16
N_KEYS = 16


def _data(link_id, key, context, pt, rng):
    return bytes([lh.LINK << 2 | lh.DATA, 0]) + link_id + bytes([context]) + ctoken.encrypt(key, _rb(rng, 16), pt)


def _wire(ifac_key, frames):
    out = []
    for name, raw in frames:
        code = ih.code(ifac_key, raw, ISZ)
        if name.startswith("forged code"):
            code = bytes([code[0] ^ 0x80]) + code[1:]
        out.append(ow.hdlc_frame(ow.ifac_mask(raw, code, ifac_key)))
    return b"".join(out)


class Node:
    def __init__(self, rng):
        import reticulum_amd as rt
        self.keys = [_rb(rng, 64) for _ in range(N_KEYS)]
        self.ks = rt.KeySet(np.frombuffer(b"".join(self.keys), np.uint8).reshape(N_KEYS, 64), device=0)
        self.tab = rt.LinkTable(32, device=0)
        self.signers = rt.LinkSigners([_rb(rng, 32) for _ in range(N_KEYS)], [_rb(rng, 32) for _ in range(N_KEYS)],
                                      [0] * N_KEYS, device=0)
        self.pending = rt.PendingLinks(8, device=0)
        self.seen = rt.PacketHashlist(1024, device=0)
        self.tid = _rb(rng, 16)
        self.ifac_key = _rb(rng, 64)

    def read(self, frames, establish=True, seen=True, **kw):
        import torch
        from reticulum_amd import pipeline
        buf = torch.frombuffer(bytearray(_wire(self.ifac_key, frames)), dtype=torch.uint8).to("cuda:0")
        args = dict(check_ifac=True, links=self.tab, signers=self.signers,
                    transport_identity=_t(np.frombuffer(self.tid, np.uint8)))
        if seen:
            args["seen"] = self.seen
        if establish:
            args["establish"] = self.pending
        args.update(kw)
        res = pipeline.inbound(self.ks, buf, _t(np.frombuffer(self.ifac_key, np.uint8)), ISZ, 2 * len(frames), **args)
        torch.cuda.synchronize()
        return res


def _open(rng, node, dest, slot, flags=0):
    link = lp.Pending(_rb(rng, 16), _rb(rng, 32), dest.public, _rb(rng, 32), flags, slot, 1)
    assert node.pending.add([link.link_id], [link.prv], [link.dest_public], [link.sig_seed], [flags], [slot],
                            [1]).tolist() == [0]
    return link


def _pt(res, i):
    off, n = int(res["pt_off"][i]), int(res["pt_len"][i])
    return res["pt"][off:off + n].cpu().numpy().tobytes()


def test_proofs_validated_inside_the_read():
    rng = np.random.Generator(np.random.PCG64(2270))
    node, d = Node(rng), Dest(rng)
    a, b, c, e = (_open(rng, node, d, s, f) for s, f in ((5, ph.PROVE_ALL), (6, 0), (7, 0), (8, 0)))
    proofs = {k: d.proof(rng, l, mtu=m) for k, l, m in (("a", a, 700), ("b", b, None), ("c", c, 500), ("e", e, 500))}
    model = {l.link_id: l.copy() for l in (a, b, c, e)}
    want = lp.run([proofs["a"], proofs["b"], d.proof(rng, c, forge=True)], model, {})
    assert [w[0] for w in want] == [lp.ACTIVATED, lp.ACTIVATED, lp.BAD_SIGNATURE]
    ka, kb = model[a.link_id].derived_key, model[b.link_id].derived_key
    forged_c = d.proof(rng, c, forge=True)
    frames = [
        ("data b early", _data(b.link_id, kb, lh.NONE, b"ahead of its proof", rng)),
        ("proof a", proofs["a"]),
        ("data a", _data(a.link_id, ka, lh.NONE, b"first packet on link a", rng)),
        ("replay a", proofs["a"]),
        ("proof b", proofs["b"]),
        ("forged code e", proofs["e"]),
        ("forged c", forged_c),
        ("proof c", proofs["c"]),
        ("data a wrong key", _data(a.link_id, node.keys[3], lh.NONE, b"under another key", rng)),
    ]
    res = node.read(frames)
    names = [n for n, _ in frames]
    at = {n: i for i, n in enumerate(names)}
    assert int(res["n_frames"]) == len(frames)
    st = res["lrproof_status"][:len(frames)].cpu().tolist()
    assert st == [lp.NOT_LRPROOF, lp.ACTIVATED, lp.NOT_LRPROOF, lp.NOT_PENDING, lp.ACTIVATED, lp.NOT_LRPROOF,
                  lp.BAD_SIGNATURE, lp.NOT_PENDING, lp.NOT_LRPROOF]
    assert res["established_link"][:len(frames)].cpu().tolist() == [-1, 5, -1, -1, 6, -1, -1, -1, -1]
    assert res["link_mtu"][at["proof a"]].item() == 700 and res["link_mtu"][at["proof b"]].item() == 500
    # the replay in the same read finds the link up (the filter defers a proof's hash to the stage, so it
    # passes there); the forged code was dropped by the access-code check and never reached the stage
    assert res["filter_status"][at["replay a"]].item() == 0 and res["ifac_status"][at["forged code e"]].item() == 2
    # DATA behind and ahead of its proof is decrypted under the new key, and proved where the flags say so
    token = res["status"][:len(frames)].cpu().tolist()
    assert token[at["data a"]] == 0 and _pt(res, at["data a"]) == b"first packet on link a"
    assert token[at["data b early"]] == 0 and _pt(res, at["data b early"]) == b"ahead of its proof"
    assert token[at["data a wrong key"]] == 2
    plen = res["proof_len"][:len(frames)].cpu().tolist()
    assert plen[at["data a"]] == 115 and plen[at["data b early"]] == 0
    row = res["proofs"][at["data a"]].cpu().numpy().tobytes()[:115]
    h = lp.packet_hash(frames[at["data a"]][1])
    assert row[:19] == b"\x0f\x00" + a.link_id + b"\x00" and row[19:51] == h
    assert ed.verify(ed.public_key(a.sig_seed), row[51:], h)
    # state, and the hash list: the proofs that reached validate_proof, the replay's included, not e's
    ids = [l.link_id for l in (a, b, c, e)]
    assert node.pending.state(ids).tolist() == [lp.ACTIVE, lp.ACTIVE, lp.HANDSHAKE, lp.PENDING]
    hs = [lp.packet_hash(r) for r in (proofs["a"], proofs["b"], forged_c, proofs["c"], proofs["e"])]
    assert node.seen.contains(hs).cpu().tolist() == [1, 1, 1, 1, 0]
    values, found = node.tab.lookup(ids)
    assert values.cpu().tolist() == [5, 6, -1, -1]
    # e's proof, sent again with the right code, brings the link up in the next read
    # while a proof replayed in a later read is dropped by the filter, whose list learned its hash from the stage
    res = node.read([("proof e", proofs["e"]), ("replay a", proofs["a"])])
    assert res["lrproof_status"][:2].cpu().tolist() == [lp.ACTIVATED, lp.NOT_LRPROOF]
    assert res["established_link"][0].item() == 8 and res["filter_status"][1].item() == 5


def test_a_read_without_a_proof_is_untouched():
    rng = np.random.Generator(np.random.PCG64(3))
    node = Node(rng)
    ids = [_rb(rng, 16), _rb(rng, 16)]
    assert node.tab.insert(ids, [0, 1]).cpu().tolist() == [0, 0]
    frames = [("data", _data(ids[k & 1], node.keys[k & 1], lh.NONE, _rb(rng, 10 + k), rng)) for k in range(9)]
    frames.insert(4, ("proof", bytes([lh.LINK << 2 | lh.PROOF, 0]) + ids[1] + b"\x00" + _rb(rng, 96)))
    with_, without = node.read(frames, seen=False), node.read(frames, establish=False, seen=False)
    assert with_["lrproof_status"][:len(frames)].cpu().tolist() == [lp.NOT_LRPROOF] * len(frames)
    import torch
    n = len(frames)
    assert set(with_) == set(without) | {"lrproof_status", "established_link", "link_mtu"}
    for k in without:
        a, b = with_[k].cpu(), without[k].cpu()
        if k in ("n_frames", "frame_status", "counts"):
            assert torch.equal(a, b), k
        elif k == "pt":
            for i in range(n):
                lo, ln = int(with_["pt_off"][i]), int(with_["pt_len"][i])
                assert ln == int(without["pt_len"][i]) and torch.equal(a[lo:lo + ln], b[lo:lo + ln]), (k, i)
        elif k == "proofs":
            for i in range(n):
                assert torch.equal(a[i, :int(with_["proof_len"][i])], b[i, :int(without["proof_len"][i])]), (k, i)
        elif k == "frame_len":
            assert torch.equal(a[:int(with_["counts"][0])], b[:int(without["counts"][0])]), k
        else:
            assert torch.equal(a[:n], b[:n]), k
    assert len(node.tab) == 2


def test_a_handshake_device_to_device():
    """Node A opens a link to a destination of node B: A's requests go through
    B's ``accept``, B's LRPROOFs through A's ``establish``, and a token made
    under A's record opens under B's."""
    import reticulum_amd as rt
    rng = np.random.Generator(np.random.PCG64(4))
    A, B = Node(rng), Node(rng)
    seed = _rb(rng, 32)
    pub = ed.public_key(seed)
    x_pub = _rb(rng, 32)
    import hashlib
    name_hash = hashlib.sha256(b"linkproof.device").digest()[:10]
    dest_hash = hashlib.sha256(name_hash + hashlib.sha256(x_pub + pub).digest()[:16]).digest()[:16]
    dests = rt.LinkDestinations([dest_hash], [seed], [rt.link.ACCEPTS | rt.link.PROVE_ALL], device=0)
    raws, ids = rt.open_requests_batch([dest_hash] * 2, [pub] * 2, [_rb(rng, 32) for _ in range(2)],
                                       [_rb(rng, 32) for _ in range(2)], [3, 4], [1, 1], mtu=1196, pending=A.pending)
    res = B.read([("request", r) for r in raws], establish=False,
                 accept=dict(destinations=dests, slots=_t(np.array([9, 10], np.int32)), nh_mtu=1196,
                             ephemeral_privates=_t(np.frombuffer(_rb(rng, 64), np.uint8).reshape(2, 32))))
    assert res["linkreq_status"][:2].cpu().tolist() == [0, 0] and res["lr_proof_len"][:2].cpu().tolist() == [118, 118]
    assert res["link_id"][:2].cpu().numpy().tobytes() == b"".join(ids)
    lrproofs = [res["lr_proofs"][k].cpu().numpy().tobytes()[:118] for k in range(2)]
    res = A.read([("proof", p) for p in lrproofs])
    assert res["lrproof_status"][:2].cpu().tolist() == [lp.ACTIVATED] * 2
    assert res["established_link"][:2].cpu().tolist() == [3, 4] and res["link_mtu"][:2].cpu().tolist() == [1196] * 2
    assert A.pending.state(ids).tolist() == [lp.ACTIVE] * 2
    # a token encrypted under A's record decrypts under B's
    pts = [b"from a to b, link one", b"and on link two"]
    toks = A.ks.encrypt_batch(pts, key_idx=np.array([3, 4], dtype=np.uint32))
    back, status = B.ks.decrypt_batch([toks[k] for k in range(2)], key_idx=np.array([9, 10], dtype=np.uint32))
    assert (status == 0).all() and back.to_list() == pts
    # and the LRRTT is nine bytes on the new link
    assert len(rt.pack_rtt(0.0123)) == 9


def test_accept_and_establish_in_one_read():
    """One node, one read: a LINKREQUEST for one of its destinations and an
    LRPROOF for one of its pending links, with DATA on both new links.  Both
    stages write the one link table, key set and signers, and share the
    ``link_mtu`` column."""
    import reticulum_amd as rt
    import link_accept_helpers as la
    rng = np.random.Generator(np.random.PCG64(5))
    node, remote = Node(rng), Dest(rng)
    own = la.Dest(_rb(rng, 16), _rb(rng, 32), la.F_ACCEPTS | ph.PROVE_ALL)
    dests = rt.LinkDestinations([own.hash], [own.seed], [own.flags], device=0)
    # the link this node opened, and the proof that comes back for it
    opened = _open(rng, node, remote, 4, ph.PROVE_ALL)
    lrproof = remote.proof(rng, opened, mtu=700)
    model = {opened.link_id: opened.copy()}
    assert lp.run([lrproof], model, {})[0][:3] == (lp.ACTIVATED, 4, 700)
    k_open = model[opened.link_id].derived_key
    # the request another node sends to this node's destination
    request = rt.link.pack_link_request(own.hash, la.x25519(_rb(rng, 32), (9).to_bytes(32, "little")),
                                        ed.public_key(_rb(rng, 32)), mtu=900)
    eph = _rb(rng, 32)
    st, (dest, link_id, mtu, peer_pub, peer_sig) = la.decide(request, [own], node.tid, 1196)
    assert st == la.ACCEPTED and mtu == 900
    k_acc, want_proof = la.establish(dest, link_id, mtu, peer_pub, eph)
    frames = [
        ("request", request),
        ("proof", lrproof),
        ("data on the accepted link", _data(link_id, k_acc, lh.NONE, b"to this node's destination", rng)),
        ("data on the opened link", _data(opened.link_id, k_open, lh.NONE, b"on the link this node opened", rng)),
    ]
    n = len(frames)
    res = node.read(frames, accept=dict(destinations=dests, slots=_t(np.array([9, 10], np.int32)), nh_mtu=1196,
                                        ephemeral_privates=_t(np.frombuffer(eph + _rb(rng, 32), np.uint8).reshape(2, 32))))
    assert int(res["n_frames"]) == n
    assert res["linkreq_status"][:n].cpu().tolist() == [la.ACCEPTED] + [la.NOT_REQUEST] * 3
    assert res["lrproof_status"][:n].cpu().tolist() == [lp.NOT_LRPROOF, lp.ACTIVATED, lp.NOT_LRPROOF, lp.NOT_LRPROOF]
    assert res["accepted_link"][:n].cpu().tolist() == [9, -1, -1, -1]
    assert res["established_link"][:n].cpu().tolist() == [-1, 4, -1, -1]
    # one column for both stages: the request's MTU on the request's frame, the proof's on the proof's
    assert res["link_mtu"][:n].cpu().tolist() == [900, 700, 0, 0]
    assert res["link_id"][0].cpu().numpy().tobytes() == link_id
    assert res["lr_proof_len"][:n].cpu().tolist() == [118, 0, 0, 0]
    assert res["lr_proofs"][0].cpu().numpy().tobytes()[:118] == want_proof
    # both new links are in the one table, and their packets of the same read are decrypted and proved
    values, found = node.tab.lookup([link_id, opened.link_id])
    assert values.cpu().tolist() == [9, 4] and len(node.tab) == 2
    assert res["status"][:n].cpu().tolist()[2:] == [0, 0]
    assert _pt(res, 2) == b"to this node's destination" and _pt(res, 3) == b"on the link this node opened"
    assert res["key_idx"][:n].cpu().tolist()[2:] == [9, 4]
    assert res["proof_len"][:n].cpu().tolist() == [0, 0, 115, 115]
    for i, seed in ((2, own.seed), (3, opened.sig_seed)):
        row = res["proofs"][i].cpu().numpy().tobytes()[:115]
        assert ed.verify(ed.public_key(seed), row[51:], lp.packet_hash(frames[i][1])), i
    # the signers' rows of both slots, the pending row, and the hash list (the proof's hash through the stage)
    s = node.signers
    assert s.peer_publics[9].cpu().numpy().tobytes() == peer_sig and s.peer_publics[4].cpu().numpy().tobytes() == remote.public
    assert s.seeds[9].cpu().numpy().tobytes() == own.seed and s.seeds[4].cpu().numpy().tobytes() == opened.sig_seed
    assert node.pending.state([opened.link_id]).tolist() == [lp.ACTIVE]
    assert node.seen.contains([lp.packet_hash(r) for _, r in frames]).cpu().tolist() == [1, 1, 1, 1]
    # a second read with both stages and neither a request nor a proof changes nothing
    res = node.read([("data again", _data(link_id, k_acc, lh.NONE, b"once more", rng))],
                    accept=dict(destinations=dests, slots=_t(np.array([10], np.int32)), nh_mtu=1196,
                                ephemeral_privates=_t(np.frombuffer(_rb(rng, 32), np.uint8).reshape(1, 32))))
    assert res["status"][0].item() == 0 and res["link_mtu"][0].item() == 0 and len(node.tab) == 2
