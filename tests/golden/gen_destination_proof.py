"""Generate tests/golden/destination_proof_vectors.json from the reference's own code.

Runs only where the reference is at hand ($RNS_REFERENCE).  Fixtures for the
proofs that come back for packets sent to SINGLE destinations
(Transport.py:2326-2363 with packet.link unset; PacketReceipt.validate_proof,
Packet.py:480-524; ProofDestination, Packet.py:376-381; Identity.prove,
Identity.py:942-953).  Real RNS.Destination objects (OUT, SINGLE) over real
identities, real packets packed for them, real PacketReceipt objects in
Transport.receipts, and every raw proof handed to the reference's own
Transport.inbound(raw, interface) from an empty packet hash list each time, so
that a second copy of a proof reaches the receipts and is not dropped as a
replay.  Packet.send is replaced by a recorder,
Reticulum.should_use_implicit_proof by the case's setting and
Reticulum.get_instance by a stub.  Transport is disabled, so the reverse-table
step (Transport.py:2338-2347) does nothing.

  identities  the recipients: Ed25519 seed and public key;
  batches     per batch: a note; `receipts`, the receipts outstanding at its
              start as [packet hash, identity index or null], null for a receipt
              whose destination is a link; `raws`, the raw packets handed to
              Transport.inbound one after another; `delivered`, per raw the hash
              of the receipt that left Transport.receipts with status DELIVERED,
              or null; `left`, the hashes still outstanding at the end.
  A batch with `from_deliver` feeds proof rows that
  destination_deliver_vectors.json already holds (83 and 115 bytes) against
  receipts for the packets they prove.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_destination_proof.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")


def main():
    sys.path.insert(0, REF)
    import RNS
    from RNS.Cryptography import Ed25519PrivateKey, X25519PrivateKey

    rng = np.random.Generator(np.random.PCG64(2349))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    RNS.loglevel = -1
    Transport, Packet, Destination, Identity = RNS.Transport, RNS.Packet, RNS.Destination, RNS.Identity

    class Owner:
        is_connected_to_shared_instance = False

    Transport.owner = Owner()
    Transport.identity = Identity()

    sent = []
    real_send, real_implicit, real_instance = Packet.send, RNS.Reticulum.should_use_implicit_proof, \
        RNS.Reticulum.get_instance
    implicit = [True]

    def send(self):
        self.pack()
        sent.append(self.raw)

    Packet.send = send
    RNS.Reticulum.should_use_implicit_proof = staticmethod(lambda: implicit[0])

    class Interface:
        """The receiving interface, as far as Transport.inbound reads it."""
        ifac_identity = None
        r_stat_rssi = r_stat_snr = r_stat_q = None
        HW_MTU, AUTOCONFIGURE_MTU, FIXED_MTU = 1064, False, False

    class Instance:
        @staticmethod
        def get_packet_rssi(packet_hash):
            return None

        get_packet_snr = get_packet_q = get_packet_rssi

        @staticmethod
        def get_first_hop_timeout(destination_hash):
            return 6

    RNS.Reticulum.get_instance = staticmethod(lambda: Instance)
    Transport.ready = True
    was_enabled = getattr(RNS.Reticulum, "_Reticulum__transport_enabled", None)
    RNS.Reticulum._Reticulum__transport_enabled = False
    iface = Interface()

    try:
        idents = [Identity() for _ in range(4)]
        outs = [Destination(i, Destination.OUT, Destination.SINGLE, "proof", "fixture%d" % k)
                for k, i in enumerate(idents)]
        out = {"reference": "RNS/Transport.py:2326-2363; RNS/Packet.py:376-381, 480-524; RNS/Identity.py:942-953",
               "generator": "tests/golden/gen_destination_proof.py",
               "identities": [{"seed": i.sig_prv_bytes.hex(), "public": i.get_public_key()[32:].hex()} for i in idents],
               "batches": []}

        def a_link():
            """A real link, as the destination of a packet sent on it."""
            class LinkOwner:
                identity = Identity()
                type = Destination.SINGLE
                hash = rb(16)
            link = RNS.Link(owner=LinkOwner, peer_pub_bytes=X25519PrivateKey.generate().public_key().public_bytes(),
                            peer_sig_pub_bytes=Ed25519PrivateKey.generate().public_key().public_bytes())
            link.link_id = link.hash = rb(16)
            link.rtt = 0.1
            return link

        class OnLink:
            """A packet sent on a link, as PacketReceipt.__init__ reads it."""

            def __init__(self, link, h):
                self.destination, self._h = link, h

            def get_hash(self):
                return self._h

            def getTruncatedHash(self):
                return self._h[:16]

        def sent_packet(k):
            """A real packet for destination k, packed (encrypted for its identity)."""
            p = Packet(outs[k], rb(20))
            p.pack()
            return p

        def received(p):
            """The sent packet as the far end unpacks it."""
            q = Packet(None, p.raw)
            assert q.unpack()
            q.receiving_interface = iface
            assert q.packet_hash == p.get_hash()
            return q

        def prove(k, p, use_implicit):
            """Identity.prove at the far end: the raw PROOF packet it sends."""
            implicit[0] = use_implicit
            del sent[:]
            idents[k].prove(received(p))
            assert len(sent) == 1
            return sent[0]

        def forged(h, sig, use_implicit, address=None, dtype=Destination.SINGLE, context=Packet.NONE):
            """A PROOF packet as Packet.pack lays a proof out, from its parts."""
            address = h[:16] if address is None else address
            return bytes([(dtype << 2) | Packet.PROOF, 0]) + address + bytes([context]) + \
                (sig if use_implicit else h + sig)

        def flip(raw, at, bit=1):
            b = bytearray(raw)
            b[at] ^= bit
            return bytes(b)

        def inbound(raw):
            Transport.packet_hashlist, Transport.packet_hashlist_prev = set(), set()
            Transport.inbound(raw, iface)

        def batch(note, receipts, raws, **more):
            """receipts: [(PacketReceipt, identity index or None)]."""
            Transport.receipts = [r for r, _ in receipts]
            Transport.active_links, Transport.reverse_table = [], {}
            delivered = []
            for raw in raws:
                before = list(Transport.receipts)
                inbound(raw)
                gone = [r for r in before if r not in Transport.receipts]
                assert len(gone) <= 1 and all(r.status == RNS.PacketReceipt.DELIVERED for r in gone), note
                assert all(r.status == RNS.PacketReceipt.SENT for r in Transport.receipts), note
                delivered.append(gone[0].hash.hex() if gone else None)
            entry = {"note": note, "receipts": [[r.hash.hex(), k] for r, k in receipts], "raws": [r.hex() for r in raws],
                     "delivered": delivered, "left": [r.hash.hex() for r in Transport.receipts]}
            entry.update(more)
            out["batches"].append(entry)
            Transport.receipts = []
            return delivered

        def receipt(k, p=None):
            p = sent_packet(k) if p is None else p
            return RNS.PacketReceipt(p), k

        H = 19                                           # where the data of a HEADER_1 packet starts

        # explicit and implicit proofs as Identity.prove makes them
        ps = [sent_packet(k) for k in (0, 1, 2, 3)]
        raws = [prove(0, ps[0], True), prove(1, ps[1], False), prove(2, ps[2], True), prove(3, ps[3], False)]
        assert [len(r) for r in raws] == [83, 115, 83, 115]
        assert all(r[2:18] == p.get_hash()[:16] for r, p in zip(raws, ps))
        r = batch("Identity.prove's proofs, implicit and explicit, one receipt each",
                  [receipt(k, p) for k, p in enumerate(ps)], raws)
        assert r == [p.get_hash().hex() for p in ps]

        # data lengths
        p = sent_packet(0)
        h, sig = p.get_hash(), idents[0].sign(p.get_hash())
        full = forged(h, sig, False)
        lens = (0, 63, 64, 65, 95, 96, 97, 160)
        r = batch("data lengths 0, 63, 64, 65, 95, 96, 97, 160 cut from (or padded behind) an explicit proof, all "
                  "addressed to the receipt: none validates but the 96; then lengths 63, 64, 65 of the signature alone",
                  [receipt(0, p)],
                  [(full + rb(64))[:H + n] for n in lens if n != 96] + [full] +
                  [forged(h, (sig + rb(1))[:n], True) for n in (63, 65)])
        assert r == [None] * 7 + [h.hex()] + [None] * 2
        r = batch("the signature alone at exactly 64 bytes", [receipt(0, p)], [forged(h, sig, True)])
        assert r == [h.hex()]

        # bit flips
        p = sent_packet(1)
        h, sig = p.get_hash(), idents[1].sign(p.get_hash())
        good_e, good_i = forged(h, sig, False), forged(h, sig, True)
        r = batch("explicit: a bit flipped in the hash at byte 0, 15, 16, 31, in R (32, 63), in S (64, 95); then the "
                  "proof itself", [receipt(1, p)],
                  [flip(good_e, H + at) for at in (0, 15, 16, 31, 32, 63, 64, 95)] + [good_e])
        assert r == [None] * 8 + [h.hex()]
        r = batch("implicit: a bit flipped in R (0, 31) and in S (32, 63), in the address (which is not consulted: "
                  "delivered)", [receipt(1, p)],
                  [flip(good_i, H + at) for at in (0, 31, 32, 63)] + [flip(good_i, 2)])
        assert r == [None] * 4 + [h.hex()]

        # another identity's signature
        p, q = sent_packet(2), sent_packet(3)
        hp, hq = p.get_hash(), q.get_hash()
        r = batch("another identity's signature, explicit and implicit; then the right ones",
                  [receipt(2, p), receipt(3, q)],
                  [forged(hp, idents[3].sign(hp), False), forged(hq, idents[2].sign(hq), True),
                   forged(hp, idents[2].sign(hp), False), forged(hq, idents[3].sign(hq), True)])
        assert r == [None, None, hp.hex(), hq.hex()]

        # an explicit proof whose hash agrees with a receipt in 16 bytes and differs after
        p = sent_packet(0)
        h = p.get_hash()
        near = h[:16] + rb(16)
        r = batch("an explicit proof whose hash agrees with the receipt's in 16 bytes and differs after, signed for "
                  "that hash and signed for the receipt's", [receipt(0, p)],
                  [forged(near, idents[0].sign(near), False), forged(near, idents[0].sign(h), False)])
        assert r == [None, None]

        # strays
        pa, pb = sent_packet(0), sent_packet(1)
        ha, hb = pa.get_hash(), pb.get_hash()
        r = batch("implicit proofs: addressed to a hash that is no receipt's but signed correctly for B (the stray "
                  "that validates); addressed to A and signed for nothing outstanding; addressed to A and signed "
                  "for A", [receipt(0, pa), receipt(1, pb)],
                  [forged(hb, idents[1].sign(hb), True, address=rb(16)), forged(ha, idents[0].sign(rb(32)), True),
                   forged(ha, idents[0].sign(ha), True)])
        assert r == [hb.hex(), None, ha.hex()]
        r = batch("an implicit proof addressed to receipt A and signed for receipt B; then A's own",
                  [receipt(0, pa), receipt(1, pb)],
                  [forged(hb, idents[1].sign(hb), True, address=ha[:16]), forged(ha, idents[0].sign(ha), True),
                   forged(hb, idents[1].sign(hb), True)])
        assert r == [hb.hex(), ha.hex(), None]

        # the same proof twice
        p = sent_packet(2)
        h = p.get_hash()
        e, i = forged(h, idents[2].sign(h), False), forged(h, idents[2].sign(h), True)
        r = batch("the same explicit proof twice", [receipt(2, p)], [e, e])
        assert r == [h.hex(), None]
        r = batch("the same implicit proof twice, then the explicit one", [receipt(2, p)], [i, i, e])
        assert r == [h.hex(), None, None]
        r = batch("a bad copy below a good one, explicit; the good one again", [receipt(2, p)], [flip(e, H + 40), e, e])
        assert r == [None, h.hex(), None]
        r = batch("a bad copy below a good one, implicit; the good one again", [receipt(2, p)], [flip(i, H + 40), i, i])
        assert r == [None, h.hex(), None]

        # a receipt whose destination is a link
        link = a_link()
        assert not hasattr(link, "identity")
        hl = rb(32)
        on_link = RNS.PacketReceipt(OnLink(link, hl))
        owner_sig = link.owner.identity.sign(hl)
        r = batch("a receipt whose destination is a link: never delivered by a proof that comes on no link, explicit "
                  "or implicit, whoever signed it", [(on_link, None), receipt(0, pa)],
                  [forged(hl, owner_sig, False), forged(hl, owner_sig, True), forged(hl, link.sign(hl), False),
                   forged(hl, idents[0].sign(hl), True)])
        assert r == [None] * 4

        # destination type LINK with no such link active; LRPROOF and RESOURCE_PRF
        p, q = sent_packet(3), sent_packet(0)
        hp, hq = p.get_hash(), q.get_hash()
        r = batch("a proof of destination type LINK for a link that is not active, explicit and implicit: delivered",
                  [receipt(3, p), receipt(0, q)],
                  [forged(hp, idents[3].sign(hp), False, address=rb(16), dtype=Destination.LINK),
                   forged(hq, idents[0].sign(hq), True, dtype=Destination.LINK)])
        assert r == [hp.hex(), hq.hex()]
        r = batch("contexts LRPROOF and RESOURCE_PRF, explicit and implicit; GROUP and PLAIN destination types "
                  "(delivered); context KEEPALIVE (delivered)",
                  [receipt(3, p), receipt(0, q), receipt(1, pb)],
                  [forged(hp, idents[3].sign(hp), False, context=Packet.LRPROOF),
                   forged(hp, idents[3].sign(hp), True, context=Packet.LRPROOF),
                   forged(hp, idents[3].sign(hp), False, context=Packet.RESOURCE_PRF),
                   forged(hp, idents[3].sign(hp), True, context=Packet.RESOURCE_PRF),
                   forged(hp, idents[3].sign(hp), False, dtype=Destination.GROUP),
                   forged(hq, idents[0].sign(hq), True, dtype=Destination.PLAIN),
                   forged(hb, idents[1].sign(hb), True, context=Packet.KEEPALIVE)])
        assert r == [None] * 4 + [hp.hex(), hq.hex(), hb.hex()]

        # the proof rows the delivery stage's fixture holds
        with open(os.path.join(HERE, "destination_deliver_vectors.json")) as f:
            dv = json.load(f)
        rows = [c for c in dv["cases"] if c["proof"] and len(bytes.fromhex(c["proof"])) == 83][:2] + \
            [c for c in dv["cases"] if c["proof"] and len(bytes.fromhex(c["proof"])) == 115][:2]
        assert len(rows) == 4
        recs, raws, want, extra = [], [], [], []
        for c in rows:
            ident = Identity.from_bytes(bytes.fromhex(dv["destinations"][c["dest"]]["private_key"]))
            dest = Destination(ident, Destination.OUT, Destination.SINGLE, "deliver", "fixture%d" % c["dest"])
            assert dest.hash.hex() == dv["destinations"][c["dest"]]["hash"]
            data = Packet(None, bytes.fromhex(c["raw"]))
            assert data.unpack()
            data.destination = dest
            recs.append((RNS.PacketReceipt(data), len(out["identities"]) + len(extra)))
            extra.append({"seed": ident.sig_prv_bytes.hex(), "public": ident.get_public_key()[32:].hex()})
            raws.append(bytes.fromhex(c["proof"]))
            want.append(data.get_hash().hex())
        out["identities"] += extra
        r = batch("proof rows of destination_deliver_vectors.json, 83 and 115 bytes, against receipts for the packets "
                  "they prove", recs, raws, from_deliver=[dv["cases"].index(c) for c in rows])
        assert r == want
    finally:
        Packet.send = real_send
        RNS.Reticulum.should_use_implicit_proof = real_implicit
        RNS.Reticulum.get_instance = real_instance
        RNS.Reticulum._Reticulum__transport_enabled = was_enabled
        Transport.receipts = []

    path = os.path.join(HERE, "destination_proof_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out["batches"]), "batches,",
          sum(len(b["raws"]) for b in out["batches"]), "proofs")


if __name__ == "__main__":
    main()
