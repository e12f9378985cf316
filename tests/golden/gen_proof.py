"""Generate tests/golden/proof_vectors.json from the reference's own code.

Runs only where the reference is at hand ($RNS_REFERENCE).  Fixtures for the
packet proofs of a link (Link.py:378-389, 943-955, 1140-1145; Packet.py:199-200,
434-459; Transport.py:2326-2363).  Real RNS.Link objects: responder links
under an owner identity, keyed by a real handshake, and for each the matching
initiator side, a link with the same id that holds the owner's signing key as
its peer_sig_pub.  Packet.send is replaced by a recorder.

  links     per link: link id, derived key, the seed it signs with and the
            public key its peer verifies with;
  proved    raw DATA packets through the responder's Link.receive: whether a
            proof was sent and, where one was, the raw proof packet
            (prove_packet -> Packet.pack), the packet hash, and the flags the
            link had (PROVE_ALL / PROVE_NONE on its destination, a channel or
            none).  Context NONE with a good and a forged token, CHANNEL with a
            good and a corrupt token, KEEPALIVE, and a PROOF packet with
            context CHANNEL;
  settled   batches of raw PROOF packets through the PROOF branch of
            Transport.inbound as it stands at Transport.py:2326-2363 (the link
            walk, the proof_hash rule, the walk over the receipts with
            validate_proof_packet and the removal), driven with real
            PacketReceipt objects: per packet the hash of the receipt that was
            delivered, or none.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_proof.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")
PROVE_ALL_FLAG, HAS_CHANNEL_FLAG = 1, 2


def main():
    sys.path.insert(0, REF)
    import RNS
    from RNS.Cryptography import Ed25519PrivateKey, Token, X25519PrivateKey

    rng = np.random.Generator(np.random.PCG64(2326))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    RNS.loglevel = -1
    iface = object()

    class Callbacks:
        proof_requested = None

    def owner():
        class Owner:
            """The destination a responder link belongs to."""
            identity = RNS.Identity()
            type = RNS.Destination.SINGLE
            hash = rb(16)
            proof_strategy = RNS.Destination.PROVE_NONE
            callbacks = Callbacks()
        return Owner

    class Channel:
        def _receive(self, plaintext):
            pass

        def _shutdown(self):
            pass

    class Dest:
        type = RNS.Destination.SINGLE

        def __init__(self):
            self.hash = rb(16)

    def pair(own):
        """A responder link of `own`, handshaken, and its initiator side."""
        peer = X25519PrivateKey.generate().public_key().public_bytes()
        peer_sig = Ed25519PrivateKey.generate().public_key().public_bytes()
        link = RNS.Link(owner=own, peer_pub_bytes=peer, peer_sig_pub_bytes=peer_sig)
        request = RNS.Packet(Dest(), peer + peer_sig + RNS.Link.signalling_bytes(500, link.mode),
                             packet_type=RNS.Packet.LINKREQUEST)
        request.pack()
        link.set_link_id(request)
        link.handshake()
        link.destination = own
        link.attached_interface = iface
        link.status = RNS.Link.ACTIVE
        link.rtt = 0.1
        # the other end: verifies with the owner's signing key (Link.validate)
        sig_pub = own.identity.get_public_key()[32:]
        far = RNS.Link(owner=owner(), peer_pub_bytes=peer, peer_sig_pub_bytes=sig_pub)
        far.link_id = far.hash = link.link_id
        far.status = RNS.Link.ACTIVE
        far.rtt = 0.1
        return link, far

    sent = []
    real_send = RNS.Packet.send

    def recorder(self):
        self.pack()
        sent.append(self.raw)

    RNS.Packet.send = recorder
    try:
        shared = owner()
        pairs = [pair(shared), pair(shared), pair(owner()), pair(owner()), pair(owner())]
        out = {"reference": "RNS/Link.py:378-389, 943-955, 1140-1145; RNS/Packet.py:199-200, 434-459; "
                            "RNS/Transport.py:2326-2363",
               "generator": "tests/golden/gen_proof.py",
               "links": [{"link_id": l.link_id.hex(), "derived_key": l.derived_key.hex(),
                          "seed": l.owner.identity.sig_prv_bytes.hex(),
                          "public": l.owner.identity.get_public_key()[32:].hex()} for l, _ in pairs]}
        assert out["links"][0]["seed"] == out["links"][1]["seed"] != out["links"][2]["seed"]

        # --- what Link.receive proves
        def link_packet(link, ptype, context, data):
            flags = (RNS.Destination.LINK << 2) | ptype
            return bytes([flags, 0]) + link.link_id + bytes([context]) + data

        def token(link, plaintext):
            return Token(link.derived_key).encrypt(plaintext)

        def forged(tok):
            return tok[:-1] + bytes([tok[-1] ^ 1])

        out["proved"] = []

        def receive(k, raw, prove_all, channel, note):
            link = pairs[k][0]
            link.destination.proof_strategy = RNS.Destination.PROVE_ALL if prove_all else RNS.Destination.PROVE_NONE
            link._channel = Channel() if channel else None
            packet = RNS.Packet(None, raw)
            assert packet.unpack()
            packet.receiving_interface = iface
            packet.link = link
            link.status = RNS.Link.ACTIVE
            sent.clear()
            link.receive(packet)
            assert len(sent) <= 1
            flags = (PROVE_ALL_FLAG if prove_all else 0) | (HAS_CHANNEL_FLAG if channel else 0)
            out["proved"].append({"note": note, "link": k, "flags": flags, "raw": raw.hex(),
                                  "packet_hash": packet.packet_hash.hex(),
                                  "proof": sent[0].hex() if sent else None})
            return sent[0] if sent else None

        D, P = RNS.Packet.DATA, RNS.Packet.PROOF
        NONE, CHANNEL, KEEPALIVE = RNS.Packet.NONE, RNS.Packet.CHANNEL, RNS.Packet.KEEPALIVE
        for k in range(5):
            for n in (0, 1, 40):
                good = link_packet(pairs[k][0], D, NONE, token(pairs[k][0], rb(n)))
                assert receive(k, good, True, k & 1, "NONE, PROVE_ALL") is not None
        k = 2
        link = pairs[k][0]
        assert receive(k, link_packet(link, D, NONE, token(link, rb(9))), False, False, "NONE, PROVE_NONE") is None
        assert receive(k, link_packet(link, D, NONE, token(link, rb(9))), False, True,
                       "NONE, PROVE_NONE, a channel") is None
        assert receive(k, link_packet(link, D, NONE, forged(token(link, rb(9)))), True, True,
                       "NONE, PROVE_ALL, forged token") is None
        assert receive(k, link_packet(link, D, NONE, rb(20)), True, True, "NONE, PROVE_ALL, token too short") is None
        assert receive(k, link_packet(link, D, CHANNEL, token(link, rb(30))), False, True, "CHANNEL, a channel")
        assert receive(k, link_packet(link, D, CHANNEL, token(link, rb(30))), True, False,
                       "CHANNEL, no channel, PROVE_ALL") is None
        assert receive(k, link_packet(link, D, CHANNEL, forged(token(link, rb(30)))), False, True,
                       "CHANNEL, a channel, corrupt token: proved all the same")
        assert receive(k, link_packet(link, D, CHANNEL, rb(5)), True, True, "CHANNEL, a channel, no token at all")
        assert receive(k, link_packet(link, D, KEEPALIVE, bytes([0xFF])), True, True, "KEEPALIVE") is None
        assert receive(k, link_packet(link, P, CHANNEL, rb(96)), True, True, "a PROOF with context CHANNEL") is None
        assert receive(k, link_packet(link, P, NONE, rb(96)), True, True, "a PROOF with context NONE") is None

        # --- what Transport.inbound does with a PROOF
        class Sent:
            """A packet sent on a link, as PacketReceipt.__init__ reads it."""

            def __init__(self, far, h):
                self.destination = far
                self._h = h

            def get_hash(self):
                return self._h

            def getTruncatedHash(self):
                return self._h[:16]

        active_links = [far for _, far in pairs[:4]]          # the last link is not in the node's list

        def proof_branch(raw, receipts):
            """Transport.py:2202, 2320-2363 for one packet; the delivered receipt or None."""
            packet = RNS.Packet(None, raw)
            if not packet.unpack() or packet.packet_type != RNS.Packet.PROOF:
                return None
            if packet.context in (RNS.Packet.LRPROOF, RNS.Packet.RESOURCE_PRF):
                return None
            if packet.destination_type == RNS.Destination.LINK:
                for link in active_links:
                    if link.link_id == packet.destination_hash:
                        packet.link = link
                        break
            if len(packet.data) == RNS.PacketReceipt.EXPL_LENGTH:
                proof_hash = packet.data[:RNS.Identity.HASHLENGTH // 8]
            else:
                proof_hash = None
            delivered = None
            for receipt in list(receipts):
                receipt_validated = False
                if proof_hash is not None:
                    if receipt.hash == proof_hash:
                        receipt_validated = receipt.validate_proof_packet(packet)
                else:
                    receipt_validated = receipt.validate_proof_packet(packet)
                if receipt_validated:
                    if receipt in receipts:
                        receipts.remove(receipt)
                    assert delivered is None
                    delivered = receipt
            return delivered

        out["settled"] = []

        def batch(note, hashes_links, raws):
            receipts = [RNS.PacketReceipt(Sent(pairs[k][1], h)) for h, k in hashes_links]
            results = []
            for raw in raws:
                d = proof_branch(raw, receipts)
                results.append(d.hash.hex() if d is not None else None)
            out["settled"].append({"note": note, "receipts": [[h.hex(), k] for h, k in hashes_links],
                                   "raws": [r.hex() for r in raws], "delivered": results,
                                   "left": [r.hash.hex() for r in receipts]})
            return results

        def proof(k, h, signer=None, context=NONE, dtype=RNS.Destination.LINK):
            sig = pairs[k if signer is None else signer][0].sign(h)
            return bytes([(dtype << 2) | P, 0]) + pairs[k][0].link_id + bytes([context]) + h + sig

        def flip(raw, at, bit=1):
            b = bytearray(raw)
            b[at] ^= bit
            return bytes(b)

        h = [rb(32) for _ in range(12)]
        good = proof(1, h[0])
        r = batch("data lengths 0, 31, 32, 95, 96, 97, 160, the exact one last", [(h[0], 1), (h[1], 1), (h[2], 1)],
                  [good[:19], good[:19 + 31], good[:19 + 32], good[:19 + 95], proof(1, h[1]) + rb(1),
                   proof(1, h[2]) + rb(64), good])
        assert r == [None] * 4 + [h[1].hex(), h[2].hex(), h[0].hex()]
        r = batch("a bit flipped in the hash at byte 0, 15, 16, 31, in R, in S; then the proof itself",
                  [(h[3], 0)], [flip(proof(0, h[3]), 19 + at) for at in (0, 15, 16, 31, 32, 63, 64, 95)]
                  + [proof(0, h[3])])
        assert r == [None] * 8 + [h[3].hex()]
        # the key is that of the link the proof arrived on, whichever link the receipt's packet went out on
        r = batch("signed by another link's key; arriving under another link with the first one's signature; a hash "
                  "no receipt holds; arriving under another link with that link's signature: delivered",
                  [(h[4], 2), (h[11], 2)], [proof(2, h[4], signer=3), proof(3, h[4], signer=2), proof(2, h[5]),
                                            proof(2, h[4]), proof(3, h[11]), proof(2, h[11])])
        assert r == [None] * 3 + [h[4].hex(), h[11].hex(), None]
        r = batch("the same proof twice; a bad copy below a good one; the shared owner key across two links",
                  [(h[6], 3), (h[7], 0), (h[8], 0)],
                  [proof(3, h[6]), proof(3, h[6]), flip(proof(0, h[7]), 19 + 40), proof(0, h[7]), proof(0, h[7]),
                   proof(1, h[8])])
        assert r == [h[6].hex(), None, None, h[7].hex(), None, h[8].hex()]
        r = batch("contexts LRPROOF and RESOURCE_PRF; destination type SINGLE; a link the node does not have",
                  [(h[9], 2), (h[10], 4)],
                  [proof(2, h[9], context=RNS.Packet.LRPROOF), proof(2, h[9], context=RNS.Packet.RESOURCE_PRF),
                   proof(2, h[9], dtype=RNS.Destination.SINGLE), proof(4, h[10]),
                   proof(2, h[9], context=RNS.Packet.KEEPALIVE)])
        out["settled"][-1]["caller"] = [2, 3]     # the verdicts that stay with the caller: NOT_LINK, NO_LINK
        assert r[:2] == [None, None] and r[4] == h[9].hex()
    finally:
        RNS.Packet.send = real_send

    path = os.path.join(HERE, "proof_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
