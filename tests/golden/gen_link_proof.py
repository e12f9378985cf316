"""Generate tests/golden/link_proof_vectors.json from the reference's own code.

Runs only where the reference is at hand ($RNS_REFERENCE).  Fixtures for the
initiator side of link establishment (Transport.py:2270-2318, Link.py:391-451,
326-333, 348-361).  Real RNS.Link initiators to real OUT destinations,
registered with Transport by Link.__init__ itself, their ephemeral keys fixed
(X25519PrivateKey.generate and Ed25519PrivateKey.generate as Link sees them
return keys drawn from the fixture's generator), and every raw LRPROOF handed
to the reference's own Transport.inbound(raw, interface): unpack, the packet
filter, the pending-link branch with its rebalance, Link.validate_proof,
load_peer, handshake and activate_link run as they stand.  Packet.send is
replaced by a recorder (it keeps the plaintext of the LRRTT),
Link.start_watchdog by nothing (it starts a thread), Reticulum.get_instance by
a stub, RNS.Link's clock by one that steps 1/64 s per reading, and no
established callback is set.  Identities, keys and times all come from the
generator's seed: a second run writes the same file.

  destinations  the identities' private keys (X25519 ‖ Ed25519 seed) and the
                destinations' hashes;
  transport_id  the node's transport identity hash;
  cases         per case a note, the link (ephemeral private key, signing
                seed, destination index, the raw request, link_id, and
                expected_hops / rebalanced as they were set before the first
                packet) and its packets in order, all through one hash list:
                the raw packet, the status the device stage is expected to
                give by name, and the link afterwards: status, expected_hops,
                rebalanced, mtu, derived_key (or null), whether the packet's
                hash entered the hash list with it, whether the link is among the
                active links, and the LRRTT plaintext with its rtt where one
                was sent.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_link_proof.py
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
    link_module = sys.modules["RNS.Link"]

    rng = np.random.Generator(np.random.PCG64(2270))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    RNS.loglevel = -1
    Transport, Link, Packet, Destination = RNS.Transport, RNS.Link, RNS.Packet, RNS.Destination

    class Owner:
        is_connected_to_shared_instance = False

    Transport.owner = Owner()
    Transport.identity = RNS.Identity.from_bytes(rb(64))

    sent = []
    real = (Packet.send, Link.start_watchdog, RNS.Reticulum.get_instance, link_module.X25519PrivateKey,
            link_module.Ed25519PrivateKey)

    def send(self):
        sent.append(bytes(self.data))

    class FixedX25519(X25519PrivateKey):
        @staticmethod
        def generate():
            return X25519PrivateKey.from_private_bytes(rb(32))

    class FixedEd25519(Ed25519PrivateKey):
        @staticmethod
        def generate():
            return Ed25519PrivateKey.from_private_bytes(rb(32))

    class Interface:
        """The receiving interface, as far as Transport.inbound reads it."""
        ifac_identity = None
        r_stat_rssi = r_stat_snr = r_stat_q = None
        HW_MTU, AUTOCONFIGURE_MTU, FIXED_MTU = 1064, False, False

    class Instance:
        """What Link asks of the Reticulum instance of a live node."""

        @staticmethod
        def get_first_hop_timeout(destination_hash):
            return 6

        @staticmethod
        def get_packet_rssi(packet_hash):
            return None

        get_packet_snr = get_packet_q = get_packet_rssi

    class Clock:
        """time, as RNS.Link reads it: every reading 1/64 s after the one before, so that the recorded RTTs (and
        with them the file) are the same from run to run."""
        now = 1700000000.0

        @classmethod
        def time(cls):
            cls.now += 0.015625
            return cls.now

        sleep = staticmethod(lambda s: None)

    real_time = link_module.time
    link_module.time = Clock
    Packet.send = send
    Link.start_watchdog = lambda self: None
    RNS.Reticulum.get_instance = staticmethod(lambda: Instance)
    link_module.X25519PrivateKey, link_module.Ed25519PrivateKey = FixedX25519, FixedEd25519
    Transport.ready = True
    was_enabled = getattr(RNS.Reticulum, "_Reticulum__transport_enabled", None)
    RNS.Reticulum._Reticulum__transport_enabled = False
    had_discovery = getattr(RNS.Reticulum, "_Reticulum__link_mtu_discovery", None)
    RNS.Reticulum._Reticulum__link_mtu_discovery = True
    names = {Link.PENDING: "PENDING", Link.HANDSHAKE: "HANDSHAKE", Link.ACTIVE: "ACTIVE", Link.CLOSED: "CLOSED"}

    try:
        idents = [RNS.Identity.from_bytes(rb(64)), RNS.Identity.from_bytes(rb(64))]
        dests = [Destination(i, Destination.OUT, Destination.SINGLE, "linkproof", "fixture%d" % k)
                 for k, i in enumerate(idents)]
        out = {"reference": "RNS/Transport.py:2270-2318, 2529-2546; RNS/Link.py:391-451, 326-333, 348-376",
               "generator": "tests/golden/gen_link_proof.py",
               "transport_id": Transport.identity.hash.hex(),
               "destinations": [{"private_key": i.get_private_key().hex(), "hash": d.hash.hex()}
                                for i, d in zip(idents, dests)],
               "cases": []}

        def sig(mtu, mode):
            v = (mtu & Link.MTU_BYTEMASK) + (((mode << 5) & Link.MODE_BYTEMASK) << 16)
            return v.to_bytes(3, "big")

        def open_link(dest=0, expected_hops=1, rebalanced=False):
            del sent[:]
            Transport.pending_links, Transport.active_links = [], []
            Transport.packet_hashlist, Transport.packet_hashlist_prev = set(), set()
            link = Link(dests[dest])
            assert link in Transport.pending_links and link.status == Link.PENDING
            link.expected_hops = expected_hops
            link.rebalanced = 1.0 if rebalanced else None
            return link

        def proof_data(link, signalling=b"", signer=None, peer_prv=None, peer_pub=None, signed_signalling=None):
            """What the responder's Link.prove sends: signature ‖ pub ‖ signalling."""
            pub = peer_pub if peer_pub is not None else \
                X25519PrivateKey.from_private_bytes(peer_prv or rb(32)).public_key().public_bytes()
            ident = signer or link.destination.identity
            signed = link.link_id + pub + link.destination.identity.get_public_key()[32:] + \
                (signalling if signed_signalling is None else signed_signalling)
            return ident.sign(signed) + pub + signalling

        def packet(link, data, hops=0, header2=False, context=Packet.LRPROOF, ptype=Packet.PROOF,
                   dtype=Destination.LINK, link_id=None):
            flags = (dtype << 2) | ptype
            lid = link.link_id if link_id is None else link_id
            if header2:
                return bytes([flags | 0x50, hops]) + Transport.identity.hash + lid + bytes([context]) + data
            return bytes([flags, hops]) + lid + bytes([context]) + data

        def flip(b, at, bit=0):
            return b[:at] + bytes([b[at] ^ (1 << bit)]) + b[at + 1:]

        def case(note, link, packets):
            """packets: (raw, expected device status by name) in order."""
            entry = {"note": note,
                     "link": {"prv": link.prv.private_bytes().hex(), "sig_seed": link.sig_prv.private_bytes().hex(),
                              "dest": dests.index(link.destination), "request": link.packet.raw.hex(),
                              "link_id": link.link_id.hex(), "expected_hops": link.expected_hops,
                              "rebalanced": link.rebalanced is not None},
                     "packets": []}
            for raw, expect in packets:
                p = Packet(None, raw)
                assert p.unpack(), note
                before, had = len(sent), p.get_hash() in Transport.packet_hashlist
                Transport.inbound(raw, Interface())
                after = {"status": names[link.status], "expected_hops": link.expected_hops,
                         "rebalanced": link.rebalanced is not None, "mtu": link.mtu,
                         "derived_key": link.derived_key.hex() if getattr(link, "derived_key", None) else None,
                         "hash_added": not had and p.get_hash() in Transport.packet_hashlist,
                         "active": link in Transport.active_links, "lrrtt": None, "rtt": None}
                if len(sent) > before:
                    assert len(sent) == before + 1
                    after["lrrtt"], after["rtt"] = sent[-1].hex(), float(link.rtt).hex()
                entry["packets"].append({"raw": raw.hex(), "expect": expect, "after": after})
            out["cases"].append(entry)
            return entry

        def one(note, data_of, expect, want_status, **kw):
            lk = {k: kw.pop(k) for k in ("dest", "expected_hops", "rebalanced") if k in kw}
            link = open_link(**lk)
            e = case(note, link, [(packet(link, data_of(link), **kw), expect)])
            assert e["packets"][0]["after"]["status"] == want_status, (note, e["packets"][0]["after"])
            return e["packets"][0]["after"]

        # 96 and 99 bytes, as HEADER_1 and HEADER_2
        for h2 in (False, True):
            name = "HEADER_2 with our transport id" if h2 else "HEADER_1"
            a = one(f"96-byte data, {name}", lambda l: proof_data(l), "ACTIVATED", "ACTIVE", header2=h2)
            assert a["mtu"] == 500 and a["active"] and a["hash_added"] and len(bytes.fromhex(a["lrrtt"])) == 9
            a = one(f"99-byte data, {name}", lambda l: proof_data(l, sig(500, 1)), "ACTIVATED", "ACTIVE", header2=h2)
            assert a["mtu"] == 500
        # the confirmed MTU
        for mtu in (400, 1196, 0x1FFFFF, 0):
            a = one(f"confirmed MTU {mtu}", lambda l: proof_data(l, sig(mtu, 1)), "ACTIVATED", "ACTIVE")
            assert a["mtu"] == (mtu or 500)
        # mode bits at 99 bytes
        for mode in range(8):
            ok = mode == Link.MODE_AES256_CBC
            one(f"mode {mode} at 99 bytes", lambda l: proof_data(l, sig(500, mode), signed_signalling=sig(500, 1)),
                "ACTIVATED" if ok else "BAD_MODE", "ACTIVE" if ok else "CLOSED")
        # lengths
        one("95-byte data", lambda l: proof_data(l)[:95], "BAD_SIZE", "PENDING")
        one("97-byte data, mode bits right", lambda l: proof_data(l) + bytes([0x20]), "BAD_SIZE", "PENDING")
        one("97-byte data, mode bits wrong", lambda l: proof_data(l) + bytes([0x40]), "BAD_MODE", "CLOSED")
        one("98-byte data", lambda l: proof_data(l, sig(500, 1))[:98], "BAD_SIZE", "PENDING")
        one("100-byte data", lambda l: proof_data(l, sig(500, 1)) + b"\x00", "BAD_SIZE", "PENDING")
        # bit flips
        one("a bit of the signature flipped", lambda l: flip(proof_data(l), 10), "BAD_SIGNATURE", "HANDSHAKE")
        one("a bit of S flipped", lambda l: flip(proof_data(l, sig(500, 1)), 40, 3), "BAD_SIGNATURE", "HANDSHAKE")
        one("a bit of peer_pub flipped", lambda l: flip(proof_data(l), 70, 5), "BAD_SIGNATURE", "HANDSHAKE")
        one("a bit of the MTU flipped", lambda l: flip(proof_data(l, sig(500, 1)), 98), "BAD_SIGNATURE", "HANDSHAKE")

        def other_id(l):
            pub = proof_data(l)[64:96]
            ident = l.destination.identity
            return ident.sign(flip(l.link_id, 3) + pub + ident.get_public_key()[32:]) + pub
        one("signed over another link id", other_id, "BAD_SIGNATURE", "HANDSHAKE")
        one("a valid proof signed by another identity", lambda l: proof_data(l, signer=idents[1]), "BAD_SIGNATURE",
            "HANDSHAKE")
        one("the second destination's own identity", lambda l: proof_data(l, sig(500, 1)), "ACTIVATED", "ACTIVE",
            dest=1)
        # keys
        one("a low-order peer_pub: zero", lambda l: proof_data(l, peer_pub=bytes(32)), "ACTIVATED", "ACTIVE")
        one("a low-order peer_pub: one", lambda l: proof_data(l, sig(500, 1), peer_pub=(1).to_bytes(32, "little")),
            "ACTIVATED", "ACTIVE")

        def high(l):
            pub = X25519PrivateKey.from_private_bytes(rb(32)).public_key().public_bytes()
            return proof_data(l, peer_pub=pub[:31] + bytes([pub[31] | 0x80]))
        one("a peer_pub with bit 255 set", high, "ACTIVATED", "ACTIVE")
        one("a peer_pub of all ones", lambda l: proof_data(l, peer_pub=b"\xff" * 32), "ACTIVATED", "ACTIVE")
        # hops: the received byte + 1 against expected_hops
        one("hops 0 at expected_hops 1", lambda l: proof_data(l), "ACTIVATED", "ACTIVE")
        one("hops 4 at expected_hops 5", lambda l: proof_data(l, sig(500, 1)), "ACTIVATED", "ACTIVE", hops=4,
            expected_hops=5)
        a = one("hops 2 at expected_hops 1, valid signature: rebalanced", lambda l: proof_data(l), "ACTIVATED",
                "ACTIVE", hops=2)
        assert a["rebalanced"] and a["expected_hops"] == 3
        a = one("hops 2 at expected_hops 1, 99 bytes: rebalanced", lambda l: proof_data(l, sig(1196, 1)), "ACTIVATED",
                "ACTIVE", hops=2)
        assert a["rebalanced"] and a["expected_hops"] == 3 and a["mtu"] == 1196
        a = one("hops 2 at expected_hops 1, invalid signature", lambda l: flip(proof_data(l), 3), "HOPS", "PENDING",
                hops=2)
        assert not a["rebalanced"] and a["expected_hops"] == 1 and not a["hash_added"]
        one("hops 2 at expected_hops 1, wrong mode", lambda l: proof_data(l, sig(500, 2), signed_signalling=sig(500, 1)),
            "HOPS", "PENDING", hops=2)
        one("hops 2 at expected_hops 1, 97 bytes", lambda l: proof_data(l) + b"\x20", "HOPS", "PENDING", hops=2)
        a = one("hops 2 at expected_hops 1 on a rebalanced link", lambda l: proof_data(l), "HOPS", "PENDING", hops=2,
                rebalanced=True)
        assert a["expected_hops"] == 1
        one("hop match on a rebalanced link", lambda l: proof_data(l), "ACTIVATED", "ACTIVE", rebalanced=True)
        # sequences
        link = open_link()
        good = packet(link, proof_data(link, sig(500, 1)))
        forged = packet(link, flip(proof_data(link, sig(500, 1)), 5))
        e = case("a forged proof, then the genuine one", link, [(forged, "BAD_SIGNATURE"), (good, "NOT_PENDING")])
        assert [p["after"]["status"] for p in e["packets"]] == ["HANDSHAKE", "HANDSHAKE"]
        link = open_link()
        good = packet(link, proof_data(link))
        e = case("the genuine proof, then a replay", link, [(good, "ACTIVATED"), (good, "NOT_PENDING")])
        assert [p["after"]["status"] for p in e["packets"]] == ["ACTIVE", "ACTIVE"]
        link = open_link()
        good = packet(link, proof_data(link))
        again = packet(link, proof_data(link))
        e = case("the genuine proof, then another one", link, [(good, "ACTIVATED"), (again, "NOT_PENDING")])
        assert not e["packets"][1]["after"]["hash_added"]
        link = open_link()
        e = case("a bad length, then the genuine proof", link,
                 [(packet(link, proof_data(link)[:95]), "BAD_SIZE"), (packet(link, proof_data(link)), "ACTIVATED")])
        assert [p["after"]["status"] for p in e["packets"]] == ["PENDING", "ACTIVE"]
        link = open_link()
        e = case("a wrong mode, then the genuine proof", link,
                 [(packet(link, proof_data(link) + b"\x40"), "BAD_MODE"), (packet(link, proof_data(link)), "NOT_PENDING")])
        assert [p["after"]["status"] for p in e["packets"]] == ["CLOSED", "CLOSED"]
        link = open_link()
        e = case("a hop mismatch with a forged signature, then the genuine proof at the expected hops", link,
                 [(packet(link, flip(proof_data(link), 1), hops=3), "HOPS"), (packet(link, proof_data(link)), "ACTIVATED")])
        link = open_link()
        e = case("a genuine proof at other hops, then a forged one at the expected hops", link,
                 [(packet(link, proof_data(link), hops=3), "ACTIVATED"),
                  (packet(link, flip(proof_data(link), 1)), "NOT_PENDING")])
        link = open_link()
        e = case("a forged proof, then proofs at the same and at other hops", link,
                 [(packet(link, flip(proof_data(link), 1)), "BAD_SIGNATURE"),
                  (packet(link, proof_data(link)), "NOT_PENDING"),
                  (packet(link, proof_data(link), hops=5), "NOT_PENDING")])
        assert [p["after"]["hash_added"] for p in e["packets"]] == [True, True, False]
        # not for this stage
        link = open_link()
        case("an unknown link id", link, [(packet(link, proof_data(link), link_id=rb(16)), "NO_LINK")])
        link = open_link()
        case("context one off", link, [(packet(link, proof_data(link), context=0xFE), "NOT_LRPROOF")])
        link = open_link()
        case("packet type DATA", link, [(packet(link, proof_data(link), ptype=Packet.DATA), "NOT_LRPROOF")])
        link = open_link()
        # the branch never reads the destination type: the fixture corrected that reading
        e = case("destination type SINGLE in the flags", link,
                 [(packet(link, proof_data(link), dtype=Destination.SINGLE), "ACTIVATED")])
        assert e["packets"][0]["after"]["status"] == "ACTIVE"
    finally:
        Packet.send, Link.start_watchdog, RNS.Reticulum.get_instance = real[0], real[1], real[2]
        link_module.X25519PrivateKey, link_module.Ed25519PrivateKey = real[3], real[4]
        link_module.time = real_time
        RNS.Reticulum._Reticulum__transport_enabled = was_enabled
        RNS.Reticulum._Reticulum__link_mtu_discovery = had_discovery

    path = os.path.join(HERE, "link_proof_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes", len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
