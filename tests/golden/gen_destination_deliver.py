"""Generate tests/golden/destination_deliver_vectors.json from the reference's own code.

Runs only where the reference is at hand ($RNS_REFERENCE).  Fixtures for DATA
packets addressed to the node's own SINGLE destinations (Transport.py:2188-2202,
Destination.py:414-429 and 622-654, Identity.py:848-898 and 942-953,
Packet.py:327-381).  Real RNS.Destination objects (IN, SINGLE) registered with
Transport, real identities, ratchets enabled through enable_ratchets on a file
in a temporary directory (so that the reload-and-retry of Destination.py:640-649
finds the same list again), and every raw packet handed to the reference's own
Transport.inbound(raw, interface): unpack, the packet filter (from an empty
hash list each time), the destination map and type rule, Destination.receive ->
Destination.decrypt -> Identity.decrypt, the receive callback, Packet.prove ->
Identity.prove all run as they stand.  Packet.send is replaced by a recorder,
Reticulum.should_use_implicit_proof by the case's setting, and
Reticulum.get_instance by a stub without phy stats.

  destinations  per destination: the identity's private key (X25519 ‖ Ed25519
                seed), the destination hash, the identity hash, its ratchet
                private keys (newest first), whether it enforces ratchets, its
                proof strategy ("ALL", "NONE", "APP");
  transport_id  the node's transport identity hash;
  cases         per case: a note, the raw packet, the destination's index (or
                null), implicit_proof, the status the device stage is expected
                to give by name, and what the reference did: `plaintext` (what
                the receive callback got, or null), `ratchet` (the rank in the
                destination's list of the ratchet whose id the callback saw as
                packet.ratchet_id, -1 for none) and `proof` (the raw PROOF packet
                handed to the interface, or null).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_destination_deliver.py
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")


def main():
    sys.path.insert(0, REF)
    import RNS
    from RNS.Cryptography import HMAC, PKCS7, Token, X25519PrivateKey, X25519PublicKey, hkdf
    from RNS.Cryptography.AES import AES_256_CBC

    rng = np.random.Generator(np.random.PCG64(2188))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    RNS.loglevel = -1
    Transport, Packet, Destination, Identity = RNS.Transport, RNS.Packet, RNS.Destination, RNS.Identity

    class Owner:
        is_connected_to_shared_instance = False

    Transport.owner = Owner()
    Transport.identity = Identity()

    sent, got = [], []
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

    RNS.Reticulum.get_instance = staticmethod(lambda: Instance)
    Transport.ready = True
    was_enabled = getattr(RNS.Reticulum, "_Reticulum__transport_enabled", None)
    RNS.Reticulum._Reticulum__transport_enabled = False

    def inbound(raw):
        Transport.packet_hashlist, Transport.packet_hashlist_prev = set(), set()
        Transport.inbound(raw, Interface())

    tmp = tempfile.TemporaryDirectory()
    try:
        # (ratchets, enforce, proof strategy)
        plan = [(None, False, "ALL"), (1, False, "NONE"), (2, False, "ALL"), (5, False, "APP"), (2, True, "ALL"),
                (0, True, "ALL")]
        strategies = {"ALL": Destination.PROVE_ALL, "NONE": Destination.PROVE_NONE, "APP": Destination.PROVE_APP}
        dests = []
        for k, (n_ratchets, enforce, prove) in enumerate(plan):
            d = Destination(Identity(), Destination.IN, Destination.SINGLE, "deliver", "fixture%d" % k)
            if n_ratchets is not None:
                d.enable_ratchets(os.path.join(tmp.name, "ratchets%d" % k))
                d.ratchets = [Identity._generate_ratchet() for _ in range(n_ratchets)]     # newest first
                d._persist_ratchets()
                if enforce:
                    assert d.enforce_ratchets()
            d.set_proof_strategy(strategies[prove])
            d.set_packet_callback(lambda data, packet: got.append((bytes(data), packet.ratchet_id)))
            dests.append(d)

        out = {"reference": "RNS/Transport.py:2188-2202; RNS/Destination.py:414-429, 622-654; "
                            "RNS/Identity.py:848-898, 942-953; RNS/Packet.py:327-381",
               "generator": "tests/golden/gen_destination_deliver.py",
               "transport_id": Transport.identity.hash.hex(),
               "destinations": [{"private_key": d.identity.get_private_key().hex(), "hash": d.hash.hex(),
                                 "identity_hash": d.identity.hash.hex(),
                                 "ratchets": [r.hex() for r in (d.ratchets or [])],
                                 "enforce": plan[k][1], "prove": plan[k][2]} for k, d in enumerate(dests)],
               "cases": []}

        def target_prv(dest, rank):
            """The private key a sender's packet is meant for: ratchet `rank`, or the identity's (None)."""
            d = dests[dest]
            if rank is None:
                return d.identity.prv
            return X25519PrivateKey.from_private_bytes(d.ratchets[rank])

        def seal(dest, rank, pt, eph_pub=None, bad_pad=False, foreign=False):
            """data = ephemeral public key ‖ token, keyed as the receiver will key it:
            Token(hkdf(64, target.exchange(ephemeral public key), identity hash))."""
            if eph_pub is None:
                eph_pub = X25519PrivateKey.generate().public_key().public_bytes()
            prv = X25519PrivateKey.generate() if foreign else target_prv(dest, rank)
            shared = prv.exchange(X25519PublicKey.from_public_bytes(eph_pub))
            key = hkdf(length=64, derive_from=shared, salt=dests[dest].identity.hash, context=None)
            if not bad_pad:
                return eph_pub + Token(key).encrypt(pt)
            iv = rb(16)
            block = PKCS7.pad(pt)[:-1] + b"\x11"                   # a last byte above the block size
            signed = iv + AES_256_CBC.encrypt(plaintext=block, key=key[32:], iv=iv)
            return eph_pub + signed + HMAC.new(key[:32], signed).digest()

        def packet(data, dest=0, dtype=Destination.SINGLE, header2=None, hops=0, context=0, dest_hash=None):
            h = dests[dest].hash if dest_hash is None else dest_hash
            flags = (dtype << 2) | Packet.DATA
            if header2 is None:
                return bytes([flags, hops]) + h + bytes([context]) + data
            return bytes([flags | (Packet.HEADER_2 << 6) | (Transport.TRANSPORT << 4), hops]) + header2 + h + \
                bytes([context]) + data

        def case(note, raw, dest, expect, use_implicit=True, plaintext=None, rank=-1):
            implicit[0] = use_implicit
            del sent[:], got[:]
            inbound(raw)
            entry = {"note": note, "raw": raw.hex(), "dest": dest, "implicit_proof": use_implicit, "expect": expect,
                     "plaintext": None, "ratchet": -1, "proof": None}
            if got:
                assert len(got) == 1, note
                entry["plaintext"] = got[0][0].hex()
                if got[0][1] is not None:
                    ids = [Identity._get_ratchet_id(X25519PrivateKey.from_private_bytes(r).public_key().public_bytes())
                           for r in dests[dest].ratchets]
                    entry["ratchet"] = ids.index(got[0][1])
            if sent:
                assert len(sent) == 1 and got, note
                entry["proof"] = sent[0].hex()
            assert (expect == "DELIVERED") == bool(got), (note, expect, got)
            if expect == "DELIVERED":
                assert got[0][0] == plaintext and entry["ratchet"] == rank, (note, entry)
                assert bool(sent) == (plan[dest][2] == "ALL"), (note, sent)
            out["cases"].append(entry)
            return entry

        ours = Transport.identity.hash
        # every destination, every candidate that can open, implicit and explicit proofs
        for k, (n_ratchets, enforce, prove) in enumerate(plan):
            ranks = list(range(n_ratchets or 0)) + [None]
            for rank in ranks:
                pt = rb(int(rng.integers(1, 60)))
                opens = not (enforce and rank is None)
                who = "the identity's key" if rank is None else "ratchet %d" % rank
                e = case(f"destination {k} ({n_ratchets} ratchets, enforce {enforce}, PROVE_{prove}): sealed for {who}",
                         packet(seal(k, rank, pt), dest=k), k, "DELIVERED" if opens else "NOT_OPENED",
                         plaintext=pt, rank=-1 if rank is None else rank)
                if prove == "ALL" and opens:
                    assert len(bytes.fromhex(e["proof"])) == 83
            pt = rb(20)
            case(f"destination {k}: sealed for a key it does not hold", packet(seal(k, None, pt, foreign=True), dest=k), k,
                 "NOT_OPENED")
        for k, rank in ((0, None), (2, 1), (4, 0)):
            pt = rb(33)
            e = case(f"destination {k}: explicit proof", packet(seal(k, rank, pt), dest=k), k, "DELIVERED",
                     use_implicit=False, plaintext=pt, rank=-1 if rank is None else rank)
            assert len(bytes.fromhex(e["proof"])) == 115
        # header forms
        pt = rb(40)
        case("HEADER_2 with our transport id", packet(seal(2, 0, pt), dest=2, header2=ours, hops=3), 2, "DELIVERED",
             plaintext=pt, rank=0)
        pt = rb(40)
        case("HEADER_1, hops 5", packet(seal(0, None, pt), hops=5), 0, "DELIVERED", plaintext=pt)
        # destination type and hash
        pt = rb(16)
        case("a GROUP packet to a SINGLE destination's hash", packet(seal(0, None, pt), dtype=Destination.GROUP), 0,
             "TYPE_MISMATCH")
        case("a PLAIN packet to a SINGLE destination's hash", packet(seal(0, None, pt), dtype=Destination.PLAIN), 0,
             "TYPE_MISMATCH")
        case("an unknown hash", packet(seal(0, None, pt), dest_hash=rb(16)), None, "NO_DESTINATION")
        # data lengths: 32 bytes of key and a token of 0, 1, 63, 64, 65 and 80 bytes
        empty = seal(0, None, b"")
        assert len(empty) == 96
        case("32-byte data", packet(empty[:32]), 0, "SHORT")
        case("33-byte data", packet(empty[:33]), 0, "NOT_OPENED")
        case("95-byte data", packet(empty[:95]), 0, "NOT_OPENED")
        case("96-byte data: an empty plaintext", packet(empty), 0, "DELIVERED", plaintext=b"")
        case("97-byte data", packet(empty + b"\x00"), 0, "NOT_OPENED")
        pt = rb(16)
        one = seal(0, None, pt[:7])
        assert len(one) == 96
        case("96-byte data: seven bytes", packet(one), 0, "DELIVERED", plaintext=pt[:7])
        two = seal(0, None, pt)
        assert len(two) == 112
        case("112-byte data", packet(two), 0, "DELIVERED", plaintext=pt)
        empty2 = seal(2, 1, b"")
        case("96-byte data on a destination with ratchets: an empty plaintext after the reload-and-retry",
             packet(empty2, dest=2), 2, "DELIVERED", plaintext=b"", rank=1)
        # the token
        pt = rb(50)
        good = seal(2, 0, pt)
        for at, what in ((len(good) - 1, "the last tag byte"), (len(good) - 32, "the first tag byte"),
                         (40, "an IV byte"), (60, "a ciphertext byte")):
            bad = bytearray(good)
            bad[at] ^= 0x01
            case(f"{what} flipped", packet(bytes(bad), dest=2), 2, "NOT_OPENED")
        case("a valid tag over bad padding, identity's key", packet(seal(0, None, rb(5), bad_pad=True)), 0, "NOT_OPENED")
        case("a valid tag over bad padding, ratchet 0 of 2", packet(seal(2, 0, rb(5), bad_pad=True), dest=2), 2,
             "NOT_OPENED")
        # the ephemeral key
        pt = rb(24)
        high = bytearray(X25519PrivateKey.generate().public_key().public_bytes())
        high[31] |= 0x80
        case("an ephemeral key with bit 255 set, identity's key", packet(seal(0, None, pt, eph_pub=bytes(high))), 0,
             "DELIVERED", plaintext=pt)
        case("an ephemeral key with bit 255 set, ratchet 1 of 2", packet(seal(2, 1, pt, eph_pub=bytes(high)), dest=2),
             2, "DELIVERED", plaintext=pt, rank=1)
        top = (2 ** 256 - 1).to_bytes(32, "little")
        case("an ephemeral key of all ones (above 2^255 + 19)", packet(seal(0, None, pt, eph_pub=top)), 0, "DELIVERED",
             plaintext=pt)
        case("a low-order ephemeral key: zero", packet(seal(0, None, pt, eph_pub=bytes(32))), 0, "DELIVERED",
             plaintext=pt)
        case("a low-order ephemeral key: one, ratchet 0", packet(seal(2, 0, pt, eph_pub=(1).to_bytes(32, "little")),
                                                                   dest=2), 2, "DELIVERED", plaintext=pt, rank=0)
        # contexts other than NONE
        for ctx in (0x01, 0x0E, 0xFA, 0xFE):
            pt = rb(30)
            case(f"context 0x{ctx:02x}", packet(seal(2, 0, pt), dest=2, context=ctx), 2, "DELIVERED", plaintext=pt,
                 rank=0)
    finally:
        Packet.send = real_send
        RNS.Reticulum.should_use_implicit_proof = real_implicit
        RNS.Reticulum.get_instance = real_instance
        RNS.Reticulum._Reticulum__transport_enabled = was_enabled
        tmp.cleanup()

    path = os.path.join(HERE, "destination_deliver_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
