"""Generate tests/golden/ifac_vectors.json from the reference's own code.

Runs only where the reference is at hand ($RNS_REFERENCE).  Fixtures for the
interface access code made and checked on the device (Transport.py:1073,
:1470-1474): the reference's Transport.transmit and Transport.inbound run for
real on a stub interface whose ifac_identity is
RNS.Identity.from_bytes(ifac_key), as Reticulum builds it
(Reticulum.py:968-971), with the key stored so that a test can sign.

Per case: the raw packet, its access code, what transmit hands to
process_outgoing, the packet inbound signs (reassembled) and the raw bytes that
reach RNS.Packet(None, raw) after the check (None where inbound returns
early).  Per ifac_size four more received packets that the reference drops: a
flipped bit in the masked body, in the access code, in byte 0's IFAC flag, and
a packet of exactly 2 + ifac_size bytes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ifac.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")

IFAC_SIZES = (1, 8, 16, 32, 33, 64)
RAW_LENGTHS = (2, 19, 47, 48, 79, 80, 383, 500)


def main():
    sys.path.insert(0, REF)
    import RNS

    rng = np.random.Generator(np.random.PCG64(1470))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    RNS.Transport.ready = True
    RNS.Transport.identity = RNS.Identity()      # inbound goes on to RNS.Packet only with one

    signed, reached = [], []

    class SpyPacket:
        """Stands where Transport.inbound builds RNS.Packet(None, raw): records raw and stops there."""

        def __init__(self, destination, raw):
            reached.append(bytes(raw))

        def unpack(self):
            return False

    class Iface:
        pass

    def make_iface(ifac_size, ifac_key):
        ident = RNS.Identity.from_bytes(ifac_key)
        assert ident is not None

        class SpyIdentity:
            def sign(self, data):
                signed.append(bytes(data))
                return ident.sign(data)

        iface = Iface()
        iface.ifac_identity = SpyIdentity()
        iface.ifac_size = ifac_size
        iface.ifac_key = ifac_key
        iface.sent = []
        iface.process_outgoing = iface.sent.append
        return iface, ident

    def receive(iface, data):
        """(reassembled packet signed or None, raw that reached RNS.Packet or None)"""
        signed.clear()
        reached.clear()
        RNS.Transport.inbound(data, iface)
        assert len(signed) <= 1 and len(reached) <= 1
        return (signed[0].hex() if signed else None), (reached[0].hex() if reached else None)

    out = {"reference": "RNS/Transport.py:1069-1102, 1441-1480; RNS/Reticulum.py:968-971",
           "generator": "tests/golden/gen_ifac.py", "cases": [], "dropped": []}
    real_packet = RNS.Packet
    RNS.Packet = SpyPacket
    try:
        for ifac_size in IFAC_SIZES:
            ifac_key = rb(64)
            iface, ident = make_iface(ifac_size, ifac_key)
            for n in RAW_LENGTHS:
                raw = bytes([int(rng.integers(0, 128)), int(rng.integers(0, 128))]) + rb(n - 2)
                signed.clear()
                RNS.Transport.transmit(iface, raw)
                assert signed == [raw]
                ifac = ident.sign(raw)[-ifac_size:]
                masked = iface.sent[-1]
                reassembled, passed = receive(iface, masked)
                out["cases"].append({"ifac_size": ifac_size, "ifac_key": ifac_key.hex(), "raw": raw.hex(),
                                     "ifac": ifac.hex(), "masked": masked.hex(),
                                     "inbound_reassembled": reassembled, "inbound_passed": passed})
            # received packets the reference drops, made from an honest 100-byte packet
            raw = bytes([int(rng.integers(0, 128)), int(rng.integers(0, 128))]) + rb(98)
            RNS.Transport.transmit(iface, raw)
            masked = iface.sent[-1]

            def flip(data, pos, bit):
                b = bytearray(data)
                b[pos] ^= bit
                return bytes(b)

            variants = [("body bit", flip(masked, 2 + ifac_size + 40, 0x10)),
                        ("code bit", flip(masked, 2 + ifac_size - 1, 0x01)),
                        ("flag bit", flip(masked, 0, 0x80)),
                        ("length 2 + ifac_size", masked[:2 + ifac_size])]
            for note, data in variants:
                reassembled, passed = receive(iface, data)
                assert passed is None, note
                out["dropped"].append({"ifac_size": ifac_size, "ifac_key": ifac_key.hex(), "note": note,
                                       "received": data.hex(), "inbound_reassembled": reassembled,
                                       "inbound_passed": passed})
    finally:
        RNS.Packet = real_packet

    # an honest packet passes unless it is the bare 2-byte header (then the masked
    # packet is exactly 2 + ifac_size bytes long and inbound returns early)
    assert all((c["inbound_passed"] == c["raw"]) == (len(c["raw"]) > 4) for c in out["cases"])
    path = os.path.join(HERE, "ifac_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
