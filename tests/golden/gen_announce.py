"""Generate tests/golden/announce_vectors.json from the reference's own code.

Runs only where the reference is at hand ($RNS_REFERENCE).  Every announce of
ed25519_vectors.json (data, destination hash and context flag, as
gen_ed25519.py recorded them) and a handful of new ones are wrapped as raw
packets the way Packet.pack lays them out, HEADER_1 and HEADER_2 (a random
transport id), with hops 0 and 5 and context NONE and PATH_RESPONSE, and each
raw packet goes through the reference's Packet.unpack and then through
Identity.validate_announce, once with only_validate_signature=True
(Transport.py:1748-1750) and once in full (:1772), each on an empty
Identity.known_destinations.  Recorded per case: the raw packet, whether unpack
succeeded, both verdicts, and the announced identity's hash
(Identity.truncated_hash of the public key, None where the data has no room
for one).  This ties where the destination hash, the context byte and the data
sit in a HEADER_2 packet to the reference and not to a model of ours.

The new ones: app data lengths on both sides of the SHA-512 block steps of the
signed message (75 | 76 without a ratchet, 43 | 44 with one), a DATA packet
that carries an announce's data, and an announce with hops = 128, which unpack
refuses.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_announce.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")

NONE, PATH_RESPONSE = 0x00, 0x0B
ANNOUNCE, DATA = 1, 0
# (header type, hops, context): every hop count and context with both headers' share
WRAPS = ((0, 0, NONE), (0, 5, PATH_RESPONSE), (1, 0, PATH_RESPONSE), (1, 5, NONE))


def main():
    sys.path.insert(0, REF)
    import RNS

    RNS.loglevel = -1
    rng = np.random.Generator(np.random.PCG64(1748))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    class Owner:
        is_connected_to_shared_instance = True
    RNS.Transport.owner = Owner()

    with open(os.path.join(HERE, "ed25519_vectors.json")) as f:
        announces = [(a["note"], bytes.fromhex(a["destination_hash"]), a["context_flag"], bytes.fromhex(a["data"]),
                      ANNOUNCE) for a in json.load(f)["announces"]]

    def honest(flag, app_len):
        ident = RNS.Identity.from_bytes(rb(64))
        pub, name_hash, random_hash, app = ident.get_public_key(), rb(10), rb(10), rb(app_len)
        ratchet = rb(32) if flag else b""
        dest = RNS.Identity.full_hash(name_hash + ident.hash)[:16]
        sig = ident.sign(dest + pub + name_hash + random_hash + ratchet + app)
        return dest, pub + name_hash + random_hash + ratchet + sig + app

    for flag, lens in ((0, (75, 76)), (1, (43, 44))):
        for n in lens:
            dest, data = honest(flag, n)
            announces.append((f"ratchet {flag}, {n} B app data: a SHA-512 block step", dest, flag, data, ANNOUNCE))
    dest, data = honest(0, 12)
    announces.append(("a DATA packet with an announce's data", dest, 0, data, DATA))

    def raw_of(dest, flag, data, ptype, header, hops, context):
        flags = header << 6 | flag << 5 | header << 4 | ptype       # destination type SINGLE; HEADER_2 in TRANSPORT
        return bytes([flags, hops]) + (rb(16) if header else b"") + dest + bytes([context]) + data

    def run(note, raw):
        verdicts = []
        unpacked = None
        for only_signature in (True, False):
            RNS.Identity.known_destinations = {}
            p = RNS.Packet(None, raw)
            unpacked = bool(p.unpack())
            verdicts.append(bool(RNS.Identity.validate_announce(p, only_validate_signature=only_signature))
                            if unpacked else False)
        data = p.data if unpacked else b""
        ident = RNS.Identity.truncated_hash(data[:64]).hex() if len(data) >= 64 else None
        return {"note": note, "raw": raw.hex(), "unpacked": unpacked, "ok_signature_only": verdicts[0],
                "ok": verdicts[1], "identity_hash": ident}

    cases = []
    for note, dest, flag, data, ptype in announces:
        for header, hops, context in WRAPS:
            tag = f"{note}; HEADER_{header + 1}, hops {hops}, context {context:#04x}"
            cases.append(run(tag, raw_of(dest, flag, data, ptype, header, hops, context)))
    dest, data = honest(1, 5)
    cases.append(run("hops 128: unpack refuses", raw_of(dest, 1, data, ANNOUNCE, 0, 128, NONE)))

    # what the generator expects of its own cases
    assert sum(c["ok"] for c in cases) == 4 * (6 + 4), sum(c["ok"] for c in cases)
    assert sum(c["ok_signature_only"] for c in cases) == 4 * (6 + 4 + 1)
    assert all(c["ok_signature_only"] for c in cases if c["ok"])

    out = {"reference": "RNS/Packet.py:236-268 (unpack), RNS/Identity.py:505-606 (validate_announce), "
                        "RNS/Transport.py:1748-1750, 1772 (internal provider)",
           "generator": "tests/golden/gen_announce.py", "cases": cases}
    path = os.path.join(HERE, "announce_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases,", sum(c["ok"] for c in cases), "valid,",
          sum(c["ok_signature_only"] for c in cases), "with a valid signature")


if __name__ == "__main__":
    main()
