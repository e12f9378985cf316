"""Generate tests/golden/ed25519_vectors.json from the reference's Ed25519 and
Identity.

Runs only in the build container (it imports /root/reference, which never
travels to the GPU box).  PyCA is not installed there, so the reference's
internal provider (RNS/Cryptography/pure25519) is what these vectors pin.

Every case records what the reference returns, and the generator asserts the
expectation of its class, so a wrong reading of the provider's rules shows
when this runs.  One reading was wrong and is recorded as the reference has
it: a key that is the identity in a non-canonical encoding (y = p+1, or
01 00..00 80) passes the subgroup test but is then multiplied with the
provider's non-unified addition, which yields (0, 0, 0, 0); such a key is
rejected for every message (unless h mod L = 0).  The same encodings as R are
accepted when the equation holds: they are the accepted non-canonical y >= p
cases; no other y >= p lies in the subgroup with a known discrete logarithm
(y mod p < 19), which the generator checks and notes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ed25519.py
"""
import base64
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
LENGTHS = (0, 1, 31, 32, 47, 48, 63, 64, 65, 111, 112, 175, 176, 191, 192, 193, 300, 1000)


def main():
    sys.path.insert(0, REF)
    import RNS
    from RNS.Cryptography import Ed25519 as E
    from RNS.Cryptography.pure25519 import basic, eddsa

    rng = np.random.Generator(np.random.PCG64(25519 + 2))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def le(v):
        return v.to_bytes(32, "little")

    def ref_verify(pk, sig, msg):
        try:
            E.Ed25519PublicKey.from_public_bytes(pk).verify(sig, msg)
            return True
        except Exception:
            return False

    def ref_sign(seed, msg):
        return E.Ed25519PrivateKey.from_private_bytes(seed).sign(msg)

    def ref_public(seed):
        return E.Ed25519PrivateKey.from_private_bytes(seed).public_key().public_bytes()

    def enc(xytz):
        return basic.encodepoint(basic.xform_extended_to_affine(xytz))

    def smul(pt, n):
        return basic.scalarmult_element_safe_slow(pt, n)

    def ext(b):
        return basic.xform_affine_to_extended(basic.decodepoint(b))

    base = basic.Base.XYTZ

    def secret_scalar(seed):
        return basic.bytes_to_clamped_scalar(eddsa.H(seed)[:32])

    public_keys = []
    for _ in range(16):
        seed = rb(32)
        public_keys.append({"seed": seed.hex(), "public": ref_public(seed).hex()})

    signatures = []
    for n in LENGTHS:
        seed, msg = rb(32), rb(n)
        sig = ref_sign(seed, msg)
        assert len(sig) == 64 and ref_verify(ref_public(seed), sig, msg)
        signatures.append({"seed": seed.hex(), "public": ref_public(seed).hex(), "msg": msg.hex(), "sig": sig.hex()})

    verify = []

    def case(cls, note, pk, sig, msg, expect):
        got = ref_verify(pk, sig, msg)
        assert got == expect, (cls, note, got, expect)
        verify.append({"class": cls, "note": note, "pk": pk.hex(), "sig": sig.hex(), "msg": msg.hex(), "ok": got})

    # ---- the reference's own selftest triple (literals only, never executed)
    src = open(os.path.join(REF, "RNS", "Cryptography", "pure25519", "ed25519_oop.py")).read()

    def unb64(s):
        return base64.b64decode(s + "=" * (-len(s) % 4))
    st_msg = re.search(r'message = b"([^"]+)"', src).group(1).encode()
    st_sk = unb64(re.search(r'b"priv0-([^"]+)"', src).group(1))
    st_vk = unb64(re.search(r'b"pub0-([^"]+)"', src).group(1))
    st_sig = unb64(re.search(r'b"sig0-([^"]+)"', src).group(1))
    assert len(st_sk) == 64 and st_sk[32:] == st_vk and ref_public(st_sk[:32]) == st_vk
    assert ref_sign(st_sk[:32], st_msg) == st_sig
    selftest = {"seed": st_sk[:32].hex(), "public": st_vk.hex(), "msg": st_msg.hex(), "sig": st_sig.hex()}
    case("selftest", "ed25519_oop.selftest", st_vk, st_sig, st_msg, True)

    # ---- single-bit flips
    seed, msg = rb(32), rb(32)
    pk, sig = ref_public(seed), ref_sign(seed, msg)
    a = secret_scalar(seed)
    case("honest", "32-byte message", pk, sig, msg, True)

    def flip(b, bit):
        o = bytearray(b)
        o[bit // 8] ^= 1 << (bit % 8)
        return bytes(o)
    for bit in (0, 7, 100, 254, 255):
        case("flip", f"R bit {bit}", pk, flip(sig, bit), msg, False)
    for bit in (0, 100, 251):
        case("flip", f"S bit {bit}", pk, flip(sig, 256 + bit), msg, False)
    for bit in (0, 100, 254, 255):
        case("flip", f"key bit {bit}", flip(pk, bit), sig, msg, False)
    for bit in (0, 255):
        case("flip", f"message bit {bit}", pk, sig, flip(msg, bit), False)
    case("flip", "message one byte longer", pk, sig, msg + b"\x00", False)

    # ---- S edges
    s_int = int.from_bytes(sig[32:], "little")
    while s_int + 15 * L >= 2 ** 256:               # S < 2^252 - 15c: almost always
        msg = rb(32)
        sig = ref_sign(seed, msg)
        s_int = int.from_bytes(sig[32:], "little")
    case("scalar", "S + L", pk, sig[:32] + le(s_int + L), msg, True)
    case("scalar", "S + 15 L", pk, sig[:32] + le(s_int + 15 * L), msg, True)
    case("scalar", "S = 2^256 - 1", pk, sig[:32] + le(2 ** 256 - 1), msg, False)
    case("scalar", "S = 0", pk, sig[:32] + le(0), msg, False)
    case("scalar", "S = L", pk, sig[:32] + le(L), msg, False)

    # ---- identity encodings
    zero = le(1)
    assert zero == basic._zero_bytes
    s = int.from_bytes(rb(32), "little") % L
    sb = enc(smul(base, s))
    case("identity", "canonical identity as key, [S]B = R", zero, sb + le(s), msg, False)

    def r_is(r_bytes, m):
        """sig with the given R (an encoding of the identity) and S = h a: [S]B = 0 + [h]A"""
        h = eddsa.Hint(r_bytes + pk + m)
        return r_bytes + le(h * a % L)
    case("identity", "canonical identity as R, [S]B = R + [h]A", pk, r_is(zero, msg), msg, False)
    for name, e in (("y = p+1", le(P + 1)), ("01 00..00 80", le(1 | (1 << 255))), ("y = p+1, sign bit set", le((P + 1) | (1 << 255)))):
        for m in (msg, b"", rb(100)):
            # not as the issue first read it: rejected (see the module docstring)
            case("identity", f"{name} as key, [S]B = R, {len(m)}-byte message", e, sb + le(s), m, False)
        case("identity", f"{name} as R, [S]B = R + [h]A", pk, r_is(e, msg), msg, True)
        case("identity", f"{name} as R, S off by one", pk, r_is(e, msg)[:32] + le((int.from_bytes(r_is(e, msg)[32:], "little") + 1) % L), msg, False)

    # ---- small-order points: [L] of arbitrary curve points
    small = {}
    y = 2
    while set(small) != {2, 4, 8}:
        y += 1
        try:
            pt = ext(le(y))
        except basic.NotOnCurve:
            continue
        t = smul(pt, L)
        order = next(o for o in (1, 2, 4, 8) if basic.is_extended_zero(smul(t, o)))
        if order > 1:
            small.setdefault(order, t)
    for order in (2, 4, 8):
        t = enc(small[order])
        # as key: grind a message with h = 0 mod order, so that [S]B = R + [h]T holds exactly
        ctr = 0
        while True:
            m = b"small order %d key %d" % (order, ctr)
            if eddsa.Hint(sb + t + m) % L % order == 0:
                break
            ctr += 1
        case("small order", f"order {order} as key, the equation holds", t, sb + le(s), m, False)
        case("small order", f"order {order} as R", pk, t + sig[32:], msg, False)
    t8 = small[8]

    # ---- mixed order: A + T8 with h = 0 mod 8, so that only the subgroup test rejects
    mixed_key = enc(basic.add_elements(ext(pk), t8))
    r = int.from_bytes(rb(32), "little") % L
    rbytes = enc(smul(base, r))
    ctr = 0
    while True:
        m = b"mixed order key %d" % ctr
        h = eddsa.Hint(rbytes + mixed_key + m) % L
        if h % 8 == 0:
            break
        ctr += 1
    mixed_sig = rbytes + le((r + h * a) % L)
    case("mixed order", "A + T8 as key, h = 0 mod 8: the cofactorless equation holds", mixed_key, mixed_sig, m, False)
    # the same S under the honest key does not verify (h differs): the case above is no accident of S
    case("mixed order", "the same signature under A", pk, mixed_sig, m, False)
    case("mixed order", "R + T8 as R", pk, enc(basic.add_elements(ext(sig[:32]), t8)) + sig[32:], msg, False)

    # ---- undecodable points
    y = 2
    while True:
        try:
            basic.decodepoint(le(y))
            y += 1
        except basic.NotOnCurve:
            break
    case("undecodable", f"y = {y} as key", le(y), sig, msg, False)
    case("undecodable", f"y = {y} as R", pk, le(y) + sig[32:], msg, False)
    case("undecodable", f"y = {y} with the sign bit as key", le(y | (1 << 255)), sig, msg, False)

    # ---- non-canonical y: which y >= p (y mod p in [0, 19)) lie in the subgroup?
    noncanonical = []
    for ym in range(19):
        try:
            pt = ext(le(ym + P))
        except basic.NotOnCurve:
            continue
        if basic.is_extended_zero(smul(pt, L)):
            noncanonical.append(ym)
            # no discrete logarithm is known, so no accepted signature can be built: honest parts around it
            case("non-canonical", f"y = p+{ym} as key", le(ym + P), sig, msg, False)
            case("non-canonical", f"y = p+{ym} as R", pk, le(ym + P) + sig[32:], msg, False)
    assert 1 in noncanonical                        # the identity, covered above with accepted cases

    # ---- a few more honest ones around the batch tests' needs
    for n in (0, 5, 167):
        sd, m = rb(32), rb(n)
        case("honest", f"{n}-byte message", ref_public(sd), ref_sign(sd, m), m, True)

    # ---- announces (Identity.validate_announce)
    class Owner:
        is_connected_to_shared_instance = True
    RNS.Transport.owner = Owner()

    class Packet:
        packet_type = RNS.Packet.ANNOUNCE
        rssi = snr = None
        hops = 1
        receiving_interface = None
        transport_id = None

        def __init__(self, destination_hash, flag, data):
            self.destination_hash, self.data = destination_hash, data
            self.context_flag = RNS.Packet.FLAG_SET if flag else RNS.Packet.FLAG_UNSET

        def get_hash(self):
            return RNS.Identity.full_hash(self.data)

    announces = []

    def announce(note, destination_hash, flag, data, expect, expect_sig):
        got = RNS.Identity.validate_announce(Packet(destination_hash, flag, data))
        got_sig = RNS.Identity.validate_announce(Packet(destination_hash, flag, data), only_validate_signature=True)
        assert (got, got_sig) == (expect, expect_sig), (note, got, got_sig)
        announces.append({"note": note, "destination_hash": destination_hash.hex(), "context_flag": int(flag),
                          "data": data.hex(), "ok": got, "ok_signature_only": got_sig})

    for flag in (0, 1):
        for app in (b"", b"app data \x00\xff", rb(40)):
            ident = RNS.Identity.from_bytes(rb(64))
            pub, name_hash, random_hash = ident.get_public_key(), rb(10), rb(10)
            ratchet = rb(32) if flag else b""
            dest = RNS.Identity.full_hash(name_hash + ident.hash)[:16]
            signed = dest + pub + name_hash + random_hash + ratchet + app
            data = pub + name_hash + random_hash + ratchet + ident.sign(signed) + app
            tag = f"ratchet {flag}, {len(app)} B app data, {len(data)} B"
            announce(tag, dest, flag, data, True, True)
            wrong = bytes([dest[0] ^ 1]) + dest[1:]
            announce(tag + ", wrong destination hash", wrong, flag, data, False, False)
            other = RNS.Identity.full_hash(rb(10) + ident.hash)[:16]
            assert other != dest
            if app:
                announce(tag + ", tampered app data", dest, flag, data[:-1] + bytes([data[-1] ^ 1]), False, False)
            else:
                assert len(data) == (180 if flag else 148)
                announce(tag + ", one byte short", dest, flag, data[:-1], False, False)
                announce(tag + ", other flag", dest, 1 - flag, data, False, False)
            # signed for another destination hash but otherwise consistent: the signature fails first
            sig_other = ident.sign(other + pub + name_hash + random_hash + ratchet + app)
            announce(tag + ", signed for another destination", dest, flag,
                     pub + name_hash + random_hash + ratchet + sig_other + app, False, False)
    # a valid signature over a destination hash that is not the identity's: only the hash check rejects
    ident = RNS.Identity.from_bytes(rb(64))
    pub, name_hash, random_hash, dest = ident.get_public_key(), rb(10), rb(10), rb(16)
    data = pub + name_hash + random_hash + ident.sign(dest + pub + name_hash + random_hash)
    announce("valid signature, destination hash not of this identity", dest, 0, data, False, True)
    announce("empty data", dest, 0, b"", False, False)
    announce("64 bytes of data", dest, 0, data[:64], False, False)

    out = {"reference": "RNS/Cryptography/Ed25519.py, pure25519/eddsa.py, basic.py, RNS/Identity.py:511-606, 907-940 "
                        "(internal provider)",
           "generator": "tests/golden/gen_ed25519.py", "public_keys": public_keys, "signatures": signatures,
           "selftest": selftest, "verify": verify, "noncanonical_subgroup_y_minus_p": noncanonical,
           "announces": announces}
    path = os.path.join(HERE, "ed25519_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes;", len(public_keys), "public keys,", len(signatures),
          "signatures,", len(verify), "verify cases,", len(announces), "announces; non-canonical subgroup y - p:",
          noncanonical)


if __name__ == "__main__":
    main()
