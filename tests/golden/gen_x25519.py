"""Generate tests/golden/x25519_vectors.json from the reference's X25519 and
Identity.

Runs only in the build container (it imports /root/reference, which never
travels to the GPU box).  PyCA is not installed there, so the reference's
internal provider (RNS/Cryptography/X25519.py) is what these vectors pin.

From RNS.Cryptography.X25519 directly: the RFC 7748 §5.2 vector, the edge
points (0, 1, p-1, p, p+1, 2^255-1, 2^255+9, 2^256-1 and the two points of
order 8: non-canonical values are taken mod p, bit 255 is ignored, low-order
points give 32 zero bytes without an error) against two scalars each,
all-0x00 and all-0xFF scalars (the clamp), 64 random pairs, 16 public keys
and a 64-step chain in which each output becomes the next scalar and the old
scalar the next point.

From RNS.Identity: the tests/identity.py KAT whole (private key, identity
hash, the 208-byte token, the plaintext), Identity.encrypt outputs with the
ephemeral private key and the IV captured by patching os.urandom, and
Identity.decrypt cases (good, flipped tag, flipped ephemeral-key byte, lengths
32 and 33, and two ratchets of which the first, the second or neither opens
the token, the last also under enforce_ratchets).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_x25519.py
"""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")

P = 2 ** 255 - 19
ORDER8 = ("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800",
          "5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157")


def main():
    sys.path.insert(0, REF)
    import RNS
    from RNS.Cryptography import X25519 as X

    rng = np.random.Generator(np.random.PCG64(25519))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def le(v):
        return v.to_bytes(32, "little")

    exchanges = []

    def add(scalar, point, note):
        out = X.curve25519(point, scalar)
        exchanges.append({"scalar": scalar.hex(), "point": point.hex(), "out": out.hex(), "note": note})
        return out

    rfc = add(bytes.fromhex("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4"),
              bytes.fromhex("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c"), "RFC 7748 5.2")
    assert rfc.hex() == "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
    s_a, s_b = rb(32), rb(32)
    edges = [("0", le(0)), ("1", le(1)), ("p-1", le(P - 1)), ("p", le(P)), ("p+1", le(P + 1)),
             ("2^255-1", le(2 ** 255 - 1)), ("2^255+9", le(2 ** 255 + 9)), ("2^256-1", le(2 ** 256 - 1)),
             ("order 8 (a)", bytes.fromhex(ORDER8[0])), ("order 8 (b)", bytes.fromhex(ORDER8[1]))]
    for name, pt in edges:
        for s in (s_a, s_b):
            out = add(s, pt, "point " + name)
            if name in ("0", "1", "p", "p+1") or name.startswith("order 8"):
                assert out == bytes(32), name      # low order: zero, and no error
    for s, name in ((bytes(32), "scalar all 0x00"), (b"\xff" * 32, "scalar all 0xFF")):
        add(s, rb(32), name)
        add(s, le(9), name + ", base point")
    for _ in range(64):
        add(rb(32), rb(32), "random")

    public_keys = []
    for _ in range(16):
        prv = rb(32)
        pub = X.X25519PrivateKey.from_private_bytes(prv).public_key().public_bytes()
        assert pub == X.curve25519_base(prv)
        public_keys.append({"private": prv.hex(), "public": pub.hex()})

    k, u = rb(32), le(9)
    chain = {"scalar": k.hex(), "point": u.hex(), "steps": 64, "outs": []}
    for _ in range(64):
        out = X.curve25519(u, k)
        chain["outs"].append(out.hex())
        k, u = out, k

    # ---- Identity -------------------------------------------------------
    src = open(os.path.join(REF, "tests", "identity.py")).read()
    ns = {}
    for line in src.splitlines():
        s = line.strip()
        if s.startswith("encrypted_message =") or s.startswith("fixed_token ="):
            name, rhs = s.split("=", 1)            # a literal only: never executed
            ns[name.strip()] = ast.literal_eval(rhs.strip())
    fixed_key0 = src.split('fixed_keys = [')[1].split('("')[1].split('"')[0]
    fid = RNS.Identity.from_bytes(bytes.fromhex(fixed_key0))
    ftok = bytes.fromhex(ns["fixed_token"])
    assert len(ftok) == 208 and fid.decrypt(ftok) == bytes.fromhex(ns["encrypted_message"])
    prv, pub, salt = bytes.fromhex(fixed_key0)[:32], fid.get_public_key()[:32], fid.get_salt()
    assert X.curve25519_base(prv) == pub and salt == fid.hash
    kat = {"source": "tests/identity.py:11-19,148-158", "private": prv.hex(), "public": pub.hex(),
           "identity_hash": fid.hash.hex(), "token": ftok.hex(), "pt": ns["encrypted_message"]}

    def encrypt_captured(ident, pt, ratchet=None):
        drawn = []
        orig = os.urandom

        def spy(n):
            b = orig(n)
            drawn.append(b)
            return b

        os.urandom = spy
        try:
            tok = ident.encrypt(pt, ratchet=ratchet)
        finally:
            os.urandom = orig
        assert [len(d) for d in drawn] == [32, 16], [len(d) for d in drawn]
        return tok, drawn[0], drawn[1]

    encrypts = []
    for L in (0, 1, 15, 16, 17, 383, 16, 383):
        pt = rb(L)
        tok, eph, iv = encrypt_captured(fid, pt)
        assert fid.decrypt(tok) == pt
        encrypts.append({"target_public": pub.hex(), "salt": salt.hex(), "pt": pt.hex(), "ephemeral_private": eph.hex(),
                         "iv": iv.hex(), "token": tok.hex()})

    decrypts = []

    def dec(tok, note, ratchets=None, enforce=False, expect_which="unset"):
        class Receiver:
            latest_ratchet_id = "unset"
        rcv = Receiver()
        pt = fid.decrypt(tok, ratchets=ratchets, enforce_ratchets=enforce, ratchet_id_receiver=rcv)
        which = None
        if pt is not None:
            which = -1
            if rcv.latest_ratchet_id is not None:
                ids = [RNS.Identity._get_ratchet_id(X.curve25519_base(r)) for r in ratchets]
                which = ids.index(rcv.latest_ratchet_id)
        if expect_which != "unset":
            assert which == expect_which, (note, which, expect_which)
        decrypts.append({"note": note, "token": tok.hex(), "ratchets": [r.hex() for r in (ratchets or [])],
                         "enforce_ratchets": enforce, "pt": None if pt is None else pt.hex(), "which": which})

    pt = rb(100)
    good, _, _ = encrypt_captured(fid, pt)
    dec(good, "good", expect_which=-1)
    flipped = bytearray(good)
    flipped[-1] ^= 1
    dec(bytes(flipped), "flipped tag", expect_which=None)
    flipped = bytearray(good)
    flipped[5] ^= 0x10
    dec(bytes(flipped), "flipped ephemeral-key byte", expect_which=None)
    dec(good[:32], "length 32", expect_which=None)
    dec(good[:33], "length 33", expect_which=None)
    r1, r2 = rb(32), rb(32)
    to_r1, _, _ = encrypt_captured(fid, pt, ratchet=X.curve25519_base(r1))
    to_r2, _, _ = encrypt_captured(fid, pt, ratchet=X.curve25519_base(r2))
    dec(to_r1, "two ratchets, the first opens", [r1, r2], expect_which=0)
    dec(to_r2, "two ratchets, the second opens", [r1, r2], expect_which=1)
    dec(good, "two ratchets, neither opens: the identity key does", [r1, r2], expect_which=-1)
    dec(good, "two ratchets, neither opens, enforce_ratchets", [r1, r2], enforce=True, expect_which=None)
    dec(to_r2, "two ratchets, the second opens, enforce_ratchets", [r1, r2], enforce=True, expect_which=1)

    out = {"reference": "RNS/Cryptography/X25519.py:49-93, RNS/Identity.py:803-904 (internal provider)",
           "generator": "tests/golden/gen_x25519.py", "exchanges": exchanges, "public_keys": public_keys,
           "chain": chain, "identity": {"private": prv.hex(), "public": pub.hex(), "salt": salt.hex(), "kat": kat,
                                        "encrypt": encrypts, "decrypt": decrypts}}
    path = os.path.join(HERE, "x25519_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes;", len(exchanges), "exchanges,", len(encrypts), "encrypts,",
          len(decrypts), "decrypts")


if __name__ == "__main__":
    main()
