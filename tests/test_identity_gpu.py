"""Identity.encrypt / Identity.decrypt for a batch on the GPU, from the X25519
exchange to the token, against the reference's recorded outputs
(tests/golden/x25519_vectors.json, RNS/Identity.py:803-904)."""
import os

import pytest

import x25519_ref as ref
from tests_helpers import b

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def idn():
    return ref.vectors()["identity"]


def test_reference_kat_token_opens_whole(idn):
    """tests/identity.py's fixed_token, all 208 bytes, with the identity's
    private key and hash alone: X25519 + HKDF + Token in one piece."""
    import reticulum_amd as rt
    kat = idn["kat"]
    pts, which = rt.identity.decrypt_batch(b(kat["private"]), b(kat["identity_hash"]), [b(kat["token"])])
    assert pts == [b(kat["pt"])] and which == [-1]


def test_encrypt_batch_reproduces_reference_tokens(idn):
    import numpy as np
    import reticulum_amd as rt
    enc = idn["encrypt"]
    toks = rt.identity.encrypt_batch(b(idn["public"]), b(idn["salt"]), [b(e["pt"]) for e in enc],
                                     ephemeral_privates=[b(e["ephemeral_private"]) for e in enc],
                                     ivs=np.frombuffer(b"".join(b(e["iv"]) for e in enc), np.uint8).reshape(-1, 16))
    for got, e in zip(toks, enc):
        assert got == b(e["token"]), len(b(e["pt"]))


def test_decrypt_batch_fixture_cases(idn):
    """Each recorded Identity.decrypt case alone (its own ratchet list), then
    the cases that share a ratchet list as one batch."""
    import reticulum_amd as rt
    prv, salt = b(idn["private"]), b(idn["salt"])
    notes = [d["note"] for d in idn["decrypt"]]
    for want in ("good", "flipped tag", "flipped ephemeral-key byte", "length 32", "length 33",
                 "two ratchets, the first opens", "two ratchets, the second opens",
                 "two ratchets, neither opens: the identity key does",
                 "two ratchets, neither opens, enforce_ratchets"):
        assert want in notes

    def expect(d):
        return None if d["pt"] is None else b(d["pt"])
    for d in idn["decrypt"]:
        pts, which = rt.identity.decrypt_batch(prv, salt, [b(d["token"])], ratchets=[b(r) for r in d["ratchets"]],
                                               enforce_ratchets=d["enforce_ratchets"])
        assert pts == [expect(d)] and which == [d["which"]], d["note"]
    for ratcheted, enforce in ((False, False), (True, False), (True, True)):
        group = [d for d in idn["decrypt"] if bool(d["ratchets"]) == ratcheted and d["enforce_ratchets"] == enforce]
        assert group
        pts, which = rt.identity.decrypt_batch(prv, salt, [b(d["token"]) for d in group],
                                               ratchets=[b(r) for r in group[0]["ratchets"]], enforce_ratchets=enforce)
        assert pts == [expect(d) for d in group]
        assert which == [d["which"] for d in group]


def test_round_trip_65_tokens_random_ephemerals(idn):
    """More than a wave of packets with os.urandom ephemerals and IVs, two
    ratchets on the receiving side; every third packet goes to the second
    ratchet's public key."""
    import reticulum_amd as rt
    prv, pub, salt = b(idn["private"]), b(idn["public"]), b(idn["salt"])
    ratchets = [os.urandom(32), os.urandom(32)]
    r_pub = rt.public_key(ratchets[1])
    pts = [os.urandom((7 * i) % 120) for i in range(65)]
    to_id = [i for i in range(65) if i % 3]
    to_r = [i for i in range(65) if i % 3 == 0]
    toks = [None] * 65
    for idx, target in ((to_id, pub), (to_r, r_pub)):
        for i, t in zip(idx, rt.identity.encrypt_batch(target, salt, [pts[i] for i in idx])):
            toks[i] = t
    assert len({t[:32] for t in toks}) == 65            # fresh ephemeral keys
    back, which = rt.identity.decrypt_batch(prv, salt, toks, ratchets=ratchets)
    assert back == pts
    assert which == [1 if i % 3 == 0 else -1 for i in range(65)]
    back, which = rt.identity.decrypt_batch(prv, salt, toks, ratchets=ratchets, enforce_ratchets=True)
    assert back == [pts[i] if i % 3 == 0 else None for i in range(65)]
    assert which == [1 if i % 3 == 0 else None for i in range(65)]
