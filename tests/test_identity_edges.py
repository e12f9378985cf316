"""The plain models of the Identity layer in tests_helpers.py
(identity_decrypt_ref, identity_encrypt_ref, announce_valid_ref) against every
case recorded from the reference (tests/golden/x25519_vectors.json,
ed25519_vectors.json), so that the GPU tests which take their expected values
from these models (tests/test_identity_edges_gpu.py) stand on the reference."""
import ed25519_ref
import x25519_ref
from tests_helpers import announce_valid_ref, b, identity_decrypt_ref, identity_encrypt_ref


def test_decrypt_model_reproduces_every_recorded_case():
    idn = x25519_ref.vectors()["identity"]
    prv, salt = b(idn["private"]), b(idn["salt"])
    cases = idn["decrypt"]
    assert len(cases) >= 10
    for d in cases:
        pt, which = identity_decrypt_ref(prv, salt, b(d["token"]), [b(r) for r in d["ratchets"]], d["enforce_ratchets"])
        assert pt == (None if d["pt"] is None else b(d["pt"])), d["note"]
        assert which == d["which"], d["note"]
    # every branch of the model is among them
    assert {d["which"] for d in cases} >= {None, -1, 0, 1}
    assert any(d["enforce_ratchets"] and d["pt"] is None for d in cases)
    assert any(len(b(d["token"])) <= 32 for d in cases)


def test_decrypt_model_opens_the_reference_kat():
    kat = x25519_ref.vectors()["identity"]["kat"]
    assert identity_decrypt_ref(b(kat["private"]), b(kat["identity_hash"]), b(kat["token"]), [], False) == (b(kat["pt"]), -1)
    assert identity_decrypt_ref(b(kat["private"]), b(kat["identity_hash"]), b(kat["token"]), [], True) == (None, None)


def test_encrypt_model_reproduces_every_recorded_token():
    idn = x25519_ref.vectors()["identity"]
    assert len(idn["encrypt"]) == 8
    for e in idn["encrypt"]:
        tok = identity_encrypt_ref(b(e["target_public"]), b(e["salt"]), b(e["pt"]), b(e["ephemeral_private"]), b(e["iv"]))
        assert tok == b(e["token"]), len(b(e["pt"]))
        assert identity_decrypt_ref(b(idn["private"]), b(e["salt"]), tok, [], False) == (b(e["pt"]), -1)


def test_announce_model_reproduces_every_recorded_announce():
    ann = ed25519_ref.vectors()["announces"]
    assert len(ann) > 25
    seen = set()
    for a in ann:
        item = (b(a["destination_hash"]), a["context_flag"], b(a["data"]))
        got = (announce_valid_ref(*item), announce_valid_ref(*item, only_validate_signature=True))
        assert got == (a["ok"], a["ok_signature_only"]), a["note"]
        seen.add(got)
    assert seen == {(True, True), (False, False), (False, True)}
