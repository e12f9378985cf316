"""Ed25519 without a GPU.

(a) the fixtures (tests/golden/ed25519_vectors.json, recorded from the
    reference's RNS.Cryptography.Ed25519 and RNS.Identity) against an
    independent big-integer implementation (tests/ed25519_ref.py): this checks
    the fixtures and the stated acceptance rule, not the product;
(b) the code of reticulum_amd/csrc/ed25519_device.h built for the host with
    address and undefined-behaviour sanitizers (tests/ed25519_host/ed_check.cpp,
    a stand-alone program run directly) against hashlib and Python integers,
    and over every fixture;
(c) the argument checks of the Python surface that raise before the library
    is loaded.
"""
import hashlib
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import ed25519_ref as ref
from tests_helpers import b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = ref.P, ref.L
LENGTHS = [0, 1, 31, 32, 47, 48, 63, 64, 65, 111, 112, 175, 176, 191, 192, 193, 300, 1000]


def le(v, n=32):
    return v.to_bytes(n, "little")


def hx(v):
    return v.hex() if v else "-"


# ---------------------------------------------------------------- fixtures --

def test_key_and_signature_fixtures_match_the_integer_reference():
    v = ref.vectors()
    assert len(v["public_keys"]) == 16
    for k in v["public_keys"]:
        assert ref.public_key(b(k["seed"])).hex() == k["public"]
    assert [len(b(s["msg"])) for s in v["signatures"]] == LENGTHS
    for s in v["signatures"] + [v["selftest"]]:
        assert ref.public_key(b(s["seed"])).hex() == s["public"]
        assert ref.sign(b(s["seed"]), b(s["msg"])).hex() == s["sig"]
        assert ref.verify(b(s["public"]), b(s["sig"]), b(s["msg"]))


def test_verify_fixtures_match_the_stated_rule():
    cases = ref.vectors()["verify"]
    for c in cases:
        assert ref.verify(b(c["pk"]), b(c["sig"]), b(c["msg"])) == c["ok"], c["note"]
    classes = {c["class"] for c in cases}
    assert {"selftest", "honest", "flip", "scalar", "identity", "small order", "mixed order", "undecodable",
            "non-canonical"} <= classes
    by_note = {c["note"]: c["ok"] for c in cases}
    assert by_note["S + L"] and by_note["S + 15 L"]
    assert not by_note["S = 2^256 - 1"] and not by_note["S = 0"] and not by_note["S = L"]
    assert all(not c["ok"] for c in cases if c["class"] in ("flip", "small order", "mixed order", "undecodable"))
    # the identity as a key is rejected in every encoding; as R only the canonical bytes are
    for c in cases:
        if c["class"] == "identity" and " as key" in c["note"]:
            assert not c["ok"], c["note"]
    assert by_note["y = p+1 as R, [S]B = R + [h]A"] and by_note["01 00..00 80 as R, [S]B = R + [h]A"]
    assert not by_note["canonical identity as R, [S]B = R + [h]A"]


def test_the_mixed_order_case_passes_a_cofactorless_check():
    """What makes the mixed-order fixture worth having: without the subgroup
    test the plain equation [S]B = R + [h]A' holds for it."""
    c = next(c for c in ref.vectors()["verify"] if c["note"].startswith("A + T8 as key"))
    pk, sig, msg = b(c["pk"]), b(c["sig"]), b(c["msg"])
    a, r = ref.decode(pk), ref.decode(sig[:32])
    h = ref.hint(sig[:32] + pk + msg) % L
    assert h % 8 == 0 and ref.mul(L, a) != ref.IDENTITY and ref.mul(8 * L, a) == ref.IDENTITY
    assert ref.mul(int.from_bytes(sig[32:], "little"), ref.BASE) == ref.add(r, ref.mul(h, a))
    assert not c["ok"]


def test_announce_fixtures_match_the_integer_reference():
    ann = ref.vectors()["announces"]
    sizes = {len(b(a["data"])) for a in ann}
    assert {147, 148, 179, 180} <= sizes
    for a in ann:
        args = (b(a["destination_hash"]), a["context_flag"], b(a["data"]))
        assert ref.validate_announce(*args) == a["ok"], a["note"]
        assert ref.validate_announce(*args, only_validate_signature=True) == a["ok_signature_only"], a["note"]
    assert any(a["ok"] and a["context_flag"] for a in ann) and any(a["ok"] and not a["context_flag"] for a in ann)
    assert any(a["ok_signature_only"] and not a["ok"] for a in ann)


# ------------------------------------------------------------- host build --

@pytest.fixture(scope="module")
def ed_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of ed25519_device.h")
    exe = str(tmp_path_factory.mktemp("ed25519_host") / "ed_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "ed25519_host", "ed_check.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.split()
        assert len(out) == len(lines)
        return out
    return run


def check(run, lines, want):
    got = run(lines)
    for line, g, w in zip(lines, got, want):
        assert g == w, line[:200]


def test_host_sha512_at_every_length(ed_check):
    rnd = random.Random(512)
    lines, want = [], []
    for n in list(range(301)) + [1000]:
        for head in (32, 64):
            h, m = rnd.randbytes(head), rnd.randbytes(n)
            lines.append(f"sha512 {h.hex()} {hx(m)}")
            want.append(hashlib.sha512(h + m).hexdigest())
    check(ed_check, lines, want)


def scalar_edges():
    rnd = random.Random(252)
    return [0, 1, L - 1, L, L + 1, 2 ** 252, 2 ** 256 - 1] + [rnd.getrandbits(256) for _ in range(8)]


def test_host_scalar_reduction_and_multiply_add(ed_check):
    rnd = random.Random(253)
    vals = scalar_edges()
    lines = ["reduce " + le(v).hex() for v in vals]
    want = [le(v % L).hex() for v in vals]
    wide = [0, 1, L, 2 ** 512 - 1, L * L, L << 256, (L << 256) - 1, 2 ** 252, 2 ** 256 - 1] + \
        [rnd.getrandbits(512) for _ in range(16)]
    lines += ["reduce " + le(v, 64).hex() for v in wide]
    want += [le(v % L).hex() for v in wide]
    for r in vals:
        for k in vals:
            a = vals[(vals.index(k) * 5 + vals.index(r) + 3) % len(vals)]
            lines.append(f"muladd {le(r).hex()} {le(k).hex()} {le(a).hex()}")
            want.append(le((r + k * a) % L).hex())
    lines.append(f"muladd {le(2 ** 256 - 1).hex()} {le(2 ** 256 - 1).hex()} {le(2 ** 256 - 1).hex()}")
    want.append(le((2 ** 256 - 1 + (2 ** 256 - 1) ** 2) % L).hex())
    check(ed_check, lines, want)


def edge_encodings():
    """Encodings from the fixtures' edge classes plus random subgroup points
    and random byte strings (about half of which decode)."""
    rnd = random.Random(255)
    encs = {b(c["pk"]) for c in ref.vectors()["verify"] if c["class"] != "flip"}
    encs |= {b(c["sig"])[:32] for c in ref.vectors()["verify"] if c["class"] != "flip"}
    encs |= {ref.encode(ref.mul(rnd.getrandbits(252), ref.BASE)) for _ in range(4)}
    encs |= {rnd.randbytes(32) for _ in range(12)}
    encs |= {ref.ZERO_BYTES, le(P - 1), le(P), le(P + 1), le(2 ** 255 - 1), le(2 ** 256 - 1), le(0), le(1 << 255)}
    return sorted(encs)


def test_host_point_operations(ed_check):
    encs = edge_encodings()
    pts = [ref.decode(e) for e in encs]
    assert sum(p is None for p in pts) >= 4 and sum(p is not None for p in pts) >= 20
    lines, want = [], []
    for e, p in zip(encs, pts):
        lines += ["decode " + e.hex(), "dbl " + e.hex(), "ingroup " + e.hex()]
        if p is None:
            want += ["fail"] * 3
        else:
            want += [le(p[0]).hex() + ":" + le(p[1]).hex(), ref.encode(ref.add(p, p)).hex(),
                     str(int(ref.mul(L, p) == ref.IDENTITY))]
    some = [(e, p) for e, p in zip(encs, pts) if p is not None][::2]
    for e1, p1 in some:
        for e2, p2 in some:
            lines.append(f"add {e1.hex()} {e2.hex()}")
            want.append(ref.encode(ref.add(p1, p2)).hex())
    check(ed_check, lines, want)


def test_host_fixed_base_and_double_scalar(ed_check):
    rnd = random.Random(256)
    lines, want = [], []
    for e in [0, 1, 2, 8, L - 1, L, L + 1, 2 ** 252, 2 ** 254, 2 ** 255 - 1] + [rnd.getrandbits(255) for _ in range(6)]:
        lines.append("base " + le(e).hex())
        want.append(ref.encode(ref.mul(e, ref.BASE)).hex())
    keys = [ref.encode(ref.mul(rnd.getrandbits(252), ref.BASE)) for _ in range(3)] + [le(P + 1), le(P - 1)]
    for key in keys:
        a = ref.decode(key)
        for s, h in [(0, 0), (1, 0), (0, 1), (1, 1), (L - 1, L - 1), (rnd.getrandbits(252), rnd.getrandbits(252))]:
            lines.append(f"dsm {le(s).hex()} {le(h).hex()} {key.hex()}")
            want.append(ref.encode(ref.add(ref.mul(s, ref.BASE), ref.neg(ref.mul(h, a)))).hex())
    check(ed_check, lines, want)


def test_host_verify_sign_public_over_every_fixture(ed_check):
    v = ref.vectors()
    lines, want = [], []
    for k in v["public_keys"]:
        lines.append("public " + k["seed"])
        want.append(k["public"])
    for s in v["signatures"] + [v["selftest"]]:
        m = hx(b(s["msg"]))
        lines += [f"public {s['seed']}", f"sign {s['seed']} - {m}", f"sign {s['seed']} {s['public']} {m}",
                  f"verify {s['public']} {s['sig']} {m}"]
        want += [s["public"], s["sig"], s["sig"], "1"]
    for c in v["verify"]:
        lines.append(f"verify {c['pk']} {c['sig']} {hx(b(c['msg']))}")
        want.append(str(int(c["ok"])))
    for a in v["announces"]:
        data, flag = b(a["data"]), a["context_flag"]
        pub, name_hash, random_hash, ratchet, sig, app = ref.announce_fields(data, flag)
        if len(pub) != 64 or len(sig) != 64:
            continue
        signed = b(a["destination_hash"]) + pub + name_hash + random_hash + ratchet + app
        lines.append(f"verify {pub[32:].hex()} {sig.hex()} {signed.hex()}")
        want.append(str(int(a["ok_signature_only"])))
    check(ed_check, lines, want)


# -------------------------------------------------------- argument checks --

@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the library fails the test."""
    from reticulum_amd import _native

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_native, "load", boom)
    monkeypatch.setattr(_native, "context", boom)


def test_wrong_lengths_raise_the_reference_messages(no_library):
    from reticulum_amd import ed25519 as ed, identity
    key, sig, seed = bytes(32), bytes(64), bytes(32)
    for bad in (0, 31, 33, 64):
        with pytest.raises(ValueError, match=f"Bad verifying key length {bad}$"):
            ed.verify(bytes(bad), sig, b"m")
        with pytest.raises(ValueError, match=f"Bad verifying key length {bad}$"):
            ed.verify_batch([key, bytes(bad)], [sig, sig], [b"a", b"b"])
        with pytest.raises(ValueError, match=f"Bad signing key length {bad}$"):
            ed.sign(bytes(bad), b"m")
        with pytest.raises(ValueError, match=f"Bad signing key length {bad}$"):
            ed.public_key(bytes(bad))
        with pytest.raises(ValueError, match=f"Bad signing key length {bad}$"):
            ed.public_keys_batch([seed, bytes(bad)])
        with pytest.raises(ValueError, match=f"Bad signing key length {bad}$"):
            identity.sign_batch(bytes(bad), [b"m"])
        with pytest.raises(ValueError, match=f"Bad verifying key length {bad}$"):
            ed.sign_batch(seed, [b"m"], public_keys=bytes(bad))
    for bad in (0, 63, 65, 32):
        with pytest.raises(ValueError, match=f"Bad signature length {bad}$"):
            ed.verify(key, bytes(bad), b"m")
        with pytest.raises(ValueError, match=f"Bad signature length {bad}$"):
            ed.verify_batch(key, [sig, bytes(bad)], [b"a", b"b"])
    with pytest.raises(ValueError, match="Bad signature length 63"):
        ed.verify_batch(key, np.zeros((2, 63), np.uint8), [b"a", b"b"])
    with pytest.raises(ValueError):
        ed.verify_batch(np.zeros((2, 32), np.int32), sig, [b"a", b"b"])
    with pytest.raises(TypeError):
        ed.verify("00" * 32, sig, b"m")
    with pytest.raises(TypeError):
        ed.verify(key, sig, "m")
    with pytest.raises(TypeError):
        ed.sign_batch(seed, ["m"])


def test_mismatched_batch_sizes_raise(no_library):
    from reticulum_amd import ed25519 as ed, identity
    key, sig = bytes(32), bytes(64)
    with pytest.raises(ValueError, match="one public key per message"):
        ed.verify_batch([key] * 3, [sig] * 2, [b"a", b"b"])
    with pytest.raises(ValueError, match="one signature per message"):
        ed.verify_batch(key, [sig] * 3, [b"a", b"b"])
    with pytest.raises(ValueError, match="one seed per message"):
        ed.sign_batch([key] * 3, [b"a", b"b"])
    with pytest.raises(ValueError, match="one signature per message"):
        identity.validate_batch(key, [sig], [b"a", b"b"])


def test_empty_batches_and_short_inputs_need_no_library(no_library):
    from reticulum_amd import ed25519 as ed, identity
    assert ed.verify_batch(bytes(32), [], []).shape == (0,)
    assert ed.verify_batch(bytes(32), [], []).dtype == bool
    assert ed.sign_batch(bytes(32), []).shape == (0, 64)
    assert ed.public_keys_batch([]).shape == (0, 32)
    assert ed.public_keys_batch(np.zeros((0, 32), np.uint8)).shape == (0, 32)
    assert identity.sign_batch(bytes(32), []) == []
    assert identity.validate_batch(bytes(32), [], []) == []
    # a signature of the wrong length is False without reaching the device (Identity.py:934-938)
    assert identity.validate_batch(bytes(32), [bytes(63), b"", bytes(65)], [b"a", b"b", b"c"]) == [False] * 3
    assert identity.validate_announces_batch([]) == []
    assert identity.validate_announces_batch([(bytes(16), 0, bytes(147)), (bytes(16), 1, bytes(179)),
                                              (bytes(16), 0, b"")], only_validate_signature=True) == [False] * 3
    # a wrong destination hash is settled on the host
    assert identity.validate_announces_batch([(bytes(16), 0, bytes(148))]) == [False]


def test_exports():
    import reticulum_amd as rt
    from reticulum_amd import _native, device, x25519
    for name in ("ed25519", "validate_batch", "sign_batch", "validate_announces_batch"):
        assert hasattr(rt, name), name
    for name in ("verify", "sign", "verify_batch"):
        assert not hasattr(rt, name), name
    assert rt.public_key is x25519.public_key and rt.public_keys_batch is x25519.public_keys_batch
    for name in ("verify_batch", "sign_batch", "public_keys_batch", "verify", "sign", "public_key"):
        assert hasattr(rt.ed25519, name), name
    for name in ("ed25519_verify", "ed25519_sign", "ed25519_public"):
        assert hasattr(device, name), name
    names = {n for n, _, _ in _native.SIGNATURES}
    assert {"rt_ed25519_verify", "rt_ed25519_verify_host", "rt_ed25519_sign", "rt_ed25519_sign_host",
            "rt_ed25519_public", "rt_ed25519_public_host"} <= names
    assert _native.ABI_VERSION == 3
