"""X25519 without a GPU.

(a) the fixtures (tests/golden/x25519_vectors.json, recorded from the
    reference's RNS.Cryptography.X25519) against an independent big-integer
    RFC 7748 ladder (tests/x25519_ref.py): this checks the fixtures, edge
    points and low-order zeros included, not the product;
(b) the field and ladder code of reticulum_amd/csrc/x25519_device.h built for
    the host with address and undefined-behaviour sanitizers
    (tests/x25519_host/fe_check.cpp, run directly) against Python integers;
(c) the argument checks of the Python surface that raise before the library
    is loaded.
"""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import x25519_ref as ref
from tests_helpers import b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ref.P
M255 = (1 << 255) - 1


# ---------------------------------------------------------------- fixtures --

def test_exchange_fixtures_match_integer_ladder():
    v = ref.vectors()
    assert len(v["exchanges"]) >= 80
    for e in v["exchanges"]:
        assert ref.ladder(b(e["scalar"]), b(e["point"])).hex() == e["out"], e["note"]
    notes = {e["note"] for e in v["exchanges"]}
    for name in ("0", "1", "p-1", "p", "p+1", "2^255-1", "2^255+9", "2^256-1", "order 8 (a)", "order 8 (b)"):
        assert "point " + name in notes
    assert {"scalar all 0x00", "scalar all 0xFF", "RFC 7748 5.2", "random"} <= notes


def test_low_order_points_give_zero_without_error():
    zero = bytes(32).hex()
    seen = 0
    for e in ref.vectors()["exchanges"]:
        if e["note"] in ("point 0", "point 1", "point p", "point p+1", "point order 8 (a)", "point order 8 (b)"):
            assert e["out"] == zero, e["note"]
            seen += 1
    assert seen == 12


def test_public_key_and_chain_fixtures_match_integer_ladder():
    v = ref.vectors()
    assert len(v["public_keys"]) == 16
    for k in v["public_keys"]:
        assert ref.ladder(b(k["private"]), ref.BASE).hex() == k["public"]
    c = v["chain"]
    k, u = b(c["scalar"]), b(c["point"])
    assert len(c["outs"]) == c["steps"] == 64
    for want in c["outs"]:
        out = ref.ladder(k, u)
        assert out.hex() == want
        k, u = out, k


def test_identity_fixtures_are_consistent():
    """The recorded Identity tokens open with hashlib HKDF of the integer
    ladder's secret through the C oracle: the three stages the KAT pins."""
    from oracle import ctoken
    idn = ref.vectors()["identity"]
    kat = idn["kat"]
    tok = b(kat["token"])
    assert len(tok) == 208
    key = ref.hkdf(64, ref.ladder(b(kat["private"]), tok[:32]), b(kat["identity_hash"]))
    assert ctoken.decrypt(key, tok[32:]) == (0, b(kat["pt"]))
    assert sorted(len(b(e["pt"])) for e in idn["encrypt"]) == [0, 1, 15, 16, 16, 17, 383, 383]
    for e in idn["encrypt"]:
        eph = b(e["ephemeral_private"])
        key = ref.hkdf(64, ref.ladder(eph, b(e["target_public"])), b(e["salt"]))
        assert ref.ladder(eph, ref.BASE) + ctoken.encrypt(key, b(e["iv"]), b(e["pt"])) == b(e["token"])


# ------------------------------------------------------------- host build --

def h32(v):
    return v.to_bytes(32, "little").hex()


@pytest.fixture(scope="module")
def fe_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of x25519_device.h")
    exe = str(tmp_path_factory.mktemp("x25519_host") / "fe_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "x25519_host", "fe_check.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.split()
        assert len(out) == len(lines)
        return out
    return run


def field_operands():
    rnd = random.Random(25519)
    return [0, 1, 2 ** 255 - 20, 2 ** 255 - 19, 2 ** 255 - 18, 2 ** 255 - 1, 2 ** 255 + 9] + \
        [rnd.getrandbits(256) for _ in range(24)]


def test_host_field_ops_match_python_integers(fe_check):
    """Operands are loaded as a point is (bit 255 dropped, values >= p kept
    unreduced), so p-1, p, p+1 and 2^255-1 go through the arithmetic as
    non-canonical limbs."""
    vals = field_operands()
    lines, want = [], []
    for x in vals:
        xm = x & M255
        for y in vals:
            ym = y & M255
            lines += [f"mul {h32(x)} {h32(y)}", f"add {h32(x)} {h32(y)}", f"sub {h32(x)} {h32(y)}"]
            want += [xm * ym % P, (xm + ym) % P, (xm - ym) % P]
        lines += [f"sq {h32(x)}", f"small {h32(x)}", f"inv {h32(x)}", f"store {h32(x)}"]
        want += [xm * xm % P, xm * 121665 % P, pow(xm, P - 2, P), xm % P]
    got = fe_check(lines)
    for line, g, w in zip(lines, got, want):
        assert g == h32(w), line


def limb_value(limbs):
    pos = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
    return sum(v << p for v, p in zip(limbs, pos))


def test_host_mul_and_square_at_the_limb_bounds(fe_check):
    """mul and square on raw limbs at the largest values the representation
    admits after one add without carry (twice a carried element's maximum:
    2^26 - 1 even, 2^25 - 1 odd, limb 1 up to 2^25 + 2^16 - 1), where the
    64-bit accumulators are fullest; also with single limbs at the bound."""
    addmax = [int(x, 16) for x in fe_check(["addmax"])[0].split(",")]
    carried = [(1 << 26) - 1 if i % 2 == 0 else (1 << 25) - 1 for i in range(10)]
    carried[1] += 1 << 16
    assert addmax == [2 * c for c in carried]        # the header's bound is the documented one
    rnd = random.Random(7)
    ops = [addmax, carried, [0] * 10]
    for i in range(10):
        ops.append([addmax[j] if j == i else 0 for j in range(10)])
        ops.append([addmax[j] if j != i else 0 for j in range(10)])
    ops += [[rnd.randint(0, m) for m in addmax] for _ in range(16)]

    def fmt(limbs):
        return ",".join("%x" % v for v in limbs)
    lines, want = [], []
    for x in ops:
        lines.append("lsq " + fmt(x))
        want.append(limb_value(x) ** 2 % P)
        for y in ops:
            lines.append(f"lmul {fmt(x)} {fmt(y)}")
            want.append(limb_value(x) * limb_value(y) % P)
    got = fe_check(lines)
    for line, g, w in zip(lines, got, want):
        assert g == h32(w), line


def test_host_ladder_matches_fixtures(fe_check):
    v = ref.vectors()
    cases = [(e["scalar"], e["point"], e["out"]) for e in v["exchanges"]]
    cases += [(k["private"], ref.BASE.hex(), k["public"]) for k in v["public_keys"]]
    got = fe_check([f"ladder {s} {p}" for s, p, _ in cases])
    for (s, p, want), g in zip(cases, got):
        assert g == want, (s, p)


# -------------------------------------------------------- argument checks --

@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the library fails the test."""
    from reticulum_amd import _native

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_native, "load", boom)
    monkeypatch.setattr(_native, "context", boom)


MSG = "Curve25519 values must be 32 bytes"


def test_wrong_lengths_raise_the_reference_message(no_library):
    import reticulum_amd as rt
    good = bytes(32)
    for bad in (b"", bytes(31), bytes(33)):
        with pytest.raises(ValueError, match=MSG):
            rt.exchange(bad, good)
        with pytest.raises(ValueError, match=MSG):
            rt.exchange(good, bad)
        with pytest.raises(ValueError, match=MSG):
            rt.public_key(bad)
        with pytest.raises(ValueError, match=MSG):
            rt.exchange_batch([good, bad], good)
        with pytest.raises(ValueError, match=MSG):
            rt.public_keys_batch([good, bad])
        with pytest.raises(ValueError, match=MSG):
            rt.identity.encrypt_batch(bad, bytes(16), [b"x"])
        with pytest.raises(ValueError, match=MSG):
            rt.identity.encrypt_batch(good, bytes(16), [b"x"], ephemeral_privates=[bad])
        with pytest.raises(ValueError, match=MSG):
            rt.identity.decrypt_batch(bad, bytes(16), [bytes(100)])
        with pytest.raises(ValueError, match=MSG):
            rt.identity.decrypt_batch(good, bytes(16), [bytes(100)], ratchets=[good, bad])
    with pytest.raises(ValueError, match=MSG):
        rt.exchange_batch(np.zeros((3, 31), np.uint8), good)
    with pytest.raises(ValueError):
        rt.exchange_batch(np.zeros((3, 32), np.int32), good)
    with pytest.raises(TypeError):
        rt.exchange("00" * 32, good)
    with pytest.raises(TypeError):
        rt.exchange_batch([good, "x" * 32], good)


def test_mismatched_batch_sizes_raise(no_library):
    import reticulum_amd as rt
    good = bytes(32)
    with pytest.raises(ValueError, match="one peer public key per private key"):
        rt.exchange_batch([good] * 3, [good] * 2)
    with pytest.raises(ValueError, match="one peer public key per private key"):
        rt.exchange_batch(np.zeros((4, 32), np.uint8), np.zeros((5, 32), np.uint8))
    with pytest.raises(ValueError, match="one ephemeral private key per plaintext"):
        rt.identity.encrypt_batch(good, bytes(16), [b"a", b"b"], ephemeral_privates=[good])
    with pytest.raises(ValueError, match="16 IV bytes per packet"):
        rt.identity.encrypt_batch(good, bytes(16), [b"a", b"b"], ephemeral_privates=[good, good],
                                  ivs=np.zeros((1, 16), np.uint8))
    with pytest.raises(TypeError, match="Token plaintext input must be bytes"):
        rt.identity.encrypt_batch(good, bytes(16), ["str"])


def test_empty_batches_need_no_library(no_library):
    import reticulum_amd as rt
    assert rt.exchange_batch([], bytes(32)).shape == (0, 32)
    assert rt.public_keys_batch(np.zeros((0, 32), np.uint8)).shape == (0, 32)
    assert rt.identity.encrypt_batch(bytes(32), bytes(16), []) == []
    # tokens of 32 bytes or fewer never reach the device (Identity.py:858,900-902)
    assert rt.identity.decrypt_batch(bytes(32), bytes(16), [b"", bytes(32)]) == ([None, None], [None, None])


def test_device_keyset_key_len_checked_first(no_library):
    import torch
    from reticulum_amd import device
    rows = torch.zeros((2, 32), dtype=torch.uint8)
    for key_len in (0, 16, 48, 65):
        with pytest.raises(ValueError, match="Token key must be 128 or 256 bits"):
            device.derive_keyset_x25519(rows, rows, key_len=key_len)


def test_exports():
    import reticulum_amd as rt
    for name in ("exchange", "exchange_batch", "public_key", "public_keys_batch", "encrypt_batch", "decrypt_batch",
                 "x25519", "identity"):
        assert hasattr(rt, name), name
    from reticulum_amd import _native
    names = [n for n, _, _ in _native.SIGNATURES]
    assert {"rt_x25519", "rt_x25519_host", "rt_keyset_create_x25519"} <= set(names)
