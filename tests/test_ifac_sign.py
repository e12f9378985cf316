"""The interface access code without a GPU.

(a) the fixture (tests/golden/ifac_vectors.json, recorded from the reference's
    Transport.transmit and Transport.inbound with the key stored) against the
    tests' model, ed25519_ref.sign with seed = ifac_key[32:]: every recorded
    code and every recorded verdict.  This ties the model the GPU tests use to
    the reference;
(b) the committed table of [2^i]B: what tools/gen_ed25519_table.py writes, and
    each entry the point ed25519_ref computes;
(c) ge_scalarmult_base_table built for the host with address and
    undefined-behaviour sanitizers (tests/ed25519_host/table_check.cpp, a
    stand-alone program run directly) against ge_scalarmult_base;
(d) the two new entry points: declared, exported, bound, ABI version unchanged;
    and the argument checks of the Python surface that raise before the library
    is loaded.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

import ed25519_ref as ref
import ifac_helpers as ih
from oracle import wire as ow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "reticulum_amd", "csrc", "ed25519_base_table.h")


# ----------------------------------------------------------------- fixture --

def test_fixture_covers_the_stated_cases():
    v = ih.vectors()
    assert {c["ifac_size"] for c in v["cases"]} == {1, 8, 16, 32, 33, 64}
    for isz in (1, 8, 16, 32, 33, 64):
        assert [len(c["raw"]) // 2 for c in v["cases"] if c["ifac_size"] == isz] == [2, 19, 47, 48, 79, 80, 383, 500]
        assert sorted(d["note"] for d in v["dropped"] if d["ifac_size"] == isz) == \
            ["body bit", "code bit", "flag bit", "length 2 + ifac_size"]
    assert os.path.getsize(ih.VECTORS) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "wire_vectors.json"))


def test_model_reproduces_every_recorded_code_and_masked_packet():
    for c in ih.vectors()["cases"]:
        key, raw, isz = bytes.fromhex(c["ifac_key"]), bytes.fromhex(c["raw"]), c["ifac_size"]
        code = ih.code(key, raw, isz)
        assert code.hex() == c["ifac"], (isz, len(raw))
        assert ow.ifac_mask(raw, code, key).hex() == c["masked"], (isz, len(raw))


def _verdict(key, isz, received):
    """Transport.inbound's IFAC block by the model: (packet signed or None, packet passed on or None)."""
    r = ih.reassemble(received, isz, lambda n, ifac: ow._hkdf(n, ifac, key))
    if r is None:
        return None, None
    ifac, new_raw = r
    return new_raw, (new_raw if ih.code(key, new_raw, isz) == ifac else None)


def test_model_reproduces_every_recorded_verdict():
    v = ih.vectors()
    rows = [(c, bytes.fromhex(c["masked"])) for c in v["cases"]] + \
           [(d, bytes.fromhex(d["received"])) for d in v["dropped"]]
    passed = 0
    for c, received in rows:
        signed, through = _verdict(bytes.fromhex(c["ifac_key"]), c["ifac_size"], received)
        assert (signed.hex() if signed is not None else None) == c["inbound_reassembled"], c.get("note")
        assert (through.hex() if through is not None else None) == c["inbound_passed"], c.get("note")
        passed += through is not None
    assert passed == 6 * 7                       # every honest packet but the bare 2-byte headers
    assert all(d["inbound_passed"] is None for d in v["dropped"])
    # the flipped body and the flipped code reach the signature and fail there; the others return before it
    for d in v["dropped"]:
        assert (d["inbound_reassembled"] is not None) == (d["note"] in ("body bit", "code bit")), d["note"]


# ------------------------------------------------------------------- table --

def _table_rows():
    src = open(TABLE).read()
    rows = re.findall(r"\{((?:0x[0-9a-f]+u(?:, )?){10})\}", src)
    return [[int(w.rstrip("u"), 16) for w in r.split(", ")] for r in rows]


def _fe(limbs):
    v, pos = 0, 0
    for i, w in enumerate(limbs):
        bits = 25 if i & 1 else 26
        assert 0 <= w < 1 << bits                # carried, and canonical
        v |= w << pos
        pos += bits
    return v


def test_committed_table_is_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ed25519_table.py"), "--stdout"],
                       capture_output=True, text=True, check=True)
    assert r.stdout == open(TABLE).read()


def test_every_table_entry_is_a_power_of_two_multiple_of_the_base_point():
    rows = _table_rows()
    assert len(rows) == 3 * 253
    for i in range(253):
        x, y = ref.mul(2 ** i, ref.BASE)
        ymx, ypx, t2d = (_fe(r) for r in rows[3 * i:3 * i + 3])
        assert ymx == (y - x) % ref.P and ypx == (y + x) % ref.P and t2d == 2 * ref.D * x * y % ref.P, i


def test_host_table_multiplication_matches_the_doubling_form(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of ed25519_device.h")
    exe = str(tmp_path / "table_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "ed25519_host", "table_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.split() == ["ok", str(1 + 253 + 2 + 64)]


# ------------------------------------------------------- ABI and arguments --

def test_entry_points_declared_exported_and_bound():
    from reticulum_amd import _native, device, pipeline, wire
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert "#define RNSTOK_ABI_VERSION 3" in header and _native.ABI_VERSION == 3
    assert "#define RT_IFAC_MISMATCH 2" in header and device.IFAC_MISMATCH == 2
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {n for n, _, _ in _native.SIGNATURES}
    lib = _native.load()
    for name in ("rt_ifac_sign", "rt_ifac_check"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in bound and hasattr(lib, name), name
    assert lib.rt_abi_version() == 3
    for mod, names in ((device, ("ifac_sign", "ifac_check")), (wire, ("transmit_batch", "receive_batch")),
                       (pipeline, ("ifac_identity",))):
        for name in names:
            assert hasattr(mod, name), name


def test_invalid_arguments_return_inval_without_a_device():
    """NULL context, and the checks that come before any device work."""
    from reticulum_amd import _native
    lib = _native.load()
    assert lib.rt_ifac_sign(None, None, None, None, None, None, None, 16, 1, None) == _native.RT_E_INVAL
    assert lib.rt_ifac_check(None, None, None, None, None, None, None, 16, None, 1, None) == _native.RT_E_INVAL
    assert b"null context" in lib.rt_last_error()


@pytest.fixture
def no_library(monkeypatch):
    from reticulum_amd import _native

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_native, "load", boom)
    monkeypatch.setattr(_native, "context", boom)


def test_host_conveniences_check_their_arguments_first(no_library):
    from reticulum_amd import wire
    assert wire.transmit_batch([], 16, bytes(64)) == []
    assert wire.receive_batch([], 16, bytes(64)) == []
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match="ifac_size"):
            wire.transmit_batch([b"ab"], bad, bytes(64))
        with pytest.raises(ValueError, match="ifac_size"):
            wire.receive_batch([b"ab"], bad, bytes(64))
    with pytest.raises(ValueError, match="64-byte ifac_key"):
        wire.transmit_batch([b"ab"], 16, bytes(32))
    with pytest.raises(ValueError, match="64-byte ifac_key"):
        wire.receive_batch([b"ab"], 16, bytes(63))
    with pytest.raises(ValueError, match="2 header bytes"):
        wire.transmit_batch([b"a"], 16, bytes(64))
