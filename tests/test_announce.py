"""Announce validation without a GPU.

(a) the fixture (tests/golden/announce_vectors.json: raw HEADER_1 and HEADER_2
    packets through the reference's Packet.unpack and both forms of
    Identity.validate_announce) against the tests' model, announce_status_ref:
    every recorded verdict and identity hash.  This ties the model the GPU
    tests use, its header arithmetic included, to the reference;
(b) the multi-span SHA-512 reader built for the host with address and
    undefined-behaviour sanitizers (tests/ed25519_host/span_reader_check.cpp, a
    stand-alone program run directly): packets in heap buffers of exactly their
    size, so a read past the packet's end is an error;
(c) the new entry point: declared, exported, bound, ABI version unchanged, and
    the argument checks of device.announce_validate, which raise before the
    library is loaded.
"""
import os
import re
import shutil
import subprocess

import pytest

import announce_helpers as ah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------- fixture --

def test_fixture_covers_the_stated_cases():
    cases = ah.vectors()["cases"]
    assert os.path.getsize(ah.VECTORS) < 200_000
    raws = [bytes.fromhex(c["raw"]) for c in cases]
    wraps = {(r[0] >> 6 & 1, r[1], r[(35 if r[0] & 0x40 else 19) - 1]) for r in raws if r[1] < 128}
    assert wraps == {(0, 0, ah.NONE), (0, 5, ah.PATH_RESPONSE), (1, 0, ah.PATH_RESPONSE), (1, 5, ah.NONE)}
    assert sum(c["ok"] for c in cases) == 40 and sum(c["ok_signature_only"] for c in cases) == 44
    assert any(not c["unpacked"] for c in cases)


def test_model_reproduces_every_recorded_case():
    seen = set()
    for c in ah.vectors()["cases"]:
        raw = bytes.fromhex(c["raw"])
        status, identity = ah.announce_status_ref(raw)
        seen.add(status)
        # Transport.py:1748-1750 and :1772, as include/rnstok.h reads a status
        assert (status in (ah.VALID, ah.BAD_DESTINATION)) == c["ok_signature_only"], c["note"]
        assert (status == ah.VALID) == c["ok"], c["note"]
        if status in (ah.VALID, ah.BAD_SIGNATURE, ah.BAD_DESTINATION):
            assert identity.hex() == c["identity_hash"], c["note"]
        else:
            assert identity == ah.ZERO
        if not c["unpacked"]:
            assert status == ah.NOT_ANNOUNCE
    assert seen == {ah.VALID, ah.NOT_ANNOUNCE, ah.SHORT, ah.BAD_SIGNATURE, ah.BAD_DESTINATION}


# ------------------------------------------------------------------ reader --

def test_host_span_reader_matches_the_contiguous_one_and_stays_inside_the_packet(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of ed25519_device.h")
    exe = str(tmp_path / "span_reader_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "ed25519_host", "span_reader_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    # two header types, two places of the signature, app data 0..333, each hashed twice
    assert r.stdout.split() == ["ok", str(2 * 2 * 334 * 2)]


# ------------------------------------------------------- ABI and arguments --

def test_entry_point_declared_exported_and_bound():
    from reticulum_amd import _native, device
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert "#define RNSTOK_ABI_VERSION 3" in header and _native.ABI_VERSION == 3
    for name, value in (("VALID", 0), ("NOT_ANNOUNCE", 1), ("SHORT", 2), ("BAD_SIGNATURE", 3), ("BAD_DESTINATION", 4)):
        assert re.search(r"#define RT_ANNOUNCE_%s\s+%d\b" % (name, value), header), name
        assert getattr(device, "ANNOUNCE_" + name) == getattr(_native, "RT_ANNOUNCE_" + name) == value
        assert getattr(ah, name) == value
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint rt_announce_validate\s*\(", code)
    lib = _native.load()
    assert "rt_announce_validate" in {n for n, _, _ in _native.SIGNATURES} and hasattr(lib, "rt_announce_validate")
    assert lib.rt_abi_version() == 3


def test_invalid_arguments_return_inval_without_a_device():
    from reticulum_amd import _native
    lib = _native.load()
    assert lib.rt_announce_validate(None, None, None, None, 1, None, None, None) == _native.RT_E_INVAL
    assert b"null context" in lib.rt_last_error()


@pytest.fixture
def no_library(monkeypatch):
    from reticulum_amd import _native

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_native, "load", boom)
    monkeypatch.setattr(_native, "context", boom)


def test_announce_validate_checks_its_arguments_first(no_library):
    import torch
    from reticulum_amd import device
    n = 3
    good = dict(pkt=torch.zeros(600, dtype=torch.uint8), pkt_off=torch.zeros(n, dtype=torch.int64),
                fields=torch.zeros((n, 96), dtype=torch.uint8), status=torch.zeros(n, dtype=torch.int32),
                identity_hash=torch.zeros((n, 16), dtype=torch.uint8))
    bad = [
        ("uint8", dict(pkt=good["pkt"].to(torch.int8))),
        ("uint8", dict(fields=good["fields"].to(torch.int32))),
        ("uint8", dict(identity_hash=good["identity_hash"].to(torch.int16))),
        ("fields", dict(fields=torch.zeros((n, 95), dtype=torch.uint8))),            # narrow records
        ("fields", dict(fields=torch.zeros(n * 96, dtype=torch.uint8))),
        ("fields", dict(fields=torch.zeros((n, 192), dtype=torch.uint8)[:, :96])),    # rows not contiguous
        ("pkt", dict(pkt=torch.zeros((2, 300), dtype=torch.uint8))),
        ("pkt_off", dict(pkt_off=torch.zeros(n, dtype=torch.int32))),
        ("pkt_off", dict(pkt_off=torch.zeros(n - 1, dtype=torch.int64))),
        ("pkt_off", dict(pkt_off=None)),
        ("status", dict(status=torch.zeros(n, dtype=torch.int64))),
        ("status", dict(status=torch.zeros(n - 1, dtype=torch.int32))),             # short
        ("status", dict(status=None)),
        ("identity_hash", dict(identity_hash=torch.zeros((n, 32), dtype=torch.uint8))),   # wrong width
        ("identity_hash", dict(identity_hash=torch.zeros((n - 1, 16), dtype=torch.uint8))),
        ("identity_hash", dict(identity_hash=torch.zeros(n * 16, dtype=torch.uint8))),
    ]
    for match, change in bad:
        with pytest.raises(ValueError, match=match):
            device.announce_validate(**{**good, **change})
    # host memory is refused too, after the shapes and still before the library
    with pytest.raises(ValueError, match="device memory"):
        device.announce_validate(**good)
    with pytest.raises(ValueError, match="device memory"):
        device.announce_validate(**{**good, "identity_hash": None})
