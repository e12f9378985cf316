"""Resource integrity hash and proof (RNS/Resource.py:436-439, 698-699,
759-760, 787-790): the fixtures made by the reference itself
(tests/golden/gen_resource_proof.py) against hashlib, and the host-only parts
of the Python layer.  The GPU side is tests/test_resource_proof_gpu.py.
"""
import hashlib
import json
import os

import pytest

from tests_helpers import b, collision_stream

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def sha(x):
    return hashlib.sha256(x).digest()


@pytest.fixture(scope="module")
def pv():
    with open(os.path.join(HERE, "golden", "resource_proof_vectors.json")) as f:
        return json.load(f)


def test_fixture_sizes_cover_the_tail_boundaries(pv):
    assert [r["size"] for r in pv["resources"]] == [0, 1, 23, 24, 51, 52, 55, 56, 63, 64, 65, 200, 1000, 5000]
    assert pv["skipped_sizes"] == []


def test_fixtures_equal_hashlib(pv):
    for r in pv["resources"] + [dict(pv["metadata"], data=pv["metadata"]["hashed"], size="metadata")]:
        data, rh = b(r["data"]), b(r["random_hash"])
        assert len(rh) == 4
        assert sha(data + rh).hex() == r["hash"], r["size"]
        assert r["truncated_hash"] == r["hash"][:32], r["size"]
        assert sha(data + b(r["hash"])).hex() == r["expected_proof"], r["size"]


def test_metadata_fixture_hashes_metadata_then_data(pv):
    m = pv["metadata"]
    packed = b(m["metadata_msgpack"])
    assert b(m["hashed"]) == len(packed).to_bytes(3, "big") + packed + b(m["data"])


def test_collision_fixture_hashes_the_colliding_part(pv):
    """After a map-hash collision the reference's retry hashes the colliding
    encrypted part (the name `data` as rebound at :450), not the segment."""
    c = pv["collision_retry"]
    stream = collision_stream(c["seed"], c["stream_len"], None, c["sdu"])
    k = c["colliding_index"]
    part = stream[k * c["sdu"]:(k + 1) * c["sdu"]]
    rh = b(c["random_hash"])
    assert rh == b(c["draws"][1]) and len(c["draws"]) == 2
    assert sha(part + rh).hex() == c["hash"]
    assert sha(part + b(c["hash"])).hex() == c["expected_proof"]
    assert sha(b(c["data"]) + rh).hex() != c["hash"]
    parts = [stream[i:i + c["sdu"]] for i in range(0, len(stream), c["sdu"])]
    assert b"".join(sha(p + rh)[:4] for p in parts).hex() == c["hashmap"]


def test_validate_proof_truth_table():
    import reticulum_amd as rt
    h, proof = sha(b"h"), sha(b"p")
    assert rt.validate_proof(h + proof, proof) is True
    assert rt.validate_proof(h + proof[:-1], proof) is False           # wrong length
    assert rt.validate_proof(h + proof + b"\0", proof) is False
    assert rt.validate_proof(b"", proof) is False
    assert rt.validate_proof(proof + h, proof) is False                # wrong half
    assert rt.validate_proof(h + sha(b"q"), proof) is False
    assert rt.validate_proof(bytearray(h + proof), memoryview(proof)) is True
    with pytest.raises(TypeError):
        rt.validate_proof("x" * 64, proof)


def test_native_table_and_abi_version():
    from reticulum_amd import _native
    names = [name for name, _, _ in _native.SIGNATURES]
    assert "rt_resource_hashes" in names and "rt_resource_hashes_host" in names
    assert _native.ABI_VERSION == 3
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert "#define RNSTOK_ABI_VERSION 3" in header


def test_exports():
    import reticulum_amd as rt
    from reticulum_amd import device, resource
    for name in ("resource_hashes", "verify_resource", "validate_proof", "prepare_resource"):
        assert getattr(rt, name) is getattr(resource, name)
    assert callable(device.resource_hashes)


def test_type_errors_before_any_library_load(monkeypatch):
    """Non-bytes arguments raise TypeError before librnstok.so is touched."""
    import reticulum_amd as rt
    from reticulum_amd import _native

    def no_load(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_native, "load", no_load)
    monkeypatch.setattr(_native, "context", no_load)
    calls = [lambda: rt.resource_hashes("text", b"1234"), lambda: rt.resource_hashes(b"data", "1234"),
             lambda: rt.verify_resource("text", b"1234", bytes(32)), lambda: rt.verify_resource(b"d", 7, bytes(32)),
             lambda: rt.verify_resource(b"d", b"1234", "h" * 32), lambda: rt.validate_proof(None, bytes(32)),
             lambda: rt.prepare_resource("text", b"stream"), lambda: rt.prepare_resource(b"data", ["stream"])]
    for i, c in enumerate(calls):
        with pytest.raises(TypeError):
            c()
