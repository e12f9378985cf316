"""Link dispatch and link keys, the parts that need no GPU:

(a) the test model's context rule (tests/link_helpers.py) against what the
    reference's own Link.receive was recorded doing for all 256 contexts, DATA
    and PROOF (tests/golden/link_vectors.json, made by gen_link.py);
(b) link_id_from_lr_packet against the reference's link ids, with and without
    signalling bytes, HEADER_1 and HEADER_2;
(c) the table's host-side arithmetic (reticulum_amd/csrc/link_host.h) built
    alone under the address and undefined-behaviour sanitizers
    (tests/link_host/book_check.cpp, run directly);
(d) the new entry points: declared, exported, bound, ABI version unchanged;
(e) argument errors that are raised before any device is touched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import link_helpers as lh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_context_rule_is_what_link_receive_was_recorded_doing():
    v = lh.vectors()
    assert len(v["context_decrypts"]) == 256 and len(v["proof_decrypts"]) == 256
    for c in range(256):
        assert (c in lh.DECRYPTED) == bool(v["context_decrypts"][c]), hex(c)
        assert lh.route(True, lh.LINK, lh.DATA, c, 7) == \
            ((lh.LINK_DECRYPT, 7, True) if v["context_decrypts"][c] else (lh.LINK_PLAIN, 7, False)), hex(c)
        assert not v["proof_decrypts"][c]
        assert lh.route(True, lh.LINK, lh.PROOF, c, 7) == (lh.LINK_PLAIN, 7, False)


def test_model_routes_outside_links():
    assert lh.route(False, lh.LINK, lh.DATA, 0, 3) == (lh.NOT_LINK, -1, False)
    for dt in (lh.SINGLE, lh.GROUP, lh.PLAIN):
        assert lh.route(True, dt, lh.DATA, 0, 3) == (lh.NOT_LINK, -1, False)
    for pt in (lh.ANNOUNCE, lh.LINKREQUEST):
        assert lh.route(True, lh.LINK, pt, 0, 3) == (lh.NOT_LINK, -1, False)
    assert lh.route(True, lh.LINK, lh.DATA, 0, None) == (lh.NO_LINK, -1, False)
    assert lh.route(True, lh.LINK, lh.DATA, 0, 5, n_keys=5) == (lh.LINK_PLAIN, 5, False)


def test_link_id_from_lr_packet_matches_the_reference():
    from reticulum_amd import link_id_from_lr_packet
    rows = lh.vectors()["link_ids"]
    assert {(r["header_type"], r["signalling"]) for r in rows} == {(0, False), (0, True), (1, False), (1, True)}
    for r in rows:
        raw = bytes.fromhex(r["raw"])
        assert link_id_from_lr_packet(raw).hex() == r["link_id"], r
        assert link_id_from_lr_packet(bytearray(raw)).hex() == r["link_id"]
    with pytest.raises(ValueError):
        link_id_from_lr_packet(bytes(18))


def test_handshake_fixture_is_the_link_key_derivation():
    """derived_key = hkdf(64 or 32, X25519(prv, peer_pub), salt=link_id,
    context=None) (Link.py:348-361), recomputed with the suite's own X25519 and
    the C oracle's HKDF: what derive_link_keys asks the device for."""
    import x25519_ref
    from oracle import ctoken
    hs = lh.vectors()["handshakes"]
    assert {h["mode"] for h in hs} == {0, 1}
    for h in hs:
        shared = x25519_ref.ladder(bytes.fromhex(h["private"]), bytes.fromhex(h["peer_public"]))
        length = 64 if h["mode"] == 1 else 32
        assert ctoken.hkdf(length, shared, bytes.fromhex(h["link_id"]), None).hex() == h["derived_key"]


def test_host_bookkeeping_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of link_host.h")
    exe = str(tmp_path / "book_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "link_host", "book_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) > 100000


NEW = ("rt_linktable_create", "rt_linktable_destroy", "rt_linktable_capacity", "rt_linktable_insert",
       "rt_linktable_remove", "rt_linktable_lookup", "rt_linktable_count", "rt_linktable_insert_host",
       "rt_linktable_remove_host", "rt_linktable_lookup_host", "rt_link_spans")


def test_entry_points_declared_exported_and_bound():
    import reticulum_amd as rt
    from reticulum_amd import _native, device, link, pipeline
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert "#define RNSTOK_ABI_VERSION 3" in header and _native.ABI_VERSION == 3
    for name, value in (("RT_LINK_OK", 0), ("RT_LINK_DUPLICATE", 1), ("RT_LINK_FULL", 2), ("RT_LINK_MISSING", 3),
                        ("RT_ROUTE_NOT_LINK", 0), ("RT_ROUTE_NO_LINK", 1), ("RT_ROUTE_LINK_PLAIN", 2),
                        ("RT_ROUTE_LINK_DECRYPT", 3)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), header), name
        assert getattr(_native, name) == value and getattr(device, name[3:]) == value
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {n for n, _, _ in _native.SIGNATURES}
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in bound and hasattr(lib, name), name
    assert lib.rt_abi_version() == 3
    for name in ("LinkTable", "derive_link_keys", "link_id_from_lr_packet"):
        assert getattr(rt, name) is getattr(link, name)
    for name in ("link_spans", "linktable_insert", "linktable_remove", "linktable_lookup", "linktable_count"):
        assert hasattr(device, name), name
    import inspect
    assert inspect.signature(pipeline.inbound).parameters["links"].default is None
    assert inspect.signature(pipeline.outbound).parameters["key_idx"].default is None


def test_invalid_arguments_return_inval_without_a_device():
    from reticulum_amd import _native
    lib = _native.load()
    E = _native.RT_E_INVAL
    assert lib.rt_linktable_create(None, 4) is None
    assert lib.rt_linktable_capacity(None) == 0
    lib.rt_linktable_destroy(None)
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.rt_linktable_insert(None, p, p, p, 1, None) == E
    assert lib.rt_linktable_remove(None, p, p, 1, None) == E
    assert lib.rt_linktable_lookup(None, p, p, p, 1, None) == E
    assert lib.rt_linktable_count(None, p, None) == E
    assert lib.rt_linktable_insert_host(None, p, p, p, 1) == E
    assert lib.rt_linktable_remove_host(None, p, p, 1) == E
    assert lib.rt_linktable_lookup_host(None, p, p, p, 1) == E
    assert lib.rt_link_spans(None, p, p, 1, 1, p, p, p, p, p, None) == E
    assert "null link table" in _native.last_error()


def test_python_argument_errors():
    import reticulum_amd as rt
    from reticulum_amd import link
    for bad in (0, -1, (1 << 29) + 1):
        with pytest.raises(ValueError):
            rt.LinkTable(bad)
    # any other mode raises the reference's TypeError (Link.py:355), before anything is computed
    for bad in (2, 0xFF, None):
        with pytest.raises(TypeError, match="Invalid link mode"):
            rt.derive_link_keys([bytes(32)], [bytes(32)], [bytes(16)], mode=bad)
    assert (link.MODE_AES128_CBC, link.MODE_AES256_CBC) == (0, 1)
    with pytest.raises(ValueError):
        link._rows([bytes(15)], 16, None, "link ids")


def test_importing_the_package_does_not_import_torch():
    import sys
    r = subprocess.run([sys.executable, "-c",
                        "import sys; sys.path.insert(0, %r); import reticulum_amd; "
                        "reticulum_amd.link_id_from_lr_packet(bytes(100)); print('torch' in sys.modules)" % ROOT],
                       capture_output=True, text=True)
    assert r.stdout.strip() == "False", (r.stdout, r.stderr)
