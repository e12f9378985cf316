"""The packet filter and the packet hash list, the parts that need no GPU:

(a) the test model (tests/filter_helpers.py) against what the reference's own
    Transport.inbound was recorded doing (tests/golden/filter_vectors.json,
    made by gen_filter.py): every combination of packet type, destination
    type, header, hops and context with the hash absent, current and previous,
    and the replayed sequences with the cull on both sides of its threshold;
(b) the model's own rule for a full generation;
(c) the new entry points: declared, exported, bound, ABI version unchanged;
(d) argument errors that are returned or raised before any device is touched.

The host side of the list adds no bookkeeping of its own: capacity rounding
and the batch limit are link_host.h's, which tests/link_host/ builds alone
under the sanitizers (tests/test_link.py)."""
import inspect
import os
import re

import numpy as np
import pytest

import filter_helpers as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_reproduces_every_recorded_case():
    v = fh.vectors()
    own = bytes.fromhex(v["own_transport_id"])
    assert len(v["cases"]) == 4 * 4 * 3 * 3 * 8 and set(v["contexts"]) == fh.ALWAYS | {fh.LRPROOF, fh.NONE}
    h = bytes(range(32))
    outcomes = set()
    for row in v["cases"]:
        ptype, dtype, header, hops, context = row[:5]
        tid = b"" if header == 0 else own if header == 1 else bytes(15) + b"\x01"
        p = fh.packet(h, ptype, dtype, context, hops, fh.HEADER_2 if header else fh.HEADER_1, tid)
        for k, where in enumerate(("absent", "current", "previous")):
            m = fh.ListModel(1000, own)
            getattr(m, where, set()).add(h)
            status, remembered = m.packet(p)
            assert (int(status == fh.PASS), int(remembered)) == tuple(row[5 + 2 * k:7 + 2 * k]), (row, where, status)
            # a dropped packet changes nothing; a hash of the previous set stays there
            assert (h in m.previous) == (where == "previous")
            assert (h in m.current) == (where == "current" or remembered)
            outcomes.add(status)
    assert outcomes == {fh.PASS, fh.OTHER_TRANSPORT, fh.BAD_ANNOUNCE, fh.HOPS, fh.DUPLICATE}


def test_model_reproduces_the_recorded_sequences():
    v = fh.vectors()
    own = bytes.fromhex(v["own_transport_id"])
    assert len(v["sequences"]) >= 5
    rotations = []
    for seq in v["sequences"]:
        m = fh.ListModel(seq["maxsize"], own)
        for k, step in enumerate(seq["steps"]):
            if step["op"] == "cull":
                before = len(m.current)
                assert m.cull() == step["rotated"], k
                rotations.append((before, seq["maxsize"], step["rotated"]))
            else:
                p = fh.packet(bytes.fromhex(step["packet_hash"]), step["packet_type"], step["destination_type"],
                              step["context"], step["hops"], step["header_type"],
                              bytes.fromhex(step["transport_id"] or ""), bytes.fromhex(step["destination_hash"]))
                transit = {p["destination_hash"]} if step["transit"] else ()
                status, remembered = m.packet(p, transit)
                assert (status == fh.PASS, remembered) == (step["passed"], step["remembered"]), (k, step, status)
            assert m.counts()[:2] == (step["current"], step["previous"]), k
    # the cull was recorded exactly at its threshold (nothing happens) and one above (it rotates)
    assert (4, 8, False) in rotations and (5, 8, True) in rotations


def test_model_full_generation():
    m = fh.ListModel(4)
    hs = [bytes([k]) * 32 for k in range(7)]
    assert m.filter([fh.packet(h) for h in hs]) == [fh.PASS] * 7
    assert m.counts() == (4, 0, 3) and m.contains(hs) == [1] * 4 + [0] * 3
    # known hashes are duplicates even now; the ones that found no room pass again
    assert m.filter([fh.packet(h) for h in hs]) == [fh.DUPLICATE] * 4 + [fh.PASS] * 3
    assert m.counts() == (4, 0, 6)
    assert m.cull() and m.filter([fh.packet(hs[5])]) == [fh.PASS] and m.counts() == (1, 4, 6)
    assert m.remove([hs[5], hs[0]]) == [fh.OK, fh.MISSING] and m.contains([hs[5], hs[0]]) == [0, 2]


NEW = ("rt_hashlist_create", "rt_hashlist_destroy", "rt_hashlist_capacity", "rt_packet_filter", "rt_hashlist_cull",
       "rt_hashlist_add", "rt_hashlist_remove", "rt_hashlist_contains", "rt_hashlist_counts", "rt_hashlist_add_host",
       "rt_hashlist_remove_host", "rt_hashlist_contains_host")


def test_entry_points_declared_exported_and_bound():
    import reticulum_amd as rt
    from reticulum_amd import _native, device, filter as flt, pipeline
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert "#define RNSTOK_ABI_VERSION 3" in header and _native.ABI_VERSION == 3
    for value, name in enumerate(("RT_FILTER_PASS", "RT_FILTER_NO_PACKET", "RT_FILTER_OTHER_TRANSPORT",
                                  "RT_FILTER_BAD_ANNOUNCE", "RT_FILTER_HOPS", "RT_FILTER_DUPLICATE")):
        assert re.search(r"#define %s\s+%d\b" % (name, value), header), name
        assert getattr(_native, name) == value and getattr(device, name[3:]) == value
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {n for n, _, _ in _native.SIGNATURES}
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in bound and hasattr(lib, name), name
    assert lib.rt_abi_version() == 3
    assert rt.PacketHashlist is flt.PacketHashlist and flt.HASHLIST_MAXSIZE == 1000000
    assert inspect.signature(flt.PacketHashlist.__init__).parameters["max_hashes"].default == 1000000
    for name in ("packet_filter", "hashlist_cull", "hashlist_add", "hashlist_remove", "hashlist_contains",
                 "hashlist_counts"):
        assert hasattr(device, name), name
    params = inspect.signature(pipeline.inbound).parameters
    assert [params[k].default for k in ("seen", "transport_identity", "transit")] == [None, None, None]
    # the kernels share the slot word with the link table through a header
    csrc = os.path.join(ROOT, "reticulum_amd", "csrc")
    for name in ("link_kernels.hip", "filter_kernels.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "table_device.h"' in text and "__hip_atomic_compare_exchange_strong" not in text, name


def test_invalid_arguments_return_inval_without_a_device():
    from reticulum_amd import _native
    lib = _native.load()
    E = _native.RT_E_INVAL
    assert lib.rt_hashlist_create(None, 4) is None
    assert lib.rt_hashlist_capacity(None) == 0
    lib.rt_hashlist_destroy(None)
    buf = np.zeros(128, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.rt_packet_filter(None, None, p, p, 1, p, None) == E
    assert lib.rt_hashlist_cull(None, None) == E
    assert lib.rt_hashlist_add(None, p, 1, None) == E
    assert lib.rt_hashlist_remove(None, p, 1, p, None) == E
    assert lib.rt_hashlist_contains(None, p, 1, p, None) == E
    assert lib.rt_hashlist_counts(None, p, None) == E
    assert lib.rt_hashlist_add_host(None, p, 1) == E
    assert lib.rt_hashlist_remove_host(None, p, 1, p) == E
    assert lib.rt_hashlist_contains_host(None, p, 1, p) == E
    assert "null hash list" in _native.last_error()
    # max_hashes 0 (and more than 2^29) is refused before the context is looked at
    fake_ctx = np.zeros(1 << 16, dtype=np.uint8)
    for bad in (0, (1 << 29) + 1):
        assert lib.rt_hashlist_create(fake_ctx.ctypes.data, bad) is None
        assert "max_hashes" in _native.last_error()


def test_python_argument_errors():
    import reticulum_amd as rt
    from reticulum_amd import link, pipeline
    for bad in (0, -1, (1 << 29) + 1):
        with pytest.raises(ValueError):
            rt.PacketHashlist(bad)
    with pytest.raises(ValueError):
        link._rows([bytes(31)], 32, None, "packet hashes")
    # seen without transport_identity: refused before anything is touched
    with pytest.raises(ValueError, match="transport_identity"):
        pipeline.inbound(None, None, None, 0, 4, seen=object())
