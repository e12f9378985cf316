"""Packet proofs of a link without a GPU.

(a) the fixture (tests/golden/proof_vectors.json: real links through the
    reference's Link.receive, prove_packet, Packet.pack and the PROOF branch of
    Transport.inbound with real PacketReceipts) against the tests' model
    (tests/proof_helpers.py): every recorded proof byte for byte, every
    recorded decision to prove or not, every recorded delivery.  This ties the
    model the GPU tests use to the reference;
(b) the new entry points: declared, exported, bound, ABI version unchanged, and
    the argument checks of the Python layer that raise before any launch.
"""
import os
import re

import pytest

import link_helpers as lh
import proof_helpers as ph
from oracle import ctoken

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vec():
    return ph.vectors()


def _links(vec):
    links = vec["links"]
    table = {bytes.fromhex(l["link_id"]): k for k, l in enumerate(links)}
    return links, table


# ----------------------------------------------------------------- fixture --

def test_fixture_covers_the_stated_cases(vec):
    assert os.path.getsize(ph.VECTORS) < 100_000
    links, _ = _links(vec)
    assert len(links) == 5 and links[0]["seed"] == links[1]["seed"] and len({l["seed"] for l in links}) == 4
    for l in links:
        assert ph.public_key(bytes.fromhex(l["seed"])).hex() == l["public"]
    notes = [c["note"] for c in vec["proved"]]
    assert sum(c["proof"] is not None for c in vec["proved"]) == 18
    for want in ("NONE, PROVE_NONE", "forged token", "CHANNEL, no channel", "corrupt token", "KEEPALIVE",
                 "a PROOF with context CHANNEL"):
        assert any(want in n for n in notes), want
    lens = {len(bytes.fromhex(r)) - 19 for b in vec["settled"] for r in b["raws"]}
    assert {0, 31, 32, 95, 96, 97, 160} <= lens
    assert sum(d is not None for b in vec["settled"] for d in b["delivered"]) == 10


def test_model_writes_the_reference_s_proof_packets(vec):
    links, table = _links(vec)
    for c in vec["proved"]:
        raw = bytes.fromhex(c["raw"])
        f = ph.unpack(raw)
        assert f["packet_hash"].hex() == c["packet_hash"]
        k = c["link"]
        assert table[f["destination_hash"]] == k
        route, link = ph.link_of(f, table)
        token_status = ctoken.decrypt(bytes.fromhex(links[k]["derived_key"]), f["data"])[0] if route == lh.LINK_DECRYPT \
            else 1
        # the link alone has the recorded flags; the others prove everything, which must not matter
        flags = [ph.PROVE_ALL | ph.HAS_CHANNEL] * 5
        flags[k] = c["flags"]
        signers = ph.Signers([bytes.fromhex(l["seed"]) for l in links], [bytes(32)] * 5, flags)
        got = ph.prove(f, route, link, token_status, signers)
        assert (got.hex() if got is not None else None) == c["proof"], c["note"]
        if got is not None:
            assert len(got) == ph.PROOF_LEN and got[0] == 0x0F and got[1] == 0 and got[18] == 0
            assert ph.verify(bytes.fromhex(links[k]["public"]), got[51:], got[19:51])


def test_model_delivers_what_the_reference_delivers(vec):
    links, table = _links(vec)
    # the node of the fixture holds the first four links
    table = {i: k for i, k in table.items() if k < 4}
    signers = ph.Signers([bytes(32)], [bytes.fromhex(l["public"]) for l in links[:4]], [0] * 4)
    seen = set()
    for b in vec["settled"]:
        receipts = ph.Receipts(16)
        hashes = [bytes.fromhex(h) for h, _ in b["receipts"]]
        assert receipts.add(hashes, list(range(len(hashes)))) == [lh.OK] * len(hashes)
        packets = [ph.unpack(bytes.fromhex(r)) for r in b["raws"]]
        got = ph.settle(packets, [ph.link_of(f, table)[1] for f in packets], signers, receipts)
        caller = b.get("caller", [])
        for j, ((status, rid), want) in enumerate(zip(got, b["delivered"])):
            seen.add(status)
            if j in caller:
                # left to the caller, whatever the reference makes of them
                assert status in (ph.NOT_LINK, ph.NO_LINK) and rid == -1, b["note"]
                continue
            assert (status == ph.DELIVERED) == (want is not None), (b["note"], j)
            assert (hashes[rid].hex() if rid >= 0 else None) == want, (b["note"], j)
        left = sorted(h.hex() for i, h in enumerate(hashes) if h[:16] in receipts.table.entries)
        assert left == sorted(b["left"]), b["note"]
    assert seen == set(range(7))


def test_model_compares_the_whole_hash():
    receipts = ph.Receipts(4)
    a = bytes(range(32))
    b = a[:16] + bytes(16)
    assert receipts.add([a, b], [0, 1]) == [lh.OK, lh.DUPLICATE] and receipts.hashes == {0: a}
    seed = bytes(range(1, 33))
    signers = ph.Signers([seed], [ph.public_key(seed)], [0])
    link_id = bytes(16)

    def fields(h):
        return ph.unpack(ph.proof_packet(link_id, h, seed))

    got = ph.settle([fields(b), fields(a), fields(a)], [0, 0, 0], signers, receipts)
    assert got == [(ph.NO_RECEIPT, -1), (ph.DELIVERED, 0), (ph.NO_RECEIPT, -1)] and len(receipts) == 0


# ------------------------------------------------------------ entry points --

NEW = ("rt_link_prove", "rt_receipt_store", "rt_proof_settle")


def test_entry_points_are_declared_bound_and_exported():
    from reticulum_amd import _native
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert re.search(r"#define RNSTOK_ABI_VERSION 3\b", header) and _native.ABI_VERSION == 3
    bound = {name for name, _, _ in _native.SIGNATURES}
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in bound and hasattr(lib, name), name
    from reticulum_amd import device
    for name in ("DELIVERED", "NOT_PROOF", "NOT_LINK", "NO_LINK", "SHORT", "NO_RECEIPT", "BAD_SIGNATURE"):
        value = int(re.search(r"#define RT_PROOF_%s\s+(\d+)" % name, header).group(1))
        assert getattr(device, "PROOF_" + name) == getattr(_native, "RT_PROOF_" + name) == getattr(ph, name) == value
    assert (device.LINK_PROVE_ALL, device.LINK_HAS_CHANNEL) == (ph.PROVE_ALL, ph.HAS_CHANNEL) == (1, 2)


def test_inbound_refuses_signers_or_receipts_without_links():
    from reticulum_amd import pipeline
    for kw in (dict(signers=object()), dict(receipts=object()), dict(signers=object(), receipts=object())):
        with pytest.raises(ValueError, match="links"):
            pipeline.inbound(None, None, None, 0, 4, **kw)
    with pytest.raises(ValueError, match="signers"):
        pipeline.inbound(None, None, None, 0, 4, links=object(), receipts=object())
