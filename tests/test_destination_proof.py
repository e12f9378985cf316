"""Proofs for packets sent to SINGLE destinations, without a GPU.

(a) the fixture (tests/golden/destination_proof_vectors.json: real
    destinations, packets and PacketReceipts through the reference's own
    Transport.inbound) against the tests' model
    (tests/destination_proof_helpers.py): every recorded delivery and every
    receipt left, with the proofs of a batch fed one call each and as one call.
    This ties the model the GPU tests use to the reference;
(b) the model's own rules where the fixture cannot speak: the scan budget, the
    lowest index among copies, keyed = 0;
(c) the host header (reticulum_amd/csrc/dproof_host.h) built alone with a small
    program under the address and undefined-behaviour sanitizers
    (tests/dproof_host/plan_check.cpp, run directly) and compared with the
    model's budget;
(d) the new entry points: declared, exported, bound, ABI version unchanged, and
    the argument checks of the Python layer that raise before any launch."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import destination_proof_helpers as dp
import link_helpers as lh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 20


@pytest.fixture(scope="module")
def vec():
    return dp.vectors()


def _receipts(vec, b, max_receipts=16):
    """The batch's receipts in the model, ids in the order listed."""
    r = dp.Receipts(max_receipts)
    keys = [bytes.fromhex(vec["identities"][k]["public"]) if k is not None else None for _, k in b["receipts"]]
    hashes = [bytes.fromhex(h) for h, _ in b["receipts"]]
    for i, (h, k) in enumerate(zip(hashes, keys)):
        assert r.add([h], [i], None if k is None else [k]) == [lh.OK]
    return r, hashes


# ----------------------------------------------------------------- fixture --

def test_fixture_covers_the_stated_cases(vec):
    assert os.path.getsize(dp.VECTORS) < 100_000
    batches = vec["batches"]
    assert 12 <= len(batches) <= 40 and sum(len(b["raws"]) for b in batches) <= 100
    for i in vec["identities"]:
        assert dp.public_key(bytes.fromhex(i["seed"])).hex() == i["public"]
    raws = [bytes.fromhex(r) for b in batches for r in b["raws"]]
    assert {0, 63, 64, 65, 95, 96, 97, 160} <= {len(r) - 19 for r in raws}
    assert {0xFF, 0x05} <= {r[18] for r in raws}                                      # LRPROOF, RESOURCE_PRF
    assert any((r[0] >> 2) & 3 == lh.LINK for r in raws)
    assert any(k is None for b in batches for _, k in b["receipts"])                  # a receipt on a link
    notes = " ".join(b["note"] for b in batches)
    for want in ("Identity.prove", "bit flipped", "another identity", "agrees with the receipt's in 16 bytes",
                 "the stray that validates", "addressed to receipt A and signed for receipt B", "twice",
                 "destination is a link", "not active", "LRPROOF"):
        assert want in notes, want
    (meet,) = [b for b in batches if "from_deliver" in b]
    assert sorted(len(bytes.fromhex(r)) for r in meet["raws"]) == [83, 83, 115, 115]
    with open(os.path.join(ROOT, "tests", "golden", "destination_deliver_vectors.json")) as f:
        dv = json.load(f)
    assert [dv["cases"][k]["proof"] for k in meet["from_deliver"]] == meet["raws"]
    assert [dp.unpack(bytes.fromhex(dv["cases"][k]["raw"]))["packet_hash"].hex() for k in meet["from_deliver"]] == \
        [h for h, _ in meet["receipts"]] == meet["delivered"]


def test_a_link_receipt_is_never_delivered_in_the_fixture(vec):
    on_link = {h for b in vec["batches"] for h, k in b["receipts"] if k is None}
    assert on_link
    for b in vec["batches"]:
        assert not on_link & {d for d in b["delivered"] if d}
        assert on_link & {h for h, _ in b["receipts"]} <= set(b["left"])


@pytest.mark.parametrize("one_call", [False, True])
def test_model_matches_the_reference(vec, one_call):
    for b in vec["batches"]:
        receipts, hashes = _receipts(vec, b)
        packets = [dp.unpack(bytes.fromhex(r)) for r in b["raws"]]
        if one_call:
            got = dp.settle(packets, receipts, BIG)
        else:
            got = [dp.settle([p], receipts, BIG)[0] for p in packets]
        for (st, rid), want, raw in zip(got, b["delivered"], b["raws"]):
            assert (st == dp.DELIVERED) == (want is not None), (b["note"], raw)
            assert (hashes[rid].hex() if rid >= 0 else None) == want, b["note"]
            assert st != dp.DEFERRED
        left = sorted(receipts.hashes[i].hex() for i in receipts.table.entries.values())
        assert left == sorted(b["left"]), b["note"]


def test_model_statuses_on_the_fixture(vec):
    seen = set()
    for b in vec["batches"]:
        receipts, _ = _receipts(vec, b)
        for raw in b["raws"]:
            raw = bytes.fromhex(raw)
            (st, _), = dp.settle([dp.unpack(raw)], receipts, BIG)
            seen.add(st)
            if raw[18] in (0xFF, 0x05):
                assert st == dp.NOT_PROOF
            elif len(raw) - 19 not in (64, 96):
                assert st == dp.BAD_LENGTH
    assert seen == {dp.DELIVERED, dp.NOT_PROOF, dp.BAD_LENGTH, dp.NO_RECEIPT, dp.BAD_SIGNATURE}


# ------------------------------------------------------------------- model --

def _world(n, keyed=None):
    rng = np.random.Generator(np.random.PCG64(64))
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(2)]
    hashes = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    r = dp.Receipts(max(n, 1))
    keys = [dp.public_key(seeds[i & 1]) for i in range(n)]
    for i in range(n):
        r.add([hashes[i]], [i], [keys[i]] if keyed is None or keyed[i] else None)
    return r, hashes, seeds, rng


def test_model_budget_whole_frames_only():
    for trials, fit in ((0, 0), (2, 0), (3, 1), (5, 1), (6, 2), (BIG, 4)):
        r, hashes, seeds, rng = _world(3)
        elsewhere = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        strays = [dp.proof_packet(hashes[k], seeds[k & 1], True, address=elsewhere) for k in (2, 0, 1)]
        strays.append(dp.proof_packet(hashes[1], seeds[0], True))          # addressed, signed by the wrong key
        got = dp.settle([dp.unpack(s) for s in strays], r, trials)
        want = [(dp.DELIVERED, k) for k in (2, 0, 1)] + [(dp.NO_RECEIPT, -1)]
        assert got == want[:fit] + [(dp.DEFERRED, -1)] * (4 - fit), trials
        assert len(r) == 3 - min(fit, 3)


def test_model_lowest_index_and_keyed_zero():
    r, hashes, seeds, rng = _world(4, keyed=[1, 0, 1, 1])
    elsewhere = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
    good = dp.proof_packet(hashes[0], seeds[0], True)
    batch = [dp.proof_packet(hashes[0], seeds[0], True, address=elsewhere), good,             # the stray is lower
             dp.proof_packet(hashes[2], seeds[0], False), dp.proof_packet(hashes[2], seeds[0], True, address=elsewhere),
             dp.proof_packet(hashes[1], seeds[1], False), dp.proof_packet(hashes[1], seeds[1], True),   # keyed = 0
             dp.proof_packet(hashes[3], seeds[0], False), dp.proof_packet(hashes[3], seeds[1], False)]  # bad, then good
    got = dp.settle([dp.unpack(p) for p in batch], r, BIG)
    assert got == [(dp.DELIVERED, 0), (dp.NO_RECEIPT, -1), (dp.DELIVERED, 2), (dp.NO_RECEIPT, -1),
                   (dp.NO_RECEIPT, -1), (dp.NO_RECEIPT, -1), (dp.BAD_SIGNATURE, -1), (dp.DELIVERED, 3)]
    assert len(r) == 1 and r.live_keyed() == []
    # with no keyed receipt left every stray is NO_RECEIPT, whatever the budget
    assert dp.settle([dp.unpack(good)], r, 0) == [(dp.NO_RECEIPT, -1)]


# ------------------------------------------------------------- host header --

@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of dproof_host.h")
    exe = str(tmp_path_factory.mktemp("dproof_host") / "plan_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "dproof_host", "plan_check.cpp")], check=True)
    return exe


def test_host_planning_under_sanitizers(plan_check):
    r = subprocess.run([plan_check], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) > 100000


def test_host_budget_agrees_with_the_model(plan_check):
    for L in (0, 1, 3, 64):
        for trials in sorted({0, 1, max(L - 1, 0), L, 2 * L - 1 if L else 0, 2 * L, 5 * L + 1}):
            strays = 4
            r = subprocess.run([plan_check, "budget"], input=f"{trials} {L} {strays}\n", capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            lines = [tuple(int(x) for x in ln.split()) for ln in r.stdout.split("\n") if ln]
            fits = [L != 0 and (k + 1) * L <= trials for k in range(strays)]
            assert lines[:strays] == [(int(f), int(L != 0 and not f)) for f in fits], (L, trials)
            assert lines[strays] == (sum(fits), sum(fits) * L)


# ------------------------------------------------------------ entry points --

NEW = ("rt_receipt_store_keyed", "rt_destination_proof_settle")


def test_entry_points_are_declared_bound_and_exported():
    from reticulum_amd import _native, device
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert re.search(r"#define RNSTOK_ABI_VERSION 3\b", header) and _native.ABI_VERSION == 3
    bound = {name for name, _, _ in _native.SIGNATURES}
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in bound and hasattr(lib, name), name
    assert "rt_destination_proof_workspace_bytes" in bound
    assert re.search(r"rt_destination_proof_settle\s+sent to SINGLE", header)             # the table of reference lines
    for name in ("DELIVERED", "NOT_PROOF", "ON_LINK", "BAD_LENGTH", "NO_RECEIPT", "BAD_SIGNATURE", "DEFERRED"):
        value = int(re.search(r"#define RT_DPROOF_%s\s+(\d+)" % name, header).group(1))
        assert getattr(device, "DPROOF_" + name) == getattr(_native, "RT_DPROOF_" + name) == getattr(dp, name) == value
    small, big = (lib.rt_destination_proof_workspace_bytes(n, m) for n, m in ((1, 8), (1 << 20, 1024)))
    assert 0 < small < big and small % 16 == 0 and big % 16 == 0
    assert lib.rt_destination_proof_workspace_bytes(1 << 30, 8) == 0                       # more than a call takes


def test_package_exports():
    import reticulum_amd as rt
    from reticulum_amd import destination, proof
    assert rt.DestinationReceipts is proof.DestinationReceipts
    assert rt.settle_destination_proofs_batch is destination.settle_destination_proofs_batch
    assert "DestinationReceipts" in proof.__all__


def test_add_refuses_bad_ids_and_key_rows():
    import torch
    from reticulum_amd.proof import DestinationReceipts
    r = object.__new__(DestinationReceipts)               # the checks come before anything touches a device
    r.device, r.max_receipts, r.table = torch.device("cpu"), 8, None
    h = [bytes(32), bytes([1]) * 32]
    with pytest.raises(ValueError, match="receipt ids"):
        r.add(h, [0, 8])
    with pytest.raises(ValueError, match="receipt ids"):
        r.add(h, [-1, 0], keys=[bytes(32)] * 2)
    with pytest.raises(ValueError, match="32 bytes each"):
        r.add(h, [0, 1], keys=[bytes(31), bytes(32)])
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        r.add(h, [0, 1], keys=np.zeros((2, 64), dtype=np.uint8))
    with pytest.raises(ValueError, match="one 32-byte row per hash"):
        r.add(h, [0, 1], keys=[bytes(32)])
    with pytest.raises(ValueError, match="32 bytes each"):
        r.add([bytes(16)], [0])


def test_inbound_with_destination_receipts_keeps_the_argument_checks():
    from reticulum_amd import pipeline
    for kw in (dict(signers=object()), dict(receipts=object())):
        with pytest.raises(ValueError, match="links"):
            pipeline.inbound(None, None, None, 0, 4, destination_receipts=object(), **kw)
    with pytest.raises(ValueError, match="signers"):
        pipeline.inbound(None, None, None, 0, 4, links=object(), receipts=object(), destination_receipts=object())
