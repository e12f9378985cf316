"""Destination delivery — what needs no GPU:
(a) the plain model (tests/destination_deliver_helpers.py) tied bit for bit to
    tests/golden/destination_deliver_vectors.json, which the reference's own
    Transport.inbound recorded over real registered destinations: status,
    plaintext, the ratchet's rank and the PROOF packet, byte for byte;
(b) the model's retry budget: whole frames only, a frame that does not fit
    defers every undecided frame behind it;
(c) reticulum_amd/csrc/destination_host.h built alone under the address and
    undefined-behaviour sanitizers (tests/destination_host/plan_check.cpp, run
    directly) and compared with the model's budget;
(d) the new entry point: declared, exported, bound, ABI version unchanged."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import destination_deliver_helpers as dd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vec():
    return dd.vectors()


@pytest.fixture(scope="module")
def dests(vec):
    return dd.fixture_dests(vec)


def test_fixture_covers_the_cases(vec):
    cases = vec["cases"]
    assert 30 <= len(cases) <= 80
    assert {len(d["ratchets"]) for d in vec["destinations"]} >= {0, 1, 2, 5}
    assert {d["prove"] for d in vec["destinations"]} == {"ALL", "NONE", "APP"}
    assert any(d["enforce"] and not d["ratchets"] for d in vec["destinations"])
    assert any(d["enforce"] and d["ratchets"] for d in vec["destinations"])
    expects = {c["expect"] for c in cases}
    assert expects >= {"DELIVERED", "NOT_OPENED", "TYPE_MISMATCH", "NO_DESTINATION", "SHORT"}
    lens = {len(c["raw"]) - (35 if c["raw"][0] & 0x40 else 19) for c in cases}
    assert lens >= {32, 33, 95, 96, 97, 112}
    assert any(c["raw"][0] & 0x40 and c["raw"][2:18] == vec["transport_id"] for c in cases)
    assert any(not c["implicit_proof"] and c["proof"] and len(c["proof"]) == 115 for c in cases)
    assert any(c["implicit_proof"] and c["proof"] and len(c["proof"]) == 83 for c in cases)
    eph = [c["raw"][19:51] for c in cases if not c["raw"][0] & 0x40]
    assert any(e[31] & 0x80 for e in eph) and any(e == bytes(32) for e in eph)
    assert any(c["raw"][18] != 0 and c["expect"] == "DELIVERED" for c in cases if not c["raw"][0] & 0x40)
    # every rank of every destination that has ratchets wins somewhere, and so does the identity's key
    for k, d in enumerate(vec["destinations"]):
        won = {c["ratchet"] for c in cases if c["dest"] == k and c["expect"] == "DELIVERED"}
        assert won >= set(range(len(d["ratchets"])))
        if not d["enforce"]:
            assert -1 in won


def test_model_matches_the_reference_case_by_case(vec, dests):
    for c in vec["cases"]:
        rec = dd.deliver([c["raw"]], dests, retry_trials=8, implicit=c["implicit_proof"])[0]
        assert rec["status"] == dd.STATUS[c["expect"]], c["note"]
        assert rec["dest"] == (-1 if c["dest"] is None else c["dest"]), c["note"]
        assert rec["plaintext"] == c["plaintext"], c["note"]
        assert rec["ratchet"] == c["ratchet"], c["note"]
        assert rec["proof"] == c["proof"], c["note"]         # the PROOF packet, byte for byte


def test_model_matches_the_reference_as_one_batch(vec, dests):
    raws = [c["raw"] for c in vec["cases"] if c["implicit_proof"]]
    want = [c for c in vec["cases"] if c["implicit_proof"]]
    budget = dd.second_pass_pairs(raws, dests)
    res = dd.deliver(raws, dests, retry_trials=budget)
    assert all(r["status"] != dd.DEFERRED for r in res)
    for c, r in zip(want, res):
        assert (r["status"], r["plaintext"], r["ratchet"], r["proof"]) == \
            (dd.STATUS[c["expect"]], c["plaintext"], c["ratchet"], c["proof"]), c["note"]
    # one row short: the last undecided frame and only it is deferred
    short = dd.deliver(raws, dests, retry_trials=budget - 1)
    deferred = [i for i, r in enumerate(short) if r["status"] == dd.DEFERRED]
    assert len(deferred) == 1
    assert all(short[i] == res[i] for i in range(len(res)) if i != deferred[0])
    # no budget: every frame its first candidate does not open and that has more is deferred
    none = dd.deliver(raws, dests, retry_trials=0)
    for r0, r in zip(none, res):
        if r0["status"] != dd.DEFERRED:
            assert r0 == r


def test_model_budget_whole_frames_only(vec, dests):
    d5 = next(k for k, d in enumerate(vec["destinations"]) if len(d["ratchets"]) == 5 and not d["enforce"])
    d1 = next(k for k, d in enumerate(vec["destinations"]) if len(d["ratchets"]) == 1 and not d["enforce"])
    by_dest = lambda k: next(c["raw"] for c in vec["cases"]                      # noqa: E731
                             if c["dest"] == k and c["expect"] == "DELIVERED" and c["ratchet"] == -1)
    raws = [by_dest(d5), by_dest(d1)]            # 5 and 1 remaining candidates
    res = dd.deliver(raws, dests, retry_trials=4)
    assert [r["status"] for r in res] == [dd.DEFERRED, dd.DEFERRED]
    res = dd.deliver(raws, dests, retry_trials=6)
    assert [r["status"] for r in res] == [dd.DELIVERED, dd.DELIVERED]
    res = dd.deliver(raws[::-1], dests, retry_trials=4)
    assert [r["status"] for r in res] == [dd.DELIVERED, dd.DEFERRED]


def test_host_planning_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of destination_host.h")
    exe = str(tmp_path / "plan_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "destination_host", "plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) > 1000000
    # the budget against the model's rule, at 0, 1, the exact fit and one past it
    rng = np.random.Generator(np.random.PCG64(7))
    for trial in range(6):
        rem = [int(x) for x in rng.integers(0, 6, 40) * (rng.random(40) < 0.5)]
        total = sum(rem)
        for retry in (0, 1, total - 1, total, total + 1):
            if retry < 0:
                continue
            r = subprocess.run([exe, "budget"], input="%d %d\n%s\n" % (retry, len(rem), " ".join(map(str, rem))),
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            lines = r.stdout.split("\n")
            start, stopped, used = 0, False, 0
            for i, v in enumerate(rem):
                fits, off = (int(x) for x in lines[i].split())
                want = bool(v) and not stopped and used + v <= retry
                assert bool(fits) == want and off == min(start, retry)
                if want:
                    used += v
                elif v:
                    stopped = True
                start += min(v, retry + 1)
            assert lines[len(rem)] == "pairs %d" % used
            if retry >= total:
                assert used == total


def test_entry_point_declared_exported_and_bound():
    from reticulum_amd import _native
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert "int rt_destination_deliver(" in header and "rt_destination_deliver_workspace_bytes(" in header
    assert re.search(r"rt_destination_deliver\s+packets for the node's", header)        # the table of reference lines
    assert re.search(r"#define RNSTOK_ABI_VERSION 3\b", header) and _native.ABI_VERSION == 3
    names = {}
    for name in ("DELIVERED", "NOT_DATA", "NO_DESTINATION", "TYPE_MISMATCH", "SHORT", "NOT_OPENED", "DEFERRED"):
        m = re.search(r"#define RT_DELIVER_%s\s+(\d+)" % name, header)
        assert m, name
        names[name] = int(m.group(1))
        assert names[name] == dd.STATUS[name]
    assert len(set(names.values())) == 7
    bound = {s[0] for s in _native.SIGNATURES}
    assert {"rt_destination_deliver", "rt_destination_deliver_workspace_bytes"} <= bound
    lib_path = _native.LIB_PATH
    if os.path.exists(lib_path):
        lib = _native.load()
        assert hasattr(lib, "rt_destination_deliver")
        small, big = (lib.rt_destination_deliver_workspace_bytes(n, r) for n, r in ((1, 0), (1024, 256)))
        assert 0 < small < big


def test_package_exports():
    import reticulum_amd
    from reticulum_amd import destination
    assert reticulum_amd.SingleDestinations is destination.SingleDestinations
    assert reticulum_amd.deliver_batch is destination.deliver_batch
    assert (destination.DELIVER_DELIVERED, destination.DELIVER_DEFERRED) == (dd.DELIVERED, dd.DEFERRED)
    assert (destination.PROVE_ALL, destination.ENFORCE_RATCHETS) == (dd.F_PROVE_ALL, dd.F_ENFORCE)
