"""Link request proofs, the initiator side of link establishment — what needs
no GPU:
(a) the plain model (tests/link_proof_helpers.py) tied bit for bit to
    tests/golden/link_proof_vectors.json, which the reference's own
    Transport.inbound recorded over real RNS.Link initiators, sequences included;
(b) link.pack_rtt against the recorded LRRTT plaintexts, and the packing of
    link.open_requests_batch against the recorded requests;
(c) reticulum_amd/csrc/lrproof_host.h built alone under the address and
    undefined-behaviour sanitizers (tests/lrproof_host/plan_check.cpp, run
    directly) and compared with the model over the fixture;
(d) the new entry point: declared, exported, bound, ABI version unchanged."""
import os
import re
import shutil
import subprocess

import pytest

import ed25519_ref as ed
import link_proof_helpers as lp
from link_accept_helpers import x25519

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vec():
    return lp.vectors()


def test_fixture_covers_the_cases(vec):
    notes = " | ".join(c["note"] for c in vec["cases"])
    for want in ("96-byte data, HEADER_1", "99-byte data, HEADER_2", "confirmed MTU 400", "confirmed MTU 1196",
                 "confirmed MTU 0", "mode 0 at 99", "mode 7 at 99", "95-byte", "97-byte data, mode bits right",
                 "97-byte data, mode bits wrong", "98-byte", "100-byte", "signature flipped", "peer_pub flipped",
                 "MTU flipped", "another link id", "another identity", "low-order peer_pub", "bit 255 set",
                 "valid signature: rebalanced", "invalid signature", "on a rebalanced link", "a forged proof, then",
                 "then a replay", "a bad length, then", "unknown link id", "context one off", "packet type DATA",
                 "destination type SINGLE"):
        assert want in notes, want
    assert len(vec["cases"]) >= 50


def test_model_matches_the_reference_on_every_case(vec):
    for c in vec["cases"]:
        link = lp.fixture_link(vec, c)
        pending = {link.link_id: link}
        for p in c["packets"]:
            st, remembered = lp.step(p["raw"], pending)
            a = p["after"]
            assert st == lp.STATUS[p["expect"]], (c["note"], st)
            assert link.state == lp.STATE[a["status"]], c["note"]
            assert (link.expected_hops, link.rebalanced) == (a["expected_hops"], a["rebalanced"]), c["note"]
            if st != lp.NOT_LRPROOF:                    # (such a packet the filter itself remembers)
                assert remembered == a["hash_added"], c["note"]
            assert (link.state == lp.ACTIVE) == a["active"], c["note"]
            if a["active"]:
                assert link.mtu == a["mtu"] and link.derived_key == a["derived_key"], c["note"]
            elif link.state == lp.PENDING:
                assert link.derived_key is None and a["derived_key"] is None, c["note"]
            # (in HANDSHAKE the reference holds a key the device never derives: nothing decrypts under it)


def test_model_batch_rules(vec):
    good = [c for c in vec["cases"] if c["packets"][0]["expect"] == "ACTIVATED" and len(c["packets"]) == 1][:3]
    links = [lp.fixture_link(vec, c, slot=5 + k) for k, c in enumerate(good)]
    raws = [good[0]["packets"][0]["raw"], b"\x00" * 40, good[0]["packets"][0]["raw"], good[1]["packets"][0]["raw"],
            good[2]["packets"][0]["raw"]]
    table = {}
    out = lp.run(raws, {l.link_id: l.copy() for l in links}, table, n_keys=7)
    assert [o[0] for o in out] == [lp.ACTIVATED, lp.NOT_LRPROOF, lp.NOT_PENDING, lp.ACTIVATED, lp.NO_SLOT]
    assert [o[1] for o in out] == [5, -1, -1, 6, -1] and table == {links[0].link_id: 5, links[1].link_id: 6}
    # a proof behind one that found no slot reads NOT_PENDING in the same call, and the link can still come up later
    pend = {links[2].link_id: links[2].copy()}
    out = lp.run([raws[4], raws[4]], pend, {}, n_keys=7)
    assert [o[0] for o in out] == [lp.NO_SLOT, lp.NOT_PENDING] and pend[links[2].link_id].state == lp.PENDING
    assert lp.run([raws[4]], pend, {}, n_keys=8)[0][:2] == (lp.ACTIVATED, 7)


def test_pack_rtt_and_request_packing(vec):
    import struct
    from reticulum_amd import link
    n = 0
    for c in vec["cases"]:
        for p in c["packets"]:
            if p["after"]["lrrtt"] is not None:
                assert link.pack_rtt(float.fromhex(p["after"]["rtt"])) == p["after"]["lrrtt"]
                n += 1
    assert n >= 20
    assert link.pack_rtt(0) == b"\xcb" + struct.pack(">d", 0.0) and len(link.pack_rtt(1)) == 9
    for c in vec["cases"][:8]:
        lk = c["link"]
        raw = link.pack_link_request(vec["destinations"][lk["dest"]]["hash"], x25519(lk["prv"], (9).to_bytes(32, "little")),
                                     ed.public_key(lk["sig_seed"]), mtu=500)
        assert raw == lk["request"] and link.link_id_from_lr_packet(raw) == lk["link_id"]
    assert len(link.pack_link_request(bytes(16), bytes(32), bytes(32), mtu=None)) == 83
    assert link.signalling_bytes(0x1FFFFF) == b"\x3f\xff\xff"
    with pytest.raises(TypeError):
        link.signalling_bytes(500, mode=0)


def _plan_line(raw, hop_match, rebalanced):
    data = raw[35 if raw[0] & 0x40 else 19:]
    b = list(data[96:99]) + [0, 0, 0]
    return "%d %d %d %d %d %d" % (len(data), b[0], b[1] if len(data) == 99 else 0, b[2] if len(data) == 99 else 0,
                                  hop_match, rebalanced)


def test_host_arithmetic_under_sanitizers(tmp_path, vec):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of lrproof_host.h")
    exe = str(tmp_path / "plan_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "lrproof_host", "plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) > 1000000
    # the same function against the fixture: the first packet of every case that reaches the rules
    lines, want = [], []
    for c in vec["cases"]:
        p = c["packets"][0]
        if p["expect"] in ("NO_LINK", "NOT_LRPROOF"):
            continue
        raw, lk = p["raw"], c["link"]
        hop = raw[1] + 1 == lk["expected_hops"]
        lines.append(_plan_line(raw, hop, lk["rebalanced"]))
        want.append(p["expect"])
    r = subprocess.run([exe, "plan"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [l.split() for l in r.stdout.split("\n")[:-1]]
    assert len(got) == len(want) > 40
    for g, w, c in zip(got, want, [c for c in vec["cases"] if c["packets"][0]["expect"] not in ("NO_LINK", "NOT_LRPROOF")]):
        st, verify = int(g[0]), int(g[1])
        a = c["packets"][0]["after"]
        if w == "BAD_SIGNATURE":
            assert st == lp.ACTIVATED and verify, c["note"]          # the signature turns it
        elif w == "ACTIVATED":
            assert verify and st in (lp.ACTIVATED, lp.HOPS), c["note"]
            assert int(g[4]) == a["mtu"], c["note"]
        else:
            assert st == lp.STATUS[w], c["note"]


def test_entry_point_declared_exported_and_bound():
    from reticulum_amd import _native, device, link
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert re.search(r"\bint\s+rt_link_establish\s*\(", header)
    assert "rt_link_establish" in {n for n, _, _ in _native.SIGNATURES}
    assert _native.ABI_VERSION == 3
    for name in ("RT_LRPROOF_ACTIVATED", "RT_LRPROOF_NO_SLOT", "RT_PENDING_HANDSHAKE"):
        assert name in header
    for name, value in (("ACTIVATED", 0), ("NOT_LRPROOF", 1), ("NO_LINK", 2), ("NOT_PENDING", 3), ("HOPS", 4),
                        ("BAD_SIZE", 6), ("BAD_MODE", 7), ("BAD_SIGNATURE", 8), ("NO_SLOT", 9)):
        assert re.search(r"#define RT_LRPROOF_%s\s+%d\b" % (name, value), header)
        assert getattr(device, "LRPROOF_" + name) == getattr(link, "LRPROOF_" + name) == value == lp.STATUS[name]
    assert (link.PENDING, link.HANDSHAKE, link.ACTIVE, link.CLOSED) == (0, 1, 2, 4)
    for name in ("PendingLinks", "establish_batch", "open_requests_batch", "pack_rtt"):
        assert hasattr(link, name)
    assert hasattr(device, "link_establish")
    lib = os.path.join(ROOT, "reticulum_amd", "librnstok.so")
    if os.path.exists(lib):
        import ctypes
        assert hasattr(ctypes.CDLL(lib), "rt_link_establish")


def test_the_arguments_line_up_with_the_header():
    from reticulum_amd import _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnstok.h")).read(), flags=re.S)
    args = re.search(r"int\s+rt_link_establish\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
    sig = {name: a for name, _, a in _native.SIGNATURES}["rt_link_establish"]
    assert len(sig) == len(args.split(","))


def test_pipeline_establish_needs_its_companions():
    torch = pytest.importorskip("torch")
    from reticulum_amd import pipeline

    class KS:
        key_len = 64
    with pytest.raises(ValueError, match="establish needs links"):
        pipeline.inbound(KS(), torch.zeros(4, dtype=torch.uint8), None, 0, 4, establish=object())
