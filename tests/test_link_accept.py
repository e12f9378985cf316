"""Link requests, host side (no GPU):
(a) the tests' plain model (tests/link_accept_helpers.py: hashlib, ed25519_ref,
    an RFC 7748 ladder) against what the reference's own Transport.inbound
    branch, Destination.receive and Link.validate_request were recorded doing
    (tests/golden/link_accept_vectors.json, made by gen_link_accept.py), bit for
    bit: accepted or rejected, link id, derived key, MTU and the LRPROOF packet;
(b) the fixed-width host arithmetic of the stage
    (reticulum_amd/csrc/linkreq_host.h) built alone under the address and
    undefined-behaviour sanitizers (tests/linkreq_host/plan_check.cpp, run
    directly) and compared with the model over the fixture;
(c) the new entry points: declared, exported, bound, ABI version unchanged;
(d) argument errors that are raised before any device is touched."""
import os
import re
import shutil
import subprocess

import pytest

import link_accept_helpers as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vec():
    return la.vectors()


def test_fixture_covers_the_cases(vec):
    notes = " | ".join(c["note"] for c in vec["cases"])
    for want in ("64-byte data, HEADER_1", "67-byte data, HEADER_2 with our", "foreign transport id", "below nh_mtu",
                 "equal to nh_mtu", "above nh_mtu", "no HW_MTU", "path_mtu 0", "mode 0", "mode 1", "mode 7",
                 "accepted with the default mode", "63-byte", "65-byte", "66-byte", "68-byte", "unknown destination",
                 "GROUP", "PLAIN", "LINK", "accept_link_requests off", "low-order peer_pub", "not a curve point",
                 "hops 0", "hops 127"):
        assert want in notes, want
    reached = {c["reached"] for c in vec["cases"]}
    assert reached == {"accepted", "transport", "destination", "validate"}


def test_model_matches_the_reference_on_every_case(vec):
    dests = la.fixture_dests(vec)
    for c in vec["cases"]:
        st, v = la.decide(c["raw"], dests, vec["transport_id"], c["nh_mtu"])
        assert st == la.STATUS[c["expect"]], c["note"]
        assert (st == la.ACCEPTED) == (c["reached"] == "accepted"), c["note"]
        # where the reference stopped: in Transport's branch, in the destination, in validate_request
        if st in (la.OTHER_TRANSPORT, la.NO_DESTINATION):
            assert c["reached"] == "transport", c["note"]
        if st == la.NOT_ACCEPTING:
            assert c["reached"] == "destination", c["note"]
        if st == la.BAD_SIZE:
            assert c["reached"] == "validate", c["note"]
        if st != la.ACCEPTED:
            continue
        dest, link_id, mtu, peer_pub, peer_sig = v
        assert dest.hash == vec["destinations"][c["dest"]]["hash"]
        assert link_id == c["link_id"], c["note"]
        assert mtu == c["mtu"] and c["mode"] == la.MODE_AES256_CBC, c["note"]
        assert peer_pub == c["peer_pub"] and peer_sig == c["peer_sig_pub"]
        key, proof = la.establish(dest, link_id, mtu, peer_pub, c["ephemeral"])
        assert key == c["derived_key"], c["note"]
        assert proof == c["lrproof"] and len(proof) == la.LRPROOF_LEN, c["note"]


def test_model_batch_rules(vec):
    dests = la.fixture_dests(vec)
    ok = [c for c in vec["cases"] if c["reached"] == "accepted" and c["nh_mtu"] == 500 and not c["raw"][0] & 0x40][:3]
    raws = [ok[0]["raw"], b"\x00" * 40, ok[0]["raw"], ok[1]["raw"], ok[2]["raw"]]
    eph = [c["ephemeral"] for c in (ok[0], ok[0], ok[1], ok[2])]
    table = {}
    out = la.accept(raws, dests, vec["transport_id"], 500, [5, 6, 9, 2], eph, table, n_keys=8)
    assert [r["status"] for r in out] == [la.ACCEPTED, la.NOT_REQUEST, la.DUPLICATE, la.NO_SLOT, la.ACCEPTED]
    assert [r["slot"] for r in out] == [5, -1, -1, -1, 2] and table == {ok[0]["link_id"]: 5, ok[2]["link_id"]: 2}
    assert out[0]["lrproof"] == ok[0]["lrproof"] and out[4]["derived_key"] == ok[2]["derived_key"]   # row 3's key
    out = la.accept([ok[1]["raw"], ok[2]["raw"]], dests, vec["transport_id"], 500, [0], [ok[1]["ephemeral"]], table, 8)
    assert [r["status"] for r in out] == [la.ACCEPTED, la.NO_SLOT]      # no slot left: not even looked up


def test_host_arithmetic_under_sanitizers(tmp_path, vec):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of linkreq_host.h")
    exe = str(tmp_path / "plan_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "linkreq_host", "plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) > 1000000
    # the same function against the model, over the fixture's requests to accepting destinations
    dests = la.fixture_dests(vec)
    lines, want = [], []
    for c in vec["cases"]:
        st, v = la.decide(c["raw"], dests, vec["transport_id"], c["nh_mtu"])
        if st not in (la.ACCEPTED, la.BAD_SIZE, la.BAD_MODE):
            continue
        at = 35 if c["raw"][0] & 0x40 else 19
        data = c["raw"][at:]
        b = list(data[64:67]) if len(data) == 67 else [0, 0, 0]
        lines.append("%d %d %d %d %d" % (len(data), b[0], b[1], b[2], -1 if c["nh_mtu"] is None else c["nh_mtu"]))
        cut = len(data) == 67 and c["nh_mtu"] is None and int.from_bytes(data[64:67], "big") & la.MTU_MASK
        want.append("%d %d %d" % ((st, v[2], 0 if cut or len(data) == 64 else 3) if st == la.ACCEPTED else (st, 0, 0)))
    r = subprocess.run([exe, "plan"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == want and len(want) > 50


NEW = ("rt_link_accept", "rt_keyset_set_rows_x25519")


def test_entry_points_declared_exported_and_bound():
    from reticulum_amd import _native, device, link, pipeline
    import reticulum_amd as rt
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    bound = {name for name, _, _ in _native.SIGNATURES}
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert name in bound and hasattr(lib, name), name
    assert _native.ABI_VERSION == 3 and lib.rt_abi_version() == 3
    # the header's codes, the bindings' and the model's are the same numbers
    for name, value in re.findall(r"#define RT_LINKREQ_(\w+)\s+(\d+)", header):
        assert getattr(device, "LINKREQ_" + name) == int(value) == getattr(link, "LINKREQ_" + name) == la.STATUS[name]
    assert int(re.search(r"#define RT_DEST_ACCEPTS (\d+)u", header).group(1)) == link.ACCEPTS == device.DEST_ACCEPTS
    assert (link.PROVE_ALL, link.HAS_CHANNEL) == (rt.proof.PROVE_ALL, rt.proof.HAS_CHANNEL)
    assert link.LRPROOF_LEN == device.LRPROOF_LEN == 118 and link.MTU == 500
    assert callable(device.link_accept) and callable(device.keyset_set_rows_x25519)
    assert callable(rt.LinkDestinations) and callable(rt.accept_requests_batch)
    assert "accept" in pipeline.inbound.__code__.co_varnames


def test_the_arguments_of_the_two_calls_line_up_with_the_header():
    from reticulum_amd import _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnstok.h")).read(), flags=re.S)
    sig = {name: args for name, _, args in _native.SIGNATURES}
    for name in NEW:
        params = re.search(r"\b%s\s*\((.*?)\);" % name, header, flags=re.S).group(1).split(",")
        assert len(params) == len(sig[name]), name


def test_pipeline_accept_needs_its_companions():
    torch = pytest.importorskip("torch")
    from reticulum_amd import pipeline

    class KS:
        key_len, n_keys = 64, 1

    buf = torch.zeros(8, dtype=torch.uint8)
    acc = {"destinations": object(), "slots": object(), "ephemeral_privates": object()}
    with pytest.raises(ValueError, match="accept needs links"):
        pipeline.inbound(KS(), buf, None, 0, 4, accept=acc)
    with pytest.raises(ValueError, match="accept needs links"):
        pipeline.inbound(KS(), buf, None, 0, 4, accept=acc, links=object())
    KS.key_len = 32
    with pytest.raises(ValueError, match="64-byte keys"):
        pipeline.inbound(KS(), buf, None, 0, 4, accept=acc, links=object(), transport_identity=buf)
    KS.key_len = 64
    with pytest.raises(ValueError, match="accept bundles"):
        pipeline.inbound(KS(), buf, None, 0, 4, accept={"slots": 1}, links=object(), transport_identity=buf)
