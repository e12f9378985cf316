"""The send side of a read, without a GPU.

(a) the tests' model (tests/reply_helpers.py) against what the reference
    recorded: Transport.transmit's sign tail, mask and IFAC flag rule in
    tests/golden/ifac_vectors.json, TCPInterface's escape and framing in
    tests/golden/wire_vectors.json.  This ties the model the GPU tests use to
    the reference;
(b) the model's own rules: frame-major order, the length rule, the capacity;
(c) the host header (reticulum_amd/csrc/reply_host.h) built alone with a small
    program under the address and undefined-behaviour sanitizers
    (tests/reply_host/plan_check.cpp, run directly);
(d) the new entry points: declared, exported, bound, ABI version unchanged, and
    the argument checks of the Python layer that raise before any launch."""
import json
import os
import re
import shutil
import subprocess

import pytest

import reply_helpers as rh
from oracle import wire as ow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


# ------------------------------------------------- model against the reference --

def test_transmit_model_is_the_reference_transmit():
    """Every recorded Transport.transmit: the model signs, takes the tail and
    masks to the recorded bytes, and sets the IFAC flag."""
    cases = _golden("ifac_vectors.json")["cases"]
    assert len(cases) >= 40 and {c["ifac_size"] for c in cases} >= {1, 16, 64}
    for c in cases:
        key, raw = bytes.fromhex(c["ifac_key"]), bytes.fromhex(c["raw"])
        masked = rh.transmit_model(raw, key, c["ifac_size"])
        assert masked.hex() == c["masked"]
        assert masked[0] & 0x80 and masked[2:2 + c["ifac_size"]].hex() == c["ifac"]
        assert len(masked) == len(raw) + c["ifac_size"]
    assert rh.transmit_model(raw) == raw                                  # no IFAC: as packed (Transport.py:1104)


def test_stream_model_is_the_reference_framing():
    """process_outgoing (TCPInterface.py:323): 7E || escape || 7E, the escape as recorded."""
    wv = _golden("wire_vectors.json")
    for e in wv["escape"]:
        data = bytes.fromhex(e["data"])
        (frame,) = rh.reply_stream_model([(0, 0, data)])
        assert frame == b"\x7e" + bytes.fromhex(e["escaped"]) + b"\x7e"
    # and over the recorded transmits: the frame of the masked packet unescapes to it
    for c in _golden("ifac_vectors.json")["cases"][:12]:
        key, raw = bytes.fromhex(c["ifac_key"]), bytes.fromhex(c["raw"])
        (frame,) = rh.reply_stream_model([(0, 0, raw)], key, c["ifac_size"])
        assert frame == ow.hdlc_frame(bytes.fromhex(c["masked"]))
        assert frame[0] == frame[-1] == 0x7E and ow.hdlc_unescape(frame[1:-1]) == bytes.fromhex(c["masked"])


def test_packet_hash_model_is_the_reference_hash():
    for u in _golden("wire_vectors.json")["unpack"]:
        if u["ok"]:
            assert rh.packet_hash(bytes.fromhex(u["raw"])).hex() == u["packet_hash"]


# ----------------------------------------------------------------------- model --

def test_gather_model_order_lengths_and_capacity():
    row = lambda tag, width=128: bytes([tag]) * width
    a = ([row(1), row(2), row(3), row(4)], [0, 5, 128, 129])
    b = ([row(5, 16), row(6, 16), row(7, 16), row(8, 16)], [16, 17, -1, 1])
    c = ([row(9), row(10), row(11), row(12)], [1, 0, 115, 0])
    replies, found = rh.gather_model([a, b, c])
    # b's 17 is longer than its 16-byte rows, a's 129 and b's -1 are out of range: nothing
    assert found == 6
    assert replies == [(0, 1, row(5, 16)), (0, 2, row(9, 1)), (1, 0, row(2, 5)), (2, 0, row(3)), (2, 2, row(11, 115)),
                       (3, 1, row(8, 1))]
    for cap in (0, 1, found - 1, found, found + 1):
        cut, f = rh.gather_model([a, b, c], cap)
        assert f == found and cut == replies[:cap]


# ------------------------------------------------------------------ host header --

@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ for the host build of reply_host.h")
    exe = str(tmp_path_factory.mktemp("reply_host") / "plan_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "reply_host", "plan_check.cpp")], check=True)
    return exe


def test_host_planning_under_sanitizers(plan_check):
    r = subprocess.run([plan_check], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) > 2000


def test_host_plan_agrees_with_the_library(plan_check):
    from reticulum_amd import _native
    lib = _native.load()
    for n in (0, 1, 1023, 1024, 1025, 1 << 20, (1 << 31) - 1):
        for S in (1, 2, 3, 4):
            for cap in (0, n, n + 1):
                r = subprocess.run([plan_check, "plan"], input=f"{n} {S} {cap}\n", capture_output=True, text=True)
                assert r.returncode == 0, r.stderr[-2000:]
                ws, count_grid, write_grid = (int(x) for x in r.stdout.split())
                blocks = (n + 1023) // 1024
                assert ws == (8 * (blocks + 1) + 15) // 16 * 16 == lib.rt_reply_gather_workspace_bytes(n, S)
                assert count_grid == blocks and write_grid == max(1, (max(n, cap) + 1023) // 1024)


# ----------------------------------------------------------------- entry points --

NEW = ("rt_reply_gather", "rt_hdlc_frame_counted", "rt_reply_remember")


def test_entry_points_are_declared_bound_and_exported():
    from reticulum_amd import _native, device
    header = open(os.path.join(ROOT, "include", "rnstok.h")).read()
    assert re.search(r"#define RNSTOK_ABI_VERSION 3\b", header) and _native.ABI_VERSION == 3
    bound = {name for name, _, _ in _native.SIGNATURES}
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in bound and hasattr(lib, name), name
    assert "rt_reply_gather_workspace_bytes" in bound and "uint64_t rt_reply_gather_workspace_bytes(" in header
    assert re.search(r"rt_reply_gather /\s+the replies of a read", header)                 # the table of reference lines
    for k, name in enumerate(("LRPROOF", "LINK_PROOF", "DEST_PROOF")):
        value = int(re.search(r"#define RT_REPLY_%s\s+(\d+)" % name, header).group(1))
        assert getattr(device, "REPLY_" + name) == getattr(_native, "RT_REPLY_" + name) == value == k
    assert lib.rt_reply_gather_workspace_bytes(1, 1) == 16
    for bad in (0, 5):
        assert lib.rt_reply_gather_workspace_bytes(8, bad) == 0
    assert lib.rt_reply_gather_workspace_bytes(1 << 31, 1) == 0                            # more than a call takes


def test_package_exports():
    import reticulum_amd as rt
    from reticulum_amd import pipeline, wire
    assert rt.reply_batch is wire.reply_batch
    assert callable(pipeline.reply) and [r for r, _ in pipeline.REPLY_SOURCES] == ["lr_proofs", "proofs", "dest_proofs"]


def test_reply_refuses_bad_arguments_before_any_launch():
    import torch
    from reticulum_amd import pipeline
    with pytest.raises(ValueError, match="at least one of lr_proofs, proofs and dest_proofs"):
        pipeline.reply({"status": torch.zeros(4, dtype=torch.int32)})
    with pytest.raises(ValueError, match="at least one of"):
        pipeline.reply({"proofs": torch.zeros((4, 128), dtype=torch.uint8)})              # rows without their lengths
    res = {"proofs": torch.zeros((4, 128), dtype=torch.uint8), "proof_len": torch.zeros(4, dtype=torch.int32)}
    with pytest.raises(ValueError, match="64-byte ifac_key"):
        pipeline.reply(res, ifac_size=16)
    with pytest.raises(ValueError, match="64-byte ifac_key"):
        pipeline.reply(res, ifac_key=torch.zeros(32, dtype=torch.uint8), ifac_size=16)
    with pytest.raises(ValueError, match="0..64"):
        pipeline.reply(res, ifac_key=torch.zeros(64, dtype=torch.uint8), ifac_size=65)
    with pytest.raises(ValueError, match="max_replies"):
        pipeline.reply(res, max_replies=-1)


def test_inbound_reply_argument_checks():
    from reticulum_amd import pipeline
    with pytest.raises(ValueError, match="at least one of signers, accept and deliver"):
        pipeline.inbound(None, None, None, 0, 4, reply=True)
    with pytest.raises(ValueError, match="True or a dict"):
        pipeline.inbound(None, None, None, 0, 4, signers=object(), reply=3)
    with pytest.raises(ValueError, match="max_replies only"):
        pipeline.inbound(None, None, None, 0, 4, signers=object(), reply={"cap": 3})
    with pytest.raises(ValueError, match="64-byte ifac_key"):
        pipeline.inbound(None, None, None, 16, 4, signers=object(), reply=True)
    # and the checks of a read without the argument come as before
    with pytest.raises(ValueError, match="links"):
        pipeline.inbound(None, None, None, 0, 4, signers=object())


def test_device_wrappers_refuse_bad_arguments_before_any_launch():
    import torch
    from reticulum_amd import device
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    outs = lambda cap: (u8(cap, 128), i32(cap), i32(cap), u8(cap), torch.zeros(2, dtype=torch.int64))
    src = (u8(4, 128), i32(4))
    with pytest.raises(ValueError, match="1 to 4 sources"):
        device.reply_gather([], *outs(4))
    with pytest.raises(ValueError, match="1 to 4 sources"):
        device.reply_gather([src] * 5, *outs(4))
    with pytest.raises(ValueError, match=r"\(cap, 128\)"):
        device.reply_gather([src], u8(4, 96), *outs(4)[1:])
    with pytest.raises(ValueError, match="torch.uint8"):
        device.reply_gather([(torch.zeros((4, 128), dtype=torch.int8), i32(4))], *outs(4))
    with pytest.raises(ValueError, match="int32"):
        device.reply_gather([(u8(4, 128), torch.zeros(4, dtype=torch.int64))], *outs(4))
    with pytest.raises(ValueError, match="int32"):
        device.reply_gather([src, (u8(4, 128), i32(5))], *outs(4))                         # another frame count
    with pytest.raises(ValueError, match=r"\(4, width\)"):
        device.reply_gather([src, (u8(5, 128), i32(4))], *outs(4))
    o = outs(4)
    with pytest.raises(ValueError, match="reply_frame"):
        device.reply_gather([src], o[0], o[1], i32(3), o[3], o[4])
    with pytest.raises(ValueError, match="reply_counts"):
        device.reply_gather([src], o[0], o[1], o[2], o[3], torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="reply_source"):
        device.reply_gather([src], o[0], o[1], o[2], u8(3), o[4])
    # counted framing
    pkt, off, ln, out = u8(512), torch.zeros(4, dtype=torch.int64), i32(4), u8(2048)
    foff, cnt = torch.zeros(5, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="n_dev"):
        device.hdlc_frame_counted(pkt, off, ln, torch.zeros(2, dtype=torch.int32), out, foff)
    with pytest.raises(ValueError, match="n_dev"):
        device.hdlc_frame_counted(pkt, off, ln, None, out, foff)
    with pytest.raises(ValueError, match="frame_off"):
        device.hdlc_frame_counted(pkt, off, ln, cnt, out, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="pkt_len"):
        device.hdlc_frame_counted(pkt, off, i32(3), cnt, out, foff)
    with pytest.raises(ValueError, match=r"\(cap, 128\)"):
        device.reply_remember(None, u8(4, 64), i32(4), cnt)
    with pytest.raises(ValueError, match="reply_len"):
        device.reply_remember(None, u8(4, 128), i32(3), cnt)


def test_reply_batch_refuses_bad_arguments():
    from reticulum_amd import wire
    with pytest.raises(ValueError, match="1 to 4 sources"):
        wire.reply_batch([])
    with pytest.raises(ValueError, match="one entry per frame"):
        wire.reply_batch([[b"a"], [b"a", b"b"]])
    with pytest.raises(ValueError, match="64-byte ifac_key"):
        wire.reply_batch([[b"a" * 20]], ifac_key=bytes(32), ifac_size=8)
    with pytest.raises(ValueError, match="at most 128"):
        wire.reply_batch([[b"a" * 129]])
    assert wire.reply_batch([[], []])[0] == b""
