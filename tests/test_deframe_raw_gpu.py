"""The HDLC deframer (k_flag_local, k_flag_gather, k_hdlc_unescape,
deframe_counts in reticulum_amd/csrc/wire_kernels.hip) on raw streams: bytes
as a peer may send them, not as the framer writes them.  In a canonical
stream 7D is always followed by 5D or 5E; here it is followed by anything,
the closing flag included, and the special bytes sit on every word, lane
(16 B) and window (256 B) edge of the unescape kernel and the flags on every
quarter (4 KiB), chunk (16 KiB) and scan-block (1024 chunks) edge of the
flag pass.

Every call goes through reticulum_amd.device.hdlc_deframe with all outputs
pre-filled with guard values (tests/deframe_helpers.py::run_device) and is
compared bit for bit with the read loop restated over numpy and
bytes.replace (ref_pairs, held to the oracle by tests/test_deframe_raw.py):
counts, every pair's offset, length, status and bytes, and every byte of
`out` outside the frames.  The framing kernels (k_hdlc_count, k_hdlc_write)
get the same deterministic treatment at the end.
"""
import numpy as np
import pytest

import deframe_helpers as dh
from deframe_helpers import BAD_LEN, CHUNK, EMPTY, FILL, FRAME, GUARD, IGUARD, OK, fill, with_flags
from oracle import wire as ow

pytestmark = pytest.mark.gpu

HW_MTU = 500


def _both(stream, hw_mtu=HW_MTU, ifac_size=0, what="", **kw):
    ref = dh.ref_pairs(stream, hw_mtu, ifac_size)
    dh.check(dh.run_device(stream, hw_mtu, ifac_size, **kw), ref, what)
    return ref


def _host_form(stream, hw_mtu, ifac_size):
    """wire.deframe (the host convenience) gives what ref_pairs gives."""
    from reticulum_amd import wire
    ref = dh.ref_pairs(stream, hw_mtu, ifac_size)
    frames, invalid, consumed = wire.deframe(stream, hw_mtu, ifac_size)
    want = dh.as_oracle(ref, stream)
    assert frames == want[0] and invalid == want[1] and consumed == ref.consumed


# ------------------------------------------- (a) short patterns at the edges --

def test_every_short_pattern_at_frame_lane_and_window_edges():
    """All 1364 strings of 1..5 bytes over {7D, 5E, 5D, 11} at frame offsets
    0, 14 and 254 and at the frame's end, where the closing flag follows the
    string and the next frame opens with 5E or 5D."""
    stream, opens = dh.pattern_stream()
    assert len(opens) == 1364 * 5 and len(stream) < 5_000_000
    arr = np.frombuffer(stream, np.uint8)
    assert (arr[opens] == 0x7E).all() and (arr[opens + FRAME + 1] == 0x7E).all()
    # the frames begin at all 16 alignments, so words and lanes see every phase
    assert set(((opens + 1) % 16).tolist()) == set(range(16))
    assert b"\x7d\x7e\x5e" in stream and b"\x7d\x7e\x5d" in stream and b"\x7d\x7d\x5e\x7e" in stream
    ref = _both(stream, hw_mtu=1000, what="patterns")
    assert {FRAME, FRAME - 1, FRAME - 2} <= set(ref.lens.tolist())        # replacements shorten the frames
    _host_form(stream, 1000, 0)


# --------------------------------------------------------- (b) position sweep --

def test_escape_patterns_at_every_offset_two_windows_deep():
    """7D 5E, 7D 5D, 7D 7D 5E, 7D 5D 5E and 7D 20 starting at every frame
    offset 0..530: every word, lane and window phase, two windows deep."""
    stream, where = dh.sweep_stream()
    assert len(where) == 5 * 531
    for p in dh.SWEEP_PATTERNS:
        offs = [o for at, q, o in where if q == p and stream[at] == 0x7E and stream[at + 1 + o:at + 1 + o + len(p)] == p
                and stream[at + 1:at + 1 + o] == fill(o)]
        assert offs == list(range(531)), p.hex()
        # the pattern straddles the word, lane and window edges of both windows
        assert {3, 15, 255, 271, 511, 527} <= set(offs)
    ref = _both(stream, hw_mtu=1000, what="sweep")
    assert ref.npairs == 2 * len(where) - 1 and (ref.status[1::2] == EMPTY).all() and (ref.status[0::2] == OK).all()


# --------------------------------------------------------- (c) dense raw bodies --

@pytest.mark.parametrize("line_phase", [None, 0, 35, 127])
def test_dense_raw_bodies(line_phase):
    """3000 unescaped bodies of 0..700 bytes thick with 7D, 5E and 5D: lanes
    that keep fewer than 8 of their 16 bytes, or none, in stream and slots
    mode."""
    stream = dh.dense_stream()
    ref = _both(stream, ifac_size=8, line_phase=line_phase, what=f"dense, line_phase {line_phase}")
    assert ref.npairs >= 3000 and len(stream) < 5_000_000
    assert {OK, BAD_LEN, EMPTY} <= set(ref.status.tolist())
    # whole lanes that keep every count from 8 (the fewest a whole lane can) to
    # 16, last lanes that keep fewer than 8, and last lanes that keep nothing
    held, kept = dh.lane_kept(stream)
    assert set(kept[held == 16].tolist()) == set(range(8, 17))
    assert set(range(8)) <= set(kept[held < 16].tolist())


def test_dense_raw_bodies_host_form():
    _host_form(dh.dense_stream(), HW_MTU, 8)


# ------------------------------------------------------------ (d) flag geometry --

GEOM_LEN = 40000
GEOM_POS = (0, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 12288, 16383, 16384, 16385, 32767, 32768, GEOM_LEN - 1)
GEOM_BACKGROUND = (100, 5000, 20000, 39000)     # frames around the runs, one of them longer than a quarter


@pytest.mark.parametrize("run", [1, 2, 3, 17, 64])
def test_flag_runs_on_quarter_and_chunk_edges(run):
    for p in GEOM_POS:
        first = min(p, GEOM_LEN - run)          # the run at len-1 ends there
        flags = set(GEOM_BACKGROUND) | set(range(first, first + run))
        stream = with_flags(GEOM_LEN, flags)
        got = np.flatnonzero(np.frombuffer(stream, np.uint8) == 0x7E)
        assert set(got.tolist()) == flags and p in flags
        _both(stream, what=f"run of {run} flags at {p}")


def test_flag_run_across_the_chunk_edge_and_lone_flags():
    flags = set(range(CHUNK - 6, CHUNK + 7))
    stream = with_flags(3 * CHUNK, flags | {50, 3 * CHUNK - 40})
    assert {CHUNK - 1, CHUNK} <= set(np.flatnonzero(np.frombuffer(stream, np.uint8) == 0x7E).tolist())
    _both(stream, what="run across 16384")
    for p in GEOM_POS:                          # a lone flag: no pair, nothing written
        ref = _both(with_flags(GEOM_LEN, {p}), what=f"lone flag at {p}")
        assert ref.npairs == 0 and ref.pos.tolist() == [p]


def test_one_chunk_of_nothing_but_flags():
    flags = set(range(CHUNK, 2 * CHUNK)) | {7, 9000, 2 * CHUNK + 30, 3 * CHUNK - 200}
    stream = with_flags(3 * CHUNK, flags)
    arr = np.frombuffer(stream, np.uint8)
    assert (arr[CHUNK:2 * CHUNK] == 0x7E).all() and (arr[:CHUNK] == 0x7E).sum() == 2 == (arr[2 * CHUNK:] == 0x7E).sum()
    ref = _both(stream, what="chunk of flags")
    assert ref.npairs == CHUNK + 3 and (ref.status == EMPTY).sum() == CHUNK - 1


def test_frame_longer_than_a_chunk():
    flags = {10, 10 + 40001, 59000}
    stream = with_flags(60000, flags)
    pos = np.flatnonzero(np.frombuffer(stream, np.uint8) == 0x7E)
    assert set(pos.tolist()) == flags and not set(pos // CHUNK) & {1}       # chunk 1 holds no flag
    ref = _both(stream, hw_mtu=262144, what="40000-byte frame")
    assert ref.lens.tolist() == [40000, 59000 - 40012] and ref.status.tolist() == [OK, OK]
    # the same frame with escapes across its first window edge, the chunk
    # edges and at its very end
    raw = bytearray(stream)
    for at in (11 + 255, CHUNK - 1, 20000, 2 * CHUNK - 1, 40009):
        raw[at:at + 2] = b"\x7d\x5e" if at % 2 else b"\x7d\x5d"
    assert raw[40011] == 0x7E and raw.count(0x7E) == 3
    ref = _both(bytes(raw), hw_mtu=262144, what="40000-byte frame with escapes")
    assert ref.lens[0] == 40000 - 5


@pytest.mark.parametrize("length", [1, 15, 16, 17, 4096, 16383, 16384, 16385, 32769])
def test_stream_lengths_and_tails(length):
    """Streams that end on and around the 16-B unit, quarter and chunk edges:
    a frame that closes inside the last 16 bytes, then a partial tail of
    1..15 bytes, no tail at all, no flag at all, nothing but flags."""
    cases = [("no flag", set()), ("all flags", set(range(length)) if length <= 4096 else {0, length - 1})]
    for tail in (0, 1, 7, 15):
        last = length - 1 - tail
        if last < 0:
            continue
        flags = {last} | ({0} if last > 0 else set()) | ({last - 22} if last - 22 > 0 else set())
        cases.append((f"tail {tail}", flags))
    for name, flags in cases:
        stream = with_flags(length, flags)
        ref = _both(stream, what=f"length {length}, {name}")
        assert ref.pos.tolist() == sorted(flags)
        if name.startswith("tail") and len(flags) > 1:
            assert length - 16 <= ref.pos[-1] and ref.consumed == ref.pos[-1]      # closes in the last 16 bytes


@pytest.mark.parametrize("ifac_size", [0, 8])
def test_frame_length_limits_go_by_the_unescaped_length(ifac_size):
    """check_frame_len at 19 | 20 and hw_mtu + ifac_size | + 1 kept bytes, from
    plain bodies and from bodies whose raw length is 10 more."""
    top = HW_MTU + ifac_size
    kept = (19, 20, top, top + 1)
    plain = [fill(n) for n in kept]
    escaped = [b"\x7d\x5e" * 5 + fill(n - 10) + b"\x7d\x5d" * 5 for n in kept]
    stream = b"\x7e" + b"\x7e".join(plain + escaped) + b"\x7e"
    ref = _both(stream, ifac_size=ifac_size, what=f"limits, ifac_size {ifac_size}")
    assert ref.lens.tolist() == list(kept) * 2 and ref.status.tolist() == [BAD_LEN, OK, OK, BAD_LEN] * 2
    assert [len(e) for e in escaped] == [n + 10 for n in kept]
    dh.check(dh.run_device(stream, HW_MTU, ifac_size, line_phase=35), ref, "limits, slots")
    _host_form(stream, HW_MTU, ifac_size)


# -------------------------------------------------- (e) more than 1024 chunks --

def test_stream_of_more_than_1024_chunks():
    """16 MiB + 2 chunks + 5 bytes: chunk counts fill one scan block and start
    a second, so k_flag_gather's part[c / 1024] is nonzero for the last three
    chunks.  Filler and flags only: a frame is its input slice."""
    MiB16 = 16 << 20
    length = MiB16 + 2 * CHUNK + 5
    rng = np.random.Generator(np.random.PCG64(1024))
    forced = [MiB16 - 1, MiB16, MiB16 + 1, MiB16 + 100, MiB16 + CHUNK - 1, MiB16 + CHUNK, MiB16 + 2 * CHUNK - 3,
              length - 3]
    pos = np.unique(np.concatenate([rng.integers(0, length, 3000), np.array(forced)]))
    arr = np.full(length, FILL, np.uint8)
    arr[pos] = 0x7E
    chunk_of = pos // CHUNK
    assert -(-length // CHUNK) == 1027 and set(forced) <= set(pos.tolist())
    assert {1023, 1024, 1025, 1026} <= set(chunk_of.tolist()) and (chunk_of < 1024).sum() > 2900
    assert length - 5 <= pos[-1]
    hw_mtu = 4096
    r = dh.run_device(arr.tobytes(), hw_mtu, 0, max_pairs=len(pos) - 1)
    npairs = len(pos) - 1
    lens = np.diff(pos) - 1
    status = np.where(lens == 0, EMPTY, np.where((lens <= 19) | (lens > hw_mtu), BAD_LEN, OK))
    assert {OK, BAD_LEN} <= set(status.tolist())
    assert r.counts.tolist()[:2] == [npairs, int(pos[-1])]
    assert np.array_equal(r.off[:npairs], pos[:-1] + 1)
    assert np.array_equal(r.len[:npairs], lens) and np.array_equal(r.status[:npairs], status)
    assert (r.off[npairs:] == IGUARD).all() and (r.len[npairs:] == IGUARD).all() and (r.status[npairs:] == IGUARD).all()
    image = np.full(r.out.size, GUARD, np.uint8)
    inside = slice(int(pos[0]) + 1, int(pos[-1]))
    image[inside] = np.where(arr[inside] == 0x7E, GUARD, arr[inside])
    assert np.array_equal(r.out, image)


# ------------------------------------------- (f) max_pairs below the pair count --

def _forty_pairs():
    rng = np.random.Generator(np.random.PCG64(40))
    bodies = []
    for k in range(40):
        body = fill(int(rng.integers(0, 300)))
        if k % 3 == 0:
            body = b"\x7d\x5e" + body + b"\x7d\x5d\x7d"
        bodies.append(body if k % 7 else b"")
    return fill(9) + b"\x7e" + b"\x7e".join(bodies) + b"\x7e" + fill(33)


@pytest.mark.parametrize("line_phase", [None, 35])
@pytest.mark.parametrize("max_pairs", [0, 1, 7, 8, 9, 39])
def test_max_pairs_below_the_pairs_present(max_pairs, line_phase):
    """The tables hold fewer entries than the stream has pairs: entries at and
    past max_pairs and the later frames' bytes stay untouched, counts[0] is
    still the true pair count and counts[1] what full capacity gives."""
    stream = _forty_pairs()
    ref = dh.ref_pairs(stream, HW_MTU, 0)
    assert ref.npairs == 40 > max_pairs
    full = dh.run_device(stream, HW_MTU, 0, line_phase=line_phase)
    dh.check(full, ref, "full capacity")
    r = dh.run_device(stream, HW_MTU, 0, line_phase=line_phase, max_pairs=max_pairs)
    dh.check(r, ref, f"max_pairs {max_pairs}")
    assert r.counts[0] == 40 and r.counts[1] == full.counts[1]


def test_max_pairs_zero_with_null_frame_arrays():
    """rt_hdlc_deframe with max_pairs = 0 and NULL frame arrays (the launch of
    k_deframe_counts alone): the counts, and `out` untouched."""
    stream = _forty_pairs()
    ref = dh.ref_pairs(stream, HW_MTU, 0)
    dh.check(dh.run_device(stream, HW_MTU, 0, max_pairs=0, null_arrays=True), ref, "NULL frame arrays")
    long_tail = stream + fill(2 * HW_MTU)
    ref = dh.ref_pairs(long_tail, HW_MTU, 0)
    assert ref.consumed == len(long_tail)
    dh.check(dh.run_device(long_tail, HW_MTU, 0, max_pairs=0, null_arrays=True), ref, "NULL frame arrays, long tail")


# ------------------------------------------------------- (g) counts[1] limits --

CONSUMED_CASES = [
    ("tail of 1000 from the last flag", b"\x7e" + fill(30) + b"\x7e" + fill(999), 1, 1000, 31),
    ("tail of 1001 from the last flag", b"\x7e" + fill(30) + b"\x7e" + fill(1000), 1, 1001, 1032),
    ("one flag in 1000 bytes", fill(400) + b"\x7e" + fill(599), 0, 1000, 0),
    ("one flag in 1001 bytes", fill(400) + b"\x7e" + fill(600), 0, 1001, 1001),
    ("no flag", fill(300), 0, None, 300),
    ("no flag in 1001 bytes", fill(1001), 0, None, 1001),
    ("a flag and nothing else", b"\x7e", 0, 1, 0),
    ("a flag first", b"\x7e" + fill(50), 0, 51, 0),
    ("a flag last", fill(50) + b"\x7e", 0, 51, 0),
]


@pytest.mark.parametrize("name,stream,pairs,held,consumed", CONSUMED_CASES,
                         ids=[c[0].replace(" ", "_") for c in CONSUMED_CASES])
def test_bytes_consumed_at_its_limits(name, stream, pairs, held, consumed):
    """counts[1] with hw_mtu = 500: the loop drops what it holds (`held`
    bytes: from the last flag on after a pair, the whole buffer with a single
    flag) only when that is longer than 2 * hw_mtu = 1000."""
    ref = dh.ref_pairs(stream, HW_MTU, 0)
    assert (ref.npairs, ref.consumed) == (pairs, consumed)
    flags = np.flatnonzero(np.frombuffer(stream, np.uint8) == 0x7E)
    assert held == (None if len(flags) == 0 else len(stream) - (int(flags[-1]) if pairs else 0))
    dh.check(dh.run_device(stream, HW_MTU, 0), ref, name)
    dh.check(dh.run_device(stream, HW_MTU, 0, max_pairs=0, null_arrays=True), ref, name + ", counts kernel")
    dh.check(dh.run_device(stream, HW_MTU, 0, max_pairs=4, line_phase=0), ref, name + ", slots")


# ------------------------------------------------------------------ framing --

FRAMING_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513)


def _framing_packets():
    pk = []
    for n in FRAMING_LENGTHS:
        pk += [b"\x7e" * n, b"\x7d" * n, (b"\x7e\x11" * n)[:n]]
    for i in range(257):
        pk.append(fill(i) + b"\x7e" + fill(256 - i))
    return pk


def test_framing_kernels_at_lane_and_window_edges():
    """k_hdlc_count / k_hdlc_write on packets of nothing but 7E, nothing but
    7D, every other byte 7E, at lengths around the 16-B lane and the 256-B
    window, and one 7E at each position of a 257-byte packet: every frame is
    the oracle's, frame_off its prefix sums, nothing is written past
    frame_off[n], and the deframer returns the packets."""
    import torch
    from reticulum_amd import device
    pk = _framing_packets()
    n = len(pk)
    assert n == 3 * len(FRAMING_LENGTHS) + 257
    want = [ow.hdlc_frame(p) for p in pk]
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64)
    lens = np.array([len(p) for p in pk], np.int32)
    off = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    dev = torch.device("cuda", 0)
    flat = torch.from_numpy(np.frombuffer(b"".join(pk), np.uint8).copy()).to(dev)
    cap = int(2 * lens.sum() + 2 * n)
    out = torch.full((cap + 256,), GUARD, dtype=torch.uint8, device=dev)
    foff = torch.full((n + 1 + 16,), IGUARD, dtype=torch.int64, device=dev)
    device.hdlc_frame(flat, torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev), out[:cap], foff[:n + 1])
    torch.cuda.synchronize(dev)
    o, fo = out.cpu().numpy(), foff.cpu().numpy()
    assert np.array_equal(fo[:n + 1], want_off) and (fo[n + 1:] == IGUARD).all()
    for i, w in enumerate(want):
        assert o[fo[i]:fo[i + 1]].tobytes() == w, (i, len(pk[i]), pk[i][:4].hex())
    total = int(fo[n])
    assert total < cap and (o[total:] == GUARD).all()
    # and back: the stream's frames are the packets (an empty packet is an empty frame)
    stream = o[:total].tobytes()
    ref = _both(stream, hw_mtu=1000, what="framed packets")
    assert ref.frames[0::2] == pk and all(f == b"" for f in ref.frames[1::2])
