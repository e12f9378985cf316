"""The send side of a read on the device (reply_kernels.hip, rt_hdlc_frame_counted,
pipeline.reply) against the plain model of tests/reply_helpers.py, byte for
byte.  Every output has guard rows or bytes behind it, checked untouched."""
import numpy as np
import pytest

import reply_helpers as rh
from oracle import wire as ow

pytestmark = pytest.mark.gpu

LENGTHS = (1, 15, 16, 17, 83, 115, 118, 127, 128)
GUARD = 0xA5


class Source:
    """One source on the device: n rows of ``width`` bytes at ``stride``, the
    first ``base`` bytes into a buffer that ends with the last row."""

    def __init__(self, rng, n, lens, width=128, stride=128, base=0):
        import torch
        self.lens = np.asarray(lens, np.int32)
        size = base + (max(n - 1, 0) * stride + width if n else 0)
        self.host = rng.integers(0, 256, max(size, 1), dtype=np.uint8)
        self.rows = [bytes(self.host[base + k * stride: base + k * stride + width]) for k in range(n)]
        self.buf = torch.from_numpy(self.host).cuda()
        self.t_rows = self.buf.as_strided((n, width), (stride, 1), base)
        self.t_lens = torch.from_numpy(self.lens).cuda()

    def pair(self):
        return self.t_rows, self.t_lens

    def model(self):
        return self.rows, self.lens


class Outputs:
    """reply_gather's outputs with two guard rows / four guard entries behind each."""

    def __init__(self, cap):
        import torch
        self.cap = cap
        self.out = torch.full((cap + 2, 128), GUARD, dtype=torch.uint8, device="cuda")
        self.len = torch.full((cap + 4,), 77, dtype=torch.int32, device="cuda")
        self.frame = torch.full((cap + 4,), 77, dtype=torch.int32, device="cuda")
        self.source = torch.full((cap + 4,), 77, dtype=torch.uint8, device="cuda")
        self.counts = torch.full((4,), 77, dtype=torch.int64, device="cuda")

    def args(self):
        c = self.cap
        return self.out[:c], self.len[:c], self.frame[:c], self.source[:c], self.counts[:2]

    def check(self, sources):
        cap = self.cap
        replies, found = rh.gather_model([s.model() for s in sources], cap)
        written = len(replies)
        assert written == min(found, cap)
        assert self.counts.cpu().tolist() == [written, found, 77, 77]
        out, ln = self.out.cpu().numpy(), self.len.cpu().numpy()
        frame, source = self.frame.cpu().numpy(), self.source.cpu().numpy()
        assert ln[:written].tolist() == [len(r) for _, _, r in replies]
        assert frame[:written].tolist() == [k for k, _, _ in replies]
        assert source[:written].tolist() == [s for _, s, _ in replies]
        want = np.zeros((written, 128), np.uint8)                     # a written row is a whole line: zeros past the reply
        for j, (_, _, r) in enumerate(replies):
            want[j, :len(r)] = np.frombuffer(r, np.uint8)
        assert np.array_equal(out[:written], want)
        # past the replies: the sentinels, rows not written; behind the outputs: the guards
        assert (ln[written:cap] == rh.NONE_LEN).all() and (frame[written:cap] == rh.NONE_FRAME).all()
        assert (source[written:cap] == rh.NONE_SOURCE).all()
        assert (out[written:] == GUARD).all()
        assert (ln[cap:] == 77).all() and (frame[cap:] == 77).all() and (source[cap:] == 77).all()
        return replies, found


def _pattern(name, n):
    k = np.arange(n)
    return {"none": k < 0, "all": k >= 0, "first": k == 0, "last": k == n - 1, "every other": k % 2 == 0,
            "block ends": k % 1024 == 1023}[name]


def _lens(rng, mask):
    return np.where(mask, rng.choice(LENGTHS, len(mask)), 0).astype(np.int32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_gather_patterns_at_the_wave_workgroup_and_scan_block_edges(n):
    from reticulum_amd import device
    rng = np.random.Generator(np.random.PCG64(n))
    for name in ("none", "all", "first", "last", "every other", "block ends"):
        src = Source(rng, n, _lens(rng, _pattern(name, n)))
        o = Outputs(n)
        device.reply_gather([src.pair()], *o.args())
        _, found = o.check([src])
        assert found == int(_pattern(name, n).sum()), name


def _mixed_sources(rng, n, S):
    """S sources at different strides, widths and misaligned bases; the lengths
    cover LENGTHS, 0 and the out-of-range -1 and 129, with frames where two and
    three sources (all of them, for S < 3) are non-zero."""
    shapes = [dict(width=128, stride=128, base=0), dict(width=128, stride=160, base=1),
              dict(width=118, stride=131, base=15), dict(width=128, stride=200, base=7)][:S]
    sources = []
    for s, shape in enumerate(shapes):
        pick = list(LENGTHS) + [0, 0, 0, -1, 129]
        lens = rng.choice(pick, n).astype(np.int32)
        lens[3 % max(n, 1)::11] = 83                      # every source non-zero on these frames
        if s < 2:
            lens[5 % max(n, 1)::13] = 115                 # two sources on these
        sources.append(Source(rng, n, lens, **shape))
    return sources


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_gather_sources_strides_and_lengths(S):
    from reticulum_amd import device
    rng = np.random.Generator(np.random.PCG64(100 + S))
    n = 257
    sources = _mixed_sources(rng, n, S)
    _, found = rh.gather_model([s.model() for s in sources])
    o = Outputs(found + 1)
    device.reply_gather([s.pair() for s in sources], *o.args())
    replies, _ = o.check(sources)
    frames = [k for k, _, _ in replies]
    if S > 1:
        assert max(frames.count(k) for k in set(frames)) == S             # every source of a frame is a reply
    # source 2's rows hold 118 bytes: its 127 and 128 are nothing
    assert all(len(r) <= 118 for _, s, r in replies if s == 2)
    assert {len(r) for _, _, r in replies} >= set(LENGTHS)


def test_gather_capacities():
    from reticulum_amd import device
    rng = np.random.Generator(np.random.PCG64(7))
    n = 1025
    sources = _mixed_sources(rng, n, 2)
    _, found = rh.gather_model([s.model() for s in sources])
    assert found > n                                                      # more replies than frames
    for cap in (0, found - 1, found, found + 1, n):
        o = Outputs(cap)
        device.reply_gather([s.pair() for s in sources], *o.args())
        o.check(sources)


def test_gather_no_frames():
    import torch
    from reticulum_amd import device
    rng = np.random.Generator(np.random.PCG64(8))
    for cap in (0, 3, 1025):
        src = Source(rng, 0, [])
        o = Outputs(cap)
        device.reply_gather([src.pair(), src.pair()], *o.args())
        o.check([src, src])
    torch.cuda.synchronize()


def test_two_calls_on_one_stream_share_a_workspace():
    import torch
    from reticulum_amd import _native, device
    rng = np.random.Generator(np.random.PCG64(9))
    n = 2049
    a = [Source(rng, n, _lens(rng, _pattern("every other", n)))]
    b = _mixed_sources(rng, 300, 3)
    ws = torch.empty(int(_native.load().rt_reply_gather_workspace_bytes(n, 3)), dtype=torch.uint8, device="cuda")
    oa, ob = Outputs(n), Outputs(400)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    device.reply_gather([s.pair() for s in a], *oa.args(), workspace=ws, stream=stream)
    device.reply_gather([s.pair() for s in b], *ob.args(), workspace=ws, stream=stream)
    stream.synchronize()
    oa.check(a)
    ob.check(b)


# ------------------------------------------------------------ counted framing --

def _framing_input(rng, n, garbage_from):
    """n packets thick with 7E and 7D; from ``garbage_from`` on the lengths and
    offsets are live garbage."""
    import torch
    lens = rng.integers(1, 300, n).astype(np.int32)
    pkts = [bytes(rng.choice([0x7E, 0x7D, 0x5E, 0x5D, 0x00, 0x41], L, p=[.3, .3, .1, .1, .1, .1]).astype(np.uint8))
            for L in lens]
    off = np.zeros(n, np.int64)
    off[1:] = np.cumsum(lens[:-1])
    g_len, g_off = lens.copy(), off.copy()
    g_len[garbage_from:] = rng.integers(1, 1 << 20, n - garbage_from)
    g_off[garbage_from:] = rng.integers(1 << 30, 1 << 40, n - garbage_from)
    buf = np.frombuffer(b"".join(pkts), np.uint8).copy()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return pkts, t(buf), t(g_off), t(g_len), t(off), t(lens)


@pytest.mark.parametrize("n", [1, 37, 1025])
def test_counted_framing(n):
    import torch
    from reticulum_amd import device
    rng = np.random.Generator(np.random.PCG64(n))
    for count in sorted({0, 1, n - 1, n, n + 5}):
        live = min(count, n)
        pkts, buf, g_off, g_len, off, lens = _framing_input(rng, n, live)
        want = b"".join(ow.hdlc_frame(p) for p in pkts[:live])
        room = sum(2 * len(p) + 2 for p in pkts) + 64
        out = torch.full((room,), GUARD, dtype=torch.uint8, device="cuda")
        foff = torch.full((n + 3,), 77, dtype=torch.int64, device="cuda")
        n_dev = torch.tensor([count, 12345], dtype=torch.int64, device="cuda")
        device.hdlc_frame_counted(buf, g_off, g_len, n_dev, out, foff[:n + 1])
        got, fo = out.cpu().numpy(), foff.cpu().numpy()
        ends = np.cumsum([0] + [len(ow.hdlc_frame(p)) for p in pkts[:live]])
        assert fo[:live + 1].tolist() == ends.tolist()
        assert (fo[live:n + 1] == len(want)).all() and (fo[n + 1:] == 77).all()
        assert bytes(got[:len(want)]) == want and (got[len(want):] == GUARD).all()
        if live == n:
            # the whole batch: what hdlc_frame gives on the same input
            out2 = torch.full((room,), GUARD, dtype=torch.uint8, device="cuda")
            foff2 = torch.full((n + 1,), 77, dtype=torch.int64, device="cuda")
            device.hdlc_frame(buf, off, lens, out2, foff2)
            assert torch.equal(out, out2) and torch.equal(foff[:n + 1], foff2)


def test_counted_framing_no_packets():
    import torch
    from reticulum_amd import device
    e8 = torch.empty(0, dtype=torch.uint8, device="cuda")
    foff = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    device.hdlc_frame_counted(e8, torch.empty(0, dtype=torch.int64, device="cuda"),
                              torch.empty(0, dtype=torch.int32, device="cuda"),
                              torch.tensor([3], dtype=torch.int64, device="cuda"), e8, foff[:1])
    assert foff.cpu().tolist() == [0, 77]


# -------------------------------------------------------------- pipeline.reply --

def _hand_built(rng, n=70):
    """An inbound result by hand: the three stages' rows with lengths 118, 115
    and 83 / 115 on scattered frames, one frame with two sources."""
    import torch
    res, sources = {}, []
    for (rows, ln), lengths, step in zip((("lr_proofs", "lr_proof_len"), ("proofs", "proof_len"),
                                          ("dest_proofs", "dest_proof_len")), ((118,), (115,), (83, 115)), (7, 3, 5)):
        lens = np.zeros(n, np.int32)
        lens[step::step * 2] = rng.choice(lengths, len(lens[step::step * 2]))
        src = Source(rng, n, lens)
        sources.append(src)
        res[rows], res[ln] = src.pair()
    return res, sources


@pytest.mark.parametrize("ifac_size", [0, 1, 16, 64])
def test_pipeline_reply_on_hand_built_results(ifac_size):
    import torch
    from reticulum_amd import pipeline
    rng = np.random.Generator(np.random.PCG64(50 + ifac_size))
    res, sources = _hand_built(rng)
    key = rng.integers(0, 256, 64, dtype=np.uint8)
    out = pipeline.reply(res, ifac_key=torch.from_numpy(key).cuda(), ifac_size=ifac_size)
    replies, found = rh.gather_model([s.model() for s in sources])
    frames = rh.reply_stream_model(replies, key.tobytes(), ifac_size)
    n = len(sources[0].lens)
    assert out["reply_counts"].cpu().tolist() == [found, found] and 10 < found < n
    foff = out["frame_off"].cpu().numpy()
    assert foff.shape == (n + 1,) and foff[:found + 1].tolist() == np.cumsum([0] + [len(f) for f in frames]).tolist()
    assert (foff[found:] == foff[n]).all()
    assert bytes(out["stream"][:int(foff[n])].cpu().numpy()) == b"".join(frames)
    assert out["reply_frame"][:found].cpu().tolist() == [k for k, _, _ in replies]
    assert out["reply_source"][:found].cpu().tolist() == [s for _, s, _ in replies]
    assert out["reply_len"].cpu().tolist() == [len(r) for _, _, r in replies] + [0] * (n - found)
    packets = out["packets"].cpu().numpy()
    assert all(bytes(packets[j, :len(r)]) == r for j, (_, _, r) in enumerate(replies))


def test_pipeline_reply_takes_the_sources_that_are_present():
    from reticulum_amd import device, pipeline
    rng = np.random.Generator(np.random.PCG64(60))
    res, sources = _hand_built(rng)
    only = {k: v for k, v in res.items() if k.startswith("dest_proof")}
    out = pipeline.reply(only, max_replies=5)
    replies, found = rh.gather_model([sources[2].model()], 5)
    assert out["reply_counts"].cpu().tolist() == [5, found] and found == 7
    w = len(replies)
    assert set(out["reply_source"][:w].cpu().tolist()) == {device.REPLY_DEST_PROOF}       # the stage's index, not 0
    assert out["reply_frame"][:w].cpu().tolist() == [k for k, _, _ in replies]
    total = int(out["frame_off"][-1])
    assert bytes(out["stream"][:total].cpu().numpy()) == b"".join(rh.reply_stream_model(replies))


def test_pipeline_reply_remembers_what_it_sent():
    import torch
    from reticulum_amd import pipeline
    from reticulum_amd.filter import PacketHashlist
    rng = np.random.Generator(np.random.PCG64(61))
    res, sources = _hand_built(rng)
    replies, found = rh.gather_model([s.model() for s in sources])
    seen = PacketHashlist(256, device="cuda")
    before = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    seen.add(before)
    out = pipeline.reply(res, max_replies=found - 2, seen=seen)
    assert out["reply_counts"].cpu().tolist() == [found - 2, found]
    hashes = np.frombuffer(b"".join(rh.packet_hash(r) for _, _, r in replies), np.uint8).reshape(found, 32)
    assert seen.contains(hashes).cpu().tolist() == [1] * (found - 2) + [0, 0]             # the written replies only
    assert seen.contains(before).cpu().tolist() == [1, 1, 1]
    assert seen.counts() == (3 + found - 2, 0, 0)                                          # and nothing else new
    torch.cuda.synchronize()


@pytest.mark.parametrize("ifac_size", [0, 16])
def test_reply_batch_from_host_bytes(ifac_size):
    from reticulum_amd import wire
    rng = np.random.Generator(np.random.PCG64(70 + ifac_size))
    n = 9
    row = lambda L: rng.integers(0, 256, L, dtype=np.uint8).tobytes()
    by_source = [[row(118) if k == 4 else None for k in range(n)],
                 [row(115) if k % 3 == 1 else b"" for k in range(n)],
                 [row(83) if k in (1, 8) else None for k in range(n)]]
    key = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    stream, frame, source = wire.reply_batch(by_source, ifac_key=key, ifac_size=ifac_size)
    sources = [([r or b"" for r in src], [len(r or b"") for r in src]) for src in by_source]
    replies, found = rh.gather_model([([r.ljust(128, b"\0") for r in rows], lens) for rows, lens in sources])
    assert found == 6 and frame.tolist() == [k for k, _, _ in replies] == [1, 1, 4, 4, 7, 8]
    assert source.tolist() == [s for _, s, _ in replies] == [1, 2, 0, 1, 1, 2]
    assert stream == b"".join(rh.reply_stream_model(replies, key, ifac_size))
