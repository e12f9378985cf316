"""The fast read-loop reference of the raw-deframe tests (tests/
deframe_helpers.py::ref_pairs: numpy for the flags, bytes.replace for the
frames) against the pure-Python oracle (oracle/wire.py::deframe, pinned by
the reference's own read loop in tests/golden/wire_vectors.json): frames
handed on, invalid lengths and what the loop keeps.  The oracle is quadratic
in the frame count, so this is the only place that runs it on raw streams;
the GPU tests (tests/test_deframe_raw_gpu.py) compare with ref_pairs alone.
"""
import numpy as np

import deframe_helpers as dh
from oracle import wire as ow


def _agree(buf, hw_mtu, ifac_size, what):
    p = dh.ref_pairs(buf, hw_mtu, ifac_size)
    assert dh.as_oracle(p, buf) == ow.deframe(buf, hw_mtu, ifac_size), what
    return p


def test_ref_pairs_on_golden_records():
    records = dh.golden_deframe_records()
    assert len(records) >= 8
    for r in records:
        buf = r["bytes"]
        p = _agree(buf, r["hw_mtu"], r["ifac_size"], r["name"])
        # and the reference's own results, as recorded
        frames, invalid, _ = dh.as_oracle(p, buf)
        assert [f.hex() for f in frames] == r["frames"] and invalid == r["invalid"], r["name"]


def test_ref_pairs_on_random_raw_streams():
    """4000 streams of 0..200 bytes over {7E, 7D, 5E, 5D, 11, 20}, with limits
    small enough that check_frame_len and the 2 * HW_MTU drop both decide."""
    rng = np.random.Generator(np.random.PCG64(391))
    alphabet = np.array([0x7E, 0x7D, 0x5E, 0x5D, 0x11, 0x20], np.uint8)
    seen = set()
    for i in range(4000):
        n = int(rng.integers(0, 201))
        w = rng.dirichlet(np.ones(6))
        buf = alphabet[rng.choice(6, n, p=w)].tobytes()
        hw_mtu, ifac_size = int(rng.choice([10, 30, 60, 500])), [None, 0, 8][int(rng.integers(0, 3))]
        p = _agree(buf, hw_mtu, ifac_size, (i, buf.hex(), hw_mtu, ifac_size))
        seen.update(p.status.tolist())
        seen.add(("held", p.consumed not in (0, n)))
        seen.add(("flags", min(len(p.pos), 2)))
    # every status, every flag count that decides counts[1], both of its outcomes
    assert seen >= {dh.OK, dh.BAD_LEN, dh.EMPTY, ("held", True), ("held", False), ("flags", 0), ("flags", 1),
                    ("flags", 2)}


def test_ref_pairs_on_one_long_raw_stream():
    """About 100 KB of the dense raw stream the GPU tests use (its first 400
    frames), and the pattern frames of the first few hundred short strings."""
    buf = dh.dense_stream()[:100000]
    p = _agree(buf, 500, 8, "dense")
    assert p.npairs > 200 and {dh.OK, dh.BAD_LEN, dh.EMPTY} <= set(p.status.tolist())
    buf = dh.pattern_stream()[0][:100000]
    _agree(buf, 500, 0, "patterns")
    buf = dh.sweep_stream()[0][:60000]
    _agree(buf, 1000, 0, "sweep")


def test_consumed_limits():
    """counts[1] at len - last == 2 * hw_mtu and len == 2 * hw_mtu, by the
    oracle: the loop drops what it holds only past the limit."""
    for buf, want in ((b"\x7e" + dh.fill(30) + b"\x7e" + dh.fill(999), 31),
                      (b"\x7e" + dh.fill(30) + b"\x7e" + dh.fill(1000), 1032),
                      (dh.fill(400) + b"\x7e" + dh.fill(599), 0),
                      (dh.fill(400) + b"\x7e" + dh.fill(600), 1001),
                      (dh.fill(300), 300), (b"\x7e", 0), (b"\x7e" + dh.fill(50), 0), (dh.fill(50) + b"\x7e", 0)):
        assert _agree(buf, 500, 0, len(buf)).consumed == want, len(buf)
