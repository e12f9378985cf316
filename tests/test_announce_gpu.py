"""rt_announce_validate (announce_kernels.hip) against the model of
tests/announce_helpers.py, which test_announce.py ties to the reference.

Packets are laid out in one device buffer that ends with the last packet,
unpacked by rt_packet_unpack and validated in place.  Every call writes into
status and identity_hash arrays that have guard rows behind them, and the
guards are checked after every call."""
import functools

import numpy as np
import pytest

import announce_helpers as ah

pytestmark = pytest.mark.gpu

GUARD = 5
SENTINEL = -77
FILL = 0xA5
CANDIDATE = (ah.VALID, ah.BAD_SIGNATURE, ah.BAD_DESTINATION)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _layout(raws, slot=None, lead=1):
    """(flat bytes, offsets, lengths): end to end after ``lead`` bytes (so the
    packets start at every alignment), or each at a multiple of ``slot``."""
    lens = np.array([len(r) for r in raws], np.int32)
    if slot:
        assert slot >= max(lens, default=0)
        offs = np.arange(len(raws), dtype=np.int64) * slot
    else:
        offs = lead + np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]) if len(raws) else \
            np.zeros(0, np.int64)
    flat = np.full(int(offs[-1] + lens[-1]) if len(raws) else 1, 0x5C, np.uint8)
    for r, o in zip(raws, offs):
        flat[o:o + len(r)] = np.frombuffer(r, np.uint8)
    return flat, offs.astype(np.int64), lens


def _validate(raws, slot=None, lead=1, identity=True, stream=None, clear_ok=(), repeat=1):
    """Unpack and validate on the device: (statuses, identity rows or None)."""
    import torch
    from reticulum_amd import device
    n = len(raws)
    flat, offs, lens = _layout(raws, slot, lead)
    pkt, off, ln = _dev(flat), _dev(offs), _dev(lens)
    fields = torch.empty((n, 96), dtype=torch.uint8, device="cuda:0")
    status = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    ident = torch.full((n + GUARD, 16), FILL, dtype=torch.uint8, device="cuda:0") if identity else None
    if n:
        device.packet_unpack(pkt, off, ln, fields)
    for i in clear_ok:
        fields[i, 0] = 0
    torch.cuda.synchronize()
    for _ in range(repeat):
        device.announce_validate(pkt, off, fields, status[:n], ident[:n] if identity else None, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    st = status.cpu().numpy()
    assert (st[n:] == SENTINEL).all(), "guard rows behind status were written"
    rows = None
    if identity:
        rows = ident.cpu().numpy()
        assert (rows[n:] == FILL).all(), "guard rows behind identity_hash were written"
        rows = rows[:n]
    return st[:n].tolist(), rows


def _want(raws, clear_ok=()):
    want = [ah.announce_status_ref(r) for r in raws]
    for i in clear_ok:
        want[i] = (ah.NOT_ANNOUNCE, ah.ZERO)
    return want


def _check(raws, **kw):
    want = _want(raws, kw.get("clear_ok", ()))
    st, rows = _validate(raws, **kw)
    assert st == [w[0] for w in want]
    if rows is not None:
        assert rows.tobytes() == b"".join(w[1] for w in want)
        # rows of records that are no candidates are zero
        assert all(w[1] == ah.ZERO for w in want if w[0] not in CANDIDATE)
    return st


@functools.lru_cache(maxsize=None)
def _pool():
    """A few packets of every outcome, keyed by the status the model gives."""
    rng = np.random.Generator(np.random.PCG64(1772))
    a = ah.Announcer(rng)
    pool = {s: [] for s in (ah.VALID, ah.NOT_ANNOUNCE, ah.SHORT, ah.BAD_SIGNATURE, ah.BAD_DESTINATION)}
    for k in range(4):
        ratchet, header = bool(k & 1), k >> 1
        dest, data = a.data(a.bytes(3 + 40 * k), ratchet)
        pool[ah.VALID].append(ah.raw_packet(dest, data, ratchet, header, hops=k))
        pool[ah.NOT_ANNOUNCE].append(ah.raw_packet(dest, data, ratchet, header, ptype=ah.DATA))
        head = 116 if ratchet else 84
        pool[ah.SHORT].append(ah.raw_packet(dest, data[:head + 63 - 20 * k], ratchet, header))
        bad = bytearray(data)
        bad[(40, 70, 100, len(data) - 1)[k]] ^= 0x10
        pool[ah.BAD_SIGNATURE].append(ah.raw_packet(dest, bytes(bad), ratchet, header))
        other, data = a.data(a.bytes(7 * k), ratchet, signed_destination=a.bytes(16))
        pool[ah.BAD_DESTINATION].append(ah.raw_packet(other, data, ratchet, header))
    for s, raws in pool.items():
        assert [ah.announce_status_ref(r)[0] for r in raws] == [s] * 4
    return pool


def _candidates():
    p = _pool()
    return [p[s][k] for k in range(4) for s in CANDIDATE]


# ----------------------------------------------------------------- fixture --

def test_fixture_one_at_a_time_and_as_one_batch():
    cases = ah.vectors()["cases"]
    raws = [bytes.fromhex(c["raw"]) for c in cases]
    st = _check(raws)
    for c, s in zip(cases, st):
        assert (s in (ah.VALID, ah.BAD_DESTINATION)) == c["ok_signature_only"] and (s == ah.VALID) == c["ok"], c["note"]
    assert set(st) == {0, 1, 2, 3, 4}
    for raw in raws:
        _check([raw], lead=0)


# ------------------------------------------------------------ reader edges --

@functools.lru_cache(maxsize=None)
def _every_length():
    """Valid announces of every app-data length that fits a 500-byte packet,
    both context flags, both header types."""
    rng = np.random.Generator(np.random.PCG64(558))
    a = ah.Announcer(rng)
    raws = []
    for header in (0, 1):
        for ratchet in (False, True):
            room = 500 - (35 if header else 19) - (180 if ratchet else 148)
            for n in range(room + 1):
                dest, data = a.data(a.bytes(n), ratchet)
                raws.append(ah.raw_packet(dest, data, ratchet, header, hops=n & 7, context=n & 0xFF,
                                          transport_id=a.bytes(16)))
            assert len(raws[-1]) == 500
    return raws


@pytest.mark.parametrize("slot", [None, 512])
def test_every_app_data_length_at_every_alignment(slot):
    """1 240 announces in one launch: app data 0..333 (HEADER_1) and 0..317
    (HEADER_2), 32 bytes less with a ratchet, which crosses every word
    alignment of both cuts and the SHA-512 block steps (64 + 16 + head + app at
    a multiple of 128 less 17: app = 75 | 76 and 203 | 204, or 43 | 44 and
    171 | 172 with a ratchet).  Every packet was signed by the model
    (ed25519_ref.sign), whose verify accepts its own signatures, so VALID is
    the model's answer for all of them; the model is also run in full on every
    seventh and on the block steps."""
    raws = _every_length()
    assert len(raws) == 334 + 302 + 318 + 286
    st, rows = _validate(raws, slot=slot)
    assert st == [ah.VALID] * len(raws)
    steps = [i for i, r in enumerate(raws) if (len(r) - (35 if r[0] & 0x40 else 19) - 64 + 16 + 64 + 17) % 128 in (0, 1)]
    assert len(steps) == 20
    for i in sorted(set(range(0, len(raws), 7)) | set(steps)):
        want = ah.announce_status_ref(raws[i])
        assert (st[i], rows[i].tobytes()) == want, i
    if slot is None:
        offs = _layout(raws)[1]
        assert {int(o) % 8 for o in offs} == set(range(8))


# ------------------------------------------------------------------- flips --

def test_flips_of_signed_and_unsigned_bytes():
    rng = np.random.Generator(np.random.PCG64(1749))
    a = ah.Announcer(rng)
    name_hash = a.bytes(10)
    dest, data = a.data(a.bytes(57), ratchet=True, name_hash=name_hash)
    raw = ah.raw_packet(dest, data, True, header=1, hops=3, context=ah.PATH_RESPONSE, transport_id=a.bytes(16))
    d = 35
    signed = {"destination hash, first byte": 18, "destination hash, last byte": 33, "X25519 key": d + 5,
              "Ed25519 key": d + 40, "name hash": d + 66, "random hash": d + 80, "ratchet": d + 100,
              "R": d + 116 + 3, "S": d + 116 + 40, "app data, first byte": d + 180, "app data, last byte": len(raw) - 1}
    unsigned = {"hops": 1, "transport id, first byte": 2, "transport id, last byte": 17, "context": 34}
    assert len(raw) == d + 180 + 57

    def flip(at, bit=0x04):
        b = bytearray(raw)
        b[at] ^= bit
        return bytes(b)
    raws = [raw] + [flip(at) for at in signed.values()] + [flip(at) for at in unsigned.values()]
    # the name hash changed and the packet signed again for it: the signature holds, the destination does not
    other = bytes([name_hash[0] ^ 1]) + name_hash[1:]
    _, redone = a.data(a.bytes(57), ratchet=True, name_hash=other, signed_destination=dest)
    raws.append(ah.raw_packet(dest, redone, True, header=1, hops=3, context=ah.PATH_RESPONSE))
    st, rows = _validate(raws)
    assert st == [w[0] for w in _want(raws)]
    assert st == [ah.VALID] + [ah.BAD_SIGNATURE] * len(signed) + [ah.VALID] * len(unsigned) + [ah.BAD_DESTINATION]
    assert rows[-1].tobytes() == a.identity and rows.tobytes() == b"".join(w[1] for w in _want(raws))


# ------------------------------------------------------------ length edges --

def test_length_edges_and_records_that_are_no_announces():
    rng = np.random.Generator(np.random.PCG64(1750))
    a = ah.Announcer(rng)
    raws, want = [], []
    for header in (0, 1):
        for ratchet in (False, True):
            head = 116 if ratchet else 84
            dest, data = a.data(b"", ratchet)
            assert len(data) == head + 64
            for r, w in ((ah.raw_packet(dest, data[:-1], ratchet, header), ah.SHORT),
                         (ah.raw_packet(dest, data, ratchet, header), ah.VALID),
                         (ah.raw_packet(dest, b"", ratchet, header), ah.SHORT),
                         (ah.raw_packet(dest, data[:64], ratchet, header), ah.SHORT),
                         # the other context flag on the same data: no room for a ratchet, or the cuts 32 bytes early
                         (ah.raw_packet(dest, data, not ratchet, header), ah.BAD_SIGNATURE if ratchet else ah.SHORT),
                         (ah.raw_packet(dest, data, ratchet, header, ptype=ah.DATA), ah.NOT_ANNOUNCE),
                         (ah.raw_packet(dest, data, ratchet, header, ptype=3), ah.NOT_ANNOUNCE),
                         (ah.raw_packet(dest, data, ratchet, header, hops=128), ah.NOT_ANNOUNCE)):
                raws.append(r)
                want.append(w)
    assert _check(raws) == want
    # valid announces whose record says ok = 0 (an earlier stage dropped them)
    valid = [r for r, w in zip(raws, want) if w == ah.VALID]
    assert _check(valid * 3, clear_ok=(0, 5, 11)) == [ah.NOT_ANNOUNCE if i in (0, 5, 11) else ah.VALID
                                                        for i in range(12)]


# -------------------------------------------------------- compaction edges --

def _pattern(name, n):
    return {"none": [], "first": [0], "last": [n - 1], "every": list(range(n)), "every 64th": list(range(0, n, 64)),
            "every second": list(range(0, n, 2))}[name]


def _mixed(n, where):
    """n records, candidates (of every verdict, in turn) at ``where``, the
    rest DATA packets, unpack failures and short announces."""
    p, cands = _pool(), _candidates()
    rest = p[ah.NOT_ANNOUNCE] + p[ah.SHORT][:2] + [p[ah.VALID][0][:1]]
    where = set(where)
    return [cands[i % len(cands)] if i in where else rest[i % len(rest)] for i in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 4097])
@pytest.mark.parametrize("pattern", ["none", "first", "last", "every", "every 64th", "every second"])
def test_compaction_edges(n, pattern):
    where = _pattern(pattern, n)
    st = _check(_mixed(n, where))
    assert [i for i, s in enumerate(st) if s in CANDIDATE] == sorted(where)
    if pattern == "none":
        assert set(st) <= {ah.NOT_ANNOUNCE, ah.SHORT}


@pytest.mark.parametrize("k", [256, 257])
def test_one_block_of_candidates_and_one_more(k):
    rng = np.random.Generator(np.random.PCG64(k))
    where = sorted(rng.choice(1000, k, replace=False).tolist())
    st = _check(_mixed(1000, where))
    assert sum(s in CANDIDATE for s in st) == k


def test_no_record_at_all():
    st, rows = _validate([])
    assert st == [] and rows.shape == (0, 16)


# ----------------------------------------------------------- wave outcomes --

@pytest.mark.parametrize("interleaved", [False, True])
def test_whole_waves_of_one_outcome_and_the_same_items_interleaved(interleaved):
    p = _pool()
    order = (ah.VALID, ah.NOT_ANNOUNCE, ah.BAD_SIGNATURE, ah.SHORT, ah.BAD_DESTINATION)
    raws = [p[s][i % 4] for s in order for i in range(64)]
    if interleaved:
        raws = [raws[64 * (i % 5) + i // 5] for i in range(320)]
    st = _check(raws, lead=0)
    assert sorted(st) == sorted(s for s in order for _ in range(64))


# ------------------------------------------------------- outputs and reuse --

def test_without_identity_output_the_statuses_are_the_same():
    raws = _mixed(300, range(0, 300, 3))
    with_rows = _check(raws)
    st, rows = _validate(raws, identity=False)
    assert rows is None and st == with_rows


def test_repeated_calls_count_from_zero():
    """The same call twice on one stream and once more on another: the
    candidate count is per call, not left over."""
    import torch
    raws = _mixed(700, range(0, 700, 2))
    want = [w[0] for w in _want(raws)]
    assert _validate(raws, repeat=2)[0] == want
    side = torch.cuda.Stream(device="cuda:0")
    st, rows = _validate(raws, stream=side, repeat=3)
    assert st == want and rows.tobytes() == b"".join(w[1] for w in _want(raws))
    assert _check(raws) == want
