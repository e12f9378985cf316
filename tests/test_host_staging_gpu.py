"""The host-pointer entry points' staging, pinned before csrc/capi_*.hip was
split out of one file: each rt_*_host call (and rt_keyset_create) takes a
staging lane, lays its arrays out in the lane's workspace, copies them in
(through the lane's pinned mirror up to 8 MiB, from the caller's pageable
arrays above that), launches, and copies the outputs back.

Bit-exact against the C oracle (hashlib for the Resource hashes): shuffled,
gapped batches whose gap and guard bytes must keep their sentinel, batches
above the pinned cap, one thread walking every lane through growing and
shrinking sizes with fresh key sets in between, argument errors followed by a
valid call on every lane, and the calls that never use the pinned mirror with
odd strides and guarded outputs.
"""
import ctypes
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import ctoken as oracle
from test_fuzz_gpu import _place
from tests_helpers import collision_stream, trial_case

pytestmark = pytest.mark.gpu

SENT = 0x5A
NONE32 = 0xFFFFFFFF
MIXED = [0, 15, 16, 17, 500]
N_LANES = 8


@pytest.fixture(scope="module")
def rt():
    import reticulum_amd
    from reticulum_amd import _native
    lib = _native.load()
    assert lib.rt_device_count() >= 1, "no HIP device visible"
    _native.context(0)
    return reticulum_amd


@pytest.fixture(scope="module")
def keys():
    rng = np.random.Generator(np.random.PCG64(5100))
    k = {64: rng.integers(0, 256, (5, 64), dtype=np.uint8), 32: rng.integers(0, 256, (5, 32), dtype=np.uint8)}
    for a in k.values():
        a.setflags(write=False)
    return k


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _check(rc):
    from reticulum_amd import _native
    _native.check(rc)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _packed(lens):
    off = np.zeros(len(lens), np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    return off, int(lens.sum())


def _mixed(rng, n):
    """n lengths: the edge lengths first, then draws from them and from 1..700."""
    lens = (MIXED * (n // len(MIXED) + 1))[:n]
    for i in range(len(MIXED), n, 2):
        lens[i] = int(rng.integers(1, 700))
    return np.asarray(lens, np.int64)


def enc_case(seed, keys, lens, per_packet, packed=False):
    """Plaintexts and token slots placed shuffled with gaps (or packed), and
    the oracle's tokens written into a sentinel-filled token buffer."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    tl = 16 + 16 * (lens // 16 + 1) + 32
    po, psize = _packed(lens) if packed else _place(rng, lens)
    to, tsize = _packed(tl) if packed else _place(rng, tl)
    c = SimpleNamespace(n=n, keys=keys, pt=rng.integers(0, 256, max(psize, 1), dtype=np.uint8), po=_u64(po),
                        pl=lens.astype(np.uint32), iv=rng.integers(0, 256, (n, 16), dtype=np.uint8), to=_u64(to),
                        tl=tl.astype(np.uint32), tsize=max(tsize, 1),
                        ki=rng.integers(0, len(keys), n).astype(np.uint32) if per_packet else None)
    c.ref = np.full(c.tsize, SENT, np.uint8)
    oracle.encrypt_batch(keys, c.pt, c.po, c.pl, c.ki, c.iv, c.ref, c.to, threads=8)
    c.ref.setflags(write=False)
    return c


def run_encrypt(ks, c):
    tok = np.full(c.tsize, SENT, np.uint8)
    _check(ks._lib.rt_encrypt_host(ks.handle, _p(c.pt), _p(c.po), _p(c.pl), _p(c.ki), _p(c.iv), _p(tok), _p(c.to),
                                   c.n))
    return tok


def dec_case(seed, e, packed=False):
    """The tokens of an encrypt case where the oracle left them, the second one
    with a flipped tag byte and the third cut to 20 bytes; the oracle's
    statuses, lengths and plaintexts, failed regions zeroed as the library
    zeroes them, in a sentinel-filled output buffer."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = SimpleNamespace(n=e.n, keys=e.keys, tok=e.ref.copy(), to=e.to, tl=e.tl.copy(), ki=e.ki)
    if e.n >= 2:
        d.tok[int(e.to[1]) + int(e.tl[1]) - 1] ^= 0x40
    if e.n >= 3:
        d.tl[2] = 20
    cap = np.maximum(d.tl.astype(np.int64) - 48, 0)
    oo, osize = _packed(cap) if packed else _place(rng, cap)
    d.oo, d.osize = _u64(oo), max(osize, 1)
    d.want = np.full(d.osize, SENT, np.uint8)
    d.want_len, d.want_st = np.zeros(e.n, np.uint32), np.zeros(e.n, np.int32)
    oracle.decrypt_batch(d.keys, d.tok, d.to, d.tl, d.ki, d.want, d.oo, d.want_len, d.want_st, threads=8)
    for i in np.nonzero(d.want_st)[0]:
        d.want[int(oo[i]):int(oo[i]) + int(cap[i])] = 0
    for a in (d.tok, d.want, d.want_len, d.want_st):
        a.setflags(write=False)
    return d


def run_decrypt(ks, d):
    """(plaintext buffer, lengths, statuses); the two arrays sit between guard
    words that must survive."""
    out = np.full(d.osize, SENT, np.uint8)
    ol, st = np.full(d.n + 2, NONE32, np.uint32), np.full(d.n + 2, -7, np.int32)
    _check(ks._lib.rt_decrypt_host(ks.handle, _p(d.tok), _p(d.to), _p(d.tl), _p(d.ki), _p(out), _p(d.oo),
                                   _p(ol[1:]), _p(st[1:]), d.n))
    assert ol[0] == ol[-1] == NONE32 and st[0] == st[-1] == -7
    return out, ol[1:-1], st[1:-1]


def run_verify(ks, d):
    st = np.full(d.n + 2, -7, np.int32)
    _check(ks._lib.rt_verify_host(ks.handle, _p(d.tok), _p(d.to), _p(d.tl), _p(d.ki), _p(st[1:]), d.n))
    assert st[0] == st[-1] == -7
    return st[1:-1]


def check_all(ks, e, d, what):
    """Encrypt, decrypt and verify of one case against the oracle: every byte
    of the output buffers, so the gaps and guards too."""
    assert np.array_equal(run_encrypt(ks, e), e.ref), what
    out, ol, st = run_decrypt(ks, d)
    assert np.array_equal(st, d.want_st) and np.array_equal(ol, d.want_len), what
    assert np.array_equal(out, d.want), what
    # only good, tag-flipped and <= 32-byte tokens here: verify's status is decrypt's
    assert set(d.want_st.tolist()) <= {0, 1, 2}
    assert np.array_equal(run_verify(ks, d), d.want_st), what


@pytest.fixture(scope="module")
def big(keys):
    """Above the pinned cap: 600 packets of 16 KiB (a few edge lengths among
    them), 9.8 MB of plaintext and as much of tokens, gapped."""
    lens = np.full(600, 16384, np.int64)
    lens[[3, 77, 300, 599]] = [0, 17, 500, 15]
    e = enc_case(5300, keys[64], lens, per_packet=True)
    d = dec_case(5301, e)
    assert int(e.tl.sum()) > (8 << 20)
    return e, d


@pytest.mark.parametrize("klen", [64, 32])
@pytest.mark.parametrize("per_packet", [False, True])
@pytest.mark.parametrize("n", [2, 65])
def test_gapped_batches_pinned_path(rt, keys, n, per_packet, klen):
    seed = 5200 + 8 * n + 2 * per_packet + (klen == 32)
    kk = keys[klen] if per_packet else keys[klen][:1]
    e = enc_case(seed, kk, _mixed(np.random.Generator(np.random.PCG64(seed)), n), per_packet)
    d = dec_case(seed + 1000, e)
    ks = rt.KeySet(kk)
    check_all(ks, e, d, (n, per_packet, klen))


def test_packed_batch_uploads_no_output_region(rt, keys):
    """No gaps between the outputs: the output region is not uploaded, so the
    sentinel the caller left there is simply overwritten."""
    e = enc_case(5250, keys[64], _mixed(np.random.Generator(np.random.PCG64(5250)), 33), True, packed=True)
    d = dec_case(5251, e, packed=True)
    check_all(rt.KeySet(keys[64]), e, d, "packed")


def test_above_the_pinned_cap(rt, keys, big):
    check_all(rt.KeySet(keys[64]), *big, "pageable branch")


def test_lane_reuse_across_sizes(rt, keys, big):
    """One thread, so consecutive calls take consecutive lanes: nine rounds of
    (new key set from host keys, encrypt, decrypt) per size step every call
    through all eight lanes.  1 packet, 100 KiB, above the cap, 1 packet: the
    workspace and the pinned mirror grow, the large call leaves the mirror
    behind, and the one-packet call after it runs on the mirror again."""
    k = keys[64]
    one = enc_case(5400, k[:1], [383], per_packet=False)     # key_idx NULL: key 0
    mid = enc_case(5401, k, np.full(200, 500, np.int64), per_packet=True)
    sizes = [(one, dec_case(5410, one)), (mid, dec_case(5411, mid)), big, (one, dec_case(5412, one))]
    for step, (e, d) in enumerate(sizes):
        for rep in range(N_LANES + 1):
            ks = rt.KeySet(k)            # rt_keyset_create returns with its upload queued on a lane
            assert np.array_equal(run_encrypt(ks, e), e.ref), (step, rep)
            out, ol, st = run_decrypt(ks, d)
            assert np.array_equal(st, d.want_st) and np.array_equal(ol, d.want_len), (step, rep)
            assert np.array_equal(out, d.want), (step, rep)


def test_verify_trials_gapped_with_empty_ranges(rt):
    """rt_verify_trials_host: tokens placed shuffled with gaps, candidate
    ranges of every length including empty ones, `first` between guard words."""
    k, toks, cands, expect = trial_case(11, n_tok=70, n_keys=9)
    rng = np.random.Generator(np.random.PCG64(5500))
    tl = np.asarray([len(t) for t in toks], np.int64)
    to, size = _place(rng, tl)
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    for i, t in enumerate(toks):
        buf[to[i]:to[i] + len(t)] = np.frombuffer(t, np.uint8)
    pair_off = np.zeros(len(toks) + 1, np.uint32)
    np.cumsum([len(c) for c in cands], out=pair_off[1:])
    assert (np.diff(pair_off.astype(np.int64)) == 0).any()
    pair_key = np.asarray([x for c in cands for x in c], np.uint32)
    want = np.asarray([c.index(x) if x >= 0 else NONE32 for c, x in zip(cands, expect.tolist())], np.uint32)
    ks = rt.KeySet(k)
    first = np.full(len(toks) + 2, 0x77777777, np.uint32)
    _check(ks._lib.rt_verify_trials_host(ks.handle, _p(buf), _p(_u64(to)), _p(tl.astype(np.uint32)), _p(pair_off),
                                         _p(pair_key), _p(first[1:]), len(toks), int(pair_off[-1])))
    assert first[0] == first[-1] == 0x77777777
    assert np.array_equal(first[1:-1], want)


def test_hkdf_host_odd_strides(rt):
    """rt_hkdf_host: ikm, salt and output rows at odd strides, a context; the
    bytes between output rows are not written."""
    from reticulum_amd import _native
    rng = np.random.Generator(np.random.PCG64(5600))
    n, ikm_len, salt_len, length = 67, 32, 16, 64
    ikm = rng.integers(0, 256, (n, 37), dtype=np.uint8)
    salt = rng.integers(0, 256, (n, 19), dtype=np.uint8)
    ctxb = rng.integers(0, 256, 5, dtype=np.uint8)
    out = np.full((n, 67), SENT, np.uint8)
    _check(_native.load().rt_hkdf_host(_native.context(0), _p(ikm), 37, ikm_len, _p(salt), 19, salt_len, _p(ctxb), 5,
                                       _p(out), 67, length, n))
    for i in range(n):
        assert out[i, :length].tobytes() == oracle.hkdf(length, ikm[i, :ikm_len].tobytes(),
                                                        salt[i, :salt_len].tobytes(), ctxb.tobytes()), i
    assert (out[:, length:] == SENT).all()


# rt_x25519_host with odd strides and guard bytes between its output rows is
# pinned by tests/test_x25519_gpu.py::test_odd_strides_leave_guard_bytes, and
# its point_off gather by ::test_point_off_at_all_byte_phases.


@pytest.mark.parametrize("dup", [None, (1, 4)])
def test_resource_hashmap_host_guarded(rt, dup):
    """rt_resource_hashmap_host: a last part of 17 bytes, the hashmap between
    guard bytes, first_collision between guard words, with and without a
    repeated part inside the window."""
    from reticulum_amd import _native
    sdu = 464
    stream = collision_stream(5700, 7 * sdu + 17, dup, sdu)
    rh = b"\x01\x02\x03\x04"
    want = oracle.map_hashes(stream, rh, sdu)
    col = oracle.first_collision(want, 224)
    assert (col is None) == (dup is None)
    data, salt = np.frombuffer(stream, np.uint8), np.frombuffer(rh, np.uint8)
    hm = np.full(len(want) + 6, SENT, np.uint8)
    fc = np.full(3, 0x77777777, np.uint32)
    _check(_native.load().rt_resource_hashmap_host(_native.context(0), _p(data), len(stream), sdu, _p(salt), 4, 224,
                                                   _p(hm[3:]), _p(fc[1:])))
    assert hm[3:-3].tobytes() == want and (hm[:3] == SENT).all() and (hm[-3:] == SENT).all()
    assert fc.tolist() == [0x77777777, NONE32 if col is None else col, 0x77777777]


@pytest.mark.parametrize("size", [0, 1001])
def test_resource_hashes_host_guarded(rt, size):
    """rt_resource_hashes_host: an odd size (and none), hash, proof and status
    between guard bytes; the advertised hash right and then wrong (32 zero
    bytes for a proof then: the reference never proves a corrupt resource)."""
    from reticulum_amd import _native
    rng = np.random.Generator(np.random.PCG64(5800 + size))
    data = rng.integers(0, 256, max(size, 1), dtype=np.uint8)
    rh = rng.integers(0, 256, 4, dtype=np.uint8)
    h = hashlib.sha256(data[:size].tobytes() + rh.tobytes()).digest()
    proof = hashlib.sha256(data[:size].tobytes() + h).digest()
    lib, ctx = _native.load(), _native.context(0)
    for expect, status in ((h, 0), (h[:31] + bytes([h[31] ^ 1]), 1)):
        ex = np.frombuffer(expect, np.uint8)
        out = np.full(32 + 3 + 32 + 3, SENT, np.uint8)        # hash at 1, proof at 36
        st = np.full(3, -7, np.int32)
        _check(lib.rt_resource_hashes_host(ctx, _p(data) if size else None, size, _p(rh), 4, _p(ex), _p(out[1:]),
                                           _p(out[36:]), _p(st[1:])))
        assert out[1:33].tobytes() == h and out[36:68].tobytes() == (bytes(32) if status else proof)
        assert (out[[0, 33, 34, 35, 68, 69]] == SENT).all()
        assert st.tolist() == [-7, status, -7]


def test_errors_leave_the_lanes_usable(rt, keys):
    """The last argument check of each of the nine entry points: RT_E_INVAL
    (a null handle from rt_keyset_create) with its message, and the valid calls
    that follow on the same context are bit-exact.  Nine rounds of (error,
    valid, valid), so whether or not the failing call took a lane, a valid call
    follows on every lane."""
    from reticulum_amd import _native
    lib, ctx = _native.load(), _native.context(0)
    k = keys[64]
    ks = rt.KeySet(k)
    e = enc_case(5900, k, [0, 17, 383], per_packet=True)
    d = dec_case(5901, e)
    buf = np.zeros(128, np.uint8)
    one64, one32, two32 = np.zeros(1, np.uint64), np.full(1, 64, np.uint32), np.zeros(2, np.uint32)
    st = np.zeros(1, np.int32)
    H = ks.handle
    errors = [
        (lambda: lib.rt_encrypt_host(H, None, _p(one64), _p(one32), None, _p(buf), _p(buf), _p(one64), 1),
         "rt_encrypt_host: null plaintext"),
        (lambda: lib.rt_decrypt_host(H, None, _p(one64), _p(one32), None, _p(buf), _p(one64), _p(two32), _p(st), 1),
         "rt_decrypt_host: null buffer"),
        (lambda: lib.rt_verify_host(H, None, _p(one64), _p(one32), None, _p(st), 1), "rt_verify_host: null tokens"),
        (lambda: lib.rt_verify_trials_host(H, None, _p(one64), _p(one32), _p(two32), None, _p(two32), 1, 0),
         "rt_verify_trials_host: null tokens"),
        (lambda: lib.rt_hkdf_host(ctx, _p(buf), 32, 32, None, 0, 0, None, 0, None, 64, 64, 1), "rt_hkdf: null output"),
        (lambda: lib.rt_x25519_host(ctx, _p(buf), 32, _p(buf), 32, None, _p(buf), 16, 2),
         "rt_x25519: out_stride smaller than 32"),
        (lambda: lib.rt_resource_hashmap_host(ctx, _p(buf), 100, 64, None, 4, 0, _p(buf), None),
         "rt_resource_hashmap_host: null buffer"),
        (lambda: lib.rt_resource_hashes_host(ctx, _p(buf), 100, None, 0, _p(buf), _p(buf), None, None),
         "rt_resource_hashes_host: expect_hash needs status"),
    ]
    for call, msg in errors:
        for rep in range(N_LANES + 1):
            assert call() == _native.RT_E_INVAL and _native.last_error() == msg, (msg, rep)
            for _ in range(2):
                assert np.array_equal(run_encrypt(ks, e), e.ref), (msg, rep)
                out, ol, got = run_decrypt(ks, d)
                assert np.array_equal(got, d.want_st) and np.array_equal(out, d.want), (msg, rep)
    for rep in range(N_LANES + 1):
        assert not lib.rt_keyset_create(ctx, _p(buf), 48, 1)
        assert _native.last_error() == "Token key must be 128 or 256 bits, not 384"
        for _ in range(2):
            fresh = rt.KeySet(k)
            assert np.array_equal(run_encrypt(fresh, e), e.ref), rep
