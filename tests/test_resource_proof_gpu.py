"""Resource integrity hash and proof on the GPU (k_resource_hashes and
k_resource_hashes_split through the C-ABI), bit-exact against hashlib and the
reference-made fixtures (tests/golden/gen_resource_proof.py).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import reticulum_amd as rt
from tests_helpers import b, collision_stream

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_EFFICIENT_SIZE = 1 * 1024 * 1024 - 1          # Resource.MAX_EFFICIENT_SIZE
# k_resource_hashes_split's LDS ring holds 2 x 64 expanded blocks of 64 B
RING_BYTES = 2 * 64 * 64


def sha(x):
    return hashlib.sha256(x).digest()


@pytest.fixture(scope="module")
def pv():
    with open(os.path.join(HERE, "golden", "resource_proof_vectors.json")) as f:
        return json.load(f)


def fixtures(pv):
    m = pv["metadata"]
    return pv["resources"] + [dict(m, data=m["hashed"], size="metadata")]


def run_device(segs, rhs, expect=None, proof=True):
    """One rt_resource_hashes launch over `segs`, segment i placed at phase
    i mod 16 of a 16-byte grid in one flat buffer.  Returns (hash, proof,
    status) as lists of bytes / a numpy array."""
    import torch
    from reticulum_amd import device
    n = len(segs)
    buf, off = bytearray(), []
    for i, s in enumerate(segs):
        base = (len(buf) + 15) // 16 * 16 + i % 16
        buf += bytes(base - len(buf)) + s
        off.append(base)
    buf += bytes(16)
    d = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    rh_len = len(rhs[0])
    rh = torch.frombuffer(bytearray(b"".join(rhs) + b"\0"), dtype=torch.uint8)[:n * rh_len].reshape(n, rh_len).cuda()
    h = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    p = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda") if proof else None
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ex = None if expect is None else torch.frombuffer(bytearray(b"".join(expect)), dtype=torch.uint8).cuda()
    device.resource_hashes(d, torch.tensor(off, dtype=torch.int64).cuda(),
                           torch.tensor([len(s) for s in segs], dtype=torch.int32).cuda(), rh, h, p, ex, st)
    torch.cuda.synchronize()
    hs = [r.tobytes() for r in h.cpu().numpy()]
    ps = [r.tobytes() for r in p.cpu().numpy()] if proof else None
    return hs, ps, st.cpu().numpy()


def check_against_hashlib(segs, rhs, hs, ps):
    for i, (s, r) in enumerate(zip(segs, rhs)):
        e = sha(s + r)
        assert hs[i] == e, (i, len(s))
        assert ps[i] == sha(s + e), (i, len(s))


def test_fixtures_host_calls(pv):
    for r in fixtures(pv):
        data, rh = b(r["data"]), b(r["random_hash"])
        h, th, proof = rt.resource_hashes(data, rh)
        assert (h.hex(), th.hex(), proof.hex()) == (r["hash"], r["truncated_hash"], r["expected_proof"]), r["size"]
        answer = rt.verify_resource(data, rh, b(r["hash"]))
        assert answer == b(r["hash"]) + b(r["expected_proof"]), r["size"]
        assert rt.validate_proof(answer, proof)


def test_fixtures_one_device_launch(pv):
    fx = fixtures(pv)
    segs, rhs = [b(r["data"]) for r in fx], [b(r["random_hash"]) for r in fx]
    hs, ps, st = run_device(segs, rhs)
    assert [h.hex() for h in hs] == [r["hash"] for r in fx]
    assert [p.hex() for p in ps] == [r["expected_proof"] for r in fx]
    assert (st == 0).all()
    hs2, ps2, st2 = run_device(segs, rhs, expect=[b(r["hash"]) for r in fx])
    assert hs2 == hs and ps2 == ps and (st2 == 0).all()


def test_corruption_is_reported_and_never_proved(pv):
    r = pv["resources"][-2]                                # 1000 B
    data, rh, h = b(r["data"]), b(r["random_hash"]), b(r["hash"])
    flipped = bytearray(data)
    flipped[517] ^= 0x04
    assert rt.verify_resource(bytes(flipped), rh, h) is None
    bad_hash = bytearray(h)
    bad_hash[31] ^= 0x01
    assert rt.verify_resource(data, rh, bytes(bad_hash)) is None
    assert rt.verify_resource(data, rh, h[:31]) is None
    assert rt.verify_resource(data, rh, h) is not None
    hs, ps, st = run_device([bytes(flipped), data, data], [rh] * 3, expect=[h, bytes(bad_hash), h])
    assert st.tolist() == [1, 1, 0]
    assert ps[0] == bytes(32) and ps[1] == bytes(32) and ps[2] == b(r["expected_proof"])
    assert hs[0] == sha(bytes(flipped) + rh) and hs[1] == h and hs[2] == h     # the computed hash either way


@pytest.fixture(scope="module")
def ragged():
    """300 segments: lengths from 0...20 000 with every residue mod 64 forced,
    4-byte random hashes; hashlib's digests computed once."""
    rng = np.random.Generator(np.random.PCG64(698))
    lens = rng.integers(0, 20001, 300)
    lens[:64] = lens[:64] // 64 * 64 + np.arange(64)
    lens[64], lens[65] = 0, 20000
    segs = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    rhs = [rng.integers(0, 256, 4, dtype=np.uint8).tobytes() for _ in segs]
    hashes = [sha(s + r) for s, r in zip(segs, rhs)]
    proofs = [sha(s + h) for s, h in zip(segs, hashes)]
    return segs, rhs, hashes, proofs


def test_ragged_launch_sender(ragged):
    segs, rhs, hashes, proofs = ragged
    assert {len(s) % 64 for s in segs} == set(range(64))
    hs, ps, st = run_device(segs, rhs)                     # run_device puts segment i at phase i mod 16
    assert hs == hashes and ps == proofs and (st == 0).all()
    hs, ps, _ = run_device(segs, rhs, proof=False)
    assert hs == hashes and ps is None


def test_ragged_launch_receiver_with_corrupt_subset(ragged):
    segs, rhs, hashes, proofs = ragged
    segs, expect = list(segs), list(hashes)
    corrupt = set(range(3, 300, 7))
    for k, i in enumerate(sorted(corrupt)):
        if k % 2 and len(segs[i]):                         # a flipped data bit ...
            s = bytearray(segs[i])
            s[(k * 131) % len(s)] ^= 1 << (k % 8)
            segs[i] = bytes(s)
        else:                                              # ... or a flipped bit of the advertised hash
            e = bytearray(expect[i])
            e[k % 32] ^= 1 << (k % 8)
            expect[i] = bytes(e)
    hs, ps, st = run_device(segs, rhs, expect=expect)
    for i in range(300):
        assert hs[i] == sha(segs[i] + rhs[i]), i
        assert st[i] == (1 if i in corrupt else 0), i
        assert ps[i] == (bytes(32) if i in corrupt else proofs[i]), i


def test_max_efficient_size_host_call():
    data = np.random.Generator(np.random.PCG64(1048575)).integers(0, 256, MAX_EFFICIENT_SIZE, dtype=np.uint8).tobytes()
    rh = b"\x9a\x01\xfe\x42"
    h, th, proof = rt.resource_hashes(data, rh)
    assert h == sha(data + rh) and th == h[:16] and proof == sha(data + h)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_both_kernels_either_side_of_the_threshold(delta):
    """Segment counts threshold - 1 (one workgroup per segment), threshold and
    threshold + 1 (one lane per segment) give hashlib's digests: lengths 0,
    63, 64, 4096, 4097, one ring wrap plus 1, and every residue mod 64."""
    from reticulum_amd import _native
    n = int(_native.load().rt_resource_hash_split_below()) + delta
    assert n >= 1
    special = [0, 63, 64, 4096, 4097, RING_BYTES + 1]
    lens = [special[i % 6] if i < 66 else (i * 37) % 701 for i in range(n)]
    if n > 254:
        assert {x % 64 for x in lens} == set(range(64))
    rng = np.random.Generator(np.random.PCG64(4096 + delta))
    pool = rng.integers(0, 256, RING_BYTES + 1 + n, dtype=np.uint8).tobytes()
    segs = [pool[i:i + x] for i, x in enumerate(lens)]
    rhs = [pool[-4 - i:len(pool) - i] for i in range(n)]
    hs, ps, st = run_device(segs, rhs)
    check_against_hashlib(segs, rhs, hs, ps)
    assert (st == 0).all()


def test_prepare_resource_reproduces_the_collision_retry(pv, monkeypatch):
    """The reference's retry after a map-hash collision hashes the colliding
    encrypted part; prepare_resource does the same unless told otherwise.
    The collision is forced as the generator forces it: under the first draw
    only, part `colliding_index` repeats an earlier part's map hash."""
    from reticulum_amd import resource
    c = pv["collision_retry"]
    stream = collision_stream(c["seed"], c["stream_len"], None, c["sdu"])
    data, draws = b(c["data"]), [b(d) for d in c["draws"]]
    real = resource.resource_hashmap

    def forced(st, rh, sdu, guard, device):
        hm, col = real(st, rh, sdu, guard, device)
        if rh == draws[0]:
            assert col is None
            return hm[:4 * c["colliding_index"]], c["colliding_index"]
        return hm, col
    monkeypatch.setattr(resource, "resource_hashmap", forced)

    it = iter(draws)
    rh, h, proof, hashmap = rt.prepare_resource(data, stream, sdu=c["sdu"], random_hash=lambda: next(it))
    assert (rh.hex(), h.hex(), proof.hex(), hashmap.hex()) == (c["random_hash"], c["hash"], c["expected_proof"],
                                                               c["hashmap"])
    k = c["colliding_index"]
    part = stream[k * c["sdu"]:(k + 1) * c["sdu"]]
    assert h == sha(part + rh) and proof == sha(part + h)

    it = iter(draws)
    rh, h, proof, hashmap = rt.prepare_resource(data, stream, sdu=c["sdu"], random_hash=lambda: next(it),
                                                rehash_segment=True)
    assert rh == draws[1] and h == sha(data + rh) and proof == sha(data + h) and hashmap.hex() == c["hashmap"]
    assert rt.verify_resource(data, rh, h) == h + proof


@pytest.mark.parametrize("rh_len", [0, 32])
def test_random_hash_lengths(rh_len):
    rng = np.random.Generator(np.random.PCG64(32 + rh_len))
    segs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 23, 24, 31, 32, 55, 56, 63, 64, 119, 120, 1000)]
    if rh_len == 0:
        segs = segs[1:] + [b""]          # keep one empty message: SHA-256(b"")
    rhs = [rng.integers(0, 256, rh_len, dtype=np.uint8).tobytes() for _ in segs]
    hs, ps, _ = run_device(segs, rhs)
    check_against_hashlib(segs, rhs, hs, ps)
    h, _, proof = rt.resource_hashes(segs[4], rhs[4])
    assert h == hs[4] and proof == ps[4]
