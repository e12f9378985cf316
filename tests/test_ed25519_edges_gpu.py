"""k_ed25519_sign / _public / _verify on the GPU where a batch can go wrong
without a fixture noticing: distinct seeds in neighbouring lanes, batches that
fill a wave, cross one and reach a third workgroup, message lengths on both
sides of every SHA-512 block-count step of both hashes, a given key that is
not the seed's, and whole waves of one outcome.  Every expected value is the
integer reference's (tests/ed25519_ref.py), computed once per module; every
comparison is bit-exact."""
import numpy as np
import pytest

import ed25519_ref as ref
from tests_helpers import b, lib_ctx, pack, ptr, u8

pytestmark = pytest.mark.gpu

# one byte below and at every length where sha512_head_msg's block count steps:
# 47|48, 175|176 (64-byte head R ‖ A ‖ msg; 111|112 is where the bit length no
# longer fits the message's last block), 79|80, 207|208 (32-byte head prefix ‖
# msg), and one block further
LENGTHS = (0, 1, 47, 48, 79, 80, 111, 112, 175, 176, 207, 208, 271, 272)
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
N = 513


def rows(items, width):
    return u8(b"".join(items), len(items), width)


def assert_rows(got, want, what, msgs):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d items differ, first %s (message lengths %s)" % (
        what, bad.size, bad[:8].tolist(), [len(msgs[i]) for i in bad[:8]])


def assert_flags(got, want, what):
    got, want = np.asarray(got, bool), np.asarray(want, bool)
    bad = np.nonzero(got != want)[0]
    assert got.shape == want.shape and bad.size == 0, "%s: items %s differ" % (what, bad[:8].tolist())


@pytest.fixture(scope="module")
def edge():
    """513 distinct seeds, message i of length LENGTHS[i % 14], and the
    reference's public keys and signatures."""
    rng = np.random.Generator(np.random.PCG64(0xED25519))
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(N)]
    assert len(set(seeds)) == N
    msgs = [rng.integers(0, 256, LENGTHS[i % len(LENGTHS)], dtype=np.uint8).tobytes() for i in range(N)]
    offs = pack(msgs)[1]
    for n in SIZES[1:]:
        assert {int(o) % 4 for o in offs[:n]} == {0, 1, 2, 3}
    pubs = [ref.public_key(s) for s in seeds]
    sigs = [ref.sign(s, m, p) for s, m, p in zip(seeds, msgs, pubs)]
    return seeds, msgs, pubs, sigs


# ---- the device forms over torch tensors

def dev_msgs(msgs):
    import torch
    flat, offs, lens = pack(msgs)
    return (torch.from_numpy(flat).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(),
            torch.from_numpy(lens.astype(np.int32)).cuda())


def dev_rows(items, width):
    import torch
    return torch.from_numpy(rows(items, width)).cuda()


def guarded(n, width):
    """n rows to write and one 0xEE row past them."""
    import torch
    return torch.full((n + 1, width), 0xEE, dtype=torch.uint8, device="cuda")


def taken(buf, n):
    out = buf.cpu().numpy()
    assert (out[n:] == 0xEE).all(), "written past item n - 1"
    return out[:n]


def device_public(seeds):
    from reticulum_amd import device
    n = len(seeds)
    out = guarded(n, 32)
    device.ed25519_public(dev_rows(seeds, 32), out[:n])
    return taken(out, n)


def device_sign(seeds, msgs, pubs=None):
    from reticulum_amd import device
    n = len(seeds)
    out = guarded(n, 64)
    device.ed25519_sign(dev_rows(seeds, 32), *dev_msgs(msgs), out[:n],
                        public_keys=None if pubs is None else dev_rows(pubs, 32))
    return taken(out, n)


def device_verify(pks, sigs, msgs):
    import torch
    from reticulum_amd import device
    n = len(msgs)
    ok = torch.full((n + 3,), 0xEE, dtype=torch.uint8, device="cuda")
    device.ed25519_verify(dev_rows(pks, 32), torch.from_numpy(np.ascontiguousarray(sigs)).cuda(), *dev_msgs(msgs), ok[:n])
    out = ok.cpu().numpy()
    assert (out[n:] == 0xEE).all(), "written past item n - 1"
    assert set(out[:n].tolist()) <= {0, 1}
    return out[:n].astype(bool)


# ---- a. sign and public keys at wave and workgroup edges

@pytest.mark.parametrize("n", SIZES)
def test_sign_and_public_keys_at_wave_and_workgroup_edges(edge, n):
    from reticulum_amd import ed25519 as ed
    seeds, msgs, pubs, sigs = (x[:n] for x in edge)
    want_pk, want_sig = rows(pubs, 32), rows(sigs, 64)
    assert_rows(ed.public_keys_batch(seeds), want_pk, "public_keys_batch", msgs)
    assert_rows(ed.sign_batch(seeds, msgs), want_sig, "sign_batch, derived keys", msgs)
    assert_rows(ed.sign_batch(seeds, msgs, public_keys=pubs), want_sig, "sign_batch, given keys", msgs)
    if n in (257, 513):
        assert_rows(device_public(seeds), want_pk, "device.ed25519_public", msgs)
        assert_rows(device_sign(seeds, msgs), want_sig, "device.ed25519_sign, derived keys", msgs)
        assert_rows(device_sign(seeds, msgs, pubs), want_sig, "device.ed25519_sign, given keys", msgs)


# ---- b. every message length from 0 to 272 in one launch

@pytest.fixture(scope="module")
def sweep():
    rng = np.random.Generator(np.random.PCG64(0xED25519 + 1))
    four = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(4)]
    four_pk = [ref.public_key(s) for s in four]
    seeds, pubs = [four[i % 4] for i in range(273)], [four_pk[i % 4] for i in range(273)]
    msgs = [rng.integers(0, 256, i, dtype=np.uint8).tobytes() for i in range(273)]
    sigs = [ref.sign(s, m, p) for s, m, p in zip(seeds, msgs, pubs)]
    flipped = [m[:-1] + bytes([m[-1] ^ 0x01]) if m else m for m in msgs]
    return seeds, pubs, msgs, sigs, flipped


def test_length_sweep_host(sweep):
    from reticulum_amd import ed25519 as ed
    lib, ctx = lib_ctx()
    seeds, pubs, msgs, sigs, flipped = sweep
    n = len(msgs)
    assert [len(m) for m in msgs] == list(range(273))
    want = rows(sigs, 64)
    got = ed.sign_batch(seeds, msgs)
    assert_rows(got, want, "sign_batch", msgs)
    assert_flags(ed.verify_batch(pubs, got, msgs), np.ones(n, bool), "verify_batch")
    rejected = np.zeros(n, bool)
    rejected[0] = True                                   # the empty message has no byte to flip
    assert_flags(ed.verify_batch(pubs, got, flipped), rejected, "verify_batch, last byte flipped")
    # the C-ABI itself: messages that do not start at offset 0
    flat, offs, lens = pack(msgs)
    flat, offs = np.concatenate([u8(b"\xA5" * 3, -1), flat]), offs + np.uint64(3)
    out = np.full((n + 1, 64), 0xEE, np.uint8)
    sd, pk = rows(seeds, 32), rows(pubs, 32)
    assert lib.rt_ed25519_sign_host(ctx, ptr(sd), 32, None, 0, ptr(flat), ptr(offs), ptr(lens), ptr(out), 64, n) == 0
    assert_rows(out[:n], want, "rt_ed25519_sign_host", msgs)
    assert (out[n] == 0xEE).all()
    ok = np.full(n + 1, 0xEE, np.uint8)
    assert lib.rt_ed25519_verify_host(ctx, ptr(pk), 32, ptr(out), 64, ptr(flat), ptr(offs), ptr(lens), ptr(ok), n) == 0
    assert ok.tolist() == [1] * n + [0xEE]


def test_length_sweep_device(sweep):
    seeds, pubs, msgs, sigs, flipped = sweep
    n = len(msgs)
    want = rows(sigs, 64)
    got = device_sign(seeds, msgs)
    assert_rows(got, want, "device.ed25519_sign, derived keys", msgs)
    assert_rows(device_sign(seeds, msgs, pubs), want, "device.ed25519_sign, given keys", msgs)
    assert_flags(device_verify(pubs, got, msgs), np.ones(n, bool), "device.ed25519_verify")
    rejected = np.zeros(n, bool)
    rejected[0] = True
    assert_flags(device_verify(pubs, got, flipped), rejected, "device.ed25519_verify, last byte flipped")


# ---- c. a given public key that is not the seed's

def test_given_key_that_is_not_the_seeds(edge):
    """The kernel hashes the key it is given, as the reference does: the result
    is the reference's bytes and a signature that neither key verifies."""
    from reticulum_amd import ed25519 as ed
    n = 65
    seeds, msgs, pubs, _ = (x[:n + 1] for x in edge)
    other = [pubs[i] if i % 5 == 0 else pubs[i + 1] for i in range(n)]        # every fifth is the seed's own
    seeds, msgs, pubs = seeds[:n], msgs[:n], pubs[:n]
    want = [ref.sign(s, m, o) for s, m, o in zip(seeds, msgs, other)]
    got = ed.sign_batch(seeds, msgs, public_keys=other)
    assert_rows(got, rows(want, 64), "sign_batch, another key given", msgs)
    assert_rows(device_sign(seeds, msgs, other), rows(want, 64), "device.ed25519_sign, another key given", msgs)
    under_own = np.array([ref.verify(p, s, m) for p, s, m in zip(pubs, want, msgs)])
    under_other = np.array([ref.verify(o, s, m) for o, s, m in zip(other, want, msgs)])
    own = np.arange(n) % 5 == 0
    assert np.array_equal(under_own, own) and np.array_equal(under_other, own)
    assert_flags(ed.verify_batch(pubs, got, msgs), under_own, "verify_batch under the seed's key")
    assert_flags(ed.verify_batch(other, got, msgs), under_other, "verify_batch under the given key")


# ---- d. whole waves of one outcome

@pytest.fixture(scope="module")
def waves(edge):
    """5 x 64 items: wave 0 honest, then one wave each of keys that do not
    decode, a key of order 8, a damaged S and a damaged message."""
    seeds, msgs, pubs, sigs = edge
    cases = ref.vectors()["verify"]
    undecodable = [b(c["pk"]) for c in cases if c["class"] == "undecodable" and c["note"].endswith("as key")]
    order8 = next(c for c in cases if c["note"] == "order 8 as key, the equation holds")
    assert len(undecodable) == 2 and all(ref.decode(k) is None for k in undecodable)
    t8 = ref.decode(b(order8["pk"]))
    assert ref.mul(4, t8) != ref.IDENTITY and ref.mul(8, t8) == ref.IDENTITY
    pks, sg, ms = [], [], []
    for j in range(320):
        wave, i = j // 64, 64 + j                        # items 64..383 of the edge set: every length, distinct keys
        pk, sig, msg = pubs[i], sigs[i], msgs[i]
        if wave == 1:
            pk = undecodable[j % 2]
        elif wave == 2:
            pk = b(order8["pk"])
            if j % 2:
                sig, msg = b(order8["sig"]), b(order8["msg"])          # for which the plain equation holds
        elif wave == 3:
            k = 32 + j % 32
            sig = sig[:k] + bytes([sig[k] ^ (1 << (j % 7))]) + sig[k + 1:]
        elif wave == 4:
            msg = msg[:-1] + bytes([msg[-1] ^ 0x40]) if msg else b"\x00"
        pks.append(pk), sg.append(sig), ms.append(msg)
    want = np.array([ref.verify(p, s, m) for p, s, m in zip(pks, sg, ms)])
    assert want.sum() == 64 and want[:64].all()          # not all-reject
    return pks, sg, ms, want


@pytest.mark.parametrize("order", ["wave by wave", "lane by lane"])
def test_whole_waves_of_one_outcome(waves, order):
    from reticulum_amd import ed25519 as ed
    pks, sigs, msgs, want = waves
    if order == "lane by lane":                          # item j of the batch comes from wave j % 5
        idx = [(j % 5) * 64 + j // 5 for j in range(320)]
        assert sorted(idx) == list(range(320))
        pks, sigs, msgs, want = [pks[i] for i in idx], [sigs[i] for i in idx], [msgs[i] for i in idx], want[idx]
        assert want[::5].all() and want.sum() == 64
    assert_flags(ed.verify_batch(pks, sigs, msgs), want, "verify_batch")
    assert_flags(device_verify(pks, rows(sigs, 64), msgs), want, "device.ed25519_verify")


# ---- e. public key -> signature -> verification without leaving the device

def test_device_round_trip_with_no_host_hop(edge):
    import torch
    from reticulum_amd import device
    n = 257
    seeds, msgs, pubs, sigs = (x[:n] for x in edge)
    d_seeds, d_msgs = dev_rows(seeds, 32), dev_msgs(msgs)
    d_pub, d_sig = guarded(n, 32), guarded(n, 64)
    ok = torch.full((n + 3,), 0xEE, dtype=torch.uint8, device="cuda")
    device.ed25519_public(d_seeds, d_pub[:n])
    device.ed25519_sign(d_seeds, *d_msgs, d_sig[:n], public_keys=d_pub[:n])
    assert d_sig[:n].stride(0) == 64
    device.ed25519_verify(d_pub[:n], d_sig[:n], *d_msgs, ok[:n])
    assert ok.cpu().numpy().tolist() == [1] * n + [0xEE] * 3
    assert_rows(taken(d_pub, n), rows(pubs, 32), "device.ed25519_public", msgs)
    assert_rows(taken(d_sig, n), rows(sigs, 64), "device.ed25519_sign", msgs)
    # one bit of S per item, a different byte from lane to lane: S mod L changes, so none verifies
    item = torch.arange(n, device="cuda")
    d_sig[item, 32 + item % 32] ^= 0x04
    device.ed25519_verify(d_pub[:n], d_sig[:n], *d_msgs, ok[:n])
    assert ok.cpu().numpy().tolist() == [0] * n + [0xEE] * 3
