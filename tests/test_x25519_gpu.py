"""k_x25519 on the GPU through the C-ABI and the device layer, bit-exact
against the reference's fixtures and the tests' own integer ladder
(tests/x25519_ref.py)."""
import numpy as np
import pytest

import x25519_ref as ref
from tests_helpers import b

pytestmark = pytest.mark.gpu


def rows(hexes):
    return np.frombuffer(b"".join(b(h) for h in hexes), np.uint8).reshape(len(hexes), 32)


@pytest.fixture(scope="module")
def pairs():
    """257 random pairs and their integer-ladder secrets, computed once."""
    rng = np.random.Generator(np.random.PCG64(255))
    sc = rng.integers(0, 256, (257, 32), dtype=np.uint8)
    pt = rng.integers(0, 256, (257, 32), dtype=np.uint8)
    want = np.stack([np.frombuffer(ref.ladder(sc[i].tobytes(), pt[i].tobytes()), np.uint8) for i in range(257)])
    sc.setflags(write=False), pt.setflags(write=False), want.setflags(write=False)
    return sc, pt, want


def host_exchange(sc, sc_stride, pt, pt_stride, off, n, out_stride=32):
    from reticulum_amd import _native
    lib, ctx = _native.load(), _native.context(0)
    out = np.full(n * out_stride, 0xEE, np.uint8)
    _native.check(lib.rt_x25519_host(ctx, sc.ctypes.data, sc_stride, None if pt is None else pt.ctypes.data, pt_stride,
                                     None if off is None else off.ctypes.data, out.ctypes.data, out_stride, n))
    return out.reshape(n, out_stride)


def test_exchange_fixtures_host_and_device():
    import torch
    from reticulum_amd import device
    ex = ref.vectors()["exchanges"]
    sc, pt, want = rows([e["scalar"] for e in ex]), rows([e["point"] for e in ex]), rows([e["out"] for e in ex])
    got = host_exchange(sc, 32, pt, 32, None, len(ex))
    for i, e in enumerate(ex):
        assert got[i].tobytes() == want[i].tobytes(), e["note"]
    out = torch.zeros((len(ex), 32), dtype=torch.uint8, device="cuda")
    device.x25519(torch.from_numpy(sc.copy()).cuda(), torch.from_numpy(pt.copy()).cuda(), out)
    assert np.array_equal(out.cpu().numpy(), want)


def test_chain_fixture():
    """64 dependent exchanges: each output is the next scalar, the old scalar
    the next point."""
    import reticulum_amd as rt
    c = ref.vectors()["chain"]
    k, u = b(c["scalar"]), b(c["point"])
    for want in c["outs"]:
        out = rt.exchange(k, u)
        assert out.hex() == want
        k, u = out, k


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_cross_wave_and_block(pairs, n):
    import reticulum_amd as rt
    sc, pt, want = pairs
    assert np.array_equal(rt.exchange_batch(sc[:n], pt[:n]), want[:n])


def test_stride0_scalar_and_stride0_point(pairs):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    sc, pt, _ = pairs
    n = 70
    one_sc = np.stack([np.frombuffer(ref.ladder(sc[0].tobytes(), pt[i].tobytes()), np.uint8) for i in range(n)])
    one_pt = np.stack([np.frombuffer(ref.ladder(sc[i].tobytes(), pt[0].tobytes()), np.uint8) for i in range(n)])
    assert np.array_equal(rt.exchange_batch(sc[0].tobytes(), pt[:n]), one_sc)
    assert np.array_equal(rt.exchange_batch(sc[:n], pt[0].tobytes()), one_pt)
    d_sc, d_pt = torch.from_numpy(sc[:n].copy()).cuda(), torch.from_numpy(pt[:n].copy()).cuda()
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    device.x25519(d_sc[:1].expand(n, 32), d_pt, out)
    assert np.array_equal(out.cpu().numpy(), one_sc)
    device.x25519(d_sc, d_pt[:1], out)
    assert np.array_equal(out.cpu().numpy(), one_pt)


def test_null_points_give_public_keys():
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    keys = ref.vectors()["public_keys"]
    prv, pub = rows([k["private"] for k in keys]), rows([k["public"] for k in keys])
    assert np.array_equal(rt.public_keys_batch(prv), pub)
    assert rt.public_key(b(keys[3]["private"])).hex() == keys[3]["public"]
    out = torch.zeros((len(keys), 32), dtype=torch.uint8, device="cuda")
    device.x25519(torch.from_numpy(prv.copy()).cuda(), None, out)
    assert np.array_equal(out.cpu().numpy(), pub)


def test_odd_strides_leave_guard_bytes(pairs):
    """point_stride 33 and out_stride 35 on the device: rows at every byte
    phase, and the 0xEE bytes between output rows are not written."""
    import torch
    from reticulum_amd import device
    sc, pt, want = pairs
    n = 67
    wide = np.full((n, 33), 0xEE, np.uint8)
    wide[:, :32] = pt[:n]
    d_pt = torch.from_numpy(wide).cuda()
    d_out = torch.full((n, 35), 0xEE, dtype=torch.uint8, device="cuda")
    device.x25519(torch.from_numpy(sc[:n].copy()).cuda(), d_pt[:, :32], d_out[:, :32])
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:, :32], want[:n])
    assert (got[:, 32:] == 0xEE).all()
    # the host entry with the same strides
    host = host_exchange(sc, 32, wide, 33, None, n, out_stride=35)
    assert np.array_equal(host[:, :32], want[:n]) and (host[:, 32:] == 0xEE).all()


def test_point_off_at_all_byte_phases(pairs):
    """Points read in place from a flat buffer at offsets of every phase mod
    4, out of order and with one offset used twice."""
    import torch
    from reticulum_amd import device
    sc, pt, want = pairs
    n = 66
    off = np.array([36 * i + i % 4 for i in range(n)], dtype=np.int64)     # 1 to 5 guard bytes between points
    assert set(int(o) % 4 for o in off) == {0, 1, 2, 3} and (np.diff(off) > 32).all()
    buf = np.full(int(off[-1]) + 32, 0xEE, np.uint8)
    for i in range(n):
        buf[off[i]:off[i] + 32] = pt[i]
    perm = np.random.Generator(np.random.PCG64(3)).permutation(n)
    perm[5] = perm[6]
    d_out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    device.x25519(torch.from_numpy(sc[perm].copy()).cuda(), torch.from_numpy(buf).cuda(), d_out,
                  point_off=torch.from_numpy(off[perm].copy()).cuda())
    got = d_out.cpu().numpy()
    assert np.array_equal(got, want[perm])
    host = host_exchange(np.ascontiguousarray(sc[perm]), 32, buf, 0, off[perm].astype(np.uint64), n)
    assert np.array_equal(host, want[perm])


def test_argument_errors():
    from reticulum_amd import _native
    lib, ctx = _native.load(), _native.context(0)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert lib.rt_x25519_host(ctx, None, 32, p, 32, None, p, 32, 1) == _native.RT_E_INVAL
    assert lib.rt_x25519_host(ctx, p, 32, p, 32, None, None, 32, 1) == _native.RT_E_INVAL
    assert lib.rt_x25519_host(ctx, p, 31, p, 32, None, p, 32, 2) == _native.RT_E_INVAL
    assert lib.rt_x25519_host(ctx, p, 32, p, 32, None, p, 16, 2) == _native.RT_E_INVAL
    assert lib.rt_x25519_host(None, p, 32, p, 32, None, p, 32, 1) == _native.RT_E_INVAL
    assert lib.rt_x25519_host(ctx, p, 32, p, 32, None, None, 32, 0) == _native.RT_OK       # n == 0, as rt_hkdf
    assert lib.rt_x25519(ctx, p, 32, None, 0, p, p, 32, 1, None) == _native.RT_E_INVAL     # offsets without points
    assert not lib.rt_keyset_create_x25519(ctx, p, 32, p, 32, None, None, 0, 0, None, 0, 48, 1, None)
    assert "128 or 256 bits" in _native.last_error()
    assert not lib.rt_keyset_create_x25519(ctx, p, 32, p, 32, None, None, 0, 0, None, 0, 64, 0, None)


@pytest.mark.parametrize("key_len", [64, 32])
def test_keyset_from_exchange_encrypts_as_the_oracle(pairs, key_len):
    """rt_keyset_create_x25519: key i = Token(hkdf(key_len, X25519(scalar_i,
    point_i), salt, None)); tokens equal the C oracle's under hashlib HKDF of
    the integer ladder's secret.  Per-row salts, then one shared salt row with
    one shared point (the sender's shape)."""
    import torch
    import reticulum_amd as rt
    from oracle import ctoken
    from reticulum_amd import device
    sc, pt, want = pairs
    n, L = 65, 47
    rng = np.random.Generator(np.random.PCG64(key_len))
    salt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, L), dtype=np.uint8)
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    d_sc, d_pt, d_salt = (torch.from_numpy(a[:n].copy()).cuda() for a in (sc, pt, salt))
    d_msg, d_iv = torch.from_numpy(msg).cuda(), torch.from_numpy(iv).cuda()
    kidx = torch.arange(n, dtype=torch.int32, device="cuda")
    tok = torch.empty((n, rt.token_len(L)), dtype=torch.uint8, device="cuda")

    ks = device.derive_keyset_x25519(d_sc, d_pt, d_salt, key_len=key_len)
    device.encrypt_uniform(ks, d_msg, L, d_iv, tok, key_idx=kidx)
    th = tok.cpu().numpy()
    for i in range(n):
        key = ref.hkdf(key_len, want[i].tobytes(), salt[i].tobytes())
        assert th[i].tobytes() == ctoken.encrypt(key, iv[i].tobytes(), msg[i].tobytes()), i

    ks = device.derive_keyset_x25519(d_sc, d_pt[:1], d_salt[:1].expand(n, 16), key_len=key_len)
    device.encrypt_uniform(ks, d_msg, L, d_iv, tok, key_idx=kidx)
    th = tok.cpu().numpy()
    for i in (0, 1, 63, 64):
        key = ref.hkdf(key_len, ref.ladder(sc[i].tobytes(), pt[0].tobytes()), salt[0].tobytes())
        assert th[i].tobytes() == ctoken.encrypt(key, iv[i].tobytes(), msg[i].tobytes()), i
