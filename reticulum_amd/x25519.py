"""X25519 on the GPU: the exchanges and public keys of
``RNS.Cryptography.X25519`` (X25519.py:49-93, 136-145) in batches, one
exchange per lane of librnstok's ``k_x25519`` kernel.

Results are those of the reference's internal provider: the scalar is clamped,
bit 255 of the peer's value is ignored, a value >= p is taken mod p, and a
low-order point gives 32 zero bytes without an error.  There is no CPU
fallback.  One exchange alone is one lane's whole ladder (INTEGRATION.md gives
the latency); ``X25519PrivateKey`` of the drop-in stays the reference's.
"""
import ctypes

import numpy as np

from . import _native

_BAD_LEN = "Curve25519 values must be 32 bytes"      # X25519.py:68-69


def _rows(x, what):
    """bytes -> one row (broadcast); list of bytes or (n, 32) uint8 array ->
    n rows.  Returns ``(array (k, 32), is_single)``."""
    if isinstance(x, (bytes, bytearray, memoryview)):
        if len(x) != 32:
            raise ValueError(_BAD_LEN)
        return np.frombuffer(bytes(x), np.uint8).reshape(1, 32), True
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8 or x.ndim != 2:
            raise ValueError(f"{what} array must be (n, 32) uint8")
        if x.shape[1] != 32:
            raise ValueError(_BAD_LEN)
        return np.ascontiguousarray(x), False
    items = list(x)
    for it in items:
        if not isinstance(it, (bytes, bytearray, memoryview)):
            raise TypeError(f"{what} items must be bytes")
        if len(it) != 32:
            raise ValueError(_BAD_LEN)
    return np.frombuffer(b"".join(bytes(i) for i in items), np.uint8).reshape(len(items), 32), False


def _batch(privates, peer_publics):
    """Validated rows and the batch size, before the library is touched."""
    sc, sc_one = _rows(privates, "privates")
    if peer_publics is None:
        return sc, sc_one, None, True, len(sc)
    pt, pt_one = _rows(peer_publics, "peer_publics")
    if not sc_one and not pt_one and len(sc) != len(pt):
        raise ValueError("need one peer public key per private key (or one bytes object to broadcast)")
    return sc, sc_one, pt, pt_one, len(pt) if sc_one else len(sc)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _run(sc, sc_one, pt, pt_one, n, device):
    out = np.zeros((n, 32), np.uint8)
    if n == 0:
        return out
    lib = _native.load()
    ctx = _native.context(device)
    _native.check(lib.rt_x25519_host(ctx, _ptr(sc), 0 if sc_one else 32, None if pt is None else _ptr(pt),
                                     0 if pt_one else 32, None, _ptr(out), 32, n))
    return out


def exchange_batch(privates, peer_publics, device=None):
    """``X25519PrivateKey.exchange`` over a batch: row i of the returned
    (n, 32) uint8 array is the shared secret of ``privates[i]`` and
    ``peer_publics[i]``.  Either side is bytes (one value for all), a list of
    bytes or an (n, 32) uint8 array."""
    return _run(*_batch(privates, peer_publics), device)


def public_keys_batch(privates, device=None):
    """``X25519PrivateKey.public_key().public_bytes()`` over a batch: an
    (n, 32) uint8 array (the exchange with the base point 9)."""
    return _run(*_batch(privates, None), device)


def exchange(private, peer_public, device=None):
    """One shared secret, as ``X25519PrivateKey.from_private_bytes(private)
    .exchange(peer_public)``, without the reference's timing pad."""
    for v in (private, peer_public):
        if not isinstance(v, (bytes, bytearray, memoryview)):
            raise TypeError("Curve25519 values must be bytes")
    return exchange_batch(private, peer_public, device)[0].tobytes()


def public_key(private, device=None):
    """The public key of one private key, 32 bytes."""
    if not isinstance(private, (bytes, bytearray, memoryview)):
        raise TypeError("Curve25519 values must be bytes")
    return public_keys_batch(private, device)[0].tobytes()
