"""Ed25519 on the GPU: the verifications, signatures and public keys of
``RNS.Cryptography.Ed25519`` in batches, one item per lane of librnstok's
``k_ed25519_*`` kernels.

Results are those of the reference's internal provider (``pure25519``): the
canonical identity encoding is refused as key and as R, points decode with y
taken mod p, both points must lie in the prime-order subgroup, S is used mod L
(so S >= L verifies), and the equation is compared on points.  A PyCA-backed
Reticulum differs on S >= L and on mixed-order keys; honest signatures agree
(include/rnstok.h states every rule).  There is no CPU fallback.  One item
alone is one lane's whole computation (INTEGRATION.md gives the latency);
``Ed25519PrivateKey`` / ``Ed25519PublicKey`` of the drop-in stay the
reference's.
"""
import ctypes

import numpy as np

from . import _native

BAD_VERIFYING_KEY = "Bad verifying key length %d"        # eddsa.py:87-88
BAD_SIGNATURE = "Bad signature length %d"                # eddsa.py:89-90
BAD_SIGNING_KEY = "Bad signing key length %d"            # eddsa.py:80-81

_BYTES = (bytes, bytearray, memoryview)


def _rows(x, width, bad_len, what):
    """bytes -> one row (broadcast); list of bytes or (n, width) uint8 array ->
    n rows.  Returns ``(array (k, width), is_single)``."""
    if isinstance(x, _BYTES):
        if len(x) != width:
            raise ValueError(bad_len % len(x))
        return np.frombuffer(bytes(x), np.uint8).reshape(1, width), True
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8 or x.ndim != 2:
            raise ValueError(f"{what} array must be (n, {width}) uint8")
        if x.shape[1] != width:
            raise ValueError(bad_len % x.shape[1])
        return np.ascontiguousarray(x), False
    items = list(x)
    for it in items:
        if not isinstance(it, _BYTES):
            raise TypeError(f"{what} items must be bytes")
        if len(it) != width:
            raise ValueError(bad_len % len(it))
    return np.frombuffer(b"".join(bytes(i) for i in items), np.uint8).reshape(len(items), width), False


def _messages(messages):
    """A list of bytes -> (flat uint8 array, uint64 offsets, uint32 lengths)."""
    items = list(messages)
    for m in items:
        if not isinstance(m, _BYTES):
            raise TypeError("messages must be bytes")
    lens = np.array([len(m) for m in items], np.uint32)
    offs = np.zeros(len(items), np.uint64)
    if len(items) > 1:
        np.cumsum(lens[:-1], dtype=np.uint64, out=offs[1:])
    flat = np.frombuffer(b"".join(bytes(m) for m in items), np.uint8)
    return flat, offs, lens


def _sized(rows, one, n, what):
    if not one and len(rows) != n:
        raise ValueError(f"need one {what} per message (or one bytes object to broadcast)")


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _msg_ptr(flat):
    return _ptr(flat) if len(flat) else None


def verify_batch(public_keys, signatures, messages, device=None):
    """``Ed25519PublicKey.verify`` over a batch: element i of the returned (n,)
    bool array says whether ``signatures[i]`` is ``public_keys[i]``'s signature
    of ``messages[i]``, where the reference would return or raise.  Keys and
    signatures are bytes (one value for all), a list of bytes or a 2-D uint8
    array; messages are a list of bytes."""
    pk, pk_one = _rows(public_keys, 32, BAD_VERIFYING_KEY, "public_keys")
    sg, sg_one = _rows(signatures, 64, BAD_SIGNATURE, "signatures")
    flat, offs, lens = _messages(messages)
    n = len(lens)
    _sized(pk, pk_one, n, "public key")
    _sized(sg, sg_one, n, "signature")
    ok = np.zeros(n, np.uint8)
    if n == 0:
        return ok.astype(bool)
    lib = _native.load()
    ctx = _native.context(device)
    _native.check(lib.rt_ed25519_verify_host(ctx, _ptr(pk), 0 if pk_one else 32, _ptr(sg), 0 if sg_one else 64,
                                             _msg_ptr(flat), _ptr(offs), _ptr(lens), _ptr(ok), n))
    return ok.astype(bool)


def sign_batch(seeds, messages, public_keys=None, device=None):
    """``Ed25519PrivateKey.sign`` over a batch: an (n, 64) uint8 array.  With
    ``public_keys`` (those of the seeds, trusted) the kernel skips deriving
    them, which halves its work."""
    sd, sd_one = _rows(seeds, 32, BAD_SIGNING_KEY, "seeds")
    pk = pk_one = None
    if public_keys is not None:
        pk, pk_one = _rows(public_keys, 32, BAD_VERIFYING_KEY, "public_keys")
    flat, offs, lens = _messages(messages)
    n = len(lens)
    _sized(sd, sd_one, n, "seed")
    if pk is not None:
        _sized(pk, pk_one, n, "public key")
    out = np.zeros((n, 64), np.uint8)
    if n == 0:
        return out
    lib = _native.load()
    ctx = _native.context(device)
    _native.check(lib.rt_ed25519_sign_host(ctx, _ptr(sd), 0 if sd_one else 32, None if pk is None else _ptr(pk),
                                           0 if pk_one or pk is None else 32, _msg_ptr(flat), _ptr(offs), _ptr(lens),
                                           _ptr(out), 64, n))
    return out


def public_keys_batch(seeds, device=None):
    """``Ed25519PrivateKey.public_key().public_bytes()`` over a batch: an
    (n, 32) uint8 array."""
    sd, _ = _rows(seeds, 32, BAD_SIGNING_KEY, "seeds")
    n = len(sd)
    out = np.zeros((n, 32), np.uint8)
    if n == 0:
        return out
    lib = _native.load()
    ctx = _native.context(device)
    _native.check(lib.rt_ed25519_public_host(ctx, _ptr(sd), 32, _ptr(out), 32, n))
    return out


def _one(v, what):
    if not isinstance(v, _BYTES):
        raise TypeError(f"{what} must be bytes")


def verify(public_key, signature, message, device=None):
    """True where the reference's ``Ed25519PublicKey.verify`` returns, False
    where it raises for a bad signature; wrong lengths raise as there."""
    _one(public_key, "public key")
    _one(signature, "signature")
    _one(message, "message")
    return bool(verify_batch(public_key, signature, [message], device)[0])


def sign(seed, message, device=None):
    """The 64-byte signature of one message."""
    _one(seed, "signing key")
    _one(message, "message")
    return sign_batch(seed, [message], device=device)[0].tobytes()


def public_key(seed, device=None):
    """The 32-byte public key of one seed."""
    _one(seed, "signing key")
    return public_keys_batch(seed, device)[0].tobytes()
