"""``Identity.encrypt`` / ``Identity.decrypt`` for a batch of packets
(RNS/Identity.py:803-904), bytes in and bytes out.

Per packet the reference draws an ephemeral X25519 key, exchanges it with the
target's public key (or ratchet), derives a 64-byte token key with HKDF
(salt = the identity hash, no context) and runs the token; the receiver does
the exchange with its own key and with every ratchet.  Here the exchanges run
in ``k_x25519`` (one lane each), the derivation and key expansion in the key
setup kernel, and the token in the encrypt / decrypt kernels; the shared
secrets and the derived keys never leave the device.  No CPU fallback.
"""
import ctypes
import hashlib
import os

import numpy as np

from . import _native, ed25519, x25519
from ._native import RT_ST_OK
from .token import KeySet, Packed

KEYSIZE = 32                # an X25519 key (Identity.KEYSIZE // 8 // 2)
DERIVED_KEY_LENGTH = 64     # Identity.DERIVED_KEY_LENGTH


def _bytes32(v, what):
    if not isinstance(v, (bytes, bytearray, memoryview)):
        raise TypeError(f"{what} must be bytes")
    if len(v) != KEYSIZE:
        raise ValueError(x25519._BAD_LEN)
    return bytes(v)


def _salt_bytes(salt):
    if salt is not None and not isinstance(salt, (bytes, bytearray, memoryview)):
        raise TypeError("salt must be bytes (the identity hash)")
    return b"" if salt is None else bytes(salt)


class _Uploads:
    """Device copies of host arrays for one call, freed on exit."""

    def __init__(self, lib, ctx):
        self.lib, self.ctx, self.bufs, self.keep = lib, ctx, [], []

    def __enter__(self):
        return self

    def up(self, arr):
        if arr is None or arr.size == 0:
            return None
        arr = np.ascontiguousarray(arr)
        d = self.lib.rt_device_alloc(self.ctx, arr.nbytes)
        if not d:
            raise _native.NativeError(_native.RT_E_NOMEM, _native.last_error())
        self.bufs.append(d)
        self.keep.append(arr)          # the source outlives the enqueued copy
        _native.check(self.lib.rt_memcpy_h2d(self.ctx, d, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes, None))
        return d

    def __exit__(self, *exc):
        for d in self.bufs:
            self.lib.rt_device_free(self.ctx, d)


def _keyset(u, scalars, scalar_stride, points, point_stride, point_off, salt, n):
    """Key i = Token(hkdf(64, X25519(scalar_i, point_i), salt, None)), built on
    the device from uploaded arrays."""
    saltb = np.frombuffer(salt, np.uint8)
    h = u.lib.rt_keyset_create_x25519(u.ctx, u.up(scalars), scalar_stride, u.up(points), point_stride,
                                      u.up(point_off), u.up(saltb), 0, len(salt), None, 0, DERIVED_KEY_LENGTH, n, None)
    if not h:
        raise _native.NativeError(-1, _native.last_error())
    ks = KeySet._adopt(h, DERIVED_KEY_LENGTH, n, u.lib, u.ctx)
    _native.check(u.lib.rt_stream_sync(u.ctx, None))     # the uploads are freed on exit
    return ks


def encrypt_batch(target_public, salt, plaintexts, ephemeral_privates=None, ivs=None, device=None):
    """``Identity.encrypt`` (Identity.py:811-833) over n plaintexts for one
    identity: ``target_public`` is its X25519 public key, or the ratchet,
    ``salt`` its hash.  Returns a list of ``ephemeral_pub || iv || ct || tag``.
    ``ephemeral_privates`` (n x 32 bytes) and ``ivs`` (n x 16) come from
    os.urandom when not given, as in the reference."""
    target = np.frombuffer(_bytes32(target_public, "target_public"), np.uint8)
    salt = _salt_bytes(salt)
    pts = list(plaintexts)
    for p in pts:
        if not isinstance(p, bytes):
            raise TypeError("Token plaintext input must be bytes")     # Token.py:88
    n = len(pts)
    if ephemeral_privates is None:
        eph = np.frombuffer(os.urandom(KEYSIZE * n), np.uint8).reshape(n, KEYSIZE)
    else:
        eph, one = x25519._rows(ephemeral_privates, "ephemeral_privates")
        if one or len(eph) != n:
            raise ValueError("need one ephemeral private key per plaintext")
    if ivs is not None:
        ivs = np.ascontiguousarray(ivs, dtype=np.uint8).reshape(-1)
        if ivs.size != 16 * n:
            raise ValueError("need 16 IV bytes per packet")
    if n == 0:
        return []
    pubs = x25519.public_keys_batch(eph, device)
    with _Uploads(_native.load(), _native.context(device)) as u:
        ks = _keyset(u, eph, KEYSIZE, target, 0, None, salt, n)
    toks = ks.encrypt_batch(pts, ivs=ivs, key_idx=np.arange(n, dtype=np.uint32))
    return [pubs[i].tobytes() + toks[i] for i in range(n)]


def decrypt_batch(private, salt, tokens, ratchets=None, enforce_ratchets=False, device=None):
    """``Identity.decrypt`` (Identity.py:857-902) over n tokens for one
    identity: ``private`` is its X25519 private key, ``salt`` its hash,
    ``ratchets`` a list of ratchet private keys tried in order before the
    identity's key (which ``enforce_ratchets`` leaves out).  Returns
    ``(plaintexts, which)``: plaintexts[i] is bytes or None; which[i] is the
    index of the ratchet that opened token i, -1 for the identity's key, or
    None.  Tokens of 32 bytes or fewer give None."""
    scalars = [_bytes32(r, "ratchet") for r in (ratchets or [])]
    R = len(scalars)
    scalars.append(_bytes32(private, "private"))
    salt = _salt_bytes(salt)
    toks = [bytes(t) for t in tokens]
    n = len(toks)
    plaintexts, which = [None] * n, [None] * n
    live = [i for i in range(n) if len(toks[i]) > KEYSIZE]            # Identity.py:858
    if not live or (enforce_ratchets and R == 0):
        return plaintexts, which
    m, C = len(live), R + 1
    # peer public keys are read in place at the head of each token
    packed = Packed.from_list([toks[i] for i in live])
    point_off = np.repeat(packed.off, C)
    rows = np.tile(np.frombuffer(b"".join(scalars), np.uint8).reshape(C, KEYSIZE), (m, 1))
    with _Uploads(_native.load(), _native.context(device)) as u:
        ks = _keyset(u, rows, KEYSIZE, packed.buf, 0, point_off, salt, m * C)
    # token j's candidates: keys j*C + r in ratchet order, the identity's key last
    tried = R if enforce_ratchets else C
    out, status, key_used = ks.decrypt_trials([toks[i][KEYSIZE:] for i in live],
                                              [range(j * C, j * C + tried) for j in range(m)])
    for j, i in enumerate(live):
        if status[j] == RT_ST_OK:
            r = int(key_used[j]) - j * C
            plaintexts[i], which[i] = out[j], (r if r < R else -1)
    return plaintexts, which


# ------------------------------------------------- signatures (Ed25519) -----

def validate_batch(sig_public, signatures, messages, device=None):
    """``Identity.validate`` (Identity.py:924-940) over a batch: a list of
    bools, element i telling whether ``signatures[i]`` is the signature of
    ``messages[i]`` under the 32-byte Ed25519 key ``sig_public`` (bytes: one
    identity; or one key per message).  A signature that is not 64 bytes long
    gives False and does not raise: the reference's assertion is swallowed by
    ``validate``'s ``except``."""
    sigs, msgs = list(signatures), list(messages)
    if len(sigs) != len(msgs):
        raise ValueError("need one signature per message")
    for v in sigs:
        if not isinstance(v, (bytes, bytearray, memoryview)):
            raise TypeError("signatures must be bytes")
    one_key = isinstance(sig_public, (bytes, bytearray, memoryview))
    keys = sig_public if one_key else list(sig_public)
    if not one_key and len(keys) != len(msgs):
        raise ValueError("need one public key per message (or one bytes object to broadcast)")
    keep = [i for i, v in enumerate(sigs) if len(v) == 64]
    out = [False] * len(msgs)
    if one_key or keep:
        ok = ed25519.verify_batch(keys if one_key else [keys[i] for i in keep], [sigs[i] for i in keep],
                                  [msgs[i] for i in keep], device)
        for i, v in zip(keep, ok):
            out[i] = bool(v)
    return out


def sign_batch(sig_private, messages, device=None):
    """``Identity.sign`` (Identity.py:907-922) over a batch: the 64-byte
    signatures of ``messages`` under the 32-byte Ed25519 seed ``sig_private``
    (the second half of ``Identity.get_private_key()``), as a list of bytes.
    The public key is derived once and handed to the signing kernel."""
    msgs = list(messages)
    if not isinstance(sig_private, (bytes, bytearray, memoryview)):
        raise TypeError("signing key must be bytes")
    if len(sig_private) != 32:
        raise ValueError(ed25519.BAD_SIGNING_KEY % len(sig_private))
    for m in msgs:
        if not isinstance(m, (bytes, bytearray, memoryview)):
            raise TypeError("messages must be bytes")
    if not msgs:
        return []
    pub = ed25519.public_key(sig_private, device)
    return [row.tobytes() for row in ed25519.sign_batch(sig_private, msgs, public_keys=pub, device=device)]


def validate_announces_batch(announces, only_validate_signature=False, device=None):
    """``Identity.validate_announce`` (Identity.py:511-606) over a batch of
    ``(destination_hash, context_flag, data)``: a list of bools.  The fields
    are cut as the reference cuts them (64-byte public key, 10-byte name hash,
    10-byte random hash, a 32-byte ratchet when the context flag is set, the
    64-byte signature, app data), the signatures over destination_hash ‖
    public_key ‖ name_hash ‖ random_hash ‖ ratchet ‖ app_data are verified on
    the device under ``data[32:64]``, and unless ``only_validate_signature``
    the destination hash must be that of the name hash and the announced
    identity.  Data too short for its fixed fields gives False.  Remembering
    destinations and ratchets, blackholed identities and logging stay with
    the caller."""
    items = list(announces)
    out = [False] * len(items)
    keep, keys, sigs, signed = [], [], [], []
    for i, (destination_hash, context_flag, data) in enumerate(items):
        data = bytes(data)
        head = 116 if context_flag else 84            # key 64, name hash 10, random hash 10, ratchet 32
        if len(data) < head + 64:
            continue
        public_key, signature, app_data = data[:64], data[head:head + 64], data[head + 64:]
        if not only_validate_signature:
            identity_hash = hashlib.sha256(public_key).digest()[:16]
            if bytes(destination_hash) != hashlib.sha256(data[64:74] + identity_hash).digest()[:16]:
                continue
        keep.append(i)
        keys.append(public_key[32:])
        sigs.append(signature)
        signed.append(bytes(destination_hash) + data[:head] + app_data)
    if keep:
        for i, v in zip(keep, ed25519.verify_batch(keys, sigs, signed, device)):
            out[i] = bool(v)
    return out
