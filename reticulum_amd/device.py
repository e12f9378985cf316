"""Device-resident batch calls over torch tensors (the measured hot path).

Thin wrappers over rt_encrypt* / rt_decrypt* (include/rnstok.h): every
buffer is a CUDA(HIP) tensor already resident in HBM, the kernels are
enqueued on the given stream (default: torch's current stream) and nothing is
synchronised.  torch is used only for device memory and streams.
"""
import ctypes
import threading

import torch

from . import _native
from .token import KeySet, token_len


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("device API needs tensors in device memory")
    if not t.is_contiguous():
        raise ValueError("device API needs contiguous tensors")
    return t.data_ptr()


def _p_rows(t):
    """A (n, row) byte matrix whose rows may sit at any stride >= row (a row
    view of a wider buffer, e.g. 128-B-aligned token rows): bytes within a
    row contiguous; the row stride is passed to the library separately."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("device API needs tensors in device memory")
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError("expected an (n, row) matrix with contiguous rows")
    return t.data_ptr()


def _p_salt(t):
    """Salt rows: contiguous (n, S), or one row broadcast to n
    (`salt[:1].expand(n, S)`, row stride 0: a batch to one identity)."""
    if t is not None and t.dim() == 2 and t.shape[0] > 1 and t.stride(0) == 0 and \
            (t.shape[1] <= 1 or t.stride(1) == 1) and t.is_cuda:
        return t.data_ptr()
    return _p(t)


def _stream(stream, device=None):
    """The HIP stream handle to launch on: ``stream``, else the current
    stream of ``device`` (the tensors' GPU, not whichever GPU is current)."""
    s = stream if stream is not None else torch.cuda.current_stream(device)
    if device is not None and s.device != torch.device(device):
        raise ValueError(f"stream is on {s.device}, the tensors on {device}")
    return s.cuda_stream


def _order_after_current(stream, *tensors):
    """A launch on a side ``stream`` that reads ``tensors`` made on the
    current stream (e.g. a key table an RCCL broadcast just filled; torch only
    makes the *current* stream wait for a collective): the side stream waits
    for the current stream first, and the tensors' memory is kept from reuse
    until the side stream is done with it (the caller may drop them at once)."""
    if stream is None:
        return
    dev = tensors[0].device
    cur = torch.cuda.current_stream(dev)
    if stream == cur:
        return
    stream.wait_stream(cur)
    for t in tensors:
        if t is not None:
            t.record_stream(stream)


def _check_u8(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.uint8:
            raise ValueError("byte buffers must be torch.uint8")


def _check_i32(n, **ts):
    """(n,) contiguous int32 device tensors (None allowed): lengths, statuses
    and key indices are read and written as 32-bit words by the kernels."""
    for name, t in ts.items():
        if t is None:
            continue
        if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous ({n},) int32 tensor")


def _check_i64(n, **ts):
    for name, t in ts.items():
        if t is not None and (t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous ({n},) int64 tensor")


def _check_rows(name, t, n, width):
    """An (n, row) uint8 matrix whose rows hold at least `width` bytes."""
    if t.dim() != 2 or t.shape[0] != n:
        raise ValueError(f"{name} must be an ({n}, row) uint8 matrix")
    if t.shape[1] < width:
        raise ValueError(f"{name} rows hold {t.shape[1]} bytes, need {width}")


def _check_iv(iv, n):
    if iv.numel() < 16 * n or (iv.dim() == 2 and iv.shape[1] != 16) or not iv.is_contiguous():
        raise ValueError(f"iv must be a contiguous ({n}, 16) uint8 tensor")


def encrypt_uniform(ks: KeySet, pt, pt_len, iv, tok, key_idx=None, stream=None):
    """pt: (n, >= pt_len) uint8 rows; iv: (n, 16) uint8; tok: (n, >=
    token_len(pt_len)) uint8 rows; key_idx: (n,) int32 or None.  pt and tok
    may be row views of wider buffers (their row stride is used)."""
    _check_u8(pt, iv, tok)
    n = pt.shape[0]
    _check_rows("pt", pt, n, pt_len)
    _check_rows("tok", tok, n, token_len(pt_len))
    _check_iv(iv, n)
    _check_i32(n, key_idx=key_idx)
    lib = _native.load()
    _native.check(lib.rt_encrypt_uniform(ks.handle, _p_rows(pt), pt.stride(0), pt_len, _p(key_idx), _p(iv),
                                         _p_rows(tok), tok.stride(0), n, _stream(stream, pt.device)))


def decrypt_uniform(ks: KeySet, tok, tok_len, pt, out_len, status, key_idx=None, stream=None):
    """tok: (n, >= tok_len) uint8 holding tok_len-byte tokens; pt: (n, >=
    tok_len - 48) uint8; out_len/status/key_idx: (n,) int32."""
    _check_u8(tok, pt)
    n = tok.shape[0]
    _check_rows("tok", tok, n, tok_len)
    _check_rows("pt", pt, n, max(tok_len - 48, 0))
    _check_i32(n, out_len=out_len, status=status, key_idx=key_idx)
    lib = _native.load()
    _native.check(lib.rt_decrypt_uniform(ks.handle, _p_rows(tok), tok.stride(0), tok_len, _p(key_idx), _p_rows(pt),
                                         pt.stride(0), _p(out_len), _p(status), n, _stream(stream, tok.device)))


# ------------------------------------------------- unit-interleaved layout --
# For batches that live on the device from end to end (rt_encrypt_interleaved,
# include/rnstok.h): 16-B unit u of packet p at 16*(u*n + p), i.e. a (U, n, 16)
# uint8 tensor, so every wave load/store is one contiguous KiB of HBM.

def units(nbytes):
    """16-B units that hold nbytes."""
    return (int(nbytes) + 15) // 16


def interleave(rows, nbytes=None):
    """(n, >= nbytes) uint8 rows -> the (units(nbytes), n, 16) interleaved
    tensor (a copy; the last unit zero-padded)."""
    n = rows.shape[0]
    L = rows.shape[1] if nbytes is None else int(nbytes)
    U = units(L)
    out = torch.zeros((n, U * 16), dtype=torch.uint8, device=rows.device)
    out[:, :L] = rows[:, :L]
    return out.view(n, U, 16).transpose(0, 1).contiguous()


def deinterleave(u, nbytes=None):
    """(U, n, 16) interleaved units -> (n, nbytes) rows (a copy)."""
    U, n, _ = u.shape
    rows = u.transpose(0, 1).reshape(n, U * 16)
    return rows[:, : (U * 16 if nbytes is None else int(nbytes))].contiguous()


# ---- rows in 128-B-aligned slots ------
LINE = 128


def aligned_rows(n, width, phase=0, device=None):
    """An (n, width) uint8 row view for the uniform entry points whose row
    stride is a multiple of 128 B and whose byte ``phase`` of every row starts
    a 128-B line: phase 0 for plaintexts, 16 for tokens (the ciphertext after
    the IV), 35 for HEADER_1 packets.  Same outputs as packed rows; the chip
    runs the token kernels 3-5 % faster on them (fewer lines straddle two
    packets).  The bytes between rows are uninitialised."""
    n, width, phase = int(n), int(width), int(phase)
    if n < 0 or width < 0 or not 0 <= phase < LINE:
        raise ValueError("aligned_rows: n, width >= 0 and 0 <= phase < 128")
    stride = max(LINE, -(-width // LINE) * LINE)
    buf = torch.empty(n * stride + LINE, dtype=torch.uint8, device=device)
    off = (-(buf.data_ptr() + phase)) % LINE
    return buf[off:off + n * stride].view(n, stride)[:, :width] if n else buf[:0].view(0, width)


def _check_units(name, t, U, n):
    if t.dtype != torch.uint8 or t.dim() != 3 or tuple(t.shape) != (U, n, 16) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous ({U}, {n}, 16) uint8 tensor of interleaved units")


def encrypt_interleaved(ks: KeySet, pt, pt_len, iv, tok, key_idx=None, stream=None):
    """Token.encrypt of n packets of pt_len bytes in the interleaved layout:
    pt (units(pt_len), n, 16), iv (n, 16), tok (token_len(pt_len)/16, n, 16).
    Tokens are bit-identical to encrypt_uniform's."""
    n = iv.shape[0]
    _check_units("pt", pt, units(pt_len), n)
    _check_units("tok", tok, token_len(pt_len) // 16, n)
    _check_u8(iv)
    _check_iv(iv, n)
    _check_i32(n, key_idx=key_idx)
    lib = _native.load()
    _native.check(lib.rt_encrypt_interleaved(ks.handle, _p(pt) if pt.numel() else None, pt_len, _p(key_idx), _p(iv),
                                             _p(tok), n, _stream(stream, tok.device)))


def decrypt_interleaved(ks: KeySet, tok, tok_len, pt, out_len, status, key_idx=None, stream=None):
    """Token.decrypt of n tokens of tok_len = 48 + 16k bytes (k >= 1) in the
    interleaved layout: tok (tok_len/16, n, 16), pt ((tok_len-48)/16, n, 16)
    (plaintext incl. its pad block, zeroed on failure), out_len/status (n,)
    int32 as decrypt_uniform."""
    n = tok.shape[1] if tok.dim() == 3 else -1
    if tok_len < 64 or tok_len % 16:
        raise ValueError("interleaved tokens must be 48 + 16*k bytes, k >= 1")
    _check_units("tok", tok, tok_len // 16, n)
    _check_units("pt", pt, (tok_len - 48) // 16, n)
    _check_i32(n, out_len=out_len, status=status, key_idx=key_idx)
    lib = _native.load()
    _native.check(lib.rt_decrypt_interleaved(ks.handle, _p(tok), tok_len, _p(key_idx), _p(pt), _p(out_len),
                                             _p(status), n, _stream(stream, tok.device)))


def verify(ks: KeySet, tok, tok_off, tok_len, status, key_idx=None, stream=None):
    """Token.verify_hmac (Token.py:77-84) over device buffers, no AES: token
    i is tok[tok_off[i] : +tok_len[i]] (int64 / int32); status (n,) int32
    receives RT_ST_OK (tag valid), RT_ST_BAD_HMAC or RT_ST_TOO_SHORT."""
    _check_u8(tok)
    n = tok_off.numel()
    _check_i64(n, tok_off=tok_off)
    _check_i32(n, tok_len=tok_len, status=status, key_idx=key_idx)
    lib = _native.load()
    _native.check(lib.rt_verify(ks.handle, _p(tok), _p(tok_off), _p(tok_len), _p(key_idx), _p(status), n,
                                _stream(stream, tok.device)))


def verify_trials(ks: KeySet, tok, tok_off, tok_len, pair_off, pair_key, first, stream=None):
    """Ratchet trials (Identity.py:865-878) over device buffers: token t is
    tok[tok_off[t] : +tok_len[t]] (int64 / int32), its candidates are
    pair_key[pair_off[t] : pair_off[t+1]] (int32, pair_off (n+1,) int32 from
    0); first (n,) int32 receives the rank of the first candidate whose key
    opens token t, or -1."""
    _check_u8(tok)
    n = tok_off.numel()
    _check_i64(n, tok_off=tok_off)
    _check_i32(n, tok_len=tok_len, first=first)
    _check_i32(n + 1, pair_off=pair_off)
    _check_i32(pair_key.numel(), pair_key=pair_key)
    lib = _native.load()
    _native.check(lib.rt_verify_trials(ks.handle, _p(tok), _p(tok_off), _p(tok_len), _p(pair_off), _p(pair_key),
                                       _p(first), n, pair_key.numel(), _stream(stream, tok.device)))


def _workspace(n, device):
    lib = _native.load()
    return torch.empty(int(lib.rt_workspace_bytes(n)), dtype=torch.uint8, device=device)


def encrypt(ks: KeySet, pt, pt_off, pt_len, iv, tok, tok_off, key_idx=None, stream=None, sort=False,
            workspace=None):
    """Variable-length batch: pt/tok flat uint8 buffers, pt_off/tok_off int64,
    pt_len int32, iv (n,16) uint8.  ``sort=True`` groups packets by length on
    the device first (same outputs; wavefronts carry similar lengths)."""
    _check_u8(pt, iv, tok)
    n = pt_off.numel()
    _check_i64(n, pt_off=pt_off, tok_off=tok_off)
    _check_i32(n, pt_len=pt_len, key_idx=key_idx)
    _check_iv(iv, n)
    lib = _native.load()
    if sort:
        ws = workspace if workspace is not None else _workspace(n, pt.device)
        _native.check(lib.rt_encrypt_ex(ks.handle, _p(pt), _p(pt_off), _p(pt_len), _p(key_idx), _p(iv), _p(tok),
                                        _p(tok_off), n, _native.RT_F_SORT_BY_LENGTH, _p(ws), _stream(stream, pt.device)))
        return
    _native.check(lib.rt_encrypt(ks.handle, _p(pt), _p(pt_off), _p(pt_len), _p(key_idx), _p(iv), _p(tok),
                                 _p(tok_off), n, _stream(stream, pt.device)))


def decrypt(ks: KeySet, tok, tok_off, tok_len, pt, pt_off, out_len, status, key_idx=None, stream=None, sort=False,
            workspace=None):
    _check_u8(tok, pt)
    n = tok_off.numel()
    _check_i64(n, tok_off=tok_off, pt_off=pt_off)
    _check_i32(n, tok_len=tok_len, out_len=out_len, status=status, key_idx=key_idx)
    lib = _native.load()
    if sort:
        ws = workspace if workspace is not None else _workspace(n, tok.device)
        _native.check(lib.rt_decrypt_ex(ks.handle, _p(tok), _p(tok_off), _p(tok_len), _p(key_idx), _p(pt),
                                        _p(pt_off), _p(out_len), _p(status), n, _native.RT_F_SORT_BY_LENGTH, _p(ws),
                                        _stream(stream, tok.device)))
        return
    _native.check(lib.rt_decrypt(ks.handle, _p(tok), _p(tok_off), _p(tok_len), _p(key_idx), _p(pt), _p(pt_off),
                                 _p(out_len), _p(status), n, _stream(stream, tok.device)))


def hkdf(ikm, out, salt=None, context=None, stream=None):
    """HKDF-SHA256 over device rows (RNS/Cryptography/HKDF.py:35-62): ikm
    (n, L) uint8, salt (n, S) uint8 or None (the reference's 32 zero bytes;
    one row expanded to (n, S) is shared, its HMAC midstates computed once),
    context a (C,) uint8 device tensor or None, out (n, length) uint8 with
    length = out.shape[1] >= 1.  Row i of out = hkdf(length, ikm[i], salt[i],
    context)."""
    _check_u8(ikm, out, salt, context)
    n = ikm.shape[0]
    if out.shape[0] != n or (salt is not None and salt.shape[0] != n):
        raise ValueError("shape mismatch")
    length = out.shape[1]
    lib = _native.load()
    ctx = _native.context(out.device.index)
    _native.check(lib.rt_hkdf(ctx, _p(ikm), ikm.stride(0), ikm.shape[1], _p_salt(salt),
                              salt.stride(0) if salt is not None else 0, salt.shape[1] if salt is not None else 0,
                              _p(context), context.numel() if context is not None else 0, _p(out), out.stride(0),
                              length, n, _stream(stream, ikm.device)))


def keyset(keys, stream=None):
    """KeySet from a device key table (Token.py:58-74 per row): ``keys`` is a
    contiguous (n_keys, 64 or 32) uint8 CUDA tensor, e.g. received by
    shard.broadcast_keys; expanded on its device on ``stream`` without a
    host round trip.  Usable from any stream right away, as derive_keyset."""
    _check_u8(keys)
    if keys.dim() != 2 or keys.shape[1] not in (32, 64) or keys.shape[0] < 1 or not keys.is_contiguous():
        raise ValueError("keys must be a contiguous (n_keys, 64 or 32) uint8 device tensor")
    n, klen = keys.shape
    lib = _native.load()
    ctx = _native.context(keys.device.index)
    _order_after_current(stream, keys)
    h = lib.rt_keyset_create_device(ctx, _p(keys), klen, n, _stream(stream, keys.device))
    if not h:
        raise _native.NativeError(-1, _native.last_error())
    return KeySet._adopt(h, klen, n, lib, ctx)


def derive_keyset(ikm, salt=None, context=None, key_len=64, stream=None):
    """Per-packet keying from device rows (Identity.py:837-846): KeySet whose
    key i is Token(hkdf(key_len, ikm[i], salt[i], context)); derived and
    expanded on the device in one launch (the derived keys never reach HBM)
    on ``stream``.  The key set is usable from any stream or host call right
    away: every later launch that reads it waits for this build first."""
    _check_u8(ikm, salt, context)
    n = ikm.shape[0]
    lib = _native.load()
    ctx = _native.context(ikm.device.index)
    _order_after_current(stream, ikm, salt, context)
    h = lib.rt_keyset_create_hkdf(ctx, _p(ikm), ikm.stride(0), ikm.shape[1], _p_salt(salt),
                                  salt.stride(0) if salt is not None else 0, salt.shape[1] if salt is not None else 0,
                                  _p(context), context.numel() if context is not None else 0, key_len, n,
                                  _stream(stream, ikm.device))
    if not h:
        raise _native.NativeError(-1, _native.last_error())
    return KeySet._adopt(h, key_len, n, lib, ctx)


def _x25519_rows(name, t, n):
    """(pointer, row stride) of 32-byte rows: an (n, >=32) uint8 matrix whose
    rows sit at any stride >= 32, or one row for all n items (shape (1, 32),
    or expanded to (n, 32) with row stride 0)."""
    if not t.is_cuda:
        raise ValueError("device API needs tensors in device memory")
    if t.dim() != 2 or t.shape[1] < 32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name} must be an (n, 32) uint8 matrix with contiguous rows")
    if t.shape[0] == 1 or (t.shape[0] == n and t.stride(0) == 0):
        return t.data_ptr(), 0
    if t.shape[0] != n or t.stride(0) < 32:
        raise ValueError(f"{name} must hold {n} rows (or one row for all) at a stride of at least 32")
    return t.data_ptr(), t.stride(0)


def _x25519_args(scalars, points, point_off, n):
    _check_u8(scalars, points)
    p_sc, s_sc = _x25519_rows("scalars", scalars, n)
    if point_off is not None:
        if points is None:
            raise ValueError("point_off needs points")
        _check_i64(n, point_off=point_off)
        return p_sc, s_sc, _p(points), 0, _p(point_off)
    if points is None:
        return p_sc, s_sc, None, 0, None
    p_pt, s_pt = _x25519_rows("points", points, n)
    return p_sc, s_sc, p_pt, s_pt, None


def x25519(scalars, points, out, point_off=None, stream=None):
    """X25519 over device rows (RNS/Cryptography/X25519.py:49-93): row i of
    out (n, >=32 uint8, any row stride) = X25519(scalars[i], points[i]).
    scalars and points are (n, 32) uint8 rows at any stride >= 32, or one row
    for all (shape (1, 32) or expanded with stride 0: the receiver's key, the
    sender's target key); points None is the base point (public keys); with
    point_off ((n,) int64) points is a flat byte buffer and point i the 32
    bytes at points[point_off[i]:], e.g. the head of each token."""
    _check_u8(out)
    if out.dim() != 2 or out.shape[1] < 32 or (out.shape[1] > 1 and out.stride(1) != 1) or \
            (out.shape[0] > 1 and out.stride(0) < 32):
        raise ValueError("out must be an (n, >=32) uint8 matrix with contiguous rows")
    n = out.shape[0]
    sc, sc_stride, pt, pt_stride, off = _x25519_args(scalars, points, point_off, n)
    lib = _native.load()
    ctx = _native.context(out.device.index)
    _native.check(lib.rt_x25519(ctx, sc, sc_stride, pt, pt_stride, off, _p_rows(out), max(out.stride(0), 32), n,
                                _stream(stream, out.device)))


def derive_keyset_x25519(scalars, points, salt=None, context=None, key_len=64, point_off=None, n=None, stream=None):
    """Identity's per-packet keying from the exchange on (Identity.py:812-829,
    861-871): KeySet whose key i is Token(hkdf(key_len, X25519(scalars[i],
    points[i]), salt[i], context)) for i < n; scalars, points and point_off
    as :func:`x25519`, salt and context as :func:`derive_keyset`.  n defaults
    to the number of offsets, else of scalar or point rows.  The shared
    secrets and the derived keys stay on the device."""
    if key_len not in (32, 64):
        raise ValueError("Token key must be 128 or 256 bits, not " + str(key_len * 8))
    _check_u8(salt, context)
    if n is None:
        n = point_off.numel() if point_off is not None else \
            max(scalars.shape[0], points.shape[0] if points is not None else 1)
    sc, sc_stride, pt, pt_stride, off = _x25519_args(scalars, points, point_off, n)
    if salt is not None and (salt.dim() != 2 or salt.shape[0] != n):
        raise ValueError(f"salt must be an ({n}, S) uint8 matrix (one row may be expanded)")
    lib = _native.load()
    ctx = _native.context(scalars.device.index)
    _order_after_current(stream, scalars, points, point_off, salt, context)
    h = lib.rt_keyset_create_x25519(ctx, sc, sc_stride, pt, pt_stride, off, _p_salt(salt),
                                    salt.stride(0) if salt is not None else 0,
                                    salt.shape[1] if salt is not None else 0, _p(context),
                                    context.numel() if context is not None else 0, key_len, n,
                                    _stream(stream, scalars.device))
    if not h:
        raise _native.NativeError(-1, _native.last_error())
    return KeySet._adopt(h, key_len, n, lib, ctx)


def map_hashes(data, out, salts, part_off=None, part_len=None, part_res=None, sdu=464, guard=0,
               first_collision=None, stream=None):
    """Resource map hashes over device buffers (Resource.py:505-506): out
    (n_parts*4,) uint8; salts (n_res, S) uint8 (random hashes); with
    part_off (int64) / part_len (int32) the parts are arbitrary slices of
    ``data`` and part_res (int32) names each part's resource, otherwise
    ``data`` is one resource cut into ``sdu``-byte parts.  first_collision
    (n_res,) int32 receives the first part index repeating a map hash of the
    previous ``guard`` parts, or -1."""
    _check_u8(data, out, salts)
    n_parts = out.numel() // 4
    lib = _native.load()
    ctx = _native.context(data.device.index)
    _native.check(lib.rt_map_hashes(ctx, _p(data), _p(part_off), _p(part_len), data.numel(), sdu, _p(salts),
                                    salts.shape[1], _p(part_res), salts.shape[0], guard, _p(out),
                                    _p(first_collision), n_parts, _stream(stream, data.device)))


def resource_hashes(data, seg_off, seg_len, random_hashes, hash_out, proof_out=None, expect_hash=None, status=None,
                    stream=None):
    """Resource integrity hash and proof over device buffers (Resource.py:
    436-439, 698-699, 759-760), one pass per segment: segment i is
    data[seg_off[i] : seg_off[i] + seg_len[i]] (seg_off (n,) int64, seg_len
    (n,) int32, any alignment, 0 allowed); hash_out (n, 32) uint8 receives
    SHA-256(segment || random_hashes[i]) and proof_out (n, 32) SHA-256(segment
    || hash).  random_hashes is (n, R) uint8 with R <= 32.  With expect_hash
    (n, 32) (receiver) status (n,) int32 receives 0 where the hash matches and
    1 where it does not (CORRUPT), the proof is taken over expect_hash and is
    32 zero bytes for a corrupt segment."""
    _check_u8(data, random_hashes, hash_out, proof_out, expect_hash)
    n = seg_off.numel()
    if seg_off.dtype != torch.int64:
        raise ValueError("seg_off must be int64")
    _check_i32(n, seg_len=seg_len, status=status)
    if random_hashes.dim() != 2 or random_hashes.shape[0] != n or random_hashes.shape[1] > 32:
        raise ValueError("random_hashes must be (n, R) with R <= 32")
    for name, t in (("hash_out", hash_out), ("proof_out", proof_out), ("expect_hash", expect_hash)):
        if t is not None and t.numel() != 32 * n:
            raise ValueError(f"{name} must hold n x 32 bytes")
    if expect_hash is not None and status is None:
        raise ValueError("expect_hash needs a status tensor")
    lib = _native.load()
    rh_len = random_hashes.shape[1]
    _native.check(lib.rt_resource_hashes(_native.context(data.device.index), _p(data), _p(seg_off), _p(seg_len),
                                         _p(random_hashes) if rh_len else None, rh_len, _p(expect_hash), _p(hash_out),
                                         _p(proof_out), _p(status), n, _stream(stream, data.device)))


# ------------------------------------------------------------------ Ed25519 --
# Device-resident forms of reticulum_amd.ed25519 (ed25519_kernels.hip): rows as
# in x25519, messages as a flat uint8 buffer with int64 offsets and int32
# lengths like the wire functions; enqueued on the stream, no sync.

def _ed_rows(name, t, n, width):
    """(pointer, row stride) of `width`-byte rows at any stride >= width, or
    one row for all n items (shape (1, width), or expanded with stride 0)."""
    if not t.is_cuda:
        raise ValueError("device API needs tensors in device memory")
    if t.dim() != 2 or t.shape[1] < width or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name} must be an (n, {width}) uint8 matrix with contiguous rows")
    if t.shape[0] == 1 or (t.shape[0] == n and t.stride(0) == 0):
        return t.data_ptr(), 0
    if t.shape[0] != n or t.stride(0) < width:
        raise ValueError(f"{name} must hold {n} rows (or one row for all) at a stride of at least {width}")
    return t.data_ptr(), t.stride(0)


def _ed_msgs(msgs, msg_off, msg_len, n):
    _check_u8(msgs)
    _check_i64(n, msg_off=msg_off)
    _check_i32(n, msg_len=msg_len)
    if msg_off is None or msg_len is None:
        raise ValueError("msg_off and msg_len are required")
    return (_p(msgs) if msgs is not None and msgs.numel() else None), _p(msg_off), _p(msg_len)


def ed25519_verify(public_keys, signatures, msgs, msg_off, msg_len, ok, stream=None):
    """Ed25519 verification over device rows (pure25519/eddsa.py checkvalid):
    ok[i] ((n,) uint8) = 1 where signatures[i] ((n, 64) rows at any stride
    >= 64) is public_keys[i]'s ((n, 32) rows, or one row for all) signature of
    the msg_len[i] bytes at msgs[msg_off[i]:], else 0.  msgs None or empty:
    every message is empty."""
    _check_u8(public_keys, signatures, ok)
    n = ok.numel()
    if not ok.is_contiguous():
        raise ValueError("ok must be a contiguous (n,) uint8 tensor")
    pk, pk_stride = _ed_rows("public_keys", public_keys, n, 32)
    sg, sg_stride = _ed_rows("signatures", signatures, n, 64)
    if n > 1 and sg_stride == 0:
        raise ValueError("signatures must hold one row per item")
    m, off, ln = _ed_msgs(msgs, msg_off, msg_len, n)
    lib = _native.load()
    ctx = _native.context(ok.device.index)
    _native.check(lib.rt_ed25519_verify(ctx, pk, pk_stride, sg, max(sg_stride, 64), m, off, ln, _p(ok), n,
                                        _stream(stream, ok.device)))


def ed25519_sign(seeds, msgs, msg_off, msg_len, out, public_keys=None, stream=None):
    """Ed25519 signatures over device rows (pure25519/eddsa.py signature): row
    i of out ((n, >=64) uint8, any row stride) = the signature of message i
    under seeds[i] ((n, 32) rows, or one row for all).  public_keys (the
    seeds', trusted) spares the kernel their derivation."""
    _check_u8(seeds, out, public_keys)
    if out.dim() != 2 or out.shape[1] < 64 or (out.shape[1] > 1 and out.stride(1) != 1) or \
            (out.shape[0] > 1 and out.stride(0) < 64):
        raise ValueError("out must be an (n, >=64) uint8 matrix with contiguous rows")
    n = out.shape[0]
    sd, sd_stride = _ed_rows("seeds", seeds, n, 32)
    pk, pk_stride = (None, 0) if public_keys is None else _ed_rows("public_keys", public_keys, n, 32)
    m, off, ln = _ed_msgs(msgs, msg_off, msg_len, n)
    lib = _native.load()
    ctx = _native.context(out.device.index)
    _native.check(lib.rt_ed25519_sign(ctx, sd, sd_stride, pk, pk_stride, m, off, ln, _p_rows(out),
                                      max(out.stride(0), 64), n, _stream(stream, out.device)))


def ed25519_public(seeds, out, stream=None):
    """Ed25519 public keys over device rows: row i of out ((n, >=32) uint8, any
    row stride) = the public key of seeds[i]."""
    _check_u8(seeds, out)
    if out.dim() != 2 or out.shape[1] < 32 or (out.shape[1] > 1 and out.stride(1) != 1) or \
            (out.shape[0] > 1 and out.stride(0) < 32):
        raise ValueError("out must be an (n, >=32) uint8 matrix with contiguous rows")
    n = out.shape[0]
    sd, sd_stride = _ed_rows("seeds", seeds, n, 32)
    lib = _native.load()
    ctx = _native.context(out.device.index)
    _native.check(lib.rt_ed25519_public(ctx, sd, sd_stride, _p_rows(out), max(out.stride(0), 32), n,
                                        _stream(stream, out.device)))


# ---------------------------------------------------------------- wire side --
# Device-resident forms of reticulum_amd.wire (wire_kernels.hip): flat uint8
# buffers, int64 offsets, int32 lengths, enqueued on the stream, no sync.

def _ctx_of(t):
    return _native.context(t.device.index)


def hdlc_frame(pkt, pkt_off, pkt_len, out, frame_off, workspace=None, stream=None):
    """HDLC framing (TCPInterface.py:44-53, 323) of n packets into ``out`` in
    order: frame i = 7E || escape(packet i) || 7E at out[frame_off[i]:
    frame_off[i+1]]; frame_off (n+1,) int64, frame_off[n] = total bytes; out
    needs sum(2*len+2) bytes at most."""
    _check_u8(pkt, out)
    n = pkt_off.numel()
    if pkt_len.numel() != n or frame_off.numel() != n + 1:
        raise ValueError("shape mismatch")
    lib = _native.load()
    ws = workspace if workspace is not None else torch.empty(
        int(lib.rt_hdlc_frame_workspace_bytes(n)), dtype=torch.uint8, device=pkt.device)
    _native.check(lib.rt_hdlc_frame(_ctx_of(pkt), _p(pkt), _p(pkt_off), _p(pkt_len), n, _p(out), _p(frame_off),
                                    _p(ws), _stream(stream, pkt.device)))


def hdlc_frame_counted(pkt, pkt_off, pkt_len, n_dev, out, frame_off, workspace=None, stream=None):
    """hdlc_frame with the packet count on the device: only the first
    min(n_dev, n) entries are packets (``n_dev``: an int64 device tensor whose
    first element is the count, e.g. reply_gather's reply_counts).  The
    entries past it contribute no bytes whatever their length says, and their
    frame_off all equal frame_off[n], so out[:frame_off[n]] is exactly the
    counted frames.  n = 0 gives frame_off[0] = 0."""
    _check_u8(pkt, out)
    n = pkt_off.numel()
    _check_i64(n, pkt_off=pkt_off)
    _check_i32(n, pkt_len=pkt_len)
    _check_i64(n + 1, frame_off=frame_off)
    if n_dev is None or n_dev.dtype != torch.int64 or n_dev.numel() < 1 or not n_dev.is_contiguous():
        raise ValueError("n_dev must be a contiguous int64 device tensor")
    lib = _native.load()
    ws = workspace if workspace is not None else torch.empty(
        int(lib.rt_hdlc_frame_workspace_bytes(n)), dtype=torch.uint8, device=pkt.device)
    if ws.numel() < int(lib.rt_hdlc_frame_workspace_bytes(n)):
        raise ValueError("workspace is smaller than rt_hdlc_frame_workspace_bytes(n)")
    _native.check(lib.rt_hdlc_frame_counted(_ctx_of(pkt), _p(pkt), _p(pkt_off), _p(pkt_len), n, _p(n_dev), _p(out),
                                            _p(frame_off), _p(ws), _stream(stream, pkt.device)))


def deframe_slots_bytes(nbytes, max_pairs):
    """Output capacity hdlc_deframe needs with ``line_phase`` (slots)."""
    return int(nbytes) + LINE * (int(max_pairs) + 1)


def hdlc_deframe(buf, out, frame_off, frame_len, status, counts, hw_mtu=262144, ifac_size=0, workspace=None,
                 stream=None, line_phase=None):
    """One pass of the HDLC read loop (TCPInterface.py:387-410) over ``buf``:
    for each consecutive flag pair k (at most frame_off.numel() pairs) the
    unescaped frame at out[frame_off[k]: frame_off[k] + frame_len[k]] with its
    RT_FRAME_* status; counts (2,) int64 = [pairs, bytes consumed].  With
    ``line_phase`` (0..127) each frame gets a 128-B-aligned slot whose byte
    line_phase starts a line (rt_hdlc_deframe_slots; ``out`` then needs
    deframe_slots_bytes(len(buf), max_pairs) bytes), else it sits at its
    position in buf."""
    _check_u8(buf, out)
    max_pairs = frame_off.numel()
    need = buf.numel() if line_phase is None else deframe_slots_bytes(buf.numel(), max_pairs)
    if frame_len.numel() != max_pairs or status.numel() != max_pairs or counts.numel() < 2 or out.numel() < need:
        raise ValueError("shape mismatch")
    lib = _native.load()
    ws = workspace if workspace is not None else torch.empty(
        int(lib.rt_hdlc_deframe_workspace_bytes(buf.numel())), dtype=torch.uint8, device=buf.device)
    if line_phase is None:
        _native.check(lib.rt_hdlc_deframe(_ctx_of(buf), _p(buf), buf.numel(), hw_mtu, ifac_size, _p(out),
                                          _p(frame_off), _p(frame_len), _p(status), _p(counts), max_pairs, _p(ws),
                                          _stream(stream, buf.device)))
    else:
        _native.check(lib.rt_hdlc_deframe_slots(_ctx_of(buf), _p(buf), buf.numel(), hw_mtu, ifac_size, int(line_phase),
                                                _p(out), _p(frame_off), _p(frame_len), _p(status), _p(counts),
                                                max_pairs, _p(ws), _stream(stream, buf.device)))


def frames_compact(frame_off, frame_len, status, counts, f_off, f_len, frame_pair, n_frames, workspace=None,
                   stream=None):
    """The frames an hdlc_deframe pass hands on (pair k < counts[0] with
    status RT_FRAME_OK; TCPInterface.py:391-401), in stream order, to the
    front of f_off (int64) / f_len (int32) / frame_pair (int64, the pair
    index); n_frames (a 0-d int64 device tensor) gets their number, and the
    entries past it are f_off 0, f_len 0, frame_pair -1.  All arrays have
    max_pairs = frame_off.numel() entries."""
    max_pairs = frame_off.numel()
    if any(t.numel() != max_pairs for t in (frame_len, status, f_off, f_len, frame_pair)) or \
            counts.numel() < 2 or n_frames.numel() != 1:
        raise ValueError("shape mismatch")
    if frame_off.dtype != torch.int64 or f_off.dtype != torch.int64 or frame_pair.dtype != torch.int64 or \
            n_frames.dtype != torch.int64 or frame_len.dtype != torch.int32 or f_len.dtype != torch.int32 or \
            status.dtype != torch.int32 or counts.dtype != torch.int64:
        raise TypeError("frames_compact: int64 offsets/pairs/counts, int32 lengths/status")
    lib = _native.load()
    ws = workspace if workspace is not None else torch.empty(
        max(1, int(lib.rt_frames_compact_workspace_bytes(max_pairs))), dtype=torch.uint8, device=frame_off.device)
    _native.check(lib.rt_frames_compact(_ctx_of(frame_off), _p(frame_off), _p(frame_len), _p(status), _p(counts),
                                        max_pairs, _p(f_off), _p(f_len), _p(frame_pair), _p(n_frames), _p(ws),
                                        _stream(stream, frame_off.device)))


def token_spans(fields, pkt_off, tok_off, tok_len, stream=None):
    """Packet.unpack's data (Packet.py:262-275), the token of each packet:
    tok_off[i] = pkt_off[i] + data_offset, tok_len[i] = data_len where
    fields[i] (an rt_packet_fields record from packet_unpack) is ok, else
    pkt_off[i] and 0.  int64 offsets, int32 lengths."""
    n = pkt_off.numel()
    if fields.numel() != 96 * n or tok_off.numel() != n or tok_len.numel() != n:
        raise ValueError("shape mismatch")
    if pkt_off.dtype != torch.int64 or tok_off.dtype != torch.int64 or tok_len.dtype != torch.int32:
        raise TypeError("token_spans: int64 offsets, int32 lengths")
    lib = _native.load()
    _native.check(lib.rt_token_spans(_ctx_of(fields), _p(fields), _p(pkt_off), n, _p(tok_off), _p(tok_len),
                                     _stream(stream, fields.device)))


# Link table (link_kernels.hip): ``tab`` is an rt_linktable handle, as
# reticulum_amd.link.LinkTable holds it; ids are (n, 16) uint8 rows.

LINK_OK, LINK_DUPLICATE, LINK_FULL, LINK_MISSING = 0, 1, 2, 3       # RT_LINK_* (include/rnstok.h)
ROUTE_NOT_LINK, ROUTE_NO_LINK, ROUTE_LINK_PLAIN, ROUTE_LINK_DECRYPT = 0, 1, 2, 3    # RT_ROUTE_*


def _link_ids(ids):
    _check_u8(ids)
    if ids.dim() != 2 or ids.shape[1] != 16 or not ids.is_contiguous():
        raise ValueError("link ids must be a contiguous (n, 16) uint8 tensor")
    return ids.shape[0]


def linktable_insert(tab, ids, values, status, stream=None):
    """Enter ids[i] -> values[i] ((n,) int32, read as uint32); status (n,)
    int32 receives LINK_OK, LINK_DUPLICATE (present already, or at a lower
    index of this batch: the earlier one stays) or LINK_FULL."""
    n = _link_ids(ids)
    _check_i32(n, values=values, status=status)
    if values is None or status is None:
        raise ValueError("values and status are required")
    _native.check(_native.load().rt_linktable_insert(tab, _p(ids), _p(values), _p(status), n,
                                                     _stream(stream, ids.device)))


def linktable_remove(tab, ids, status, stream=None):
    """Remove ids[i]; status (n,) int32 receives LINK_OK or LINK_MISSING."""
    n = _link_ids(ids)
    _check_i32(n, status=status)
    if status is None:
        raise ValueError("status is required")
    _native.check(_native.load().rt_linktable_remove(tab, _p(ids), _p(status), n, _stream(stream, ids.device)))


def linktable_lookup(tab, ids, values_out, found_out, stream=None):
    """values_out[i] ((n,) int32) = the value of ids[i], -1 on a miss;
    found_out[i] ((n,) uint8) = 1 / 0."""
    n = _link_ids(ids)
    _check_i32(n, values_out=values_out)
    _check_u8(found_out)
    if values_out is None or found_out is None or found_out.numel() != n or not found_out.is_contiguous():
        raise ValueError(f"values_out must be ({n},) int32 and found_out a contiguous ({n},) uint8 tensor")
    _native.check(_native.load().rt_linktable_lookup(tab, _p(ids), _p(values_out), _p(found_out), n,
                                                     _stream(stream, ids.device)))


def linktable_count(tab, count_out, stream=None):
    """count_out (a one-element int32 device tensor) = entries present."""
    _check_i32(1, count_out=count_out)
    if count_out is None:
        raise ValueError("count_out is required")
    _native.check(_native.load().rt_linktable_count(tab, _p(count_out), _stream(stream, count_out.device)))


def link_spans(tab, fields, pkt_off, n_keys, tok_off, tok_len, key_idx, link, route, stream=None):
    """token_spans plus the link dispatch (Transport.py:2161-2176,
    Link.py:941-1148) over packet_unpack's records: route[i] ((n,) uint8) is
    ROUTE_NOT_LINK, ROUTE_NO_LINK, ROUTE_LINK_PLAIN or ROUTE_LINK_DECRYPT,
    link[i] ((n,) int32) the table's value for the packet's destination hash
    or -1; where the route is ROUTE_LINK_DECRYPT tok_off[i] / tok_len[i] are
    the packet's data and key_idx[i] ((n,) int32) the value, elsewhere the
    span is empty at pkt_off[i] and key_idx 0.  ``n_keys`` is the size of the
    key set the batch is decrypted with: a link whose value is not below it is
    never decrypted."""
    n = pkt_off.numel()
    if fields.numel() != 96 * n or route.numel() != n:
        raise ValueError("shape mismatch")
    _check_u8(fields, route)
    _check_i64(n, pkt_off=pkt_off, tok_off=tok_off)
    _check_i32(n, tok_len=tok_len, key_idx=key_idx, link=link)
    if any(t is None for t in (tok_off, tok_len, key_idx, link)):
        raise ValueError("tok_off, tok_len, key_idx and link are required")
    if not 0 <= int(n_keys) <= 0xFFFFFFFF:
        raise ValueError("n_keys must be a uint32")
    _native.check(_native.load().rt_link_spans(tab, _p(fields), _p(pkt_off), n, int(n_keys), _p(tok_off), _p(tok_len),
                                               _p(key_idx), _p(link), _p(route), _stream(stream, fields.device)))


# Packet hash list and packet filter (filter_kernels.hip): ``lst`` is an
# rt_hashlist handle, as reticulum_amd.filter.PacketHashlist holds it; hashes
# are (n, 32) uint8 rows.

FILTER_PASS, FILTER_NO_PACKET, FILTER_OTHER_TRANSPORT = 0, 1, 2       # RT_FILTER_* (include/rnstok.h)
FILTER_BAD_ANNOUNCE, FILTER_HOPS, FILTER_DUPLICATE = 3, 4, 5
HASHLIST_ABSENT, HASHLIST_CURRENT, HASHLIST_PREVIOUS = 0, 1, 2


def _packet_hashes(hashes):
    _check_u8(hashes)
    if hashes.dim() != 2 or hashes.shape[1] != 32 or not hashes.is_contiguous():
        raise ValueError("packet hashes must be a contiguous (n, 32) uint8 tensor")
    return hashes.shape[0]


def packet_filter(lst, fields, transport_identity, status, transit=None, stream=None):
    """Transport.packet_filter and the remember step of Transport.inbound
    (Transport.py:1377-1427, 1525-1545) over packet_unpack's records, as if the
    packets came one after another in index order: status[i] ((n,) int32) is
    FILTER_PASS or the rule that dropped the packet, a dropped packet's
    fields[i].ok becomes 0, and every packet that passes is entered into the
    list's current generation unless it is a link request proof or its
    destination hash is in ``transit`` (an rt_linktable handle, or None).
    ``transport_identity`` is the node's 16-byte transport id on the device."""
    _check_u8(fields, transport_identity)
    if fields.dim() != 2 or fields.shape[1] != 96 or not fields.is_contiguous():
        raise ValueError("fields must be a contiguous (n, 96) uint8 tensor")
    n = fields.shape[0]
    if transport_identity.numel() != 16 or not transport_identity.is_contiguous():
        raise ValueError("transport_identity must be 16 contiguous bytes")
    _check_i32(n, status=status)
    if status is None:
        raise ValueError("status is required")
    _native.check(_native.load().rt_packet_filter(lst, transit, _p(transport_identity), _p(fields), n, _p(status),
                                                  _stream(stream, fields.device)))


def hashlist_cull(lst, device, stream=None):
    """The job loop's step (Transport.py:656-658): the current generation
    becomes the previous one when it holds more than max_hashes // 2 entries.
    Decided on the device; nothing is read back."""
    _native.check(_native.load().rt_hashlist_cull(lst, _stream(stream, device)))


def hashlist_add(lst, hashes, stream=None):
    """Enter hashes[i] into the current generation (Transport.add_packet_hash)."""
    n = _packet_hashes(hashes)
    _native.check(_native.load().rt_hashlist_add(lst, _p(hashes), n, _stream(stream, hashes.device)))


def hashlist_remove(lst, hashes, status, stream=None):
    """Remove hashes[i] from the current generation; status (n,) int32
    receives LINK_OK or LINK_MISSING."""
    n = _packet_hashes(hashes)
    _check_i32(n, status=status)
    if status is None:
        raise ValueError("status is required")
    _native.check(_native.load().rt_hashlist_remove(lst, _p(hashes), n, _p(status), _stream(stream, hashes.device)))


def hashlist_contains(lst, hashes, found_out, stream=None):
    """found_out[i] ((n,) uint8) = HASHLIST_ABSENT, HASHLIST_CURRENT or
    HASHLIST_PREVIOUS (in the previous generation only)."""
    n = _packet_hashes(hashes)
    _check_u8(found_out)
    if found_out is None or found_out.numel() != n or not found_out.is_contiguous():
        raise ValueError(f"found_out must be a contiguous ({n},) uint8 tensor")
    _native.check(_native.load().rt_hashlist_contains(lst, _p(hashes), n, _p(found_out),
                                                      _stream(stream, hashes.device)))


def hashlist_counts(lst, out, stream=None):
    """out (a three-element int32 device tensor) = entries in the current
    generation, in the previous one, and the overflow count."""
    _check_i32(3, out=out)
    if out is None:
        raise ValueError("out is required")
    _native.check(_native.load().rt_hashlist_counts(lst, _p(out), _stream(stream, out.device)))


# Announce validation (announce_kernels.hip)

ANNOUNCE_VALID, ANNOUNCE_NOT_ANNOUNCE, ANNOUNCE_SHORT = 0, 1, 2       # RT_ANNOUNCE_* (include/rnstok.h)
ANNOUNCE_BAD_SIGNATURE, ANNOUNCE_BAD_DESTINATION = 3, 4


def announce_validate(pkt, pkt_off, fields, status, identity_hash=None, stream=None):
    """Identity.validate_announce (Identity.py:505-606) over packet_unpack's
    records, each announce read inside its packet pkt[pkt_off[i]:]: status[i]
    ((n,) int32) is ANNOUNCE_VALID, ANNOUNCE_NOT_ANNOUNCE (fields[i].ok is 0, or
    another packet type), ANNOUNCE_SHORT, ANNOUNCE_BAD_SIGNATURE or
    ANNOUNCE_BAD_DESTINATION (the signature holds, the destination hash is not
    this identity's).  validate_announce(only_validate_signature=True)
    (Transport.py:1748-1750) is true for VALID and BAD_DESTINATION, the full
    check (:1772) for VALID.  identity_hash ((n, 16) uint8, optional) receives
    the announced identity's hash where the signature was checked and zeros
    elsewhere: the handle for the caller's part (blackholed identities, the
    known-destination key check, Identity.remember, ratchets, ingress limits).
    Nothing is synchronised."""
    _check_u8(pkt, fields, identity_hash)
    if fields.dim() != 2 or fields.shape[1] != 96 or not fields.is_contiguous():
        raise ValueError("fields must be a contiguous (n, 96) uint8 tensor")
    n = fields.shape[0]
    if pkt.dim() != 1:
        raise ValueError("pkt must be a flat uint8 buffer")
    _check_i64(n, pkt_off=pkt_off)
    _check_i32(n, status=status)
    if pkt_off is None or status is None:
        raise ValueError("pkt_off and status are required")
    if identity_hash is not None and (identity_hash.dim() != 2 or identity_hash.shape != (n, 16)
                                      or not identity_hash.is_contiguous()):
        raise ValueError(f"identity_hash must be a contiguous ({n}, 16) uint8 tensor")
    if not pkt.is_cuda or not pkt.is_contiguous():
        raise ValueError("device API needs contiguous tensors in device memory")
    for t in (pkt_off, fields, status, identity_hash):
        if t is not None and t.device != pkt.device:
            raise ValueError(f"every array must be on the packets' device {pkt.device}, one is on {t.device}")
    if n == 0:
        return
    lib = _native.load()
    _native.check(lib.rt_announce_validate(_ctx_of(pkt), _p(pkt), _p(pkt_off), _p(fields), n, _p(status),
                                           _p(identity_hash), _stream(stream, pkt.device)))


# Packet proofs on a link (proof_kernels.hip): ``signers`` is a
# reticulum_amd.proof.LinkSigners (or anything with its seeds, publics,
# peer_publics, flags and n_links), ``receipts`` a reticulum_amd.proof.ReceiptTable.

LINK_PROVE_ALL, LINK_HAS_CHANNEL = 1, 2                                 # RT_LINK_* flags (include/rnstok.h)
PROOF_DELIVERED, PROOF_NOT_PROOF, PROOF_NOT_LINK, PROOF_NO_LINK = 0, 1, 2, 3    # RT_PROOF_*
PROOF_SHORT, PROOF_NO_RECEIPT, PROOF_BAD_SIGNATURE = 4, 5, 6
PROOF_LEN = 115              # flags, hops, link id (16), context, packet hash (32), signature (64)


def _check_fields(fields):
    _check_u8(fields)
    if fields.dim() != 2 or fields.shape[1] != 96 or not fields.is_contiguous():
        raise ValueError("fields must be a contiguous (n, 96) uint8 tensor")
    return fields.shape[0]


def _same_device(dev, *ts):
    for t in ts:
        if t is not None and t.device != dev:
            raise ValueError(f"every array must be on one device: {dev} and {t.device}")


def link_prove(fields, route, link, status, signers, proofs, proof_len, stream=None):
    """Link.receive's packet.prove() (Link.py:943-955, 1140-1145, 378-389) over
    packet_unpack's records, link_spans' ``route`` ((n,) uint8) and ``link``
    ((n,) int32) and the decrypt's token ``status`` ((n,) int32).  Record i is
    proved when it is an ok DATA packet with 0 <= link[i] < signers.n_links and
    either its context is NONE, its route ROUTE_LINK_DECRYPT, its token status
    0 and the link's flags have LINK_PROVE_ALL, or its context is CHANNEL and
    the flags have LINK_HAS_CHANNEL (whatever the token status).  Then
    proof_len[i] ((n,) int32) = 115 and row i of ``proofs`` ((n, >=115) uint8 at
    any row stride) is the LINK PROOF packet the reference sends: 0x0F, hops 0,
    the link id, context 0, the packet hash and its signature under the link's
    seed (ed25519_sign's, bit for bit).  Elsewhere proof_len[i] = 0 and the
    row is not written.  Nothing is synchronised."""
    n = _check_fields(fields)
    _check_u8(route, proofs, signers.seeds, signers.publics, signers.flags)
    if route.numel() != n or not route.is_contiguous():
        raise ValueError(f"route must be a contiguous ({n},) uint8 tensor")
    _check_i32(n, link=link, status=status, proof_len=proof_len)
    if link is None or status is None or proof_len is None:
        raise ValueError("link, status and proof_len are required")
    _check_rows("proofs", proofs, n, PROOF_LEN)
    n_links = int(signers.n_links)
    sd, stride = _ed_rows("signers.seeds", signers.seeds, n_links, 32)
    pk, pk_stride = _ed_rows("signers.publics", signers.publics, n_links, 32)
    if pk_stride != stride:
        raise ValueError("signers.seeds and signers.publics must have the same rows")
    if signers.flags.numel() != n_links or not signers.flags.is_contiguous():
        raise ValueError(f"signers.flags must be a contiguous ({n_links},) uint8 tensor")
    _same_device(fields.device, route, link, status, proofs, proof_len, signers.seeds, signers.publics, signers.flags)
    if n == 0:
        return
    _native.check(_native.load().rt_link_prove(_ctx_of(fields), _p(fields), _p(route), _p(link), _p(status), sd, pk,
                                               stride, _p(signers.flags), n_links, _p_rows(proofs),
                                               max(proofs.stride(0), PROOF_LEN), _p(proof_len), n,
                                               _stream(stream, fields.device)))


def receipt_store(receipts, hashes, ids, status, stream=None):
    """The second half of ReceiptTable.add: receipts.hashes[ids[i]] = hashes[i]
    ((n, 32) uint8) where the insert's status[i] is LINK_OK."""
    n = _packet_hashes(hashes)
    _check_i32(n, ids=ids, status=status)
    if ids is None or status is None:
        raise ValueError("ids and status are required")
    _same_device(hashes.device, ids, status, receipts.hashes)
    _native.check(_native.load().rt_receipt_store(receipts.handle, _p(receipts.hashes), receipts.max_receipts,
                                                  _p(hashes), _p(ids), _p(status), n,
                                                  _stream(stream, hashes.device)))


def proof_settle(pkt, pkt_off, fields, link, signers, receipts, proof_status, receipt, stream=None):
    """The receipts' branch of Transport.inbound's PROOF handling
    (Transport.py:2326-2363, Packet.py:434-459) over packet_unpack's records,
    each proof read inside its packet pkt[pkt_off[i]:], as if the packets came
    one after another in index order.  ``link`` is link_spans' ((n,) int32),
    ``signers.peer_publics`` the links' peer signing keys, ``receipts`` a
    ReceiptTable.  proof_status[i] ((n,) int32) is PROOF_NOT_PROOF (not ok, no
    PROOF, or context LRPROOF / RESOURCE_PRF), PROOF_NOT_LINK, PROOF_NO_LINK,
    PROOF_SHORT (data under 96 bytes), PROOF_NO_RECEIPT (no receipt holds
    data[:32], or a lower index of the batch delivered it),
    PROOF_BAD_SIGNATURE, or PROOF_DELIVERED; receipt[i] ((n,) int32) is the
    delivered receipt's id, which leaves the table inside the call, and -1
    elsewhere.  Nothing is synchronised."""
    n = _check_fields(fields)
    _check_u8(pkt, signers.peer_publics)
    if pkt.dim() != 1 or not pkt.is_cuda or not pkt.is_contiguous():
        raise ValueError("pkt must be a flat contiguous uint8 buffer in device memory")
    _check_i64(n, pkt_off=pkt_off)
    _check_i32(n, link=link, proof_status=proof_status, receipt=receipt)
    if pkt_off is None or link is None or proof_status is None or receipt is None:
        raise ValueError("pkt_off, link, proof_status and receipt are required")
    n_links = int(signers.n_links)
    pp = signers.peer_publics
    if pp.dim() != 2 or pp.shape != (n_links, 32) or not pp.is_contiguous():
        raise ValueError(f"signers.peer_publics must be a contiguous ({n_links}, 32) uint8 tensor")
    _same_device(pkt.device, pkt_off, fields, link, proof_status, receipt, pp, receipts.hashes)
    if n == 0:
        return
    _native.check(_native.load().rt_proof_settle(receipts.handle, _p(receipts.hashes), receipts.max_receipts, _p(pkt),
                                                 _p(pkt_off), _p(fields), _p(link), _p(pp), n_links, _p(proof_status),
                                                 _p(receipt), n, _stream(stream, pkt.device)))


# Proofs for packets sent to SINGLE destinations (dproof_kernels.hip):
# ``receipts`` is a reticulum_amd.proof.DestinationReceipts.

DPROOF_DELIVERED, DPROOF_NOT_PROOF, DPROOF_ON_LINK, DPROOF_BAD_LENGTH = 0, 1, 2, 3      # RT_DPROOF_*
DPROOF_NO_RECEIPT, DPROOF_BAD_SIGNATURE, DPROOF_DEFERRED = 4, 5, 6


def _check_keyed_receipts(r):
    m = r.max_receipts
    _check_u8(r.hashes, r.keys, r.keyed)
    for name, t, shape in (("hashes", r.hashes, (m, 32)), ("keys", r.keys, (m, 32)), ("keyed", r.keyed, (m,))):
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"receipts.{name} must be a contiguous {shape} uint8 tensor")


def receipt_store_keyed(receipts, hashes, keys, ids, status, stream=None):
    """The second half of DestinationReceipts.add: where the insert's status[i]
    is LINK_OK, receipts.hashes[ids[i]] = hashes[i] ((n, 32) uint8),
    receipts.keys[ids[i]] = keys[i] ((n, 32) uint8) and receipts.keyed[ids[i]]
    = 1; with ``keys`` None the key row is left alone and keyed is 0."""
    n = _packet_hashes(hashes)
    _check_i32(n, ids=ids, status=status)
    if ids is None or status is None:
        raise ValueError("ids and status are required")
    if keys is not None:
        _check_u8(keys)
        if keys.dim() != 2 or tuple(keys.shape) != (n, 32) or not keys.is_contiguous():
            raise ValueError(f"keys must be a contiguous ({n}, 32) uint8 tensor")
    _check_keyed_receipts(receipts)
    _same_device(hashes.device, keys, ids, status, receipts.hashes, receipts.keys, receipts.keyed)
    _native.check(_native.load().rt_receipt_store_keyed(receipts.handle, _p(receipts.hashes), _p(receipts.keys),
                                                        _p(receipts.keyed), receipts.max_receipts, _p(hashes),
                                                        _p(keys), _p(ids), _p(status), n,
                                                        _stream(stream, hashes.device)))


def destination_proof_settle(pkt, pkt_off, fields, receipts, dproof_status, receipt, link=None, n_links=0,
                             stream=None):
    """Transport.inbound's PROOF handling for a proof that arrives on no active
    link (Transport.py:2326-2363, PacketReceipt.validate_proof,
    Packet.py:480-524) over packet_unpack's records, each proof read inside its
    packet pkt[pkt_off[i]:], as if the packets came one after another in index
    order.  ``receipts`` is a DestinationReceipts; ``link`` is link_spans'
    ((n,) int32) with ``n_links`` the number of active links, or None: no link
    is active.  dproof_status[i] ((n,) int32) is DPROOF_NOT_PROOF (not ok, no
    PROOF, or context LRPROOF / RESOURCE_PRF), DPROOF_ON_LINK (destination type
    LINK and 0 <= link[i] < n_links: proof_settle's), DPROOF_BAD_LENGTH (data
    of neither 64 nor 96 bytes), DPROOF_NO_RECEIPT (explicit: no keyed receipt
    holds data[:32]; implicit: no keyed receipt validates; either: a lower
    index of the batch delivered it), DPROOF_BAD_SIGNATURE (explicit only),
    DPROOF_DEFERRED (an implicit proof that had to be tried against the whole
    table and whose frame did not fit receipts.scan_trials, as every such
    proof behind it) or DPROOF_DELIVERED; receipt[i] ((n,) int32) is the
    delivered receipt's id, which leaves the table inside the call, and -1
    elsewhere.  Nothing is synchronised."""
    n = _check_fields(fields)
    _check_u8(pkt)
    if pkt.dim() != 1 or not pkt.is_cuda or not pkt.is_contiguous():
        raise ValueError("pkt must be a flat contiguous uint8 buffer in device memory")
    _check_i64(n, pkt_off=pkt_off)
    _check_i32(n, link=link, dproof_status=dproof_status, receipt=receipt)
    if pkt_off is None or dproof_status is None or receipt is None:
        raise ValueError("pkt_off, dproof_status and receipt are required")
    n_links = int(n_links) if link is not None else 0
    if n_links < 0:
        raise ValueError("n_links is not negative")
    _check_keyed_receipts(receipts)
    _same_device(pkt.device, pkt_off, fields, link, dproof_status, receipt, receipts.hashes, receipts.keys,
                 receipts.keyed)
    if n == 0:
        return
    work = receipts.work_for(n, stream=stream)
    _same_device(pkt.device, work)
    _native.check(_native.load().rt_destination_proof_settle(
        receipts.handle, _p(receipts.hashes), _p(receipts.keys), _p(receipts.keyed), receipts.max_receipts,
        int(receipts.scan_trials), _p(work), work.numel(), _p(pkt), _p(pkt_off), _p(fields), _p(link), n_links,
        _p(dproof_status), _p(receipt), n, _stream(stream, pkt.device)))


# Link requests (linkreq_kernels.hip): ``destinations`` is a
# reticulum_amd.link.LinkDestinations, ``links`` a LinkTable, ``signers`` a
# reticulum_amd.proof.LinkSigners or None.

LINKREQ_ACCEPTED, LINKREQ_NOT_REQUEST, LINKREQ_OTHER_TRANSPORT = 0, 1, 2      # RT_LINKREQ_* (include/rnstok.h)
LINKREQ_NO_DESTINATION, LINKREQ_NOT_ACCEPTING, LINKREQ_BAD_SIZE, LINKREQ_BAD_MODE = 3, 4, 6, 7
LINKREQ_DUPLICATE, LINKREQ_NO_SLOT = 8, 9
DEST_ACCEPTS = 4             # RT_DEST_ACCEPTS, beside LINK_PROVE_ALL and LINK_HAS_CHANNEL
LRPROOF_LEN = 118            # flags, hops, link id (16), context, signature (64), pub (32), signalling (3)


def link_accept(ks: KeySet, links, destinations, transport_identity, pkt, pkt_off, fields, slots, ephemeral_privates,
                status, accepted, link_id, link_mtu, lr_proofs, lr_proof_len, nh_mtu=500, signers=None, stream=None):
    """The responder side of link establishment (Transport.py:2127-2158,
    Destination.py:414-435, Link.py:186-227, 336-376) over packet_unpack's
    records, each request read inside its packet pkt[pkt_off[i]:].  ``slots``
    ((m,) int32) is the caller's free list and ``ephemeral_privates`` ((m, 32)
    uint8) its randomness: valid request r in index order takes slots[r] and
    row r.  ``nh_mtu`` is the receiving interface's next-hop MTU
    (Transport.py:2138-2141), None for an interface without HW_MTU.

    status[i] ((n,) int32) is LINKREQ_ACCEPTED, NOT_REQUEST, OTHER_TRANSPORT,
    NO_DESTINATION, NOT_ACCEPTING, BAD_SIZE, BAD_MODE, DUPLICATE (the id is in
    ``links`` or at a lower index of the batch) or NO_SLOT; accepted[i] ((n,)
    int32) the slot or -1; link_id ((n, 16) uint8) and link_mtu ((n,) int32)
    are set for every valid request; row i of lr_proofs ((n, >=118) uint8 at
    any row stride) is the LRPROOF packet where lr_proof_len[i] ((n,) int32) is
    118, untouched where it is 0.  When the call has run, ``links`` maps each
    accepted id to its slot, record slot of ``ks`` (64-byte keys) is the
    link's handshake key, and with ``signers`` the slot's rows hold the peer's
    signing key, the destination's flags and (one row per link) its seed and
    public key.  Nothing is synchronised, and neither shared secrets nor
    derived keys leave the device."""
    n = _check_fields(fields)
    _check_u8(pkt, transport_identity, ephemeral_privates, link_id, lr_proofs)
    if ks.key_len != 64:
        raise ValueError("a link's key set holds 64-byte keys")
    if pkt.dim() != 1 or not pkt.is_cuda or not pkt.is_contiguous():
        raise ValueError("pkt must be a flat contiguous uint8 buffer in device memory")
    _check_i64(n, pkt_off=pkt_off)
    _check_i32(n, status=status, accepted=accepted, link_mtu=link_mtu, lr_proof_len=lr_proof_len)
    if any(t is None for t in (pkt_off, status, accepted, link_mtu, lr_proof_len)):
        raise ValueError("pkt_off, status, accepted, link_mtu and lr_proof_len are required")
    if transport_identity.numel() != 16 or not transport_identity.is_contiguous():
        raise ValueError("transport_identity is the node's 16-byte transport id")
    m = slots.numel()
    _check_i32(m, slots=slots)
    if ephemeral_privates.dim() != 2 or ephemeral_privates.shape != (m, 32) or not ephemeral_privates.is_contiguous():
        raise ValueError(f"ephemeral_privates must be a contiguous ({m}, 32) uint8 tensor, one row per slot")
    if link_id.dim() != 2 or link_id.shape != (n, 16) or not link_id.is_contiguous():
        raise ValueError(f"link_id must be a contiguous ({n}, 16) uint8 tensor")
    _check_rows("lr_proofs", lr_proofs, n, LRPROOF_LEN)
    d = destinations
    sg = [None, None, 0, None, None]
    n_links = 0xFFFFFFFF
    if signers is not None:
        n_links = int(signers.n_links)
        sd, stride = _ed_rows("signers.seeds", signers.seeds, n_links, 32)
        pk, pk_stride = _ed_rows("signers.publics", signers.publics, n_links, 32)
        if pk_stride != stride:
            raise ValueError("signers.seeds and signers.publics must have the same rows")
        if stride == 0 and d.n > 1:
            raise ValueError("signers with one shared seed row serve one destination; give them one row per link")
        pp = signers.peer_publics
        if pp.dim() != 2 or pp.shape != (n_links, 32) or not pp.is_contiguous():
            raise ValueError(f"signers.peer_publics must be a contiguous ({n_links}, 32) uint8 tensor")
        if signers.flags.numel() != n_links or not signers.flags.is_contiguous():
            raise ValueError(f"signers.flags must be a contiguous ({n_links},) uint8 tensor")
        sg = [sd, pk, stride, _p(pp), _p(signers.flags)]
        _same_device(pkt.device, signers.seeds, signers.publics, pp, signers.flags)
    _same_device(pkt.device, pkt_off, fields, transport_identity, slots, ephemeral_privates, status, accepted, link_id,
                 link_mtu, lr_proofs, lr_proof_len, d.seeds, d.publics, d.flags)
    if n == 0:
        return
    nh = -1 if nh_mtu is None else int(nh_mtu)
    if not -1 <= nh <= 0xFFFFFFFF:
        raise ValueError("nh_mtu must be a uint32 or None")
    _native.check(_native.load().rt_link_accept(
        links.handle, ks.handle, d.table.handle, _p(d.seeds), _p(d.publics), _p(d.flags), d.n, _p(transport_identity),
        nh, _p(pkt), _p(pkt_off), _p(fields), n, _p(slots) if m else None, _p(ephemeral_privates) if m else None, m,
        n_links, sg[0], sg[1], sg[2], sg[3], sg[4], _p(status), _p(accepted), _p(link_id), _p(link_mtu),
        _p_rows(lr_proofs), max(lr_proofs.stride(0), LRPROOF_LEN), _p(lr_proof_len), _stream(stream, pkt.device)))


def keyset_set_rows_x25519(ks: KeySet, scalars, points, salt, rows, mask=None, point_off=None, stream=None):
    """Rewrites records of an existing key set of 64-byte keys on the device:
    for every item i that ``mask`` ((n,) uint8, None: all) selects, record
    rows[i] ((n,) int32, distinct) becomes Token(hkdf(64, X25519(scalars[i],
    points[i]), salt[i])); scalars, points and point_off as :func:`x25519`,
    salt (n, S) with S a multiple of 4 up to 64.  Enqueued on ``stream``:
    launches on that stream after it see the new rows; ordering other streams
    is the caller's part."""
    n = rows.numel()
    _check_i32(n, rows=rows)
    _check_u8(salt, mask)
    if ks.key_len != 64:
        raise ValueError("rows are rewritten in a key set of 64-byte keys")
    if salt.dim() != 2 or salt.shape[0] != n or not salt.is_contiguous():
        raise ValueError(f"salt must be a contiguous ({n}, S) uint8 matrix")
    if mask is not None and (mask.numel() != n or not mask.is_contiguous()):
        raise ValueError(f"mask must be a contiguous ({n},) uint8 tensor")
    sc, sc_stride, pt, pt_stride, off = _x25519_args(scalars, points, point_off, n)
    _order_after_current(stream, scalars, points, point_off, salt, rows, mask)
    _native.check(_native.load().rt_keyset_set_rows_x25519(ks.handle, sc, sc_stride, pt, pt_stride, off, _p(salt),
                                                           salt.stride(0), salt.shape[1], _p(rows), _p(mask), n,
                                                           _stream(stream, rows.device)))


# Link request proofs (lrproof_kernels.hip): ``pending`` is a
# reticulum_amd.link.PendingLinks, ``links`` a LinkTable, ``signers`` a
# reticulum_amd.proof.LinkSigners or None, ``seen`` a
# reticulum_amd.filter.PacketHashlist or None.

LRPROOF_ACTIVATED, LRPROOF_NOT_LRPROOF, LRPROOF_NO_LINK, LRPROOF_NOT_PENDING = 0, 1, 2, 3   # RT_LRPROOF_*
LRPROOF_HOPS, LRPROOF_BAD_SIZE, LRPROOF_BAD_MODE, LRPROOF_BAD_SIGNATURE, LRPROOF_NO_SLOT = 4, 6, 7, 8, 9
PENDING_PENDING, PENDING_HANDSHAKE, PENDING_ACTIVE, PENDING_CLOSED = 0, 1, 2, 4            # RT_PENDING_*: Link's


def link_establish(ks: KeySet, links, pending, pkt, pkt_off, fields, status, established, link_mtu, signers=None,
                   seen=None, stream=None):
    """The initiator side of link establishment (Transport.py:2270-2318,
    Link.py:391-451, 348-361) over packet_unpack's records, each proof read
    inside its packet pkt[pkt_off[i]:], as if the packets came one after
    another in index order.  ``pending`` holds the links this node has
    requested: their ephemeral keys, the destinations' signing keys, the slots
    they are to take, and their state.

    status[i] ((n,) int32) is LRPROOF_ACTIVATED, NOT_LRPROOF, NO_LINK,
    NOT_PENDING (the link is not PENDING, or a lower index of the batch decided
    it), HOPS or BAD_SIZE (ignored: the link stays PENDING), BAD_MODE (the link
    is CLOSED), BAD_SIGNATURE (the link stays in HANDSHAKE for good) or NO_SLOT
    (the row's slot is not below ks.n_keys and signers.n_links, or ``links``
    has no room: the link stays PENDING); established[i] ((n,) int32) the slot
    or -1 and link_mtu[i] ((n,) int32) the link's MTU or 0.  When the call has
    run, ``links`` maps each activated link id to its slot, record slot of
    ``ks`` (64-byte keys) is the link's handshake key, with ``signers`` the
    slot's rows hold the destination's signing key, the row's flags and (one
    row per link) the link's own seed and public key, and the rows of
    ``pending`` carry the new state, hops, rebalanced and mtu.  With ``seen``
    the hashes of the proofs that reached Link.validate_proof enter the hash
    list (Transport.py:2314).  Nothing is synchronised, and neither private
    keys, shared secrets nor derived keys leave the device."""
    n = _check_fields(fields)
    _check_u8(pkt)
    if ks.key_len != 64:
        raise ValueError("a link's key set holds 64-byte keys")
    if pkt.dim() != 1 or not pkt.is_cuda or not pkt.is_contiguous():
        raise ValueError("pkt must be a flat contiguous uint8 buffer in device memory")
    _check_i64(n, pkt_off=pkt_off)
    _check_i32(n, status=status, established=established, link_mtu=link_mtu)
    if any(t is None for t in (pkt_off, status, established, link_mtu)):
        raise ValueError("pkt_off, status, established and link_mtu are required")
    p = pending
    sg = [None, None, 0, None, None]
    n_links = 0xFFFFFFFF
    if signers is not None:
        n_links = int(signers.n_links)
        sd, stride = _ed_rows("signers.seeds", signers.seeds, n_links, 32)
        pk, pk_stride = _ed_rows("signers.publics", signers.publics, n_links, 32)
        if pk_stride != stride:
            raise ValueError("signers.seeds and signers.publics must have the same rows")
        if stride == 0:
            raise ValueError("a link this node opens signs with its own key: give the signers one row per link")
        pp = signers.peer_publics
        if pp.dim() != 2 or pp.shape != (n_links, 32) or not pp.is_contiguous():
            raise ValueError(f"signers.peer_publics must be a contiguous ({n_links}, 32) uint8 tensor")
        if signers.flags.numel() != n_links or not signers.flags.is_contiguous():
            raise ValueError(f"signers.flags must be a contiguous ({n_links},) uint8 tensor")
        sg = [sd, pk, stride, _p(pp), _p(signers.flags)]
        _same_device(pkt.device, signers.seeds, signers.publics, pp, signers.flags)
    _same_device(pkt.device, pkt_off, fields, status, established, link_mtu, p.privates, p.row_state)
    if n == 0:
        return
    _native.check(_native.load().rt_link_establish(
        p.table.handle, p.max_pending, _p(p.privates), _p(p.dest_publics), _p(p.sig_seeds), _p(p.sig_publics),
        _p(p.flags), _p(p.slots), _p(p.expected_hops), _p(p.rebalanced), _p(p.row_state), _p(p.mtu), links.handle,
        ks.handle, n_links, _p(pkt), _p(pkt_off), _p(fields), n, sg[0], sg[1], sg[2], sg[3], sg[4],
        seen.handle if seen is not None else None, _p(status), _p(established), _p(link_mtu),
        _stream(stream, pkt.device)))


# Destination delivery (destination_kernels.hip): ``destinations`` is a
# reticulum_amd.destination.SingleDestinations.

DELIVER_DELIVERED, DELIVER_NOT_DATA, DELIVER_NO_DESTINATION, DELIVER_TYPE_MISMATCH = 0, 1, 2, 3   # RT_DELIVER_*
DELIVER_SHORT, DELIVER_NOT_OPENED, DELIVER_DEFERRED = 4, 5, 6
DEST_ENFORCE_RATCHETS = 8    # RT_DEST_ENFORCE_RATCHETS, beside LINK_PROVE_ALL
DEST_PROOF_IMPLICIT_LEN, DEST_PROOF_EXPLICIT_LEN = 83, 115


def destination_deliver(destinations, pkt, pkt_off, fields, pt, pt_off, pt_len, status, deliver_status, destination,
                        ratchet, dest_proofs, dest_proof_len, implicit_proof=True, pt_shift=0, stream=None):
    """The DATA packets for the node's own SINGLE destinations
    (Transport.py:2188-2202, Destination.py:414-429, 622-654,
    Identity.py:848-898, 942-953) over packet_unpack's records, each packet read
    inside pkt[pkt_off[i]:]; at most destinations.max_frames records.

    deliver_status[i] ((n,) int32) is DELIVER_NOT_DATA (not ok, no DATA packet,
    or destination type LINK), NO_DESTINATION, TYPE_MISMATCH (the hash is a
    destination's, the packet's type is not SINGLE), SHORT (data of 32 bytes or
    fewer), DELIVERED, NOT_OPENED (no candidate key opens the token, or the
    padding fails under the one that verifies) or DEFERRED (the frame's
    remaining candidates did not fit ``retry_trials`` after its first candidate
    failed; so is every undecided frame behind it, and nothing else is written
    for them).  destination[i] is the row or -1 and ratchet[i] the rank of the
    ratchet that opened the frame (-1: the identity's key, or nothing).  For
    DELIVERED and NOT_OPENED frames status[i] and pt_len[i] are the token
    decrypt's and the plaintext lies at pt[pt_off[i]:], pt_off[i] ((n,) int64,
    written for these frames) = the token's offset + ``pt_shift``; the three
    are left alone elsewhere.  A DELIVERED frame of a PROVE_ALL destination has
    dest_proof_len[i] = 83 (``implicit_proof``) or 115 and the PROOF packet in
    row i of dest_proofs ((n, >=115) uint8 at any row stride); elsewhere the
    length is 0 and the row untouched.  Nothing is synchronised, and neither
    shared secrets nor derived keys leave the device."""
    n = _check_fields(fields)
    d = destinations
    _check_u8(pkt, pt, dest_proofs)
    for name, t in (("pkt", pkt), ("pt", pt)):
        if t.dim() != 1 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name} must be a flat contiguous uint8 buffer in device memory")
    _check_i64(n, pkt_off=pkt_off, pt_off=pt_off)
    _check_i32(n, pt_len=pt_len, status=status, deliver_status=deliver_status, destination=destination,
               ratchet=ratchet, dest_proof_len=dest_proof_len)
    if any(t is None for t in (pkt_off, pt_off, pt_len, status, deliver_status, destination, ratchet, dest_proof_len)):
        raise ValueError("pkt_off, pt_off, pt_len, status, deliver_status, destination, ratchet and dest_proof_len "
                         "are required")
    _check_rows("dest_proofs", dest_proofs, n, DEST_PROOF_EXPLICIT_LEN)
    if n > d.max_frames:
        raise ValueError(f"the destinations' scratch serves {d.max_frames} frames per call, got {n}")
    if not 0 <= int(pt_shift) <= 16:
        raise ValueError("pt_shift is 0 .. 16")
    _same_device(pkt.device, pkt_off, fields, pt, pt_off, pt_len, status, deliver_status, destination, ratchet,
                 dest_proofs, dest_proof_len, d.privates, d.identity_hashes, d.seeds, d.publics, d.flags,
                 d.ratchet_off, d.ratchets, d.work)
    if n == 0:
        return
    _order_after_current(stream, d.ratchets, d.ratchet_off)
    _native.check(_native.load().rt_destination_deliver(
        d.table.handle, d.n, _p(d.privates), _p(d.identity_hashes), _p(d.seeds), _p(d.publics), _p(d.flags),
        _p(d.ratchet_off), _p(d.ratchets), d.ratchets.shape[0], d.scratch.handle, d.max_frames, d.retry_trials,
        _p(d.work), d.work_bytes, _p(pkt), _p(pkt_off), _p(fields), n, 1 if implicit_proof else 0, int(pt_shift),
        _p(pt), _p(pt_off), _p(pt_len), _p(status), _p(deliver_status), _p(destination), _p(ratchet),
        _p_rows(dest_proofs), max(dest_proofs.stride(0), DEST_PROOF_EXPLICIT_LEN), _p(dest_proof_len),
        _stream(stream, pkt.device)))


def ifac_mask(pkt, pkt_off, pkt_len, ifac, ifac_key, out, out_off, stream=None):
    """Transport.transmit's IFAC step (Transport.py:1069-1101): packet i plus
    its access code ifac[i] (n, ifac_size) -> pkt_len[i] + ifac_size masked
    bytes at out[out_off[i]:]; ifac_key (K,) uint8, K <= 64."""
    _check_u8(pkt, ifac, ifac_key, out)
    n = pkt_off.numel()
    if pkt_len.numel() != n or ifac.shape[0] != n or out_off.numel() != n:
        raise ValueError("shape mismatch")
    lib = _native.load()
    _native.check(lib.rt_ifac_mask(_ctx_of(pkt), _p(pkt), _p(pkt_off), _p(pkt_len), _p(ifac), ifac.shape[1],
                                   _p(ifac_key), ifac_key.numel(), _p(out), _p(out_off), n, _stream(stream, pkt.device)))


def ifac_unmask(pkt, pkt_off, pkt_len, ifac_key, ifac_out, out, out_off, status, out_len=None, stream=None):
    """Transport.inbound's IFAC step up to the signature check
    (Transport.py:1441-1475): status[i] = 0 with the IFAC in ifac_out[i] (n,
    ifac_size) and the unmasked packet (pkt_len[i] - ifac_size bytes) at
    out[out_off[i]:], or 1 where the reference drops the packet first.
    out_len (n,) int32, if given, receives pkt_len[i] - ifac_size where the
    status is 0 and 0 elsewhere (packet_unpack's lengths)."""
    _check_u8(pkt, ifac_key, ifac_out, out)
    n = pkt_off.numel()
    if pkt_len.numel() != n or ifac_out.shape[0] != n or out_off.numel() != n or status.numel() != n or \
            (out_len is not None and (out_len.numel() != n or out_len.dtype != torch.int32)):
        raise ValueError("shape mismatch")
    lib = _native.load()
    _native.check(lib.rt_ifac_unmask(_ctx_of(pkt), _p(pkt), _p(pkt_off), _p(pkt_len), ifac_out.shape[1],
                                     _p(ifac_key), ifac_key.numel(), _p(ifac_out), _p(out), _p(out_off), _p(status),
                                     _p(out_len), n, _stream(stream, pkt.device)))


IFAC_OK, IFAC_DROPPED, IFAC_MISMATCH = 0, 1, 2      # RT_IFAC_* (include/rnstok.h)


def _ifac_sign_args(seed, public_key, pkt, pkt_off, pkt_len, ifac):
    _check_u8(seed, public_key, pkt, ifac)
    if seed.numel() != 32 or public_key.numel() != 32:
        raise ValueError("seed and public_key are 32 bytes each")
    n = pkt_off.numel()
    _check_i64(n, pkt_off=pkt_off)
    _check_i32(n, pkt_len=pkt_len)
    if ifac.dim() != 2 or ifac.shape[0] != n or not 1 <= ifac.shape[1] <= 64:
        raise ValueError(f"access codes must be an ({n}, 1..64) uint8 matrix")
    return n


def ifac_sign(seed, public_key, pkt, pkt_off, pkt_len, ifac_out, stream=None):
    """The access code Transport.transmit makes (Transport.py:1073):
    ifac_out[i] ((n, ifac_size) uint8, ifac_size 1..64) = the last ifac_size
    bytes of the signature of packet i (pkt[pkt_off[i]:][:pkt_len[i]]) under
    the interface identity's 32-byte ``seed`` (ifac_key[32:64]) and its
    ``public_key`` (ed25519_public of the seed).  A packet of length 0 is
    skipped (its offset is never used) and its row zeroed."""
    n = _ifac_sign_args(seed, public_key, pkt, pkt_off, pkt_len, ifac_out)
    lib = _native.load()
    _native.check(lib.rt_ifac_sign(_ctx_of(pkt), _p(seed), _p(public_key), _p(pkt), _p(pkt_off), _p(pkt_len),
                                   _p(ifac_out), ifac_out.shape[1], n, _stream(stream, pkt.device)))


def ifac_check(seed, public_key, pkt, pkt_off, pkt_len, ifac, status, stream=None):
    """Transport.inbound's access-code check (Transport.py:1470-1474) after
    ifac_unmask: where status[i] is IFAC_OK and ifac[i] ((n, ifac_size)) is
    not the tail of the signature of packet i, status[i] becomes
    IFAC_MISMATCH and pkt_len[i] 0 (so unpack and the token stages drop the
    packet, the reference's ``return``).  Entries with another status, or of
    length 0, are left as they are."""
    n = _ifac_sign_args(seed, public_key, pkt, pkt_off, pkt_len, ifac)
    _check_i32(n, status=status)
    if status is None:
        raise ValueError("status is required")
    lib = _native.load()
    _native.check(lib.rt_ifac_check(_ctx_of(pkt), _p(seed), _p(public_key), _p(pkt), _p(pkt_off), _p(pkt_len),
                                    _p(ifac), ifac.shape[1], _p(status), n, _stream(stream, pkt.device)))


# The replies of a read (reply_kernels.hip)

REPLY_LRPROOF, REPLY_LINK_PROOF, REPLY_DEST_PROOF = 0, 1, 2       # RT_REPLY_* (include/rnstok.h)
REPLY_MAX_SOURCES = 4


def reply_gather(sources, out, reply_len, reply_frame, reply_source, reply_counts, workspace=None, stream=None):
    """The replies of a read as one dense batch.  ``sources`` is a sequence of
    one to four (rows, len) pairs over the same n frames: rows an (n, width)
    uint8 matrix at any row stride >= width, len (n,) int32, where 0 (or
    anything outside 1 .. min(128, width)) means nothing for that frame.
    Reply j, in the order of the frames and within a frame of the sources,
    goes to out[j] (out: (cap, 128) uint8, contiguous; bytes past the reply
    zeroed) with reply_len[j], reply_frame[j] ((cap,) int32) and
    reply_source[j] ((cap,) uint8); reply_counts ((2,) int64) = [written =
    min(found, cap), found].  Entries past ``written`` read 0, -1 and 0xFF and
    their rows are not written."""
    sources = list(sources)
    if not 1 <= len(sources) <= REPLY_MAX_SOURCES:
        raise ValueError("reply_gather takes 1 to 4 sources")
    if out.dim() != 2 or out.shape[1] != LINE or not out.is_contiguous():
        raise ValueError("out must be a contiguous (cap, 128) uint8 matrix")
    _check_u8(out, reply_source, *[rows for rows, _ in sources])
    cap = out.shape[0]
    dev = out.device
    n = sources[0][1].numel()
    for rows, ln in sources:
        _check_i32(n, len=ln)
        if rows.dim() != 2 or rows.shape[0] != n or rows.shape[1] < 1:
            raise ValueError(f"every source's rows must be an ({n}, width) uint8 matrix")
        _same_device(dev, rows, ln)
    _check_i32(cap, reply_len=reply_len, reply_frame=reply_frame)
    _check_i64(2, reply_counts=reply_counts)
    if reply_len is None or reply_frame is None or reply_counts is None or reply_source is None or \
            reply_source.numel() != cap or not reply_source.is_contiguous():
        raise ValueError(f"reply_len, reply_frame ({cap},) int32, reply_source ({cap},) uint8 and reply_counts (2,) "
                         "int64 are required")
    _same_device(dev, reply_len, reply_frame, reply_source, reply_counts)
    if cap and out.data_ptr() % LINE:
        raise ValueError("out must start on a 128-byte line")
    lib = _native.load()
    S = len(sources)
    need = int(lib.rt_reply_gather_workspace_bytes(n, S))
    if need == 0:
        raise ValueError("reply_gather takes at most 2**31 - 1 frames")
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=dev)
    if ws.numel() < need or ws.device != dev:
        raise ValueError("workspace is smaller than rt_reply_gather_workspace_bytes(n, S)")
    c_rows = (ctypes.c_void_p * S)(*[_p_rows(rows) for rows, _ in sources])
    c_len = (ctypes.c_void_p * S)(*[_p(ln) for _, ln in sources])
    c_stride = (ctypes.c_uint64 * S)(*[max(rows.stride(0), rows.shape[1]) for rows, _ in sources])
    c_width = (ctypes.c_uint32 * S)(*[rows.shape[1] for rows, _ in sources])
    _native.check(lib.rt_reply_gather(_ctx_of(out), S, c_rows, c_stride, c_width, c_len, n, _p(out), _p(reply_len),
                                      _p(reply_frame), _p(reply_source), _p(reply_counts), cap, _p(ws),
                                      _stream(stream, dev)))


def reply_remember(lst, packets, reply_len, reply_counts, stream=None):
    """Enter the packet hashes of the first reply_counts[0] rows of ``packets``
    ((cap, 128) uint8, as reply_gather wrote them) into the hash list ``lst``
    (an rt_hashlist handle): Transport.outbound's add_packet_hash for what it
    broadcasts (Transport.py:1343-1345).  Counted on the device."""
    _check_u8(packets)
    if packets.dim() != 2 or packets.shape[1] != LINE or not packets.is_contiguous():
        raise ValueError("packets must be a contiguous (cap, 128) uint8 matrix")
    cap = packets.shape[0]
    _check_i32(cap, reply_len=reply_len)
    _check_i64(2, reply_counts=reply_counts)
    if reply_len is None or reply_counts is None:
        raise ValueError("reply_len and reply_counts are required")
    _native.check(_native.load().rt_reply_remember(lst, _p(packets), LINE, _p(reply_len), _p(reply_counts), cap,
                                                   _stream(stream, packets.device)))


def packet_unpack(pkt, pkt_off, pkt_len, fields, stream=None):
    """Packet.unpack + get_hash (Packet.py:242-275, 342-353): fields (n, 96)
    uint8 receives one rt_packet_fields record per packet
    (reticulum_amd.wire.FIELDS_DTYPE)."""
    _check_u8(pkt, fields)
    n = pkt_off.numel()
    if pkt_len.numel() != n or fields.numel() != 96 * n:
        raise ValueError("shape mismatch")
    lib = _native.load()
    _native.check(lib.rt_packet_unpack(_ctx_of(pkt), _p(pkt), _p(pkt_off), _p(pkt_len), _p(fields), n,
                                       _stream(stream, pkt.device)))


def pack_headers(flags, hops, destination_hash, context, out, out_off, transport_id=None, stream=None):
    """Packet.pack's header (Packet.py:167-228) for n packets at
    out[out_off[i]:]: flags, hops, [transport_id], destination hash, context
    (19 or 35 bytes).  flags/hops/context (n,) uint8; hashes (n, 16) uint8."""
    _check_u8(flags, hops, destination_hash, context, out, transport_id)
    n = flags.numel()
    lib = _native.load()
    _native.check(lib.rt_packet_pack_headers(_ctx_of(out), _p(flags), _p(hops), _p(transport_id),
                                             _p(destination_hash), _p(context), _p(out), _p(out_off), n,
                                             _stream(stream, out.device)))


# ------------------------------------------------------- host-origin path --

def copy_to_host(dst, src, stream=None):
    """Enqueue ``dst.copy_(src)`` for a device tensor ``src`` and a host tensor
    ``dst`` of the same size, both contiguous, through rt_memcpy_d2h: a pinned
    ``dst`` is written by GPU stores into the mapped host buffer
    (copy_kernels.hip; 54 GB/s alone and 87 GB/s beside a copy-engine H2D on
    MI355X, against 30 GB/s for the copy engine's D2H,
    profiles/r03n_pcie_probe.json), a pageable one by hipMemcpyAsync.  Like
    ``copy_(non_blocking=True)`` nothing is synchronised: ``dst`` is valid
    once ``stream`` (default: the current stream of src's GPU) has run."""
    if not src.is_cuda or dst.is_cuda:
        raise ValueError("copy_to_host copies a device tensor into a host tensor")
    if not src.is_contiguous() or not dst.is_contiguous():
        raise ValueError("copy_to_host needs contiguous tensors")
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() != nbytes:
        raise ValueError("copy_to_host: size mismatch")
    if nbytes == 0:
        return
    lib = _native.load()
    _native.check(lib.rt_memcpy_d2h(_ctx_of(src), dst.data_ptr(), src.data_ptr(), nbytes,
                                    _stream(stream, src.device)))


def copy_to_host_upto(dst, src, nbytes_dev, stream=None):
    """Enqueue the copy of the first min(dst size, nbytes_dev) bytes of the
    device tensor ``src`` into the pinned host tensor ``dst``, where
    ``nbytes_dev`` is a one-element int64 DEVICE tensor read at run time (e.g.
    ``frame_off[n]`` from hdlc_frame: the stream's length, which the host
    does not know without a sync; zero or negative copies nothing) — GPU
    stores into the mapped buffer (rt_memcpy_d2h_upto).  Nothing is
    synchronised; bytes of ``dst`` past the count are left as they were."""
    if not src.is_cuda or dst.is_cuda or not dst.is_pinned():
        raise ValueError("copy_to_host_upto copies a device tensor into a pinned host tensor")
    if not src.is_contiguous() or not dst.is_contiguous():
        raise ValueError("copy_to_host_upto needs contiguous tensors")
    if nbytes_dev.dtype != torch.int64 or nbytes_dev.numel() != 1 or not nbytes_dev.is_cuda:
        raise TypeError("nbytes_dev: one int64 element on the device")
    if nbytes_dev.device != src.device:
        raise ValueError("nbytes_dev must be on src's device")
    nbytes = min(src.numel() * src.element_size(), dst.numel() * dst.element_size())
    if nbytes == 0:
        return
    lib = _native.load()
    _native.check(lib.rt_memcpy_d2h_upto(_ctx_of(src), dst.data_ptr(), src.data_ptr(), nbytes, _p(nbytes_dev),
                                         _stream(stream, src.device)))


# ------------------------------------------------------------ launch clock --

CLOCK_KERNELS = ("encrypt", "decrypt")      # RT_CLOCK_ENCRYPT, RT_CLOCK_DECRYPT
REALTIME_HZ = 100e6                         # s_memrealtime ticks per second


def clock_summary(words):
    """The rt_clock_stamps words (8 ints) as per-kernel figures: the run's
    sustained shader clock (cycles / real-time ticks x 100 MHz), the cycles
    per launch (the mean workgroup span: one persistent workgroup per CU)
    and the mean workgroup span in ms.  Kernels with no stamped launch are
    left out."""
    out = {}
    for k, name in enumerate(CLOCK_KERNELS):
        cyc, ticks, wgs, launches = (int(x) for x in words[4 * k:4 * k + 4])
        if wgs == 0 or ticks == 0:
            continue
        out[name] = {"clock_ghz": cyc / ticks * REALTIME_HZ / 1e9, "cycles_per_launch": cyc / wgs,
                     "wg_span_ms": ticks / wgs / REALTIME_HZ * 1e3, "launches": launches,
                     "workgroups_per_launch": wgs / launches if launches else None}
    return out


class LaunchClock:
    """Stamp every encrypt/decrypt launch of a block on ``device``'s context
    (rt_clock_stamps) and read the run's clock afterwards::

        with device.LaunchClock(dev) as lc:
            ...launches...
        lc.summary()      # syncs the device, then clock_summary(words)

    Stamping is per context, i.e. process-wide for the device: every launch
    on it from any thread or stream while the block is open is stamped into
    this object's words.  One block per device at a time (a nested or
    concurrent block raises RuntimeError instead of mixing stamps), and the
    exit waits for the device, so no launch still adds to the words once the
    block is closed."""

    _open = set()               # device indices with an open block
    _open_lock = threading.Lock()

    def __init__(self, dev=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        self.dev = dev
        self._index = dev.index if dev.index is not None else torch.cuda.current_device()
        self.acc = torch.zeros(8, dtype=torch.int64, device=dev)
        self._ctx = _native.context(self._index)

    def __enter__(self):
        with LaunchClock._open_lock:
            if self._index in LaunchClock._open:
                raise RuntimeError(f"a LaunchClock is already open on cuda:{self._index}: stamping is per context")
            LaunchClock._open.add(self._index)
        try:
            # the zeroed words are ordered before any launch the block enqueues
            torch.cuda.synchronize(self.dev)
            _native.check(_native.load().rt_clock_stamps(self._ctx, self.acc.data_ptr()))
        except BaseException:
            with LaunchClock._open_lock:
                LaunchClock._open.discard(self._index)
            raise
        return self

    def __exit__(self, *exc):
        try:
            _native.check(_native.load().rt_clock_stamps(self._ctx, None))
            # launches already queued still add to acc: let them land before
            # the block counts as closed (and before acc can be freed)
            torch.cuda.synchronize(self.dev)
        finally:
            with LaunchClock._open_lock:
                LaunchClock._open.discard(self._index)
        return False

    def words(self):
        torch.cuda.synchronize(self.dev)
        return [int(x) for x in self.acc.cpu()]

    def summary(self):
        return clock_summary(self.words())
