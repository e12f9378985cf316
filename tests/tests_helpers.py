"""Small helpers shared by the test modules."""
import ctypes
import functools

import numpy as np


def b(h):
    return bytes.fromhex(h)


def u8(data, *shape):
    return np.frombuffer(bytes(data), np.uint8).reshape(*shape).copy()


def pack(msgs):
    """A list of bytes -> (flat uint8 array, uint64 offsets, uint32 lengths)."""
    lens = np.array([len(m) for m in msgs], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return u8(b"".join(msgs) or b"\x00", -1), offs, lens


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def lib_ctx():
    from reticulum_amd import _native
    return _native.load(), _native.context(0)


# ---- plain models of the Identity layer (RNS/Identity.py), built from the
# tests' integer references and the C oracle's token alone

@functools.lru_cache(maxsize=None)
def _ladder(scalar, point):
    import x25519_ref
    return x25519_ref.ladder(scalar, point)


def identity_decrypt_ref(private, salt, token, ratchets, enforce):
    """``Identity.decrypt`` (Identity.py:857-902) for one token: ``(plaintext |
    None, which)``.  A token of 32 bytes or fewer gives ``(None, None)``;
    otherwise every ratchet in order and then the identity's key (left out under
    ``enforce``) derives a token key from its exchange with token[:32], and the
    first that opens token[32:] wins: ``which`` is that ratchet's index, or -1
    for the identity's key."""
    import x25519_ref
    from oracle import ctoken
    token = bytes(token)
    if len(token) <= 32:
        return None, None
    tried = [(bytes(r), i) for i, r in enumerate(ratchets or [])]
    if not enforce:
        tried.append((bytes(private), -1))
    for scalar, which in tried:
        key = x25519_ref.hkdf(64, _ladder(scalar, token[:32]), salt)
        status, pt = ctoken.decrypt(key, token[32:])
        if status == 0:
            return pt, which
    return None, None


def identity_encrypt_ref(target_public, salt, pt, eph, iv):
    """``Identity.encrypt`` (Identity.py:811-833) with the ephemeral private key
    and the IV given: ephemeral_pub ‖ iv ‖ ct ‖ tag."""
    import x25519_ref
    from oracle import ctoken
    key = x25519_ref.hkdf(64, _ladder(bytes(eph), bytes(target_public)), salt)
    return _ladder(bytes(eph), x25519_ref.BASE) + ctoken.encrypt(key, bytes(iv), bytes(pt))


def announce_valid_ref(destination_hash, context_flag, data, only_validate_signature=False):
    """``Identity.validate_announce`` (Identity.py:511-606) for one announce."""
    import ed25519_ref
    return ed25519_ref.validate_announce(bytes(destination_hash), context_flag, bytes(data), only_validate_signature)


def trial_case(seed, n_tok=40, n_keys=12):
    """Tokens under random keys of a key set and candidate lists in which the
    right key sits at a random rank, is missing, or appears twice; plus
    malformed and too-short tokens that no key opens."""
    import numpy as np
    from oracle import ctoken
    rng = np.random.Generator(np.random.PCG64(seed))
    keys = rng.integers(0, 256, (n_keys, 64), dtype=np.uint8)
    toks, cands, expect = [], [], []
    for t in range(n_tok):
        k = int(rng.integers(0, n_keys))
        pt = rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()
        tok = ctoken.encrypt(keys[k].tobytes(), rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), pt)
        others = [i for i in rng.permutation(n_keys).tolist() if i != k][: int(rng.integers(0, 6))]
        mode = t % 5
        if mode == 0:                      # right key missing
            cand, exp = others, -1
        elif mode == 1:                    # right key twice
            cand = others + [k, k]
            exp = k
        elif mode == 2:                    # malformed: ciphertext not whole blocks
            tok, cand, exp = tok[:-33] + tok[-32:], others + [k], -1
        elif mode == 3:                    # too short
            tok, cand, exp = tok[:32], [k], -1
        else:
            pos = int(rng.integers(0, len(others) + 1))
            cand = others[:pos] + [k] + others[pos:]
            exp = k
        toks.append(tok)
        cands.append(cand)
        expect.append(exp)
    return keys, toks, cands, np.array(expect)


def collision_stream(seed, length, dup, sdu=464):
    """The input stream of a Resource collision-guard fixture
    (tests/golden/gen_resource.py): `length` seeded random bytes with part
    dup[1] overwritten by a copy of part dup[0] (no copy when dup is None or
    names one part)."""
    import numpy as np
    stream = bytearray(np.random.Generator(np.random.PCG64(seed)).integers(0, 256, length, dtype=np.uint8).tobytes())
    if dup and dup[0] != dup[1]:
        a, c = dup
        stream[c * sdu:(c + 1) * sdu] = stream[a * sdu:(a + 1) * sdu]
    return bytes(stream)
