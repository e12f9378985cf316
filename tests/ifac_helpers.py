"""Shared by tests/test_ifac_sign.py and tests/test_ifac_sign_gpu.py: the
fixture recorded from the reference's Transport (tests/golden/ifac_vectors.json)
and the tests' own model of the access code, ed25519_ref.sign with the seed
Identity.from_bytes takes from an ifac_key (its bytes 32..63)."""
import functools
import json
import os

import ed25519_ref as ref

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ifac_vectors.json")


@functools.lru_cache(maxsize=None)
def vectors():
    with open(VECTORS) as f:
        return json.load(f)


def seed_of(ifac_key):
    return bytes(ifac_key)[32:64]


@functools.lru_cache(maxsize=None)
def public_of(seed):
    return ref.public_key(seed)


@functools.lru_cache(maxsize=None)
def signature(seed, msg):
    """The 64-byte signature; computed once per (seed, message) for the whole run."""
    return ref.sign(seed, msg, public_of(seed))


def code(ifac_key, raw, ifac_size):
    """Transport.py:1073: sign(raw)[-ifac_size:]."""
    return signature(seed_of(ifac_key), bytes(raw))[-ifac_size:]


def reassemble(received, ifac_size, mask_of):
    """Transport.inbound up to the check (Transport.py:1441-1468): (ifac,
    new_raw) or None where it returns before signing.  mask_of(length, ifac):
    the HKDF mask."""
    if len(received) <= 2 or not received[0] & 0x80 or len(received) <= 2 + ifac_size:
        return None
    ifac = received[2:2 + ifac_size]
    mask = mask_of(len(received), ifac)
    un = bytes(b ^ mask[i] if i <= 1 or i > ifac_size + 1 else b for i, b in enumerate(received))
    return ifac, bytes([un[0] & 0x7F, un[1]]) + un[2 + ifac_size:]
