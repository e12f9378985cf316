"""The X25519 tests' own reference: a plain big-integer RFC 7748 §5 ladder,
independent of the product and of the fixtures' generator, and the fixture
file."""
import functools
import hashlib
import hmac
import json
import os

P = 2 ** 255 - 19
A24 = 121665
VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x25519_vectors.json")


def ladder(scalar: bytes, point: bytes) -> bytes:
    """X25519(scalar, point) as RFC 7748 §5 writes it: decodeScalar25519,
    decodeUCoordinate (bit 255 masked, non-canonical values accepted), the
    255-step ladder, x2 * z2^(p-2)."""
    assert len(scalar) == 32 and len(point) == 32
    k = int.from_bytes(scalar, "little")
    k &= ~7
    k &= (1 << 255) - 1
    k |= 1 << 254
    x1 = (int.from_bytes(point, "little") & ((1 << 255) - 1)) % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (k >> t) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b, c, d = (x2 + z2) % P, (x2 - z2) % P, (x3 + z3) % P, (x3 - z3) % P
        aa, bb, da, cb = a * a % P, b * b % P, d * a % P, c * b % P
        e = (aa - bb) % P
        x3, z3 = (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P
        x2, z2 = aa * bb % P, e * (aa + A24 * e) % P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


BASE = (9).to_bytes(32, "little")


def hkdf(length, ikm, salt, context=b""):
    """RFC 5869 with SHA-256 from hashlib / hmac (salt None or empty: 32 zero bytes)."""
    prk = hmac.new(salt or bytes(32), ikm, hashlib.sha256).digest()
    out, block, i = b"", b"", 1
    while len(out) < length:
        block = hmac.new(prk, block + context + bytes([i % 256]), hashlib.sha256).digest()
        out += block
        i += 1
    return out[:length]


@functools.lru_cache(maxsize=None)
def vectors():
    with open(VECTORS) as f:
        return json.load(f)
