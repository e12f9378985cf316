"""The Ed25519 tests' own reference: big-integer arithmetic written from the
curve equation -x^2 + y^2 = 1 + d x^2 y^2 in affine coordinates and
``hashlib.sha512``, independent of the product and of the fixtures' generator,
and the fixture file.

``verify`` states the acceptance rule of the reference's internal provider
 in group terms; the fixtures, recorded from the reference
itself, are what it is checked against."""
import functools
import hashlib
import json
import os

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ed25519_vectors.json")
IDENTITY = (0, 1)
ZERO_BYTES = (1).to_bytes(32, "little")


def inv(x):
    return pow(x, P - 2, P)


def add(p, q):
    """The affine addition law of a twisted Edwards curve with a = -1; complete
    on this curve, so it also doubles and handles the identity and small orders."""
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * inv(1 + t) % P, (y1 * y2 + x1 * x2) * inv(1 - t) % P)


def neg(p):
    return (-p[0] % P, p[1])


def _padd(p, q):
    """The same law on projective points (X : Y : Z), x = X/Z, y = Y/Z, so that
    a scalar multiplication needs one inversion instead of two per step."""
    (x1, y1, z1), (x2, y2, z2) = p, q
    a = z1 * z2 % P
    b = a * a % P
    c = x1 * x2 % P
    dd = y1 * y2 % P
    e = D * c * dd % P
    f, g = (b - e) % P, (b + e) % P
    return (a * f * ((x1 + y1) * (x2 + y2) - c - dd) % P, a * g * (dd + c) % P, f * g % P)


def mul(n, p):
    pp, q = (p[0], p[1], 1), (0, 1, 1)
    for bit in bin(n)[2:] if n else "":
        q = _padd(q, q)
        if bit == "1":
            q = _padd(q, pp)
    zi = inv(q[2])
    return (q[0] * zi % P, q[1] * zi % P)


def on_curve(p):
    x, y = p
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def decode(s):
    """A point from 32 bytes, or None: y = the low 255 bits mod p (not required
    below p), x the square root of (y^2 - 1)/(d y^2 + 1) whose parity is bit 255
    (x = 0 with the bit set stays 0)."""
    v = int.from_bytes(s, "little")
    y = (v & ((1 << 255) - 1)) % P
    xx = (y * y - 1) * inv(D * y * y + 1) % P
    x = pow(xx, (P + 3) // 8, P)
    if (x * x - xx) % P:
        x = x * SQRT_M1 % P
    if (x * x - xx) % P or not on_curve((x, y)):
        return None
    if (x & 1) != (v >> 255):
        x = -x % P
    return (x, y)


def encode(p):
    x, y = p
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


BASE = decode((4 * inv(5) % P).to_bytes(32, "little"))


def hint(m):
    return int.from_bytes(hashlib.sha512(m).digest(), "little")


def expand(seed):
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little")
    a = (a & ((1 << 254) - 8)) | (1 << 254)
    return a, h[32:]


@functools.lru_cache(maxsize=None)
def _public_key(seed):
    return encode(mul(expand(seed)[0] % L, BASE))


def public_key(seed):
    """Remembered per seed: sign() without a public key derives it on every call."""
    return _public_key(bytes(seed))


def sign(seed, msg, pk=None):
    a, prefix = expand(seed)
    if pk is None:
        pk = public_key(seed)
    r = hint(prefix + msg) % L
    rb = encode(mul(r, BASE))
    return rb + ((r + hint(rb + pk + msg) * a) % L).to_bytes(32, "little")


def verify(pk, sig, msg):
    """The internal provider's rule: canonical identity bytes rejected, both
    points decode, [L]A = [L]R = identity, [S mod L]B = R + [h mod L]A as
    points; and a key that is the identity in another encoding is rejected
    unless h mod L is 0."""
    if len(pk) != 32 or len(sig) != 64:
        return False
    if pk == ZERO_BYTES or sig[:32] == ZERO_BYTES:
        return False
    a, r = decode(pk), decode(sig[:32])
    if a is None or r is None:
        return False
    if mul(L, a) != IDENTITY or mul(L, r) != IDENTITY:
        return False
    s = int.from_bytes(sig[32:], "little") % L
    h = hint(sig[:32] + pk + msg) % L
    if a == IDENTITY and h != 0:
        return False
    return mul(s, BASE) == add(r, mul(h, a))


def announce_fields(data, context_flag):
    """Identity.validate_announce's cuts: (public_key, name_hash, random_hash,
    ratchet, signature, app_data)."""
    if context_flag:
        return data[:64], data[64:74], data[74:84], data[84:116], data[116:180], data[180:]
    return data[:64], data[64:74], data[74:84], b"", data[84:148], data[148:]


def validate_announce(destination_hash, context_flag, data, only_validate_signature=False):
    pub, name_hash, random_hash, ratchet, sig, app_data = announce_fields(data, context_flag)
    if len(pub) != 64 or len(sig) != 64:
        return False
    if not verify(pub[32:], sig, destination_hash + pub + name_hash + random_hash + ratchet + app_data):
        return False
    if only_validate_signature:
        return True
    identity_hash = hashlib.sha256(pub).digest()[:16]
    return destination_hash == hashlib.sha256(name_hash + identity_hash).digest()[:16]


@functools.lru_cache(maxsize=None)
def vectors():
    with open(VECTORS) as f:
        return json.load(f)
