"""A plain model of the link request stage (Transport.py:2127-2158,
Destination.py:414-435, Link.py:186-227, 336-376) for the tests: hashlib,
tests/ed25519_ref.py and an RFC 7748 ladder, no device and no reference code.
tests/test_link_accept.py ties it to the fixture bit for bit; the GPU tests
compare the device stage against it."""
import hashlib
import hmac
import json
import os

import ed25519_ref as ed

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "link_accept_vectors.json")

ACCEPTED, NOT_REQUEST, OTHER_TRANSPORT, NO_DESTINATION, NOT_ACCEPTING = 0, 1, 2, 3, 4
BAD_SIZE, BAD_MODE, DUPLICATE, NO_SLOT = 6, 7, 8, 9
STATUS = {"ACCEPTED": ACCEPTED, "NOT_REQUEST": NOT_REQUEST, "OTHER_TRANSPORT": OTHER_TRANSPORT,
          "NO_DESTINATION": NO_DESTINATION, "NOT_ACCEPTING": NOT_ACCEPTING, "BAD_SIZE": BAD_SIZE,
          "BAD_MODE": BAD_MODE, "DUPLICATE": DUPLICATE, "NO_SLOT": NO_SLOT}
F_PROVE_ALL, F_HAS_CHANNEL, F_ACCEPTS = 1, 2, 4
LINKREQUEST, SINGLE, LINK, DATA = 2, 0, 3, 0
MTU, MTU_MASK, MODE_AES256_CBC = 500, 0x1FFFFF, 1
LRPROOF_LEN = 118
P = 2 ** 255 - 19


def vectors():
    with open(VECTORS) as f:
        v = json.load(f)
    for d in v["destinations"]:
        d["private_key"] = bytes.fromhex(d["private_key"])
        d["seed"] = d["private_key"][32:]
        d["hash"] = bytes.fromhex(d["hash"])
    v["transport_id"] = bytes.fromhex(v["transport_id"])
    for c in v["cases"]:
        for k in ("raw", "ephemeral", "link_id", "derived_key", "peer_pub", "peer_sig_pub", "lrproof"):
            if k in c:
                c[k] = bytes.fromhex(c[k])
    return v


def x25519(scalar, point):
    """RFC 7748 §5 as X25519PrivateKey.exchange runs it under the reference's
    internal provider (X25519.py:139-145): the scalar clamped, the point's 256
    bits taken mod p as they are (bit 255 is not masked there, unlike
    curve25519()), a low-order point gives zeros."""
    k = int.from_bytes(scalar, "little")
    k = (k & ~7 & ((1 << 255) - 1)) | (1 << 254)
    x1 = int.from_bytes(point, "little") % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        bit = (k >> t) & 1
        if swap ^ bit:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = bit
        a, b, c, d = (x2 + z2) % P, (x2 - z2) % P, (x3 + z3) % P, (x3 - z3) % P
        aa, bb, da, cb = a * a % P, b * b % P, d * a % P, c * b % P
        e = (aa - bb) % P
        x3, z3 = (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P
        x2, z2 = aa * bb % P, e * (aa + 121665 * e) % P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


def hkdf(length, ikm, salt):
    prk = hmac.new(salt, ikm, hashlib.sha256).digest()
    out, t, i = b"", b"", 1
    while len(out) < length:
        t = hmac.new(prk, t + bytes([i & 255]), hashlib.sha256).digest()
        out += t
        i += 1
    return out[:length]


def signalling(mtu, mode=MODE_AES256_CBC):
    return ((mtu & MTU_MASK) + (((mode << 5) & 0xE0) << 16)).to_bytes(3, "big")


class Dest:
    def __init__(self, hash_, seed, flags):
        self.hash, self.seed, self.flags = hash_, seed, flags
        self.public = ed.public_key(seed)


def unpack(raw):
    """(header_2, hops, transport id, destination hash, data offset) or None."""
    if len(raw) < 2:
        return None
    h2 = (raw[0] >> 6) & 1
    at = 35 if h2 else 19
    if raw[1] >= 128 or len(raw) < at:
        return None
    return h2, raw[1], raw[2:18] if h2 else None, raw[at - 17:at - 1], at


def decide(raw, dests, transport_id, nh_mtu):
    """The rules that need no key.  (status, None) or (ACCEPTED, (dest, link_id,
    mtu, peer_pub, peer_sig_pub))."""
    u = unpack(raw)
    if u is None or raw[0] & 3 != LINKREQUEST:
        return NOT_REQUEST, None
    h2, _, tid, dh, at = u
    if h2 and tid != transport_id:
        return OTHER_TRANSPORT, None
    dest = next((d for d in dests if d.hash == dh), None)
    if dest is None or (raw[0] >> 2) & 3 != SINGLE:
        return NO_DESTINATION, None
    if not dest.flags & F_ACCEPTS:
        return NOT_ACCEPTING, None
    data = raw[at:]
    hashable = bytes([raw[0] & 0x0F]) + (raw[18:] if h2 else raw[2:])
    path_mtu = int.from_bytes(data[64:67], "big") & MTU_MASK if len(data) == 67 else 0
    mode = (data[64] & 0xE0) >> 5 if len(data) > 64 else MODE_AES256_CBC
    if path_mtu:
        if nh_mtu is None:
            data, path_mtu = data[:-3], 0          # the packet, and so the link id, keeps the three bytes
        elif nh_mtu < path_mtu:
            if mode != MODE_AES256_CBC:
                return BAD_MODE, None
            path_mtu = nh_mtu & MTU_MASK
    if len(data) not in (64, 67):
        return BAD_SIZE, None
    mode = (data[64] & 0xE0) >> 5 if len(data) == 67 else MODE_AES256_CBC
    if mode != MODE_AES256_CBC:
        return BAD_MODE, None
    if len(data) > 64:
        hashable = hashable[:-(len(data) - 64)]
    link_id = hashlib.sha256(hashable).digest()[:16]
    return ACCEPTED, (dest, link_id, path_mtu or MTU, data[:32], data[32:64])


def establish(dest, link_id, mtu, peer_pub, ephemeral):
    """(derived_key, LRPROOF packet) of an accepted request."""
    pub = x25519(ephemeral, (9).to_bytes(32, "little"))
    derived = hkdf(64, x25519(ephemeral, peer_pub), link_id)
    sg = signalling(mtu)
    signature = ed.sign(dest.seed, link_id + pub + dest.public + sg, dest.public)
    return derived, bytes([0x0F, 0]) + link_id + b"\xff" + signature + pub + sg


def accept(raws, dests, transport_id, nh_mtu, slots, ephemerals, table, n_keys, n_links=None):
    """The stage over a batch, in index order.  ``table`` (dict link id ->
    slot) is updated.  Per record a dict: status, slot, link_id, mtu, and for an
    accepted one derived_key, lrproof, peer_sig_pub, dest."""
    out, r = [], 0
    for raw in raws:
        st, v = decide(raw, dests, transport_id, nh_mtu)
        rec = {"status": st, "slot": -1, "link_id": None, "mtu": None, "lrproof": None}
        if st == ACCEPTED:
            dest, link_id, mtu, peer_pub, peer_sig = v
            rec.update(link_id=link_id, mtu=mtu)
            mine, r = r, r + 1
            limit = n_keys if n_links is None else min(n_keys, n_links)
            if mine >= len(slots) or not 0 <= slots[mine] < limit:
                rec["status"] = NO_SLOT
            elif link_id in table:
                rec["status"] = DUPLICATE
            else:
                table[link_id] = slots[mine]
                key, proof = establish(dest, link_id, mtu, peer_pub, ephemerals[mine])
                rec.update(slot=slots[mine], derived_key=key, lrproof=proof, peer_sig_pub=peer_sig, dest=dest)
        out.append(rec)
    return out


def fixture_dests(v):
    return [Dest(d["hash"], d["seed"], (F_ACCEPTS if d["accepts"] else 0) | (F_PROVE_ALL if k == 0 else 0)
                 | (F_HAS_CHANNEL if k == 1 else 0)) for k, d in enumerate(v["destinations"])]
