"""A plain model of destination delivery (Transport.py:2188-2202,
Destination.py:414-429, 622-654, Identity.py:848-898, 942-953) for the tests:
hashlib, oracle/cpuref.py's token, tests/ed25519_ref.py and the RFC 7748 ladder
of tests/link_accept_helpers.py; no device and no reference code.
tests/test_destination_deliver.py ties it to the fixture bit for bit; the GPU
tests compare the device stage against it."""
import hashlib
import json
import os

import ed25519_ref as ed
from link_accept_helpers import hkdf, unpack
from link_accept_helpers import x25519 as _ladder
from oracle import cpuref

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "destination_deliver_vectors.json")

DELIVERED, NOT_DATA, NO_DESTINATION, TYPE_MISMATCH, SHORT, NOT_OPENED, DEFERRED = 0, 1, 2, 3, 4, 5, 6
STATUS = {"DELIVERED": DELIVERED, "NOT_DATA": NOT_DATA, "NO_DESTINATION": NO_DESTINATION,
          "TYPE_MISMATCH": TYPE_MISMATCH, "SHORT": SHORT, "NOT_OPENED": NOT_OPENED, "DEFERRED": DEFERRED}
F_PROVE_ALL, F_ENFORCE = 1, 8
DATA, SINGLE, GROUP, PLAIN, LINK = 0, 0, 1, 2, 3
ST_OK, ST_TOO_SHORT, ST_BAD_HMAC, ST_BAD_CT_LEN, ST_BAD_PAD = 0, 1, 2, 3, 4
BASE = (9).to_bytes(32, "little")

_exchanges = {}


def x25519(scalar, point):
    """The ladder, remembered: the tests reuse a few ephemeral keys."""
    k = (bytes(scalar), bytes(point))
    if k not in _exchanges:
        _exchanges[k] = _ladder(*k)
    return _exchanges[k]


def vectors():
    with open(VECTORS) as f:
        v = json.load(f)
    for d in v["destinations"]:
        for k in ("private_key", "hash", "identity_hash"):
            d[k] = bytes.fromhex(d[k])
        d["ratchets"] = [bytes.fromhex(r) for r in d["ratchets"]]
    v["transport_id"] = bytes.fromhex(v["transport_id"])
    for c in v["cases"]:
        c["raw"] = bytes.fromhex(c["raw"])
        for k in ("plaintext", "proof"):
            if c[k] is not None:
                c[k] = bytes.fromhex(c[k])
    return v


class Dest:
    def __init__(self, hash_, private_key, identity_hash, ratchets, flags):
        self.hash, self.prv, self.seed = hash_, private_key[:32], private_key[32:]
        self.identity_hash, self.ratchets, self.flags = identity_hash, list(ratchets), flags
        self.public = ed.public_key(self.seed)

    def candidates(self):
        return self.ratchets + ([] if self.flags & F_ENFORCE else [self.prv])


def fixture_dests(v):
    return [Dest(d["hash"], d["private_key"], d["identity_hash"], d["ratchets"],
                 (F_PROVE_ALL if d["prove"] == "ALL" else 0) | (F_ENFORCE if d["enforce"] else 0))
            for d in v["destinations"]]


def make_dest(rng, n_ratchets, flags):
    """A destination with keys from ``rng`` (numpy Generator); the identity hash
    and the destination hash are what the reference derives them from."""
    rb = lambda n: rng.integers(0, 256, n, dtype="uint8").tobytes()      # noqa: E731
    prv, seed = rb(32), rb(32)
    identity_hash = hashlib.sha256(x25519(prv, BASE) + ed.public_key(seed)).digest()[:16]
    name_hash = hashlib.sha256(b"deliver.test").digest()[:10]
    dest_hash = hashlib.sha256(name_hash + identity_hash).digest()[:16]
    return Dest(dest_hash, prv + seed, identity_hash, [rb(32) for _ in range(n_ratchets)], flags)


def packet_hash(raw):
    h2 = (raw[0] >> 6) & 1
    return hashlib.sha256(bytes([raw[0] & 0x0F]) + (raw[18:] if h2 else raw[2:])).digest()


def token_key(candidate, eph_pub, identity_hash):
    return hkdf(64, x25519(candidate, eph_pub), identity_hash)


def seal(dest, rank, pt, eph_prv, iv):
    """data = ephemeral public key ‖ token for candidate ``rank`` of ``dest``
    (None: the identity's key), as Identity.encrypt builds it."""
    target = dest.prv if rank is None else dest.ratchets[rank]
    eph_pub = x25519(eph_prv, BASE)
    key = hkdf(64, x25519(eph_prv, x25519(target, BASE)), dest.identity_hash)
    return eph_pub + cpuref.encrypt(key, iv, pt)


def packet(data, dest_hash, dtype=SINGLE, ptype=DATA, header2=None, hops=0, context=0):
    flags = (dtype << 2) | ptype
    if header2 is None:
        return bytes([flags, hops]) + dest_hash + bytes([context]) + data
    return bytes([flags | 0x40 | 0x10, hops]) + header2 + dest_hash + bytes([context]) + data


def _verifies(key, token):
    return cpuref.hmac_sha256(key[:32], token[:-32]) == token[-32:]


def proof_packet(dest, raw, implicit):
    ph = packet_hash(raw)
    sig = ed.sign(dest.seed, ph, dest.public)
    return bytes([0x03, 0]) + ph[:16] + b"\x00" + (b"" if implicit else ph) + sig


def deliver(raws, dests, retry_trials, implicit=True):
    """The stage over a batch, in index order.  Per record a dict: status,
    dest (row or -1), ratchet, and for DELIVERED / NOT_OPENED frames
    token_status, plaintext (DELIVERED) and proof (or None)."""
    out, undecided = [], []
    for i, raw in enumerate(raws):
        rec = {"status": NOT_DATA, "dest": -1, "ratchet": -1, "token_status": None, "plaintext": None, "proof": None}
        out.append(rec)
        u = unpack(raw)
        if u is None or raw[0] & 3 != DATA or (raw[0] >> 2) & 3 == LINK:
            continue
        dh, at = u[3], u[4]
        row = next((k for k, d in enumerate(dests) if d.hash == dh), None)
        if row is None:
            rec["status"] = NO_DESTINATION
            continue
        rec["dest"] = row
        if (raw[0] >> 2) & 3 != SINGLE:
            rec["status"] = TYPE_MISMATCH
            continue
        data = raw[at:]
        if len(data) <= 32:
            rec["status"] = SHORT
            continue
        d, eph, token = dests[row], data[:32], data[32:]
        cands = d.candidates()
        rec["status"] = NOT_OPENED
        rec["token_status"] = ST_TOO_SHORT if len(token) <= 32 else ST_BAD_HMAC
        if not cands or len(token) < 64 or (len(token) - 48) % 16:
            continue
        if _verifies(token_key(cands[0], eph, d.identity_hash), token):
            rec["winner"] = 0
        elif len(cands) > 1:
            undecided.append(i)
    # the second pass: whole frames into the budget, in stream order
    start = 0
    for i in undecided:
        raw = raws[i]
        at = unpack(raw)[4]
        d = dests[out[i]["dest"]]
        cands, eph, token = d.candidates(), raw[at:at + 32], raw[at + 32:]
        ask = min(len(cands) - 1, retry_trials + 1)
        fits = start + ask <= retry_trials
        start += ask
        if not fits:
            out[i].update(status=DEFERRED, token_status=None)
            continue
        for c in range(1, len(cands)):
            if _verifies(token_key(cands[c], eph, d.identity_hash), token):
                out[i]["winner"] = c
                break
    for i, rec in enumerate(out):
        c = rec.pop("winner", None)
        if c is None:
            continue
        raw = raws[i]
        at = unpack(raw)[4]
        d = dests[rec["dest"]]
        st, pt = cpuref.decrypt(token_key(d.candidates()[c], raw[at:at + 32], d.identity_hash), raw[at + 32:])
        rec["token_status"] = st
        if st == ST_OK:
            rec.update(status=DELIVERED, plaintext=pt, ratchet=c if c < len(d.ratchets) else -1)
            if d.flags & F_PROVE_ALL:
                rec["proof"] = proof_packet(d, raw, implicit)
    return out


def second_pass_pairs(raws, dests):
    """The retry budget with which no frame of the batch is deferred: the
    remaining candidates of every frame its first candidate does not open."""
    big = 1 << 30
    res = deliver(raws, dests, big)
    total = 0
    for raw, rec in zip(raws, res):
        if rec["status"] in (DELIVERED, NOT_OPENED) and rec["token_status"] is not None:
            d = dests[rec["dest"]]
            cands = d.candidates()
            at = unpack(raw)[4]
            token = raw[at + 32:]
            if not cands or len(token) < 64 or (len(token) - 48) % 16:
                continue
            if not _verifies(token_key(cands[0], raw[at:at + 32], d.identity_hash), token):
                total += len(cands) - 1
    return total
