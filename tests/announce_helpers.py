"""A plain model of announce validation for the tests: Packet.unpack by
oracle/wire.py, Identity.validate_announce's cuts and Ed25519 by ed25519_ref.
test_announce.py ties it to the reference's recorded verdicts
(tests/golden/announce_vectors.json); the GPU tests hold the kernels to it."""
import functools
import hashlib
import json
import os

import numpy as np

import ed25519_ref as ref
from oracle import wire as ow

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "announce_vectors.json")

VALID, NOT_ANNOUNCE, SHORT, BAD_SIGNATURE, BAD_DESTINATION = 0, 1, 2, 3, 4      # RT_ANNOUNCE_*
ANNOUNCE, DATA = 1, 0
NONE, PATH_RESPONSE = 0x00, 0x0B
ZERO = bytes(16)


@functools.lru_cache(maxsize=None)
def vectors():
    with open(VECTORS) as f:
        return json.load(f)


def status_of_fields(f):
    """(status, identity hash) for one unpacked packet (oracle.wire.unpack's
    dict, or None where unpack fails)."""
    if f is None or f["packet_type"] != ANNOUNCE:
        return NOT_ANNOUNCE, ZERO
    data, flag = f["data"], f["context_flag"]
    if len(data) < (116 if flag else 84) + 64:
        return SHORT, ZERO
    pub, name_hash, random_hash, ratchet, sig, app = ref.announce_fields(data, flag)
    identity = hashlib.sha256(pub).digest()[:16]
    dest = f["destination_hash"]
    if not ref.verify(pub[32:], sig, dest + pub + name_hash + random_hash + ratchet + app):
        return BAD_SIGNATURE, identity
    if dest != hashlib.sha256(name_hash + identity).digest()[:16]:
        return BAD_DESTINATION, identity
    return VALID, identity


@functools.lru_cache(maxsize=None)
def announce_status_ref(raw):
    """(RT_ANNOUNCE_* status, the identity_hash row) the device must give for
    the raw packet."""
    return status_of_fields(ow.unpack(raw))


class Announcer:
    """An identity that announces: the model's key pair and signatures."""

    def __init__(self, rng):
        self.rng = rng
        self.seed = self.bytes(32)
        self.pub = self.bytes(32) + ref.public_key(self.seed)        # X25519 half (any bytes), Ed25519 half
        self.identity = hashlib.sha256(self.pub).digest()[:16]

    def bytes(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def destination(self, name_hash):
        return hashlib.sha256(name_hash + self.identity).digest()[:16]

    def data(self, app=b"", ratchet=False, name_hash=None, signed_destination=None):
        """(destination hash, announce data); signed for ``signed_destination``
        when given (a valid signature over a hash that is not the identity's)."""
        name_hash = name_hash or self.bytes(10)
        head = self.pub + name_hash + self.bytes(10) + (self.bytes(32) if ratchet else b"")
        dest = signed_destination or self.destination(name_hash)
        sig = ref.sign(self.seed, dest + head + app, self.pub[32:])
        return dest, head + sig + app


def raw_packet(dest, data, ratchet=False, header=0, hops=0, context=NONE, ptype=ANNOUNCE, transport_id=None, dtype=0):
    """Packet.pack's layout; HEADER_2 packets are in TRANSPORT, ``dtype`` is the destination type (0: SINGLE)."""
    flags = header << 6 | int(ratchet) << 5 | header << 4 | dtype << 2 | ptype
    tid = (transport_id or bytes(range(16))) if header else b""
    return bytes([flags, hops]) + tid + dest + bytes([context]) + data

