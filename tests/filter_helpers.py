"""A plain model of the packet filter and the packet hash list — TEST ONLY.

Two Python sets stand for Transport.packet_hashlist and packet_hashlist_prev;
the rules are Transport.packet_filter (Transport.py:1377-1427) and the
remember step of Transport.inbound (Transport.py:1525-1545), the cull is the
job loop's (Transport.py:656-658), and the overflow rule is the device list's
own (a generation holds at most max_hashes entries).  tests/test_packet_filter.py
ties the model to what the reference itself was recorded doing
(tests/golden/filter_vectors.json, made by gen_filter.py)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = os.path.join(ROOT, "tests", "golden", "filter_vectors.json")

PASS, NO_PACKET, OTHER_TRANSPORT, BAD_ANNOUNCE, HOPS, DUPLICATE = range(6)      # RT_FILTER_*
OK, MISSING = 0, 3                                                              # RT_LINK_OK, RT_LINK_MISSING
DATA, ANNOUNCE, LINKREQUEST, PROOF = 0, 1, 2, 3                                 # Packet.py:60-63
SINGLE, GROUP, PLAIN, LINK = 0, 1, 2, 3                                         # Destination.py types
HEADER_1, HEADER_2 = 0, 1
NONE, RESOURCE, RESOURCE_REQ, RESOURCE_PRF, CACHE_REQUEST, CHANNEL = 0x00, 0x01, 0x03, 0x05, 0x08, 0x0E
KEEPALIVE, LRPROOF = 0xFA, 0xFF
ALWAYS = frozenset((KEEPALIVE, RESOURCE_REQ, RESOURCE_PRF, RESOURCE, CACHE_REQUEST, CHANNEL))


def vectors():
    with open(VECTORS) as f:
        return json.load(f)


def capacity(max_hashes):
    c = 2
    while c < 2 * max_hashes:
        c *= 2
    return c


def decide(p, own, present):
    """The status of one packet: p is a dict with ok, header_type,
    packet_type, destination_type, context, hops (as on the wire) and
    transport_id; ``present``: its hash is in either set."""
    if not p["ok"]:
        return NO_PACKET
    if p["header_type"] == HEADER_2 and p["packet_type"] != ANNOUNCE and p["transport_id"] != own:
        return OTHER_TRANSPORT
    if p["context"] in ALWAYS:
        return PASS
    if p["destination_type"] in (PLAIN, GROUP):
        if p["packet_type"] == ANNOUNCE:
            return BAD_ANNOUNCE
        return HOPS if p["hops"] + 1 > 1 else PASS
    if not present:
        return PASS
    if p["packet_type"] == ANNOUNCE:
        return PASS if p["destination_type"] == SINGLE else BAD_ANNOUNCE
    return DUPLICATE


class ListModel:
    def __init__(self, max_hashes, own=bytes(16)):
        self.max = max_hashes
        self.capacity = capacity(max_hashes)
        self.own = own
        self.current, self.previous, self.overflow = set(), set(), 0

    def _enter(self, h):
        """Transport.add_packet_hash, with the device list's rule for a full generation."""
        if h not in self.current and len(self.current) >= self.max:
            self.overflow += 1
            return False
        self.current.add(h)
        return True

    def add(self, hashes):
        for h in hashes:
            self._enter(h)

    def packet(self, p, transit=()):
        """(status, remembered) of one packet, processed after all before it."""
        h = p["packet_hash"]
        status = decide(p, self.own, h in self.current or h in self.previous)
        if status != PASS:
            return status, False
        if (p["packet_type"] == PROOF and p["context"] == LRPROOF) or p["destination_hash"] in transit:
            return status, False
        return status, self._enter(h)

    def filter(self, packets, transit=()):
        return [self.packet(p, transit)[0] for p in packets]

    def cull(self):
        if len(self.current) > self.max // 2:
            self.previous, self.current = self.current, set()
            return True
        return False

    def remove(self, hashes):
        out = []
        for h in hashes:
            out.append(OK if h in self.current else MISSING)
            self.current.discard(h)
        return out

    def contains(self, hashes):
        return [1 if h in self.current else 2 if h in self.previous else 0 for h in hashes]

    def counts(self):
        return len(self.current), len(self.previous), self.overflow


def packet(packet_hash, packet_type=DATA, destination_type=SINGLE, context=NONE, hops=0, header_type=HEADER_1,
           transport_id=bytes(16), destination_hash=bytes(16), ok=1):
    return {"ok": ok, "header_type": header_type, "packet_type": packet_type, "destination_type": destination_type,
            "context": context, "hops": hops, "transport_id": transport_id, "destination_hash": destination_hash,
            "packet_hash": packet_hash}


def records(packets):
    """The packets as rt_packet_fields records ((n, 96) uint8), forged: only
    the bytes the filter reads are filled in."""
    out = np.zeros((len(packets), 96), dtype=np.uint8)
    for r, p in zip(out, packets):
        r[0], r[2], r[3] = p["ok"], p["hops"], p["header_type"]
        r[1] = p["header_type"] << 6 | p["destination_type"] << 2 | p["packet_type"]
        r[6], r[7], r[8] = p["destination_type"], p["packet_type"], p["context"]
        r[20:36] = np.frombuffer(p["transport_id"], np.uint8)
        r[36:52] = np.frombuffer(p["destination_hash"], np.uint8)
        r[52:84] = np.frombuffer(p["packet_hash"], np.uint8)
    return out


def hashes_for_home(rng, cap, home, n, tag=None):
    """n distinct 32-byte hashes whose home slot (bytes 0..3, little endian,
    modulo the capacity) is `home`; with `tag` they also share bytes 4..7."""
    out = []
    while len(out) < n:
        b = bytearray(rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
        w = (int.from_bytes(b[0:4], "little") & ~(cap - 1)) | home
        b[0:4] = (w & 0xFFFFFFFF).to_bytes(4, "little")
        if tag is not None:
            b[4:8] = tag
        if bytes(b) not in out:
            out.append(bytes(b))
    return out
