"""A plain model of the link table and of the route rule — TEST ONLY.

The table is a dict (id -> value) beside the capacity; the route rule is
Transport.inbound's walk of active_links (Transport.py:2161-2176) followed by
Link.receive's branches (Link.py:941-1158), written out as sets of constants.
tests/test_link.py ties the context rule to what the reference's own
Link.receive was recorded doing (tests/golden/link_vectors.json)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = os.path.join(ROOT, "tests", "golden", "link_vectors.json")

OK, DUPLICATE, FULL, MISSING = 0, 1, 2, 3                          # RT_LINK_*
NOT_LINK, NO_LINK, LINK_PLAIN, LINK_DECRYPT = 0, 1, 2, 3           # RT_ROUTE_*
DATA, ANNOUNCE, LINKREQUEST, PROOF = 0, 1, 2, 3                    # Packet.py:60-63
SINGLE, GROUP, PLAIN, LINK = 0, 1, 2, 3                            # Destination.py types
# Packet.py:72-92: the contexts whose branch of Link.receive calls decrypt
NONE, RESOURCE, RESOURCE_ADV, RESOURCE_REQ, RESOURCE_HMU, RESOURCE_PRF, RESOURCE_ICL, RESOURCE_RCL = range(8)
CACHE_REQUEST, REQUEST, RESPONSE, CHANNEL = 0x08, 0x09, 0x0A, 0x0E
KEEPALIVE, LINKIDENTIFY, LINKCLOSE, LRRTT = 0xFA, 0xFB, 0xFC, 0xFE
DECRYPTED = frozenset((NONE, LINKIDENTIFY, REQUEST, RESPONSE, LRRTT, LINKCLOSE, RESOURCE_ADV, RESOURCE_REQ,
                       RESOURCE_HMU, RESOURCE_ICL, RESOURCE_RCL, CHANNEL))


def vectors():
    with open(VECTORS) as f:
        return json.load(f)


def capacity(max_links):
    c = 2
    while c < 2 * max_links:
        c *= 2
    return c


class TableModel:
    def __init__(self, max_links):
        self.capacity = capacity(max_links)
        self.entries = {}

    def insert(self, ids, values):
        """Statuses of a batch.  A batch that would overfill the table is not
        modelled: which of its new ids get the last slots is unspecified."""
        out = []
        for i, v in zip(ids, values):
            if i in self.entries:
                out.append(DUPLICATE)
            elif len(self.entries) >= self.capacity:
                out.append(FULL)
            else:
                self.entries[i] = int(v)
                out.append(OK)
        return out

    def remove(self, ids):
        return [OK if self.entries.pop(i, None) is not None else MISSING for i in ids]

    def lookup(self, ids):
        return [self.entries.get(i, -1) for i in ids], [i in self.entries for i in ids]

    def __len__(self):
        return len(self.entries)


def route(ok, destination_type, packet_type, context, value, n_keys=1 << 32):
    """(route, link, decrypted) of one packet; value: the table's value for
    its destination hash, or None."""
    if not ok or destination_type != LINK or packet_type not in (DATA, PROOF):
        return NOT_LINK, -1, False
    if value is None:
        return NO_LINK, -1, False
    if packet_type == DATA and context in DECRYPTED and value < n_keys:
        return LINK_DECRYPT, value, True
    return LINK_PLAIN, value, False


def ids_for_home(rng, cap, home, n, tag=None):
    """n distinct ids whose home slot (bytes 0..3, little endian, modulo the
    capacity) is `home`; with `tag` they also share bytes 4..7."""
    out = []
    while len(out) < n:
        b = bytearray(rng.integers(0, 256, 16, dtype=np.uint8).tobytes())
        w = (int.from_bytes(b[0:4], "little") & ~(cap - 1)) | home
        b[0:4] = (w & 0xFFFFFFFF).to_bytes(4, "little")
        if tag is not None:
            b[4:8] = tag
        if bytes(b) not in out:
            out.append(bytes(b))
    return out
