"""A plain model of the link request proof stage (the initiator side of link
establishment: Transport.py:2270-2318, Link.py:391-451) for the tests:
hashlib, ed25519_ref and the RFC 7748 ladder of link_accept_helpers, tied to
tests/golden/link_proof_vectors.json bit for bit."""
import hashlib
import json
import os

import ed25519_ref as ed
from link_accept_helpers import hkdf, signalling, unpack, x25519

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "link_proof_vectors.json")

ACTIVATED, NOT_LRPROOF, NO_LINK, NOT_PENDING, HOPS, BAD_SIZE, BAD_MODE, BAD_SIGNATURE, NO_SLOT = 0, 1, 2, 3, 4, 6, 7, 8, 9
STATUS = {"ACTIVATED": ACTIVATED, "NOT_LRPROOF": NOT_LRPROOF, "NO_LINK": NO_LINK, "NOT_PENDING": NOT_PENDING,
          "HOPS": HOPS, "BAD_SIZE": BAD_SIZE, "BAD_MODE": BAD_MODE, "BAD_SIGNATURE": BAD_SIGNATURE, "NO_SLOT": NO_SLOT}
PENDING, HANDSHAKE, ACTIVE, CLOSED = 0, 1, 2, 4
STATE = {"PENDING": PENDING, "HANDSHAKE": HANDSHAKE, "ACTIVE": ACTIVE, "CLOSED": CLOSED}
PKT_PROOF, CTX_LRPROOF, MODE_AES256_CBC, MTU_MASK, MTU = 3, 0xFF, 1, 0x1FFFFF, 500


def vectors():
    with open(VECTORS) as f:
        v = json.load(f)
    for d in v["destinations"]:
        d["private_key"] = bytes.fromhex(d["private_key"])
        d["sig_public"] = ed.public_key(d["private_key"][32:])
        d["hash"] = bytes.fromhex(d["hash"])
    v["transport_id"] = bytes.fromhex(v["transport_id"])
    for c in v["cases"]:
        for k in ("prv", "sig_seed", "request", "link_id"):
            c["link"][k] = bytes.fromhex(c["link"][k])
        for p in c["packets"]:
            p["raw"] = bytes.fromhex(p["raw"])
            for k in ("derived_key", "lrrtt"):
                if p["after"][k] is not None:
                    p["after"][k] = bytes.fromhex(p["after"][k])
    return v


class Pending:
    """One pending link as the device keeps it."""

    def __init__(self, link_id, prv, dest_public, sig_seed=bytes(32), flags=0, slot=0, expected_hops=1,
                 rebalanced=False):
        self.link_id, self.prv, self.dest_public, self.sig_seed = link_id, prv, dest_public, sig_seed
        self.flags, self.slot, self.expected_hops, self.rebalanced = flags, slot, expected_hops, rebalanced
        self.state, self.mtu, self.derived_key, self.peer_pub = PENDING, 0, None, None

    def copy(self):
        p = Pending(self.link_id, self.prv, self.dest_public, self.sig_seed, self.flags, self.slot,
                    self.expected_hops, self.rebalanced)
        p.state, p.mtu, p.derived_key, p.peer_pub = self.state, self.mtu, self.derived_key, self.peer_pub
        return p


def packet_hash(raw):
    h2 = (raw[0] >> 6) & 1
    return hashlib.sha256(bytes([raw[0] & 0x0F]) + (raw[18:] if h2 else raw[2:])).digest()


def step(raw, pending, room=lambda link: True):
    """One packet against ``pending`` (dict link id -> Pending), as
    Transport.inbound takes it.  Returns (status, remembered): what the device
    stage reports, and whether the packet's hash enters the hash list.
    ``room(link)``: whether the link's slot can be taken (else NO_SLOT)."""
    u = unpack(raw)
    if u is None or raw[0] & 3 != PKT_PROOF or raw[u[4] - 1] != CTX_LRPROOF:
        return NOT_LRPROOF, False
    _, hops, _, link_id, at = u
    hops += 1                                           # Transport.py:1496
    data = raw[at:]
    link = pending.get(link_id)
    if link is None:
        return NO_LINK, False
    if link.state == ACTIVE:                            # no longer among the pending links
        return NOT_PENDING, False
    if link.state != PENDING:
        return NOT_PENDING, hops == link.expected_hops
    good_len = len(data) in (96, 99)
    mode = data[96] >> 5 if len(data) > 96 else MODE_AES256_CBC
    confirmed = int.from_bytes(data[96:99], "big") & MTU_MASK if len(data) == 99 else None
    sig_ok = None
    if good_len and mode == MODE_AES256_CBC:
        signed = link_id + data[64:96] + link.dest_public + (signalling(confirmed) if len(data) == 99 else b"")
        sig_ok = ed.verify(link.dest_public, data[:64], signed)
    if hops != link.expected_hops:
        if not (sig_ok and not link.rebalanced):
            return HOPS, False
        if not room(link):
            return NO_SLOT, False
        link.rebalanced, link.expected_hops = True, hops
    if mode != MODE_AES256_CBC:
        link.state = CLOSED
        return BAD_MODE, True
    if not good_len:
        return BAD_SIZE, True
    if not sig_ok:
        link.state = HANDSHAKE
        return BAD_SIGNATURE, True
    if not room(link):
        return NO_SLOT, False
    link.peer_pub = data[64:96]
    link.derived_key = hkdf(64, x25519(link.prv, link.peer_pub), link_id)
    link.state, link.mtu = ACTIVE, confirmed or MTU
    return ACTIVATED, True


def run(raws, pending, table=None, n_keys=1 << 30, n_links=None, table_room=1 << 30):
    """A batch in index order.  ``table`` (dict link id -> slot) gains the
    activated links.  Returns per record (status, slot or -1, mtu, remembered)."""
    table = {} if table is None else table

    def room(link):
        limit = n_keys if n_links is None else min(n_keys, n_links)
        return 0 <= link.slot < limit and link.link_id not in table and len(table) < table_room

    out, stalled = [], set()
    for raw in raws:
        hit = pending.get(unpack(raw)[3]) if unpack(raw) else None
        if hit is not None and hit.link_id in stalled and raw[0] & 3 == PKT_PROOF and raw[unpack(raw)[4] - 1] == 0xFF:
            # the one rule of the batch that is the device's own: a proof that found no slot has still decided
            # its link for the rest of the call, though the row stays PENDING for the next one
            out.append((NOT_PENDING, -1, 0, False))
            continue
        st, rem = step(raw, pending, room)
        if st == NO_SLOT:
            stalled.add(hit.link_id)
        if st == ACTIVATED:
            table[hit.link_id] = hit.slot
            out.append((st, hit.slot, hit.mtu, rem))
        else:
            out.append((st, -1, 0, rem))
    return out


def fixture_link(vec, case, slot=0, flags=0):
    lk = case["link"]
    return Pending(lk["link_id"], lk["prv"], vec["destinations"][lk["dest"]]["sig_public"], lk["sig_seed"], flags, slot,
                   lk["expected_hops"], lk["rebalanced"])
