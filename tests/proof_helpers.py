"""A plain model of the packet proofs of a link — TEST ONLY.

What device.link_prove, ReceiptTable and device.proof_settle are to compute
(include/rnstok.h), on raw packets in plain Python: the unpack is oracle.wire's,
the route rule link_helpers', the signatures tests/ed25519_ref.py's.
tests/test_proof.py ties every rule here to what the reference's own
Link.receive, prove_packet and Transport PROOF branch were recorded doing
(tests/golden/proof_vectors.json, written by tests/golden/gen_proof.py)."""
import functools
import json
import os

import ed25519_ref as ed
import link_helpers as lh
from oracle import wire as ow

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proof_vectors.json")

PROVE_ALL, HAS_CHANNEL = 1, 2                                          # RT_LINK_* flags
DELIVERED, NOT_PROOF, NOT_LINK, NO_LINK, SHORT, NO_RECEIPT, BAD_SIGNATURE = range(7)   # RT_PROOF_*
LRPROOF = 0xFF
PROOF_LEN = 115
TOKEN_OK = 0


def vectors():
    with open(VECTORS) as f:
        return json.load(f)


sign = functools.lru_cache(maxsize=None)(ed.sign)
verify = functools.lru_cache(maxsize=None)(ed.verify)
public_key = functools.lru_cache(maxsize=None)(ed.public_key)


class Signers:
    """seeds: one per link or one for all; peer_publics and flags one per link."""

    def __init__(self, seeds, peer_publics, flags):
        self.n_links = len(peer_publics)
        self.seeds = list(seeds) * (self.n_links if len(seeds) == 1 else 1)
        self.peer_publics, self.flags = list(peer_publics), list(flags)
        assert len(self.seeds) == len(self.flags) == self.n_links


def proof_packet(link_id, packet_hash, seed):
    """Link.prove_packet's packet as Packet.pack writes it (Packet.py:199-200)."""
    return bytes([lh.LINK << 2 | lh.PROOF, 0]) + link_id + bytes([lh.NONE]) + packet_hash + sign(seed, packet_hash)


def prove(f, route, link, token_status, signers):
    """The proof of one packet (f: oracle.wire.unpack's fields, or None where
    an earlier stage dropped it), or None: rt_link_prove's rule."""
    if f is None or f["packet_type"] != lh.DATA or not 0 <= link < signers.n_links:
        return None
    flags = signers.flags[link]
    if f["context"] == lh.CHANNEL:
        proved = bool(flags & HAS_CHANNEL)
    elif f["context"] == lh.NONE:
        proved = bool(flags & PROVE_ALL) and route == lh.LINK_DECRYPT and token_status == TOKEN_OK
    else:
        proved = False
    return proof_packet(f["destination_hash"], f["packet_hash"], signers.seeds[link]) if proved else None


class Receipts:
    """ReceiptTable: hash[:16] -> id beside the full hashes by id."""

    def __init__(self, max_receipts):
        self.table = lh.TableModel(max_receipts)
        self.hashes = {}

    def add(self, hashes, ids):
        st = self.table.insert([h[:16] for h in hashes], ids)
        for h, i, s in zip(hashes, ids, st):
            if s == lh.OK:
                self.hashes[int(i)] = h
        return st

    def remove(self, hashes):
        return self.table.remove([h[:16] for h in hashes])

    def __len__(self):
        return len(self.table)


def settle(packets, links, signers, receipts):
    """rt_proof_settle over a batch, one packet after another: packets are
    oracle.wire.unpack's fields (None: dropped), links the link table's value
    per packet (-1: none).  Returns [(status, receipt id or -1)] and removes
    what was delivered from ``receipts``."""
    out = []
    for f, link in zip(packets, links):
        if f is None or f["packet_type"] != lh.PROOF or f["context"] in (LRPROOF, lh.RESOURCE_PRF):
            out.append((NOT_PROOF, -1))
        elif f["destination_type"] != lh.LINK:
            out.append((NOT_LINK, -1))
        elif not 0 <= link < signers.n_links:
            out.append((NO_LINK, -1))
        elif len(f["data"]) < 96:
            out.append((SHORT, -1))
        else:
            h, sig = f["data"][:32], f["data"][32:96]
            rid = receipts.table.entries.get(h[:16])
            if rid is None or receipts.hashes.get(rid) != h:
                out.append((NO_RECEIPT, -1))
            elif not verify(signers.peer_publics[link], sig, h):
                out.append((BAD_SIGNATURE, -1))
            else:
                del receipts.table.entries[h[:16]]
                out.append((DELIVERED, rid))
    return out


def link_of(f, table):
    """link_spans' (route, link) for unpacked fields f; table: link id -> value."""
    if f is None:
        return lh.NOT_LINK, -1
    r, link, _ = lh.route(True, f["destination_type"], f["packet_type"], f["context"],
                          table.get(f["destination_hash"]))
    return r, link


unpack = ow.unpack
