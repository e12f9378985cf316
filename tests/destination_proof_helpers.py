"""A plain model of settling the proofs for packets sent to SINGLE
destinations — TEST ONLY.

What DestinationReceipts and device.destination_proof_settle are to compute
(include/rnstok.h), on raw packets in plain Python: the unpack is oracle.wire's,
the table link_helpers', the signatures tests/ed25519_ref.py's.
tests/test_destination_proof.py ties every rule here to what the reference's
own Transport.inbound was recorded doing with real receipts
(tests/golden/destination_proof_vectors.json, written by
tests/golden/gen_destination_proof.py)."""
import functools
import json
import os

import ed25519_ref as ed
import link_helpers as lh
from oracle import wire as ow

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "destination_proof_vectors.json")

DELIVERED, NOT_PROOF, ON_LINK, BAD_LENGTH, NO_RECEIPT, BAD_SIGNATURE, DEFERRED = range(7)     # RT_DPROOF_*
LRPROOF = 0xFF
IMPLICIT, EXPLICIT = 64, 96


def vectors():
    with open(VECTORS) as f:
        return json.load(f)


sign = functools.lru_cache(maxsize=None)(ed.sign)
verify = functools.lru_cache(maxsize=None)(ed.verify)
public_key = functools.lru_cache(maxsize=None)(ed.public_key)
unpack = ow.unpack


def proof_packet(packet_hash, seed, implicit, address=None, dtype=lh.SINGLE, context=lh.NONE):
    """The PROOF packet Identity.prove sends for a packet (Identity.py:942-953,
    Packet.py:376-381), or one addressed elsewhere."""
    address = packet_hash[:16] if address is None else address
    sig = sign(seed, packet_hash)
    return bytes([dtype << 2 | lh.PROOF, 0]) + address + bytes([context]) + (sig if implicit else packet_hash + sig)


class Receipts:
    """DestinationReceipts: hash[:16] -> id beside hash and key (None: not keyed) by id."""

    def __init__(self, max_receipts):
        self.max_receipts = max_receipts
        self.table = lh.TableModel(max_receipts)
        self.hashes, self.keys = {}, {}

    def add(self, hashes, ids, keys=None):
        st = self.table.insert([h[:16] for h in hashes], ids)
        for k, (h, i, s) in enumerate(zip(hashes, ids, st)):
            if s == lh.OK:
                self.hashes[int(i)] = h
                self.keys[int(i)] = None if keys is None else keys[k]
        return st

    def remove(self, hashes):
        return self.table.remove([h[:16] for h in hashes])

    def live_keyed(self):
        return sorted(i for i in self.table.entries.values() if self.keys.get(i) is not None)

    def __len__(self):
        return len(self.table)


def settle(packets, receipts, scan_trials, links=None, n_links=0):
    """rt_destination_proof_settle over a batch: packets are oracle.wire.unpack's
    fields (None: dropped), links the link table's value per packet (-1: none)
    or None.  Returns [(status, receipt id or -1)] and removes what was
    delivered from ``receipts``.  A proof is judged against the receipts
    outstanding at the start of the call; a receipt goes to the lowest index
    that validates it."""
    at_start = dict(receipts.table.entries)
    live = receipts.live_keyed()
    L = len(live)
    gone, strays, out = set(), 0, []

    def deliver(rid):
        if rid in gone:
            return NO_RECEIPT, -1
        gone.add(rid)
        del receipts.table.entries[receipts.hashes[rid][:16]]
        return DELIVERED, rid

    for k, f in enumerate(packets):
        if f is None or f["packet_type"] != lh.PROOF or f["context"] in (LRPROOF, lh.RESOURCE_PRF):
            out.append((NOT_PROOF, -1))
            continue
        if f["destination_type"] == lh.LINK and links is not None and 0 <= links[k] < n_links:
            out.append((ON_LINK, -1))
            continue
        data = f["data"]
        if len(data) not in (IMPLICIT, EXPLICIT):
            out.append((BAD_LENGTH, -1))
            continue
        if len(data) == EXPLICIT:
            h, sig = data[:32], data[32:]
            rid = at_start.get(h[:16])
            if rid is None or receipts.hashes[rid] != h or receipts.keys[rid] is None:
                out.append((NO_RECEIPT, -1))
            elif verify(receipts.keys[rid], sig, h):
                out.append(deliver(rid))
            else:
                out.append((NO_RECEIPT if rid in gone else BAD_SIGNATURE, -1))
            continue
        rid = at_start.get(f["destination_hash"])
        if rid is not None and receipts.keys[rid] is not None and verify(receipts.keys[rid], data, receipts.hashes[rid]):
            out.append(deliver(rid))
            continue
        # a stray: every live keyed receipt, where its frame fits the budget
        rank, strays = strays, strays + 1
        if L == 0:
            out.append((NO_RECEIPT, -1))
        elif (rank + 1) * L > scan_trials:
            out.append((DEFERRED, -1))
        else:
            hit = [i for i in live if verify(receipts.keys[i], data, receipts.hashes[i])]
            out.append(deliver(hit[0]) if hit else (NO_RECEIPT, -1))
    return out
