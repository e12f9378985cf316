"""Generate tests/golden/filter_vectors.json from the reference's own code.

Runs only where the reference is at hand ($RNS_REFERENCE).  Fixtures for the
packet filter and the packet hash list (Transport.py:107-108, 656-658,
1372-1427, 1525-1545):

  cases      for every combination of packet type, destination type, header
             (HEADER_1, HEADER_2 with the node's own transport id, HEADER_2
             with a foreign one), hops 0, 1, 2 on the wire, and context (the
             six contexts packet_filter lets through, LRPROOF, and NONE):
             whether the reference's Transport.inbound handed the packet on
             and whether it remembered its hash, with the hash absent, in
             packet_hashlist, and in packet_hashlist_prev only.  Each row is
             [packet_type, destination_type, header, hops, context,
              passed_absent, remembered_absent, passed_current,
              remembered_current, passed_previous, remembered_previous];
  sequences  replayed packets, one list per scenario: every step is a packet
             (its unpacked fields, its hash, whether its destination hash was
             in Transport.link_table) or a cull, with what the reference did
             and the sizes of the two sets afterwards.  Transport.hashlist_maxsize
             is set to `maxsize` on the class for the scenario.

How the reference is driven: Transport.inbound itself runs on the raw packet
(no interface), with Transport.owner and Transport.identity stubbed,
packet_filter wrapped by a recorder of its result and add_packet_hash by a
recorder that still adds; Transport.local_client_interfaces is an empty list
whose membership test, the first thing inbound does after the remember step
(Transport.py:1551), raises, which ends the call there.  The cull is the
reference's Transport.jobs(), run with nothing else due.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_filter.py
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")

CONTEXTS = (0xFA, 0x03, 0x05, 0x01, 0x08, 0x0E, 0xFF, 0x00)
H1, H2_OWN, H2_FOREIGN = 0, 1, 2


def main():
    sys.path.insert(0, REF)
    import RNS
    from RNS import Transport

    rng = np.random.Generator(np.random.PCG64(1377))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    RNS.loglevel = -1
    own = rb(16)

    class Owner:
        is_connected_to_shared_instance = False

    class Identity:
        hash = own

    class Stop(Exception):
        pass

    class NoClients(list):
        def __contains__(self, item):
            raise Stop()

    Transport.owner = Owner
    Transport.identity = Identity
    Transport.ready = True
    Transport.local_client_interfaces = NoClients()

    seen = {}
    real_filter, real_add = Transport.packet_filter, Transport.add_packet_hash

    def filter_recorder(packet):
        seen["packet"] = packet
        seen["passed"] = real_filter(packet)
        return seen["passed"]

    def add_recorder(packet_hash):
        seen["remembered"] = True
        real_add(packet_hash)

    Transport.packet_filter = staticmethod(filter_recorder)
    Transport.add_packet_hash = staticmethod(add_recorder)

    def make_raw(ptype, dtype, header, hops, context, dest=None, data=None):
        flags = (0x40 | 0x10 if header else 0) | dtype << 2 | ptype
        tid = b"" if header == H1 else own if header == H2_OWN else rb(16)
        return bytes([flags, hops]) + tid + (dest or rb(16)) + bytes([context]) + (data or rb(40))

    def inbound(raw):
        """(passed, remembered, packet) of one run of Transport.inbound."""
        seen.clear()
        try:
            Transport.inbound(raw, None)
        except Stop:
            assert seen.get("passed") is True
        assert "passed" in seen, "the packet did not reach packet_filter"
        return bool(seen["passed"]), bool(seen.get("remembered")), seen["packet"]

    def packet_hash(raw):
        p = RNS.Packet(None, raw)
        assert p.unpack()
        return p.packet_hash

    out = {"reference": "RNS/Transport.py:107-108, 656-658, 1372-1427, 1430-1551 (Transport.inbound itself up to the "
                        "remember step; Transport.jobs for the cull); RNS/Packet.py:242-275, 342-353",
           "generator": "tests/golden/gen_filter.py", "own_transport_id": own.hex(), "contexts": list(CONTEXTS)}

    # --- every combination, with the hash absent, current, previous
    cases = []
    for ptype in range(4):
        for dtype in range(4):
            for header in (H1, H2_OWN, H2_FOREIGN):
                for hops in (0, 1, 2):
                    for context in CONTEXTS:
                        raw = make_raw(ptype, dtype, header, hops, context)
                        h = packet_hash(raw)
                        row = [ptype, dtype, header, hops, context]
                        for where in ("absent", "current", "previous"):
                            Transport.packet_hashlist = {h} if where == "current" else set()
                            Transport.packet_hashlist_prev = {h} if where == "previous" else set()
                            Transport.link_table = {}
                            passed, remembered, p = inbound(raw)
                            assert p.hops == hops + 1 and p.packet_hash == h
                            assert (h in Transport.packet_hashlist) == (remembered or where == "current")
                            # remembering never takes a hash out of the previous set
                            assert (h in Transport.packet_hashlist_prev) == (where == "previous")
                            row += [int(passed), int(remembered)]
                        cases.append(row)
    out["cases"] = cases

    # --- sequences
    def run(maxsize, steps):
        Transport.hashlist_maxsize = maxsize
        Transport.packet_hashlist, Transport.packet_hashlist_prev = set(), set()
        Transport.link_table = {}
        now = time.time() + 3600.0
        for name in dir(Transport):
            if name.endswith("_last_checked"):
                setattr(Transport, name, now)
        rows = []
        for step in steps:
            if step == "cull":
                before = (Transport.packet_hashlist, Transport.packet_hashlist_prev)
                Transport.link_table = {}
                Transport.jobs()
                rotated = Transport.packet_hashlist is not before[0]
                assert rotated == (Transport.packet_hashlist_prev is before[0])
                rows.append({"op": "cull", "rotated": rotated})
            else:
                raw, transit = step
                p0 = RNS.Packet(None, raw)
                assert p0.unpack()
                Transport.link_table = {p0.destination_hash: None} if transit else {}
                passed, remembered, p = inbound(raw)
                rows.append({"op": "packet", "packet_type": p.packet_type, "destination_type": p.destination_type,
                             "header_type": p.header_type, "hops": p0.hops, "context": p.context,
                             "transport_id": p.transport_id.hex() if p.transport_id else None,
                             "destination_hash": p.destination_hash.hex(), "packet_hash": p.packet_hash.hex(),
                             "transit": bool(transit), "passed": passed, "remembered": remembered})
            rows[-1]["current"] = len(Transport.packet_hashlist)
            rows[-1]["previous"] = len(Transport.packet_hashlist_prev)
        return {"maxsize": maxsize, "steps": rows}

    DATA, ANNOUNCE, LINKREQUEST, PROOF = 0, 1, 2, 3
    SINGLE, GROUP, PLAIN, LINK = 0, 1, 2, 3
    sequences = []

    # a link packet replayed, its copy for another transport node, then as relayed to this node
    dest, data = rb(16), rb(60)
    a = make_raw(DATA, LINK, H1, 0, 0x00, dest, data)
    a_foreign = make_raw(DATA, LINK, H2_FOREIGN, 3, 0x00, dest, data)
    a_own = make_raw(DATA, LINK, H2_OWN, 3, 0x00, dest, data)
    assert packet_hash(a) == packet_hash(a_foreign) == packet_hash(a_own)
    sequences.append(run(1000, [(a_foreign, 0), (a, 0), (a, 0), (a_own, 0), (a_foreign, 0)]))

    # announces: SINGLE passes again and again, LINK does not; PLAIN never
    s_ann = make_raw(ANNOUNCE, SINGLE, H1, 0, 0x00)
    l_ann = make_raw(ANNOUNCE, LINK, H1, 0, 0x00)
    p_ann = make_raw(ANNOUNCE, PLAIN, H1, 0, 0x00)
    sequences.append(run(1000, [(s_ann, 0), (s_ann, 0), (l_ann, 0), (l_ann, 0), (p_ann, 0), (p_ann, 0)]))

    # deferred hashes: a link request proof and a packet of a link in transit pass every time
    lrproof = make_raw(PROOF, LINK, H1, 0, 0xFF)
    carried = make_raw(DATA, LINK, H1, 1, 0x00)
    sequences.append(run(1000, [(lrproof, 0), (lrproof, 0), (carried, 1), (carried, 1), (carried, 0), (carried, 0),
                                (carried, 1)]))

    # packets that never consult the list are remembered all the same
    keep = make_raw(DATA, LINK, H1, 0, 0xFA)
    plain = make_raw(DATA, PLAIN, H1, 0, 0x00)
    far = make_raw(DATA, GROUP, H1, 1, 0x00)
    sequences.append(run(1000, [(keep, 0), (keep, 0), (plain, 0), (plain, 0), (far, 0)]))

    # the cull on both sides of its threshold (maxsize 8: more than 4 entries), a hash forgotten only
    # after the second rotation, and a SINGLE announce moved out of the previous set
    pk = [make_raw(DATA, SINGLE, H1, 0, 0x00) for _ in range(12)]
    sequences.append(run(8, [(pk[0], 0), (pk[1], 0), (pk[2], 0), (pk[3], 0), "cull", (pk[0], 0), (pk[4], 0), "cull",
                             (pk[0], 0), (pk[5], 0), "cull", (s_ann, 0), (pk[6], 0), (pk[7], 0), (pk[8], 0),
                             (pk[9], 0), "cull", (s_ann, 0), (pk[0], 0), (pk[6], 0), (pk[10], 0), (pk[11], 0),
                             (pk[5], 0), (keep, 0), "cull", (pk[6], 0), (s_ann, 0), (pk[0], 0)]))
    out["sequences"] = sequences

    path = os.path.join(HERE, "filter_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
