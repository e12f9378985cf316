"""Generate tests/golden/link_accept_vectors.json from the reference's own code.

Runs only where the reference is at hand ($RNS_REFERENCE).  Fixtures for the
responder side of link establishment (Transport.py:2127-2158,
Destination.py:414-435, Link.py:186-227, 336-376).  Real RNS.Destination
objects (IN, SINGLE) registered with Transport, real identities, and every raw
LINKREQUEST handed to the reference's own Transport.inbound(raw, interface)
with a stub interface that carries HW_MTU, AUTOCONFIGURE_MTU and FIXED_MTU:
unpack, the packet filter (from an empty hash list each time), the link
request branch with its transport id rule, destination map, destination type
and MTU step, then Destination.receive -> incoming_link_request ->
Link.validate_request -> handshake, prove all run as they stand.  Packet.send
and Transport.register_link are replaced by recorders,
Destination.incoming_link_request and Link.validate_request are wrapped to
note that they were reached, Link.start_watchdog is replaced by nothing (it
starts a thread), and Reticulum.get_instance by a stub without phy stats.

  destinations  per destination: the identity's private key (X25519 ‖ Ed25519
                seed), its hash, whether it accepts link requests;
  transport_id  the node's transport identity hash;
  cases         per case: a note, the raw request, nh_mtu (the value
                Transport.py:2138-2141 computes, or null for an interface
                without HW_MTU), how far the reference took it (`reached`:
                "transport" dropped inside Transport.inbound, "destination" by
                Destination.incoming_link_request, "validate" by
                Link.validate_request, "accepted"), the status the device stage
                is expected to give by name, and for an accepted request the
                ephemeral private key read back from the link, link_id,
                derived_key, mtu, mode, peer_pub, peer_sig_pub and the raw
                LRPROOF packet.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_link_accept.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")

P = 2 ** 255 - 19
D = (-121665 * pow(121666, P - 2, P)) % P


def not_on_curve():
    """32 bytes whose y has no x on edwards25519."""
    y = 2
    while True:
        xx = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
        if xx != 0 and pow(xx, (P - 1) // 2, P) != 1:
            return y.to_bytes(32, "little")
        y += 1


def main():
    sys.path.insert(0, REF)
    import RNS
    from RNS.Cryptography import Ed25519PrivateKey, X25519PrivateKey

    rng = np.random.Generator(np.random.PCG64(2127))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    RNS.loglevel = -1
    Transport, Link, Packet, Destination = RNS.Transport, RNS.Link, RNS.Packet, RNS.Destination

    class Owner:
        is_connected_to_shared_instance = False

    Transport.owner = Owner()
    Transport.identity = RNS.Identity()

    sent, registered, validated, received = [], [], [], []
    real = (Packet.send, Transport.register_link, Link.start_watchdog, Link.validate_request,
            Destination.incoming_link_request)

    def send(self):
        self.pack()
        sent.append(self.raw)

    def validate_request(owner, data, packet):
        validated.append(bytes(data))
        return real[3](owner, data, packet)

    def incoming_link_request(self, data, packet):
        received.append(bytes(data))
        return real[4](self, data, packet)

    Packet.send = send
    Transport.register_link = staticmethod(lambda link: registered.append(link))
    Link.start_watchdog = lambda self: None
    Link.validate_request = staticmethod(validate_request)
    Destination.incoming_link_request = incoming_link_request

    class Interface:
        """The receiving interface, as far as Transport.inbound reads it."""
        ifac_identity = None
        r_stat_rssi = r_stat_snr = r_stat_q = None

        def __init__(self, hw_mtu, autoconfigure=False, fixed=False):
            self.HW_MTU, self.AUTOCONFIGURE_MTU, self.FIXED_MTU = hw_mtu, autoconfigure, fixed

    def interface_for(nh_mtu, how):
        """An interface for which Transport.py:2138-2141 computes nh_mtu."""
        if nh_mtu is None:
            return Interface(None)
        if how == "plain":
            assert nh_mtu == RNS.Reticulum.MTU
            return Interface(1064)                      # neither autoconfigured nor fixed: Reticulum.MTU
        return Interface(nh_mtu, autoconfigure=how == "auto", fixed=how == "fixed")

    class Instance:
        """What Link.__update_phy_stats asks of the Reticulum instance of a live node."""

        @staticmethod
        def get_packet_rssi(packet_hash):
            return None

        get_packet_snr = get_packet_q = get_packet_rssi

    real_instance = RNS.Reticulum.get_instance
    RNS.Reticulum.get_instance = staticmethod(lambda: Instance)
    Transport.ready = True
    # the node is no transport node (Reticulum.__init__ reads that from its configuration)
    was_enabled = getattr(RNS.Reticulum, "_Reticulum__transport_enabled", None)
    RNS.Reticulum._Reticulum__transport_enabled = False

    def inbound(raw, interface):
        """One run of the reference's Transport.inbound over a raw packet, from an empty packet hash list."""
        Transport.packet_hashlist, Transport.packet_hashlist_prev = set(), set()
        Transport.inbound(raw, interface)

    try:
        dests = []
        for k, accepts in enumerate((True, True, False)):
            d = Destination(RNS.Identity(), Destination.IN, Destination.SINGLE, "linkaccept", "fixture%d" % k)
            d.accept_link_requests = accepts
            dests.append(d)

        out = {"reference": "RNS/Transport.py:2127-2158; RNS/Destination.py:414-435; RNS/Link.py:186-227, 336-376; "
                            "RNS/Packet.py:170-185",
               "generator": "tests/golden/gen_link_accept.py",
               "transport_id": Transport.identity.hash.hex(),
               "destinations": [{"private_key": d.identity.get_private_key().hex(), "hash": d.hash.hex(),
                                 "accepts": bool(d.accept_link_requests)} for d in dests],
               "cases": []}

        LR = Packet.LINKREQUEST
        SINGLE = Destination.SINGLE

        def keys():
            return (X25519PrivateKey.generate().public_key().public_bytes()
                    + Ed25519PrivateKey.generate().public_key().public_bytes())

        def sig(mtu, mode):
            v = (mtu & Link.MTU_BYTEMASK) + (((mode << 5) & Link.MODE_BYTEMASK) << 16)
            return v.to_bytes(3, "big")

        def request(data, dest=0, dtype=SINGLE, header2=None, hops=0, dest_hash=None):
            h = dests[dest].hash if dest_hash is None else dest_hash
            flags = (dtype << 2) | LR
            if header2 is None:
                return bytes([flags, hops]) + h + b"\x00" + data
            return bytes([flags | (Packet.HEADER_2 << 6) | (Transport.TRANSPORT << 4), hops]) + header2 + h + b"\x00" + data

        def case(note, raw, nh_mtu, expect, how="fixed", dest=0):
            packet = Packet(None, raw)
            assert packet.unpack() and packet.packet_type == LR, note
            del sent[:], registered[:], validated[:], received[:]
            inbound(raw, interface_for(nh_mtu, how))
            entry = {"note": note, "raw": raw.hex(), "nh_mtu": nh_mtu, "dest": dest, "expect": expect}
            if registered:
                link = registered[0]
                assert len(registered) == 1 and len(sent) == 1 and len(sent[0]) == 118, note
                assert link in dests[dest].links
                entry.update(reached="accepted", ephemeral=link.prv.private_bytes().hex(), link_id=link.link_id.hex(),
                             derived_key=link.derived_key.hex(), mtu=link.mtu, mode=link.mode,
                             peer_pub=link.peer_pub_bytes.hex(), peer_sig_pub=link.peer_sig_pub_bytes.hex(),
                             lrproof=sent[0].hex())
            else:
                assert not sent, note
                entry["reached"] = "validate" if validated else "destination" if received else "transport"
            want = {"ACCEPTED": "accepted", "OTHER_TRANSPORT": "transport", "NO_DESTINATION": "transport",
                    "NOT_ACCEPTING": "destination", "BAD_SIZE": "validate"}.get(expect)
            if want is not None:
                assert entry["reached"] == want, (note, entry["reached"])
            else:
                assert expect == "BAD_MODE" and entry["reached"] in ("transport", "validate"), (note, entry["reached"])
            out["cases"].append(entry)
            return entry

        ours, foreign = Transport.identity.hash, rb(16)
        # header forms, 64 and 67 bytes
        for n_sig in (0, 3):
            data = keys() + (sig(500, 1) if n_sig else b"")
            case(f"{64 + n_sig}-byte data, HEADER_1", request(data), 500, "ACCEPTED")
            case(f"{64 + n_sig}-byte data, HEADER_2 with our transport id", request(data, header2=ours, hops=3), 500,
                 "ACCEPTED")
            case(f"{64 + n_sig}-byte data, HEADER_2 with a foreign transport id", request(data, header2=foreign), 500,
                 "OTHER_TRANSPORT")
        # the MTU step
        e = case("path_mtu 400 below nh_mtu 500", request(keys() + sig(400, 1)), 500, "ACCEPTED")
        assert e["mtu"] == 400
        e = case("path_mtu equal to nh_mtu 1196", request(keys() + sig(1196, 1)), 1196, "ACCEPTED", how="auto")
        assert e["mtu"] == 1196
        e = case("path_mtu 8192 above nh_mtu 1196: clamped", request(keys() + sig(8192, 1)), 1196, "ACCEPTED")
        assert e["mtu"] == 1196
        e = case("path_mtu 8192 above an interface that is neither autoconfigured nor fixed: Reticulum.MTU",
                 request(keys() + sig(8192, 1)), 500, "ACCEPTED", how="plain")
        assert e["mtu"] == 500
        e = case("path_mtu 0x1FFFFF, nh_mtu 262144", request(keys() + sig(0x1FFFFF, 1)), 262144, "ACCEPTED")
        assert e["mtu"] == 262144
        e = case("path_mtu 1196, no HW_MTU: the signalling bytes are cut off", request(keys() + sig(1196, 1)), None,
                 "ACCEPTED")
        assert e["mtu"] == 500
        e = case("path_mtu 0: absent", request(keys() + sig(0, 1)), 1196, "ACCEPTED")
        assert e["mtu"] == 500
        e = case("path_mtu 0, no HW_MTU", request(keys() + sig(0, 1)), None, "ACCEPTED")
        assert e["mtu"] == 500
        # mode bits
        for mode in range(8):
            expect = "ACCEPTED" if mode == Link.MODE_AES256_CBC else "BAD_MODE"
            case(f"mode {mode}, path_mtu 500 at nh_mtu 500", request(keys() + sig(500, mode)), 500, expect)
            case(f"mode {mode}, path_mtu 8192 above nh_mtu 1196", request(keys() + sig(8192, mode)), 1196, expect)
            case(f"mode {mode}, path_mtu 0", request(keys() + sig(0, mode)), 1196, expect)
            e = case(f"mode {mode}, path_mtu 1196, no HW_MTU: accepted with the default mode",
                     request(keys() + sig(1196, mode)), None, "ACCEPTED")
            assert e["mode"] == Link.MODE_DEFAULT
        # data lengths
        for n in (63, 65, 66, 68):
            data = (keys() + sig(500, 1) + rb(1))[:n]
            case(f"{n}-byte data", request(data), 500, "BAD_SIZE")
            case(f"{n}-byte data, no HW_MTU", request(data), None, "BAD_SIZE")
        # destinations
        case("an unknown destination", request(keys(), dest_hash=rb(16)), 500, "NO_DESTINATION")
        for name, dtype in (("GROUP", Destination.GROUP), ("PLAIN", Destination.PLAIN), ("LINK", Destination.LINK)):
            case(f"destination type {name} in the flags", request(keys() + sig(500, 1), dtype=dtype), 500,
                 "NO_DESTINATION")
        case("a second destination with its own identity", request(keys() + sig(500, 1), dest=1), 500, "ACCEPTED",
             dest=1)
        case("accept_link_requests off", request(keys() + sig(500, 1), dest=2), 500, "NOT_ACCEPTING", dest=2)
        # keys
        k = keys()
        case("a low-order peer_pub: zero", request(bytes(32) + k[32:] + sig(500, 1)), 500, "ACCEPTED")
        case("a low-order peer_pub: one", request((1).to_bytes(32, "little") + k[32:]), 500, "ACCEPTED")
        case("a peer_pub with bit 255 set", request(k[:31] + bytes([k[31] | 0x80]) + k[32:]), 500, "ACCEPTED")
        case("a peer_sig_pub that is not a curve point", request(k[:32] + not_on_curve() + sig(500, 1)), 500,
             "ACCEPTED")
        # hops
        case("hops 0", request(keys() + sig(500, 1), hops=0), 500, "ACCEPTED")
        case("hops 127", request(keys() + sig(500, 1), hops=127), 500, "ACCEPTED")
    finally:
        (Packet.send, Transport.register_link, Link.start_watchdog, Link.validate_request,
         Destination.incoming_link_request) = real[0], staticmethod(real[1]), real[2], staticmethod(real[3]), real[4]
        RNS.Reticulum.get_instance = real_instance
        RNS.Reticulum._Reticulum__transport_enabled = was_enabled

    path = os.path.join(HERE, "link_accept_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
