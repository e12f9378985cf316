"""Generate tests/golden/link_vectors.json from the reference's own code.

Runs only where the reference is at hand ($RNS_REFERENCE).  Fixtures for the
link dispatch and the link keys (Transport.py:2161-2176, Link.py:336-361,
941-1158):

  context_decrypts  for every context byte 0..255, whether the reference's
                    Link.receive calls Link.decrypt on a DATA packet: a real
                    responder Link in state ACTIVE with a channel attached,
                    its decrypt replaced by a recorder (which returns None, so
                    nothing past the call runs);
  proof_decrypts    the same for PROOF packets (never);
  handshakes        real Link.handshake calls: private key, peer public key,
                    link_id, derived_key, for MODE_AES256_CBC and, by setting
                    `mode` on the link, MODE_AES128_CBC;
  link_ids          Link.link_id_from_lr_packet for link requests with and
                    without signalling bytes, HEADER_1 (packed by Packet.pack)
                    and HEADER_2 (the same request as a transport node
                    forwards it, Transport.py:1537-1546).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_link.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RNS_REFERENCE", "/root/reference")


def main():
    sys.path.insert(0, REF)
    import RNS
    from RNS.Cryptography import Ed25519PrivateKey, X25519PrivateKey

    rng = np.random.Generator(np.random.PCG64(2161))

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    RNS.loglevel = -1

    class Owner:
        """The destination a responder link belongs to (Link.__init__: owner.identity.sig_prv)."""
        identity = RNS.Identity()
        type = RNS.Destination.SINGLE
        hash = rb(16)

    class Channel:
        def _receive(self, plaintext):
            pass

        def _shutdown(self):
            pass

    iface = object()

    def responder(mode=RNS.Link.MODE_AES256_CBC):
        peer = X25519PrivateKey.generate().public_key().public_bytes()
        peer_sig = Ed25519PrivateKey.generate().public_key().public_bytes()
        link = RNS.Link(owner=Owner, peer_pub_bytes=peer, peer_sig_pub_bytes=peer_sig)
        link.mode = mode
        return link, peer, peer_sig

    out = {"reference": "RNS/Link.py:336-361, 941-1158; RNS/Packet.py:342-353; RNS/Transport.py:2161-2176",
           "generator": "tests/golden/gen_link.py"}

    # --- which packets Link.receive decrypts
    link, _, _ = responder()
    link.link_id = link.hash = rb(16)
    link.request_time = 0.0                  # validate_request sets it on a live node; rtt_packet reads it
    link.attached_interface = iface
    link._channel = Channel()
    calls = []

    def recorder(ciphertext):
        calls.append(bytes(ciphertext))
        return None

    link.decrypt = recorder

    def decided(packet_type, context):
        flags = (RNS.Destination.LINK << 2) | packet_type
        data = rb(64)
        packet = RNS.Packet(None, bytes([flags, 0]) + link.link_id + bytes([context]) + data)
        assert packet.unpack() and packet.context == context and packet.packet_type == packet_type
        packet.receiving_interface = iface
        packet.link = link
        link.status = RNS.Link.ACTIVE
        calls.clear()
        link.receive(packet)
        assert calls in ([], [data])
        return len(calls)

    real_prove = RNS.Packet.prove
    RNS.Packet.prove = lambda self, destination=None: None     # CHANNEL proves before it decrypts (Link.py:1144)
    try:
        out["context_decrypts"] = [decided(RNS.Packet.DATA, c) for c in range(256)]
        out["proof_decrypts"] = [decided(RNS.Packet.PROOF, c) for c in range(256)]
    finally:
        RNS.Packet.prove = real_prove
    assert sum(out["context_decrypts"]) == 12 and not any(out["proof_decrypts"])

    # --- link ids of link requests
    class Dest:
        type = RNS.Destination.SINGLE

        def __init__(self):
            self.hash = rb(16)

    def link_request(signalling, mode=RNS.Link.MODE_AES256_CBC, data=None):
        data = rb(64) if data is None else data
        if signalling:
            data += RNS.Link.signalling_bytes(int(rng.integers(500, 70000)), mode)
        packet = RNS.Packet(Dest(), data, packet_type=RNS.Packet.LINKREQUEST)
        packet.pack()
        return packet

    out["link_ids"] = []
    for signalling in (False, True, False, True):
        packet = link_request(signalling)
        raw1 = packet.raw
        # as a transport node forwards it: HEADER_2, transport id inserted (Transport.py:1537-1546)
        raw2 = bytes([raw1[0] | (RNS.Packet.HEADER_2 << 6) | (RNS.Transport.TRANSPORT << 4), 3]) + rb(16) + raw1[2:]
        for raw in (raw1, raw2):
            p = RNS.Packet(None, raw)
            assert p.unpack() and p.packet_type == RNS.Packet.LINKREQUEST
            out["link_ids"].append({"raw": raw.hex(), "header_type": p.header_type, "signalling": signalling,
                                    "link_id": RNS.Link.link_id_from_lr_packet(p).hex()})
        assert out["link_ids"][-1]["link_id"] == out["link_ids"][-2]["link_id"]

    # --- handshakes
    out["handshakes"] = []
    for mode in (RNS.Link.MODE_AES256_CBC,) * 5 + (RNS.Link.MODE_AES128_CBC,) * 3:
        link, peer, peer_sig = responder(mode)
        request = link_request(True, RNS.Link.MODE_AES256_CBC, data=peer + peer_sig)
        link.set_link_id(request)
        link.handshake()
        assert link.status == RNS.Link.HANDSHAKE and len(link.derived_key) == (64 if mode == 1 else 32)
        out["handshakes"].append({"mode": mode, "private": link.prv.private_bytes().hex(), "peer_public": peer.hex(),
                                  "link_id": link.link_id.hex(), "derived_key": link.derived_key.hex()})

    path = os.path.join(HERE, "link_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
