"""A plain model of the send side of a read (reticulum_amd.pipeline.reply):
which rows of the stages' sparse outputs are replies and in which order
(rt_reply_gather), and the byte stream they make (Transport.transmit's sign +
mask, Transport.py:1069-1104, then TCPInterface's framing, :323)."""
import hashlib

import ed25519_ref as ed
from oracle import wire as ow

ROW = 128
NONE_LEN, NONE_FRAME, NONE_SOURCE = 0, -1, 0xFF      # the entries past the replies


def taken(length, width=ROW):
    """The length rule: 1 .. min(128, the source's row width), else nothing."""
    return 1 <= length <= min(ROW, width)


def gather_model(sources, cap=None):
    """``sources``: a list of (rows, lens) with rows[k] the bytes source s holds
    for frame k (at least lens[k] of them where the length is taken; its row
    width is len(rows[k])) and lens[k] an int.  Returns (replies, found):
    replies is the list of (frame, source, bytes) in frame-major, source-minor
    order cut to ``cap``; found counts them all."""
    n = len(sources[0][1])
    out = []
    for k in range(n):
        for s, (rows, lens) in enumerate(sources):
            if taken(int(lens[k]), len(rows[k])):
                out.append((k, s, bytes(rows[k][:int(lens[k])])))
    found = len(out)
    return (out if cap is None else out[:cap]), found


def transmit_model(raw, ifac_key=None, ifac_size=0):
    """Transport.transmit up to process_outgoing for one packet: with IFAC the
    access code is the tail of the interface identity's signature
    (Identity.from_bytes(ifac_key) signs with ifac_key[32:64]) and the packet
    is masked; without, the packet goes out as packed."""
    if not ifac_size:
        return bytes(raw)
    sig = ed.sign(bytes(ifac_key[32:64]), bytes(raw))
    return ow.ifac_mask(bytes(raw), sig[-ifac_size:], bytes(ifac_key))


def reply_stream_model(replies, ifac_key=None, ifac_size=0):
    """The frames of ``replies`` (gather_model's list), one bytes object per
    reply; the stream is their concatenation."""
    return [ow.hdlc_frame(transmit_model(raw, ifac_key, ifac_size)) for _, _, raw in replies]


def packet_hash(raw):
    """Packet.get_hash (Packet.py:342-353)."""
    raw = bytes(raw)
    part = bytes([raw[0] & 0x0F]) + (raw[18:] if (raw[0] >> 6) & 1 else raw[2:])
    return hashlib.sha256(part).digest()
