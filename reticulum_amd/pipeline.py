"""A Reticulum interface's packet path, device-resident end to end
("what surrounds the token on the interface path ... needed
for a true end-to-end node pipeline").

Outbound, as a node sends DATA packets through an interface with IFAC:
    Token.encrypt            Token.py:87-97 (Packet.pack -> Destination/Link.encrypt)
    Packet.pack header       Packet.py:178-228
    IFAC sign                Transport.py:1073 (with ifac_size; else the
                             caller supplies the access codes)
    IFAC mask                Transport.py:1075-1101 (transmit)
    HDLC framing             TCPInterface.py:44-53, 323 (process_outgoing)
Inbound, as the interface's read loop hands frames to Transport:
    HDLC deframing           TCPInterface.py:387-410 (read_loop)
    IFAC unmask              Transport.py:1441-1468 (inbound)
    IFAC check               Transport.py:1470-1474 (with check_ifac; else
                             `ifac` is returned for the caller's own check)
    Packet.unpack + hash     Packet.py:242-275, 342-353
    packet filter            Transport.py:1377-1427, 1525-1545 (with seen)
    announce validation      Identity.py:505-606, Transport.py:1748-1750, 1772
                             (with announces)
    proofs settled           Transport.py:2326-2363, Packet.py:434-459 (with
                             receipts, after the link dispatch)
    Token.decrypt            Token.py:100-114 (Link/Identity.decrypt)
    packets proved           Link.py:943-955, 1140-1145, 378-389 (with signers)
    link requests answered   Transport.py:2127-2158, Link.py:186-227, 336-376
                             (with accept, between the filter and the dispatch)
    packets for the node's   Transport.py:2188-2202, Identity.py:848-898, 942-953
    SINGLE destinations      (with deliver: opened and proved, after the decrypt)
    replies sent             Transport.py:1069-1104, 1199-1356, 1343-1345 (with
                             reply, or pipeline.reply on the result: the rows of
                             accept, signers and deliver gathered, signed, masked
                             and framed for the socket the read came from)

Every stage is one of reticulum_amd.device's kernels, the rearranging of
offsets and lengths between them included (frames_compact, token_spans), and
nothing is synchronised: sizes the host does not know (the number of frames
in a stream) stay on the device, and entries past them carry length 0, which
every later stage rejects like the reference does (a frame too short for its
IFAC, a packet too short for its header, a token too short for its tag).
With ``stream`` given, every launch and every temporary is on that stream
(allocated there, so the caching allocator never hands a temporary to other
work before the stream is done with it) and so are the results: the caller
makes its own stream wait on it before reading them.
"""
import contextlib

import torch

from . import device
from .token import KeySet, token_len

HEADER_1_LEN = 19           # flags, hops, destination hash (16), context: Packet.py:178-228
FRAME_OK = 0                # RT_FRAME_OK (include/rnstok.h)
# Outbound builds its packets in 128-B-aligned slots with each HEADER_1
# packet's token ciphertext (packet + 19 + 16 B of IV) starting on a line: the
# token encrypt and the IFAC mask then fetch fewer lines twice (DESIGN.md §3,
# "Rows in 128-B-aligned slots"; §4.8).
CT_PHASE = HEADER_1_LEN + 16


_ifac_public = {}          # (device index, seed bytes) -> the seed's public key on that device


def ifac_identity(ifac_key):
    """(seed, public key) of the interface identity Reticulum builds from a
    64-byte ``ifac_key`` (device uint8): Identity.from_bytes(ifac_key)
    (Reticulum.py:968-971) signs with ifac_key[32:64].  The public key is
    computed once per key and device (device.ed25519_public) and kept; looking
    it up reads the key back to the host."""
    if ifac_key.numel() != 64:
        raise ValueError("the access code is signed with a 64-byte ifac_key (Identity.from_bytes)")
    seed = ifac_key[32:64]
    tag = (ifac_key.device.index, bytes(seed.tolist()))
    pub = _ifac_public.get(tag)
    if pub is None:
        pub = torch.empty((1, 32), dtype=torch.uint8, device=ifac_key.device)
        device.ed25519_public(seed.view(1, 32), pub)
        torch.cuda.current_stream(ifac_key.device).synchronize()
        _ifac_public[tag] = pub
    return seed, pub


def outbound(ks: KeySet, pt, iv, destination_hash, context, ifac=None, ifac_key=None, flags=None, hops=None,
             stream=None, aligned=True, ifac_size=None, key_idx=None):
    """n DATA packets of one length L, one link key (or, with ``key_idx`` (n,)
    int32, packet i under key key_idx[i] of ``ks``: one call that sends on
    many links): pt (n, L) uint8, iv (n,
    16), destination_hash (n, 16), context (n,) uint8, flags/hops (n,) uint8
    (default 0: HEADER_1 DATA, hop 0), ifac (n, ifac_size) the access codes
    (the tail of the interface identity's signature of each packet, made by
    the caller; None or zero columns: an interface without IFAC, no mask),
    ifac_key (K,) uint8 (unused without IFAC).  With ``ifac`` None and
    ``ifac_size`` (1..64) given the codes are made on the device instead
    (device.ifac_sign between pack and mask, Transport.py:1073), signed with
    ifac_key[32:64] of a 64-byte ifac_key.  Returns (stream, frame_off): the HDLC
    byte stream is stream[:frame_off[n]] (int64 on the device), frame i at
    stream[frame_off[i]:frame_off[i+1]].  ``aligned`` (default) builds the
    packets in 128-B-aligned slots (token ciphertext on a line); False packs
    them end to end.  The stream is the same either way."""
    with _on(stream):      # temporaries allocated on the stream that uses them
        n, L = pt.shape
        dev = pt.device
        flags = flags if flags is not None else torch.zeros(n, dtype=torch.uint8, device=dev)
        hops = hops if hops is not None else torch.zeros(n, dtype=torch.uint8, device=dev)
        pl = HEADER_1_LEN + token_len(L)
        sign = ifac is None and bool(ifac_size)
        if sign:
            seed, pub = ifac_identity(ifac_key)
        isz = ifac_size if sign else ifac.shape[1] if ifac is not None else 0
        if aligned:
            raw = device.aligned_rows(n, pl, CT_PHASE, dev)
            stride = raw.stride(0)
            flat = raw.as_strided((n * stride,), (1,))
        else:
            stride = pl
            flat = torch.empty(n * stride, dtype=torch.uint8, device=dev)
            raw = flat.view(n, pl)
        device.encrypt_uniform(ks, pt, L, iv, raw[:, HEADER_1_LEN:], key_idx=key_idx, stream=stream)
        off = torch.arange(n, dtype=torch.int64, device=dev) * stride
        device.pack_headers(flags, hops, destination_hash, context, flat, off, stream=stream)
        if isz:
            ml = pl + isz
            masked = torch.empty(n * ml, dtype=torch.uint8, device=dev)
            m_off = torch.arange(n, dtype=torch.int64, device=dev) * ml
            p_len = torch.full((n,), pl, dtype=torch.int32, device=dev)
            if sign:
                ifac = torch.empty((n, isz), dtype=torch.uint8, device=dev)
                device.ifac_sign(seed, pub, flat, off, p_len, ifac, stream=stream)
            device.ifac_mask(flat, off, p_len, ifac, ifac_key, masked, m_off, stream=stream)
        else:
            # an interface without IFAC transmits the packet as packed
            # (Transport.py:1069-1071: the mask applies only with ifac_identity)
            ml, masked, m_off = pl, flat, off
        framed = torch.empty(n * (2 * ml + 2), dtype=torch.uint8, device=dev)
        frame_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        device.hdlc_frame(masked, m_off, torch.full((n,), ml, dtype=torch.int32, device=dev), framed, frame_off,
                          stream=stream)
    return framed, frame_off


# The sources of a read's replies, in the order the reply stage numbers them
# (device.REPLY_LRPROOF, REPLY_LINK_PROOF, REPLY_DEST_PROOF): the rows of
# ``accept``, ``signers`` and ``deliver`` with their length columns.
REPLY_SOURCES = (("lr_proofs", "lr_proof_len"), ("proofs", "proof_len"), ("dest_proofs", "dest_proof_len"))


def _check_reply_ifac(ifac_key, ifac_size):
    if not 0 <= int(ifac_size) <= 64:
        raise ValueError("ifac_size must be 0..64")
    if ifac_size and (ifac_key is None or ifac_key.numel() != 64):
        raise ValueError("the access code is signed with a 64-byte ifac_key (Identity.from_bytes)")


def reply(res, ifac_key=None, ifac_size=0, max_replies=None, seen=None, stream=None):
    """The send side of a read: what ``inbound`` left to be transmitted, as the
    framed byte stream for the socket the read came from.  ``res`` is an
    ``inbound`` result (or any dict of the same columns); of ``lr_proofs``,
    ``proofs`` and ``dest_proofs`` (each with its length column) the ones
    present are the sources, numbered in that fixed order whichever are there
    (device.REPLY_LRPROOF, REPLY_LINK_PROOF, REPLY_DEST_PROOF).  The reference
    sends each of these packets on the interface its frame came in on, in the
    order of its loop over the frames (Identity.py:942-953, Link.py:366-389,
    Transport.py:1199-1356), so the replies are ordered by frame, then by
    source.

    The rows are gathered (device.reply_gather); with ``ifac_size`` > 0 every
    reply gets its access code and is masked under the 64-byte ``ifac_key``
    (device.ifac_sign, ifac_mask; Transport.py:1069-1101), without it the
    packets go out as packed (:1104); the result is framed by
    device.hdlc_frame_counted, which takes the number of replies from the
    device.  With ``seen`` (a :class:`reticulum_amd.filter.PacketHashlist`) the
    packet hashes of the replies enter the list, as Transport.outbound does for
    what it broadcasts (Transport.py:1343-1345): an echo of the node's own
    reply is then dropped as a replay.

    Returns a dict of device tensors: ``stream`` (uint8) and ``frame_off``
    ((max_replies + 1,) int64): the bytes to send are
    stream[:frame_off[max_replies]], reply j at stream[frame_off[j]:
    frame_off[j + 1]]; ``reply_counts`` ((2,) int64: [written, found]),
    ``reply_frame`` and ``reply_len`` (int32), ``reply_source`` (uint8) and
    ``packets`` ((max_replies, 128) uint8: the raw replies).  ``max_replies``
    defaults to the number of frames, one reply per frame, which is what the
    stages of ``inbound`` can produce; replies beyond it (found > written) stay
    with the caller.  Nothing is synchronised, except that the interface
    identity's public key is computed once per ``ifac_key`` and device
    (:func:`ifac_identity`)."""
    have = [k for k, (rows, ln) in enumerate(REPLY_SOURCES) if res.get(rows) is not None and res.get(ln) is not None]
    if not have:
        raise ValueError("reply needs at least one of lr_proofs, proofs and dest_proofs with its length column "
                         "(inbound with accept, signers or deliver)")
    _check_reply_ifac(ifac_key, ifac_size)
    # the source index is the stage's, so absent stages before a present one are empty sources
    first = res[REPLY_SOURCES[have[0]][0]]
    n, dev = first.shape[0], first.device
    cap = n if max_replies is None else int(max_replies)
    if cap < 0:
        raise ValueError("max_replies must be >= 0")
    if ifac_size:
        seed, pub = ifac_identity(ifac_key)
    with _on(stream):      # temporaries allocated on the stream that uses them
        sources = []
        nothing = None
        for k in range(have[-1] + 1):
            if k in have:
                sources.append((res[REPLY_SOURCES[k][0]], res[REPLY_SOURCES[k][1]]))
            else:
                if nothing is None:
                    nothing = (torch.empty((n, 1), dtype=torch.uint8, device=dev),
                               torch.zeros(n, dtype=torch.int32, device=dev))
                sources.append(nothing)
        packets = torch.empty((cap, device.LINE), dtype=torch.uint8, device=dev)      # the allocator's blocks start on a line
        reply_len = torch.empty(cap, dtype=torch.int32, device=dev)
        reply_frame = torch.empty(cap, dtype=torch.int32, device=dev)
        reply_source = torch.empty(cap, dtype=torch.uint8, device=dev)
        reply_counts = torch.empty(2, dtype=torch.int64, device=dev)
        device.reply_gather(sources, packets, reply_len, reply_frame, reply_source, reply_counts, stream=stream)
        if seen is not None:
            device.reply_remember(seen.handle, packets, reply_len, reply_counts, stream=stream)
        flat = packets.view(-1)
        # every entry's offset lies inside its buffer, the empty ones past the
        # replies included: ifac_mask reads a length-0 entry's two header bytes
        p_off = torch.arange(cap, dtype=torch.int64, device=dev) * device.LINE
        if ifac_size:
            ml = device.LINE + ifac_size
            ifac = torch.empty((cap, ifac_size), dtype=torch.uint8, device=dev)
            device.ifac_sign(seed, pub, flat, p_off, reply_len, ifac, stream=stream)
            masked = torch.empty(max(cap * ml, 1), dtype=torch.uint8, device=dev)
            m_off = torch.arange(cap, dtype=torch.int64, device=dev) * ml
            device.ifac_mask(flat, p_off, reply_len, ifac, ifac_key, masked, m_off, stream=stream)
            m_len = reply_len + ifac_size      # past the replies: not a length, and not read as one
        else:
            # an interface without IFAC transmits the packet as packed (Transport.py:1104)
            ml, masked, m_off, m_len = device.LINE, flat, p_off, reply_len
        framed = torch.empty(max(cap * (2 * ml + 2), 1), dtype=torch.uint8, device=dev)
        frame_off = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        device.hdlc_frame_counted(masked, m_off, m_len, reply_counts, framed, frame_off, stream=stream)
    return {"stream": framed, "frame_off": frame_off, "reply_counts": reply_counts, "reply_frame": reply_frame,
            "reply_source": reply_source, "reply_len": reply_len, "packets": packets}


_reply = reply             # inbound's ``reply`` argument hides the name


def inbound(ks: KeySet, buf, ifac_key, ifac_size, max_pairs, hw_mtu=262144, stream=None, aligned=None,
            check_ifac=False, links=None, seen=None, transport_identity=None, transit=None, announces=False,
            signers=None, receipts=None, accept=None, establish=None, deliver=None,
            implicit_proof=True, destination_receipts=None, reply=None):
    """One read of an interface's byte stream ``buf`` (uint8 on the device)
    through deframing, IFAC unmask (skipped for ``ifac_size`` 0, an interface
    without access codes: then frames with the IFAC flag set are dropped, as
    Transport.py:1482-1486 does), unpack and token decrypt, for at most
    ``max_pairs`` consecutive flag pairs (a stream of n frames has 2n - 1:
    frames and the empty gaps between them).

    Returns a dict of device tensors.  Per flag pair k: ``frame_status``
    (RT_FRAME_*; -1 past the pairs found), ``frame_len`` (its unescaped
    length) and ``counts`` = [pairs, bytes
    consumed] as the read loop leaves them (TCPInterface.py:391-411).  The
    frames the read loop hands on (RT_FRAME_OK) are compacted in stream order
    into the first ``n_frames`` (a device scalar) entries of the per-frame
    arrays, whose remaining entries are empty: ``frame_pair`` (their pair
    index), ``ifac_status`` (0: unmasked; 1: dropped before the signature
    check; 2, with ``check_ifac`` only: the access code does not match),
    ``ifac`` (the access code, for the caller's signature check where
    ``check_ifac`` is off),
    ``fields`` (rt_packet_fields; ok = 0 where unpack fails), and the token's
    outcome: ``status`` (RT_* token status; TOO_SHORT where there is no
    packet) with the plaintext at ``pt[pt_off[i]: pt_off[i] + pt_len[i]]``.
    Compacting first keeps the per-packet kernels' waves full (the gaps
    between frames would otherwise be half of every wave).  With ``aligned``
    the deframer writes every frame into its own 128-B-aligned slot
    (rt_hdlc_deframe_slots: a HEADER_1 packet's token ciphertext on a line,
    128 B more buffer per pair of max_pairs), the unmasked packets stay at
    those offsets and each plaintext starts on a line too; otherwise frames
    sit at their stream offsets.  Only the offsets differ (DESIGN.md §4.8:
    −8 % for the path, mostly the unmask reading slotted frames).  The default
    (None) takes slots when their padding is at most the stream's own size
    (a Reticulum stream has about two pairs per packet; a max_pairs sized for
    a stream of nothing but flags would multiply the buffers instead).

    ``check_ifac`` (with ``ifac_size`` > 0 and a 64-byte ``ifac_key``) runs
    the reference's access-code check on the device (device.ifac_check after
    the unmask, Transport.py:1470-1474): a packet whose code is not the tail
    of the interface identity's signature of it gets ``ifac_status`` 2 and is
    dropped there, as the reference returns: unpack reports ok = 0, its token
    status is TOO_SHORT and nothing of it is decrypted.

    ``links`` (a :class:`reticulum_amd.link.LinkTable`) dispatches every packet
    to its link between unpack and decrypt (device.link_spans in place of
    token_spans; Transport.py:2161-2176, Link.py:941-1148): a packet is
    decrypted only when it is a LINK DATA packet whose destination hash is in
    the table and whose context Link.receive decrypts, and then under key
    ``key_idx`` = the table's value of ``ks``; every other packet has status
    TOO_SHORT.  The result gains ``route`` (uint8, device.ROUTE_*), ``link``
    (the table's value or -1) and ``key_idx`` (int32).  The caller filters by
    ``link`` for what stays with it: the initiator-only and responder-only
    contexts, whether a channel exists, and the attached interface.

    ``seen`` (a :class:`reticulum_amd.filter.PacketHashlist`) runs
    Transport.packet_filter and the remember step of Transport.inbound between
    unpack and the spans (device.packet_filter; Transport.py:1377-1427,
    1525-1545), with or without ``links``, over the frames in stream order: a
    packet for another transport node than ``transport_identity`` (required
    with ``seen``: the node's 16-byte transport id, uint8 on the device), a
    PLAIN or GROUP packet from further than one hop and a packet whose hash the
    list holds are dropped as every other dropped packet is (ok = 0 in
    ``fields``, an empty span, status TOO_SHORT), and a packet that passes is
    remembered unless it is a link request proof or its destination hash is in
    ``transit`` (a LinkTable standing for Transport.link_table, the links this
    node carries for others).  A packet the access-code check dropped never
    reaches the list.  The result gains ``filter_status`` (int32 per frame,
    device.FILTER_*).  Calling ``seen.cull()`` is the caller's part, as the
    reference's job loop does it.  Out of scope: the hop decrement for
    local-client and shared-instance interfaces (Transport.py:1520-1523), and
    a node connected to a shared instance, for which the reference's filter
    always passes and remembers nothing: such a node passes ``seen=None``.

    ``announces`` validates every announce of the read where it lies in its
    packet (device.announce_validate, after unpack and after the packet filter
    when ``seen`` is given; Identity.validate_announce, Identity.py:505-606).
    The result gains ``announce_status`` (int32 per frame, device.ANNOUNCE_*)
    and ``announce_identity`` (uint8, max_pairs x 16: the announced identity's
    hash where the signature was checked, zeros elsewhere).
    validate_announce(only_validate_signature=True) (Transport.py:1748-1750) is
    true for ANNOUNCE_VALID and ANNOUNCE_BAD_DESTINATION, the full check
    (:1772) for ANNOUNCE_VALID; an announce that an earlier stage dropped (a
    forged access code with ``check_ifac``, a replay with ``seen``) has ok = 0
    and reads ANNOUNCE_NOT_ANNOUNCE like every frame that is no announce.
    Spans, link dispatch and decrypt are untouched.  Blackholed identities, the
    known-destination key check, Identity.remember, ratchets and ingress
    limiting stay with the caller, keyed by ``announce_identity``.

    ``signers`` (a :class:`reticulum_amd.proof.LinkSigners`, row l for the link
    whose table value is l) and ``receipts`` (a
    :class:`reticulum_amd.proof.ReceiptTable`), with ``links``, handle the
    packet proofs of the read: ``signers`` alone proves, ``receipts`` beside it
    (the proofs are verified under the signers' ``peer_publics``; a node that
    proves nothing gives its links flags 0) also settles.  With ``receipts`` the
    proofs that arrive are settled after the link dispatch
    (device.proof_settle; Transport.py:2326-2363, Packet.py:434-459): the
    result gains ``proof_status`` (int32 per frame, device.PROOF_*) and
    ``receipt`` (int32: the delivered receipt's id, which has left the table,
    or -1).  With ``signers`` the packets a link proves are proved after the
    decrypt (device.link_prove; Link.py:943-955, 1140-1145, 378-389): the
    result gains ``proofs`` (uint8, max_pairs x 128: the 115-byte LINK PROOF
    packet where ``proof_len`` is 115) and ``proof_len`` (int32 per frame, 115
    or 0).  A packet an earlier stage dropped is neither proved nor settled.
    The proof rows are raw packets: ``reply`` sends them.  The caller's part
    are links that prove by callback (PROVE_APP: flags 0, the caller signs
    the ``packet_hash`` column of ``fields`` with device.ed25519_sign).

    ``accept`` answers the link requests of the read that are addressed to the
    node's own destinations (device.link_accept, after unpack and the packet
    filter and before the link dispatch; Transport.py:2127-2158,
    Destination.py:414-435, Link.py:186-227, 336-376).  It is a dict, or an
    object with these attributes: ``destinations`` (a
    :class:`reticulum_amd.link.LinkDestinations`), ``slots`` ((m,) int32, the
    caller's free slots), ``ephemeral_privates`` ((m, 32) uint8, fresh
    randomness, row r for the r-th valid request of the read) and ``nh_mtu``
    (the interface's next-hop MTU, Transport.py:2138-2141; None for an
    interface without HW_MTU; default 500).  It needs ``links``,
    ``transport_identity`` and a ``ks`` of 64-byte keys.  An accepted request
    enters ``links``, record slot of ``ks`` and, with ``signers``, the slot's
    rows before the dispatch runs, so a packet on the new link that follows
    its request in the same read is decrypted under the new key (and proved,
    for a PROVE_ALL destination) as the reference's loop over the frames would.
    One difference: a link packet that precedes its request in the same read
    is dispatched too, where the reference finds no link yet.  A request an
    earlier stage dropped (a forged access code, a replay) has ok = 0 and reads
    LINKREQ_NOT_REQUEST.  The result gains ``linkreq_status`` (int32 per
    frame, device.LINKREQ_*), ``accepted_link`` (int32: the slot or -1),
    ``link_id`` (uint8, max_pairs x 16) and ``link_mtu`` (int32) for every valid
    request, ``lr_proofs`` (uint8, max_pairs x 128: the 118-byte LRPROOF packet
    where ``lr_proof_len`` is 118) and ``lr_proof_len`` (``reply`` sends the rows).  The links' host state (watchdog, timeouts, callbacks, the LRRTT that
    activates the link) stay with the caller, keyed by the slot.  Out of scope:
    the initiator side, requests in transit for other nodes, PROVE_APP and the
    per-interface ingress limits.

    ``establish`` (a :class:`reticulum_amd.link.PendingLinks`) validates the
    link request proofs of the read that answer the node's own link requests
    (device.link_establish, beside ``accept`` between the packet filter and the
    link dispatch; Transport.py:2270-2318, Link.py:391-451).  It needs
    ``links`` and a ``ks`` of 64-byte keys.  A link that comes up enters
    ``links``, record slot of ``ks`` and, with ``signers``, the slot's rows
    before the dispatch runs, so a packet on the new link that follows its
    proof in the same read is decrypted (and proved, where the row's flags say
    so); one that precedes the proof is dispatched too, the difference
    ``accept`` has.  With ``seen`` the hashes of the proofs that reached
    Link.validate_proof enter the list, which the filter left to this stage.
    The result gains ``lrproof_status`` (int32 per frame, device.LRPROOF_*),
    ``established_link`` (int32: the slot or -1) and ``link_mtu`` (int32; shared
    with ``accept``: a frame is a request or a proof).  Sending the LRRTT
    (link.pack_rtt), timeouts and callbacks stay with the caller, who reads
    ``establish.state()`` / ``hops()``.  Out of scope: proofs in transit for
    other nodes.

    ``deliver`` (a :class:`reticulum_amd.destination.SingleDestinations`) opens
    and proves the DATA packets of the read that are addressed to the node's
    own SINGLE destinations (device.destination_deliver, after the decrypt and
    the link proofs; Transport.py:2188-2202, Identity.py:848-898, 942-953).  It
    needs ``links`` (which may be an empty table: without one every packet is
    decrypted under key 0) and ``max_pairs`` <= ``deliver.max_frames``.  It
    touches only frames the link dispatch leaves at route 0: a frame an
    earlier stage dropped (a forged access code, a replay) has ok = 0 and reads
    DELIVER_NOT_DATA, and the link frames' ``status``, ``pt_len``, ``route``,
    ``key_idx`` and proofs are what they are without ``deliver``.  The result
    gains ``deliver_status`` (int32 per frame, device.DELIVER_*),
    ``destination`` (int32: the row or -1), ``ratchet`` (int32: the rank of the
    ratchet that opened the frame, -1 for the identity's key or for nothing;
    the caller derives latest_ratchet_id from it), ``dest_proofs`` (uint8,
    max_pairs x 128: the PROOF packet, 83 bytes with ``implicit_proof`` and 115
    without) and ``dest_proof_len``; ``pt_off``, ``pt_len`` and ``status``
    become valid for the DELIVERED and NOT_OPENED frames.  GROUP and PLAIN
    destinations, the PROVE_APP callback (its frames are delivered, not
    proved), the ratchet reload-and-retry, ratchet rotation, DEFERRED frames
    and the receive callbacks stay with the caller; ``reply`` sends the proof
    rows.

    ``destination_receipts`` (a
    :class:`reticulum_amd.proof.DestinationReceipts`) settles the proofs of the
    read for packets this node sent to SINGLE destinations, explicit and
    implicit (device.destination_proof_settle, after the packet filter and
    after the link proofs' settling where that runs; Transport.py:2326-2363,
    Packet.py:480-524).  It needs neither ``links`` nor ``signers``: with
    ``links`` a proof of destination type LINK whose link is in the table
    (with ``signers``: whose ``link`` is below ``signers.n_links``) is left to
    ``receipts``, without it no link is active.  The result gains
    ``dproof_status`` (int32 per frame, device.DPROOF_*) and ``dproof_receipt``
    (int32: the delivered receipt's id, which has left the table, or -1).  The
    reverse-table transport of proofs, timeouts, culling, delivery callbacks
    and DPROOF_DEFERRED frames stay with the caller.

    ``reply`` (True, or a dict with ``max_replies``) sends what the read
    produced: at the end of the read the rows of ``accept``, ``signers`` and
    ``deliver`` (at least one of them is needed) go through :func:`reply` with
    the read's own ``ifac_key``, ``ifac_size`` and ``seen``, and the result
    gains ``reply``, that function's dict: ``reply["stream"][:reply["frame_off"]
    [-1]]`` is what goes back on the socket.  Without the argument the read
    makes exactly the calls it makes without it."""
    if reply is not None and reply is not False:
        if reply is not True and not isinstance(reply, dict):
            raise ValueError("reply is True or a dict with max_replies")
        if signers is None and accept is None and deliver is None:
            raise ValueError("reply needs at least one of signers, accept and deliver: the stages that write replies")
        reply_args = {} if reply is True else dict(reply)
        if set(reply_args) - {"max_replies"}:
            raise ValueError("reply takes max_replies only")
        _check_reply_ifac(ifac_key, ifac_size)
    else:
        reply_args = None
    if deliver is not None and (links is None or max_pairs > deliver.max_frames):
        raise ValueError("deliver needs links (an empty table will do) and max_pairs <= deliver.max_frames")
    if establish is not None and (links is None or ks.key_len != 64):
        raise ValueError("establish needs links and a key set of 64-byte keys")
    if accept is not None:
        get = accept.get if isinstance(accept, dict) else lambda k, d=None: getattr(accept, k, d)
        if links is None or transport_identity is None or ks.key_len != 64:
            raise ValueError("accept needs links, transport_identity and a key set of 64-byte keys")
        acc = (get("destinations"), get("slots"), get("ephemeral_privates"), get("nh_mtu", 500))
        if acc[0] is None or acc[1] is None or acc[2] is None:
            raise ValueError("accept bundles destinations, slots, ephemeral_privates and nh_mtu")
    if seen is not None and transport_identity is None:
        raise ValueError("seen needs transport_identity, the node's 16-byte transport id")
    if (signers is not None or receipts is not None) and links is None:
        raise ValueError("signers and receipts need links, the table that finds each packet's link")
    if receipts is not None and signers is None:
        raise ValueError("receipts needs signers: a proof is verified under its link's peer_publics row")
    if aligned is None:
        aligned = device.LINE * (max_pairs + 1) <= buf.numel()
    if check_ifac and ifac_size:
        seed, pub = ifac_identity(ifac_key)
    with _on(stream):      # temporaries allocated on the stream that uses them
        dev = buf.device
        # (at least one byte: an empty read still gives every later stage a
        # buffer to point at; no frame ever reaches into it)
        nout = device.deframe_slots_bytes(buf.numel(), max_pairs) if aligned else buf.numel()
        out = torch.empty(max(nout, 1), dtype=torch.uint8, device=dev)
        d_off = torch.empty(max_pairs, dtype=torch.int64, device=dev)
        d_len = torch.empty(max_pairs, dtype=torch.int32, device=dev)
        d_st = torch.full((max_pairs,), -1, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        device.hdlc_deframe(buf, out, d_off, d_len, d_st, counts, hw_mtu=hw_mtu, ifac_size=ifac_size, stream=stream,
                            line_phase=CT_PHASE if aligned else None)
        # the frames handed on, to the front in stream order; empty entries past them
        f_off = torch.empty(max_pairs, dtype=torch.int64, device=dev)
        f_len = torch.empty(max_pairs, dtype=torch.int32, device=dev)
        frame_pair = torch.empty(max_pairs, dtype=torch.int64, device=dev)
        n_frames = torch.empty((), dtype=torch.int64, device=dev)
        device.frames_compact(d_off, d_len, d_st, counts, f_off, f_len, frame_pair, n_frames, stream=stream)
        ifac = torch.empty((max_pairs, ifac_size), dtype=torch.uint8, device=dev)
        # with slots every frame (and the unmasked packet written at its
        # offset) has its token ciphertext on a line, and each plaintext,
        # written 16 B into its token's span, starts on one too
        pt_shift = 16 if aligned else 0
        if ifac_size:
            ifac_status = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            p_len = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            un = torch.empty_like(out)
            device.ifac_unmask(out, f_off, f_len, ifac_key, ifac, un, f_off, ifac_status, out_len=p_len,
                               stream=stream)
            if check_ifac:
                device.ifac_check(seed, pub, un, f_off, p_len, ifac, ifac_status, stream=stream)
        else:
            # no IFAC on the interface: a packet with the IFAC flag set is
            # dropped, the others go to unpack as they are
            # (Transport.py:1482-1486); the empty entries past the frames
            # (f_len 0) stay dropped
            un = out
            # flag byte of each frame; entries past the frames (f_len 0, f_off
            # unspecified) are never read out of range and never count as flagged
            first = out[f_off.clamp(0, out.numel() - 1)]
            flagged = ((first & 0x80) != 0) & (f_len > 0)
            drop = flagged | (f_len <= 2)
            ifac_status = drop.to(torch.int32)
            p_len = torch.where(drop, torch.zeros_like(f_len), f_len)
        fields = torch.empty((max_pairs, 96), dtype=torch.uint8, device=dev)
        device.packet_unpack(un, f_off, p_len, fields, stream=stream)
        if seen is not None:
            filter_status = seen.filter(fields, transport_identity, transit=transit, stream=stream)
        if announces:
            announce_status = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            announce_identity = torch.empty((max_pairs, 16), dtype=torch.uint8, device=dev)
            device.announce_validate(un, f_off, fields, announce_status, announce_identity, stream=stream)
        if accept is not None:
            linkreq_status = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            accepted_link = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            link_id = torch.empty((max_pairs, 16), dtype=torch.uint8, device=dev)
            link_mtu = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            lr_proofs = torch.empty((max_pairs, device.LINE), dtype=torch.uint8, device=dev)
            lr_proof_len = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            device.link_accept(ks, links, acc[0], transport_identity, un, f_off, fields, acc[1], acc[2],
                               linkreq_status, accepted_link, link_id, link_mtu, lr_proofs, lr_proof_len,
                               nh_mtu=acc[3], signers=signers, stream=stream)
        if establish is not None:
            lrproof_status = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            established_link = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            proof_mtu = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            device.link_establish(ks, links, establish, un, f_off, fields, lrproof_status, established_link, proof_mtu,
                                  signers=signers, seen=seen, stream=stream)
            # a frame is a request or a proof: one column for both stages
            link_mtu = torch.maximum(link_mtu, proof_mtu) if accept is not None else proof_mtu
        tok_off = torch.empty(max_pairs, dtype=torch.int64, device=dev)
        tok_len = torch.empty(max_pairs, dtype=torch.int32, device=dev)
        key_idx = None
        if links is not None:
            key_idx = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            link = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            route = torch.empty(max_pairs, dtype=torch.uint8, device=dev)
            device.link_spans(links.handle, fields, f_off, ks.n_keys, tok_off, tok_len, key_idx, link, route,
                              stream=stream)
            if receipts is not None:
                proof_status = torch.empty(max_pairs, dtype=torch.int32, device=dev)
                receipt = torch.empty(max_pairs, dtype=torch.int32, device=dev)
                device.proof_settle(un, f_off, fields, link, signers, receipts, proof_status, receipt, stream=stream)
        else:
            device.token_spans(fields, f_off, tok_off, tok_len, stream=stream)
        if destination_receipts is not None:
            dproof_status = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            dproof_receipt = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            active = (signers.n_links if signers is not None else 0x7FFFFFFF) if links is not None else 0
            device.destination_proof_settle(un, f_off, fields, destination_receipts, dproof_status, dproof_receipt,
                                            link=link if links is not None else None, n_links=active, stream=stream)
        pt = torch.empty_like(un)
        pt_len = torch.empty(max_pairs, dtype=torch.int32, device=dev)
        status = torch.empty(max_pairs, dtype=torch.int32, device=dev)
        # each plaintext (at most its token's length - 48 bytes) is written inside its own token's span
        pt_off = tok_off + pt_shift if pt_shift else tok_off
        device.decrypt(ks, un, tok_off, tok_len, pt, pt_off, pt_len, status, key_idx=key_idx, stream=stream)
        if signers is not None:
            proofs = torch.empty((max_pairs, device.LINE), dtype=torch.uint8, device=dev)
            proof_len = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            device.link_prove(fields, route, link, status, signers, proofs, proof_len, stream=stream)
        if deliver is not None:
            deliver_status = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            destination = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            ratchet = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            dest_proofs = torch.empty((max_pairs, device.LINE), dtype=torch.uint8, device=dev)
            dest_proof_len = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            if not pt_shift:
                pt_off = pt_off.clone()        # tok_off itself stays the spans'
            device.destination_deliver(deliver, un, f_off, fields, pt, pt_off, pt_len, status, deliver_status,
                                       destination, ratchet, dest_proofs, dest_proof_len,
                                       implicit_proof=implicit_proof, pt_shift=pt_shift, stream=stream)
    res = {"pt": pt, "pt_off": pt_off, "pt_len": pt_len, "status": status, "ifac": ifac,
           "ifac_status": ifac_status, "fields": fields, "frame_pair": frame_pair, "n_frames": n_frames,
           "frame_status": d_st, "frame_len": d_len, "counts": counts}
    if links is not None:
        res.update(route=route, link=link, key_idx=key_idx)
    if seen is not None:
        res["filter_status"] = filter_status
    if announces:
        res.update(announce_status=announce_status, announce_identity=announce_identity)
    if signers is not None:
        res.update(proofs=proofs, proof_len=proof_len)
    if receipts is not None:
        res.update(proof_status=proof_status, receipt=receipt)
    if destination_receipts is not None:
        res.update(dproof_status=dproof_status, dproof_receipt=dproof_receipt)
    if accept is not None:
        res.update(linkreq_status=linkreq_status, accepted_link=accepted_link, link_id=link_id, link_mtu=link_mtu,
                   lr_proofs=lr_proofs, lr_proof_len=lr_proof_len)
    if establish is not None:
        res.update(lrproof_status=lrproof_status, established_link=established_link, link_mtu=link_mtu)
    if deliver is not None:
        res.update(deliver_status=deliver_status, destination=destination, ratchet=ratchet, dest_proofs=dest_proofs,
                   dest_proof_len=dest_proof_len)
    if reply_args is not None:
        res["reply"] = _reply(res, ifac_key=ifac_key, ifac_size=ifac_size, seen=seen, stream=stream, **reply_args)
    return res


def _on(stream):
    """torch plumbing on the pipeline's stream (the device calls take it explicitly)."""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
