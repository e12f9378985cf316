"""One mixed read of real size, and the model of all of pipeline.inbound over it — TEST ONLY.

``compose`` is the host model of one ``pipeline.inbound`` call with every stage
on: the stage models of the helpers beside this file, called in the order the
pipeline runs its stages, each over the whole read before the next (which is
how the device runs them).  Nothing of a device result enters it: the rows the
stages hand on are modelled too, so the reply stream is rh.gather_model over
modelled rows.

``build`` makes the read: N frames of every kind the stages know, placed by a
fixed rule so that the reply-producing kinds sit on the wave and workgroup edges
of the 256-thread stages (and, for N = 1025, of the 1024-frame blocks of the
scans), with whole waves of noise and of one kind, the meetings of equal hashes,
link ids and receipts across workgroups, and the capacity limits.

Same-read ordering.  The device runs a stage over all frames before the next
stage; the reference runs all stages per frame.  The one documented difference
that this world holds, once per layout, is pipeline.inbound's docstring on
``accept`` ("One difference: a link packet that precedes its request in the
same read is dispatched too, where the reference finds no link yet"): frame
EARLY_DATA.  Everything else in the world is ordered so that both agree.
"""
import copy

import numpy as np

import announce_helpers as aa
import destination_deliver_helpers as dd
import destination_proof_helpers as dp
import ed25519_ref as ed
import filter_helpers as fh
import ifac_helpers as ih
import link_accept_helpers as la
import link_helpers as lh
import link_proof_helpers as lp
import proof_helpers as ph
import reply_helpers as rh
from oracle import ctoken
from oracle import wire as ow

SEED = 577
ISZ = 16
N = 577                      # 2 x 256 + 64 + 1: two workgroups, a wave and a lone lane of every 256-thread stage
N_SCAN = 1025                # SCAN_BLOCK / RG_BLOCK (wire_device.h, reply_host.h) is 1024 frames: one block and a lone frame
N_KEYS = 256                 # key records = signer rows
PRE_LINKS = 4                # links 0, 1 prove all, 2, 3 prove nothing
PENDING_SLOT = 6
FIRST_SLOT = 8               # the accept stage's free slots: FIRST_SLOT ..
POOL = 96                    # link receipts outstanding
DEST_POOL = 32               # keyed destination receipts outstanding: what one stray proof costs the model to scan
MAX_RECEIPTS = 128
MAX_HASHES = 8192
TOO_SHORT = 1
FRAME_OK, FRAME_BAD_LEN, FRAME_EMPTY = 0, 1, 2
HW_MTU = 262144
BASE = dd.BASE

(LINK_PROVED, SINGLE_PROVED, REQUEST, LINK_PLAIN, RECEIPT_PROOF, SINGLE_PLAIN, DEST_PROOF, ANNOUNCE, OTHER_TRANSPORT,
 BAD_CODE, NOISE, LRPROOF, MEETING) = range(13)
CYCLE = (LINK_PROVED, SINGLE_PROVED, REQUEST, LINK_PLAIN, RECEIPT_PROOF, SINGLE_PLAIN, DEST_PROOF, ANNOUNCE,
         OTHER_TRANSPORT, BAD_CODE, NOISE)
REPLY_KINDS = (LINK_PROVED, REQUEST, SINGLE_PROVED)
EDGES = (0, 63, 64, 255, 256, 511, 512, 575, 576, 1023, 1024)
NOISE_WAVE, REPLY_WAVE = range(128, 192), range(320, 384)
# the meetings: the first of each pair in workgroup 0, the second in workgroup 1
EARLY_DATA, DATA_A, SINGLE_A, REQUEST_A, PROOF_A, LATE_DATA = 19, 20, 21, 22, 23, 24
DATA_B, SINGLE_B, REQUEST_B, PROOF_B = 300, 301, 302, 303
LAYOUTS = 4                  # 0..2: reply kind L on every edge; 3: the LRPROOF alone at the last frame, and the caps
CAPS = dict(retry_trials=8, scan_trials=DEST_POOL, max_replies=100)


def _rng(*key):
    return np.random.Generator(np.random.PCG64([SEED, *key]))


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


class Node:
    """The host state of one node: what pipeline.inbound is given, as the
    stage models keep it.  A stage whose attribute is None is off."""

    def __init__(self, ifac_key, tid, keys, table):
        self.ifac_key, self.tid, self.keys, self.table = ifac_key, tid, list(keys), dict(table)
        self.signers = None          # ph.Signers with one seed per link
        self.accept = None           # dict: dests ([la.Dest]), slots, ephemerals, nh_mtu
        self.pending = None          # dict link id -> lp.Pending
        self.deliver = None          # dict: dests ([dd.Dest]), retry_trials, implicit
        self.receipts = None         # ph.Receipts
        self.dest_receipts = None    # dp.Receipts
        self.max_receipts = MAX_RECEIPTS     # of both receipt tables
        self.scan_trials = 4 * MAX_RECEIPTS
        self.seen = None             # fh.ListModel
        self.announces = False

    def only(self, *stages):
        """A copy with the stages not named switched off (links always stay)."""
        c = copy.deepcopy(self)
        for s in ("signers", "accept", "pending", "deliver", "receipts", "dest_receipts", "seen"):
            if s not in stages:
                setattr(c, s, None)
        c.announces = "announces" in stages
        return c


# ---------------------------------------------------------------- the model

def deframe_pairs(wire, hw_mtu=HW_MTU, ifac_size=0):
    """The read loop over ``wire`` pair by pair (TCPInterface.py:387-410):
    [(status, length, frame or None)] and the bytes consumed."""
    flag = bytes([ow.FLAG])
    pairs, start = [], wire.find(flag)
    if start < 0:
        return pairs, 0
    while True:
        end = wire.find(flag, start + 1)
        if end < 0:
            return pairs, start
        frame = ow.hdlc_unescape(wire[start + 1:end])
        if not frame:
            pairs.append((FRAME_EMPTY, 0, None))
        elif ow.check_frame_len(len(frame), hw_mtu, ifac_size):
            pairs.append((FRAME_OK, len(frame), frame))
        else:
            pairs.append((FRAME_BAD_LEN, len(frame), None))
        start = end


def compose(node, wire, ifac_size, max_pairs, check_ifac=True, reply=True, max_replies=None):
    """pipeline.inbound(ks, wire, ifac_key, ifac_size, max_pairs, ...) over the
    state ``node`` (left as it is: the state after the read is out["node"]).
    Every per-frame column has max_pairs entries, as the device's have: the
    entries past the frames are frames nothing was handed on for."""
    nd = copy.deepcopy(node)
    out = {"node": nd}
    pairs, consumed = deframe_pairs(wire, HW_MTU, ifac_size)
    assert len(pairs) <= max_pairs
    out["frame_status"] = [p[0] for p in pairs] + [-1] * (max_pairs - len(pairs))
    out["frame_len"] = [p[1] for p in pairs]
    out["counts"] = [len(pairs), consumed]
    out["frame_pair"] = [k for k, p in enumerate(pairs) if p[0] == FRAME_OK]
    frames = [p[2] for p in pairs if p[0] == FRAME_OK]
    n = out["n_frames"] = len(frames)
    m = max_pairs
    # ---- access codes (Transport.py:1441-1486)
    ifac_status, ifac, raws = [1] * m, [None] * m, [None] * m
    for i, fr in enumerate(frames):
        if ifac_size:
            r = ow.ifac_unmask(fr, ifac_size, nd.ifac_key)
            if r is None:
                continue
            ifac[i], raw = r
            if check_ifac and ih.code(nd.ifac_key, raw, ifac_size) != ifac[i]:
                ifac_status[i] = 2
                continue
        else:
            if len(fr) <= 2 or fr[0] & 0x80:
                continue
            raw = fr
        ifac_status[i], raws[i] = 0, raw
    out.update(ifac_status=ifac_status, ifac=ifac)
    # ---- unpack; from here on f[i] is None for a frame some stage dropped
    f = [ow.unpack(r) if r is not None else None for r in raws]
    # ---- the packet filter (Transport.py:1377-1427, 1525-1545)
    if nd.seen is not None:
        fstat = []
        for i in range(m):
            if f[i] is None:
                fstat.append(fh.NO_PACKET)
                continue
            p = fh.packet(f[i]["packet_hash"], f[i]["packet_type"], f[i]["destination_type"], f[i]["context"],
                          f[i]["hops"], f[i]["header_type"], f[i]["transport_id"] or b"", f[i]["destination_hash"])
            st, _ = nd.seen.packet(p)
            fstat.append(st)
            if st != fh.PASS:
                f[i] = None
        out["filter_status"] = fstat
    out["ok"] = [int(x is not None) for x in f]
    out["unpacked"] = f                     # Packet.unpack's fields of the frames handed on to the stages
    live = [raws[i] if f[i] is not None else b"" for i in range(m)]
    n_keys = len(nd.keys)
    n_links = nd.signers.n_links if nd.signers is not None else None
    # ---- announces
    if nd.announces:
        ann = [aa.announce_status_ref(live[i]) if f[i] is not None else (aa.NOT_ANNOUNCE, aa.ZERO) for i in range(m)]
        out["announce_status"], out["announce_identity"] = [a[0] for a in ann], [a[1] for a in ann]
    # ---- link requests
    mtu = [0] * m
    if nd.accept is not None:
        a = nd.accept
        recs = la.accept(live, a["dests"], nd.tid, a["nh_mtu"], a["slots"], a["ephemerals"], nd.table, n_keys, n_links)
        for r in recs:
            if r["status"] == la.ACCEPTED:
                s = r["slot"]
                nd.keys[s] = r["derived_key"]
                if nd.signers is not None:
                    nd.signers.peer_publics[s], nd.signers.flags[s] = r["peer_sig_pub"], r["dest"].flags & 3
                    nd.signers.seeds[s] = r["dest"].seed
        out["linkreq_status"] = [r["status"] for r in recs]
        out["accepted_link"] = [r["slot"] for r in recs]
        out["link_id"] = [r["link_id"] or bytes(16) for r in recs]
        out["lr_proofs"] = [r["lrproof"] for r in recs]
        mtu = [r["mtu"] or 0 for r in recs]
    # ---- link request proofs
    if nd.pending is not None:
        by_slot = {p.slot: p for p in nd.pending.values()}
        res = lp.run(live, nd.pending, nd.table, n_keys, n_links)
        for i, (st, slot, pm, remembered) in enumerate(res):
            if st == lp.ACTIVATED:
                p = by_slot[slot]
                nd.keys[slot] = p.derived_key
                if nd.signers is not None:
                    nd.signers.peer_publics[slot], nd.signers.flags[slot] = p.dest_public, p.flags & 3
                    nd.signers.seeds[slot] = p.sig_seed
            if remembered and nd.seen is not None:
                nd.seen.add([lp.packet_hash(live[i])])
            mtu[i] = max(mtu[i], pm)
        out["lrproof_status"] = [r[0] for r in res]
        out["established_link"] = [r[1] for r in res]
    if nd.accept is not None or nd.pending is not None:
        out["link_mtu"] = mtu
    # ---- link dispatch
    route, link, key_idx, dec = [], [], [], []
    for x in f:
        r, l, d = (lh.NOT_LINK, -1, False) if x is None else lh.route(
            True, x["destination_type"], x["packet_type"], x["context"], nd.table.get(x["destination_hash"]), n_keys)
        route.append(r), link.append(l), key_idx.append(l if d else 0), dec.append(d)
    out.update(route=route, link=link, key_idx=key_idx)
    # ---- the proofs that arrive
    if nd.receipts is not None:
        s = ph.settle(f, link, nd.signers, nd.receipts)
        out["proof_status"], out["receipt"] = [x[0] for x in s], [x[1] for x in s]
    if nd.dest_receipts is not None:
        s = dp.settle(f, nd.dest_receipts, nd.scan_trials, links=link,
                      n_links=n_links if n_links is not None else 0x7FFFFFFF)
        out["dproof_status"], out["dproof_receipt"] = [x[0] for x in s], [x[1] for x in s]
    # ---- token decrypt
    status, pt = [TOO_SHORT] * m, [b""] * m
    for i in range(m):
        if dec[i]:
            st, p = ctoken.decrypt(nd.keys[key_idx[i]], f[i]["data"])
            status[i], pt[i] = st, p if st == 0 else b""
    # ---- link proofs
    if nd.signers is not None:
        out["proofs"] = [ph.prove(f[i], route[i], link[i], status[i], nd.signers) for i in range(m)]
    # ---- delivery
    if nd.deliver is not None:
        d = nd.deliver
        recs = dd.deliver(live, d["dests"], d["retry_trials"], d["implicit"])
        for i, r in enumerate(recs):
            if r["status"] in (dd.DELIVERED, dd.NOT_OPENED):
                status[i], pt[i] = r["token_status"], r["plaintext"] or b""
        out["deliver_status"] = [r["status"] for r in recs]
        out["destination"] = [r["dest"] for r in recs]
        out["ratchet"] = [r["ratchet"] for r in recs]
        out["dest_proofs"] = [r["proof"] for r in recs]
    out.update(status=status, pt=pt)
    # ---- the send side
    if reply:
        sources = []
        for k in ("lr_proofs", "proofs", "dest_proofs"):
            rows = out.get(k) or [None] * m
            sources.append(([(r or b"").ljust(rh.ROW, b"\0") for r in rows], [len(r or b"") for r in rows]))
        while sources and out.get(("lr_proofs", "proofs", "dest_proofs")[len(sources) - 1]) is None:
            sources.pop()                                   # absent stages behind the last present one are no sources
        cap = m if max_replies is None else max_replies
        replies, found = rh.gather_model(sources, cap)
        if nd.seen is not None:
            nd.seen.add([rh.packet_hash(r) for _, _, r in replies])
        out["replies"], out["reply_counts"] = replies, [len(replies), found]
        out["reply_frames"] = rh.reply_stream_model(replies, nd.ifac_key, ifac_size)
    return out


def lengths(rows):
    return [len(r or b"") for r in rows]


# ---------------------------------------------------------------- the world

class World:
    """The node of the mixed read, the remote ends its frames come from, and
    the frames by kind: instance k of a kind is the same packet in every
    layout, so what a layout costs the host model is paid once."""

    def __init__(self):
        rng = _rng(0)
        self.ifac_key, self.tid, self.other_tid = _rb(rng, 64), _rb(rng, 16), _rb(rng, 16)
        self.keys = [_rb(rng, 64) for _ in range(N_KEYS)]
        self.link_ids = [_rb(rng, 16) for _ in range(PRE_LINKS)]
        self.seeds = [_rb(rng, 32) for _ in range(N_KEYS)]                 # the node's signing seed per link row
        self.peer_seeds = [_rb(rng, 32) for _ in range(PRE_LINKS)]         # the peers' of the links that exist
        self.peer_publics = [ed.public_key(s) for s in self.peer_seeds] + [_rb(rng, 32) for _ in range(N_KEYS - PRE_LINKS)]
        self.flags = [ph.PROVE_ALL, ph.PROVE_ALL] + [0] * (N_KEYS - 2)
        self.dests = [dd.make_dest(rng, 0, dd.F_PROVE_ALL), dd.make_dest(rng, 2, dd.F_PROVE_ALL), dd.make_dest(rng, 1, 0)]
        self.ldests = [la.Dest(d.hash, d.seed, la.F_ACCEPTS | (d.flags & dd.F_PROVE_ALL)) for d in self.dests]
        self.ephemerals = [_rb(rng, 32) for _ in range(N_KEYS - FIRST_SLOT)]
        self.slots = list(range(FIRST_SLOT, N_KEYS))
        # the link this node asked for, and the destination that answers
        self.remote_seed = _rb(rng, 32)
        self.remote_public = ed.public_key(self.remote_seed)
        self.opened = lp.Pending(_rb(rng, 16), _rb(rng, 32), self.remote_public, _rb(rng, 32), ph.PROVE_ALL,
                                 PENDING_SLOT, 1)
        # receipts of what this node sent: on links 2 and 3, and to two remote SINGLE destinations
        self.link_hashes = [_rb(rng, 32) for _ in range(POOL)]
        self.dest_hashes = [_rb(rng, 32) for _ in range(DEST_POOL)]
        self.recipient_seeds = [_rb(rng, 32), _rb(rng, 32)]
        self.dest_keys = [ed.public_key(self.recipient_seeds[r & 1]) for r in range(DEST_POOL)]
        self._made = {}

    # -- the node's state at the start of a read
    def node(self, caps=False):
        nd = Node(self.ifac_key, self.tid, self.keys, dict(zip(self.link_ids, range(PRE_LINKS))))
        nd.signers = ph.Signers(self.seeds, self.peer_publics, self.flags)
        nd.accept = dict(dests=self.ldests, slots=self.slots, ephemerals=self.ephemerals, nh_mtu=500)
        nd.pending = {self.opened.link_id: self.opened.copy()}
        nd.deliver = dict(dests=self.dests, retry_trials=CAPS["retry_trials"] if caps else 1024, implicit=True)
        nd.receipts = ph.Receipts(MAX_RECEIPTS)
        assert nd.receipts.add(self.link_hashes, range(POOL)) == [lh.OK] * POOL
        nd.dest_receipts = dp.Receipts(MAX_RECEIPTS)
        assert nd.dest_receipts.add(self.dest_hashes, range(DEST_POOL), self.dest_keys) == [lh.OK] * DEST_POOL
        if caps:
            nd.scan_trials = CAPS["scan_trials"]
        nd.seen = fh.ListModel(MAX_HASHES, self.tid)
        nd.announces = True
        return nd

    # -- frames
    def _link_data(self, rng, link_id, key, context, text):
        return bytes([lh.LINK << 2 | lh.DATA, 0]) + link_id + bytes([context]) + ctoken.encrypt(key, _rb(rng, 16), text)

    def instance(self, kind, k):
        """The raw packet of instance k of a kind (the BAD_CODE kind's packet is
        good: the wire gives it the bad code)."""
        if (kind, k) not in self._made:
            self._made[kind, k] = self._make(kind, k, _rng(1, kind, k))
        return self._made[kind, k]

    def _make(self, kind, k, rng):
        text = _rb(rng, 1 + (7 * k) % 90)
        if kind in (LINK_PROVED, BAD_CODE):
            return self._link_data(rng, self.link_ids[k % 2], self.keys[k % 2], lh.NONE, text)
        if kind == LINK_PLAIN:
            link = 2 + k % 2
            raw = self._link_data(rng, self.link_ids[link], self.keys[link], (lh.NONE, lh.RESPONSE, lh.KEEPALIVE)[k % 3], text)
            return raw[:-1] + bytes([raw[-1] ^ 1]) if k % 8 == 7 else raw          # a tag that does not verify
        if kind == REQUEST:
            return self.request(k)[0]
        if kind == SINGLE_PROVED:
            d, rank = ((0, None), (1, 0), (1, 1), (1, None))[k % 4]
            return dd.packet(dd.seal(self.dests[d], rank, text, _rb(rng, 32), _rb(rng, 16)), self.dests[d].hash)
        if kind == SINGLE_PLAIN:
            return dd.packet(dd.seal(self.dests[2], (0, None)[k % 2], text, _rb(rng, 32), _rb(rng, 16)), self.dests[2].hash)
        if kind == RECEIPT_PROOF:
            link = 2 + k % 2
            h = self.link_hashes[k] if k < POOL else _rb(rng, 32)
            sig = ph.sign(self.peer_seeds[link if k % 8 != 6 else 5 - link], h)     # 6 of 8: the other peer's key
            return bytes([lh.LINK << 2 | lh.PROOF, 0]) + self.link_ids[link] + bytes([lh.NONE]) + h + sig
        if kind == DEST_PROOF:
            h = self.dest_hashes[k] if k < DEST_POOL else _rb(rng, 32)      # past the pool: no receipt
            seed = self.recipient_seeds[(k & 1) ^ (k % 16 == 9)]                    # 9 of 16: the other recipient's key
            if k % 16 == 5:
                return dp.proof_packet(h, seed, True, address=_rb(rng, 16))        # a stray that validates
            return dp.proof_packet(h, seed, k % 4 == 3 and k < DEST_POOL)            # (an implicit proof of nothing known is a stray)
        if kind == ANNOUNCE:
            dest, data = aa.Announcer(rng).data(app=text[:20], ratchet=bool(k & 2))
            if k & 1:
                data = data[:-1] + bytes([data[-1] ^ 1])                            # tampered
            return aa.raw_packet(dest, data, ratchet=bool(k & 2))
        if kind == OTHER_TRANSPORT:
            return dd.packet(_rb(rng, 80), self.dests[0].hash, header2=self.other_tid)
        if kind == NOISE:
            if k & 1:
                return bytes([lh.LINK << 2 | lh.DATA, 0]) + _rb(rng, 16) + b"\x00" + _rb(rng, 70)
            return _rb(rng, 24 + (5 * k) % 97)
        if kind == LRPROOF:
            pub = la.x25519(_rb(rng, 32), BASE)
            sg = lp.signalling(700)
            o = self.opened
            sig = ed.sign(self.remote_seed, o.link_id + pub + self.remote_public + sg, self.remote_public)
            return bytes([0x0F, 0]) + o.link_id + b"\xff" + sig + pub + sg
        raise ValueError(kind)

    def request(self, k, dest=None, mtu=0):
        """(raw, the initiator's ephemeral private key, its signing seed) of
        link request k; ``mtu`` 0: by k, 500 signalled or no signalling."""
        rng = _rng(2, k)
        prv, seed = _rb(rng, 32), _rb(rng, 32)
        d = self.dests[k % 3 if dest is None else dest]
        mtu = mtu or (500, None)[k % 2]
        raw = b"\x02\x00" + d.hash + b"\x00" + la.x25519(prv, BASE) + ed.public_key(seed) + \
            (la.signalling(mtu) if mtu else b"")
        return raw, prv, seed


def kinds_of(layout, n=N):
    """The kind of every frame of a layout: the fixed rule."""
    kinds = [CYCLE[(i + layout) % len(CYCLE)] for i in range(n)]
    wave_kind = REPLY_KINDS[layout % 3] if layout < 3 else LINK_PROVED
    for i in NOISE_WAVE:
        kinds[i] = NOISE
    for i in REPLY_WAVE:
        kinds[i] = wave_kind
    if layout < 3:
        for i in EDGES:
            if i < n:
                kinds[i] = REPLY_KINDS[layout]
    else:
        # the reply kinds leave this layout's edges free: the kinds that settle receipts take last lanes of waves
        for i, kind in ((63, RECEIPT_PROOF), (255, DEST_PROOF), (447, RECEIPT_PROOF), (511, DEST_PROOF)):
            kinds[i] = kind
        kinds[n - 1] = LRPROOF
    for i in (EARLY_DATA, DATA_A, SINGLE_A, REQUEST_A, PROOF_A, LATE_DATA, DATA_B, SINGLE_B, REQUEST_B, PROOF_B):
        kinds[i] = MEETING
    return kinds


MEETING_REQUEST = 1 << 20        # the request instance of the meetings, outside the cycle's


def build(world, layout, n=N):
    """The frames of a layout: [(kind, raw)]."""
    w = world
    kinds = kinds_of(layout, n)
    count, frames = {}, [None] * n
    for i, kind in enumerate(kinds):
        if kind != MEETING:
            k = count.get(kind, 0)
            count[kind] = k + 1
            frames[i] = (kind, w.instance(kind, k))
    rng = _rng(3, layout, n)
    # the same link DATA frame and the same SINGLE frame twice, in different workgroups
    frames[DATA_A] = frames[DATA_B] = (MEETING, w.instance(LINK_PROVED, 1 << 20))
    frames[SINGLE_A] = frames[SINGLE_B] = (MEETING, w.instance(SINGLE_PROVED, (1 << 20) + 1))
    # two link requests with one link id (the id does not cover the signalling bytes): to the PROVE_ALL destination 0
    req_a = w.request(MEETING_REQUEST, dest=0, mtu=500)[0]
    frames[REQUEST_A], frames[REQUEST_B] = (MEETING, req_a), (MEETING, w.request(MEETING_REQUEST, dest=0, mtu=600)[0])
    # two PROOFs for one link receipt: the second carries a byte more, which Packet.py:434-459 does not read
    proof = w.instance(RECEIPT_PROOF, POOL - 1)
    frames[PROOF_A], frames[PROOF_B] = (MEETING, proof), (MEETING, proof + b"\x00")
    # DATA on the link REQUEST_A opens, behind it and (the documented difference, once) ahead of it.  Its key is
    # the one the stage derives for the request's rank among the valid requests of the read.
    rank = sum(1 for i in range(REQUEST_A) if kinds[i] == REQUEST)
    st, (dest, link_id, mtu, peer_pub, _) = la.decide(req_a, w.ldests, w.tid, 500)
    assert st == la.ACCEPTED
    key, _ = la.establish(dest, link_id, mtu, peer_pub, w.ephemerals[rank])
    frames[EARLY_DATA] = (MEETING, w._link_data(rng, link_id, key, lh.NONE, b"ahead of its request"))
    frames[LATE_DATA] = (MEETING, w._link_data(rng, link_id, key, lh.NONE, b"behind its request"))
    return frames


def wire_of(world, frames, ifac_size):
    """The framed stream.  With access codes every frame is masked under its
    code, the BAD_CODE kind's under a code with one bit flipped; without,
    packets go as they are and the BAD_CODE kind's carry the IFAC flag."""
    out = []
    for kind, raw in frames:
        if ifac_size:
            code = ih.code(world.ifac_key, raw, ifac_size)
            if kind == BAD_CODE:
                code = bytes([code[0] ^ 0x80]) + code[1:]
            out.append(ow.hdlc_frame(ow.ifac_mask(raw, code, world.ifac_key)))
        else:
            out.append(ow.hdlc_frame(bytes([raw[0] | 0x80]) + raw[1:] if kind == BAD_CODE else raw))
    return b"".join(out)


def peer_node(world, frames):
    """The other ends of the read, as one node: it holds the receipts of every
    packet of ``frames`` that asks for a proof, the pending links of its
    requests and the links 0 and 1, so that it can read the node's replies."""
    w = world
    rng = _rng(4)
    nd = Node(w.ifac_key, _rb(rng, 16), [_rb(rng, 64) for _ in range(N_KEYS)], dict(zip(w.link_ids[:2], (0, 1))))
    node_publics = [ed.public_key(s) for s in w.seeds[:PRE_LINKS]] + [_rb(rng, 32) for _ in range(N_KEYS - PRE_LINKS)]
    nd.signers = ph.Signers([_rb(rng, 32) for _ in range(N_KEYS)], node_publics, [0] * N_KEYS)
    nd.max_receipts = 1024
    nd.receipts, nd.dest_receipts, nd.pending = ph.Receipts(1024), dp.Receipts(1024), {}
    nd.scan_trials = 4096
    sent, slot = set(), FIRST_SLOT
    for kind, raw in frames:
        f = ow.unpack(raw)
        if f is None or raw in sent:
            continue
        sent.add(raw)
        if f["packet_type"] == lh.DATA and f["destination_type"] == lh.LINK:
            nd.receipts.add([f["packet_hash"]], [len(nd.receipts.hashes)])
        elif f["packet_type"] == lh.DATA and f["destination_type"] == lh.SINGLE and not f["header_type"]:
            d = next((x for x in w.dests if x.hash == f["destination_hash"]), None)
            if d is not None:
                nd.dest_receipts.add([f["packet_hash"]], [len(nd.dest_receipts.hashes)], [d.public])
    for k in [MEETING_REQUEST] + list(range(sum(1 for kind, _ in frames if kind == REQUEST))):
        dest = 0 if k == MEETING_REQUEST else None
        raw, prv, seed = w.request(k, dest=dest, mtu=500 if k == MEETING_REQUEST else 0)
        link_id = la.decide(raw, w.ldests, w.tid, 500)[1][1]
        d = w.dests[0 if k == MEETING_REQUEST else k % 3]
        nd.pending[link_id] = lp.Pending(link_id, prv, d.public, seed, 0, slot, 1)
        slot += 1
    return nd


# ---------------------------------------------------------------- the 8-frame world of the reply test

REPLY_N_KEYS, REPLY_SLOT, REPLY_PEER_SLOT = 8, 4, 6


def reply_world():
    """The world of tests/test_reply_pipeline_gpu.py, made on the host alone:
    the node, its peer's link request, and the eight frames the peer sent."""
    rng = np.random.Generator(np.random.PCG64(1069))
    w = dict(rng=rng, ifac_key=_rb(rng, 64), tid=_rb(rng, 16), peer_tid=_rb(rng, 16))
    keys = [_rb(rng, 64) for _ in range(REPLY_N_KEYS)]
    link_ids = [_rb(rng, 16), _rb(rng, 16)]
    seeds = [_rb(rng, 32) for _ in range(REPLY_N_KEYS)]
    dests = [dd.make_dest(rng, 0, dd.F_PROVE_ALL), dd.make_dest(rng, 2, dd.F_PROVE_ALL)]
    # the peer opens a link to destination 1 of the node: the request, and the pending link on its side
    prv, sig_seed = _rb(rng, 32), _rb(rng, 32)
    request = b"\x02\x00" + dests[1].hash + b"\x00" + la.x25519(prv, BASE) + ed.public_key(sig_seed) + la.signalling(500)
    ldests = [la.Dest(d.hash, d.seed, la.F_ACCEPTS) for d in dests]
    link_id = la.decide(request, ldests, w["tid"], 500)[1][1]
    opened = lp.Pending(link_id, prv, dests[1].public, sig_seed, 0, REPLY_PEER_SLOT, 1)

    def link_data(k, text):
        return bytes([lh.LINK << 2 | lh.DATA, 0]) + link_ids[k] + b"\x00" + ctoken.encrypt(keys[k], _rb(rng, 16), text)

    def single(k, rank, text):
        return dd.packet(dd.seal(dests[k], rank, text, _rb(rng, 32), _rb(rng, 16)), dests[k].hash)

    frames = [
        ("link 0", link_data(0, b"on link 0")),
        ("noise", bytes([lh.LINK << 2 | lh.DATA, 0]) + _rb(rng, 16) + b"\x00" + _rb(rng, 70)),
        ("single 0", single(0, None, b"to destination 0")),
        ("request", request),
        ("link 1", link_data(1, b"on link 1")),
        ("single 1", single(1, 0, b"by the newest ratchet")),
        ("more noise", _rb(rng, 40)),
        ("link 0 again", link_data(0, b"and one more")),
    ]
    w.update(keys=keys, link_ids=link_ids, seeds=seeds, dests=dests, ldests=ldests, opened=opened, link_id=link_id,
             frames=frames, peer_publics=[_rb(np.random.Generator(np.random.PCG64(k)), 32) for k in range(REPLY_N_KEYS)],
             flags=[ph.PROVE_ALL, ph.PROVE_ALL] + [0] * (REPLY_N_KEYS - 2),
             ephemerals=[_rb(np.random.Generator(np.random.PCG64(77)), 64)[k * 32:k * 32 + 32] for k in range(2)])
    return w


def reply_node(w, seen=True):
    """The node of the reply test as it reads with ``signers``, ``accept`` and ``deliver``."""
    nd = Node(w["ifac_key"], w["tid"], w["keys"], dict(zip(w["link_ids"], (0, 1))))
    nd.signers = ph.Signers(w["seeds"], w["peer_publics"], w["flags"])
    nd.accept = dict(dests=w["ldests"], slots=[REPLY_SLOT, REPLY_SLOT + 1], ephemerals=w["ephemerals"], nh_mtu=500)
    nd.deliver = dict(dests=w["dests"], retry_trials=32, implicit=True)
    if seen:
        nd.seen = fh.ListModel(1024, w["tid"])
    return nd


def reply_wire(w):
    return b"".join(ow.hdlc_frame(ow.ifac_mask(r, ih.code(w["ifac_key"], r, ISZ), w["ifac_key"])) for _, r in w["frames"])
