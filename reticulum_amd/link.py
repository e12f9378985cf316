"""Links on the device: which link an inbound packet belongs to, and the keys
of a batch of links.

A Reticulum node has many links at once.  Transport.inbound finds the link of
each DATA packet by its destination hash (Transport.py:2161-2176: the first
link in ``active_links`` whose ``link_id`` matches) and Link.receive decides by
context whether the packet is decrypted (Link.py:941-1148).  :class:`LinkTable`
keeps the link ids in device memory (16-byte id -> the index of the link's key
in a :class:`KeySet`), ``pipeline.inbound(..., links=table)`` runs the lookup
and the decision between unpack and decrypt, and :func:`derive_link_keys`
builds the keys of a batch of links from their handshakes (Link.py:348-361).

Value v of the table means key v of the key set the batch is decrypted with
(INTEGRATION.md §6).  For links that others open to this node the device keeps
the two in step itself: :class:`LinkDestinations` holds the node's own
destinations, and ``pipeline.inbound(..., accept=...)`` / ``device.link_accept``
answer the link requests of a read (Transport.py:2127-2158, Link.py:186-227),
entering each new link into the table, its key into the key set and its rows
into the signers under one slot of the caller's free list.
"""
import contextlib
import hashlib

import numpy as np

from . import _native
from .token import KeySet  # noqa: F401  (the type derive_link_keys returns)

MODE_AES128_CBC, MODE_AES256_CBC = 0x00, 0x01          # Link.py:94-95
ECPUBSIZE = 64                                        # Link.py:73: X25519 + Ed25519 public keys
LINK_ID_LEN = 16                                      # Reticulum.TRUNCATED_HASHLENGTH // 8
HEADER_2 = 0x01
MTU = 500                                             # Reticulum.MTU: a link's MTU without signalling
LRPROOF_LEN = 118                                     # Packet.py:170-185 around Link.prove's proof data
# what became of a record in the link request stage: RT_LINKREQ_* (include/rnstok.h)
LINKREQ_ACCEPTED, LINKREQ_NOT_REQUEST, LINKREQ_OTHER_TRANSPORT = 0, 1, 2
LINKREQ_NO_DESTINATION, LINKREQ_NOT_ACCEPTING, LINKREQ_BAD_SIZE, LINKREQ_BAD_MODE = 3, 4, 6, 7
LINKREQ_DUPLICATE, LINKREQ_NO_SLOT = 8, 9
# a destination's flags: the two a new link's signer row inherits (proof.PROVE_ALL, proof.HAS_CHANNEL), and
ACCEPTS, PROVE_ALL, HAS_CHANNEL = 4, 1, 2             # RT_DEST_ACCEPTS, RT_LINK_PROVE_ALL, RT_LINK_HAS_CHANNEL


def link_id_from_lr_packet(raw):
    """Link.link_id_from_lr_packet (Link.py:336-342) for a packed link
    request ``raw``: the truncated SHA-256 of the packet's hashable part
    (Packet.py:342-353: flags & 0x0F, then everything after the hop count, or
    after the transport id of a HEADER_2 packet) without the signalling bytes
    that follow the two public keys where the data is longer than 64 bytes."""
    raw = bytes(raw)
    header_2 = (raw[0] >> 6) & 1 == HEADER_2
    data_at = 35 if header_2 else 19
    if len(raw) < data_at:
        raise ValueError("packet too short for its header")
    hashable = bytes([raw[0] & 0x0F]) + (raw[18:] if header_2 else raw[2:])
    extra = len(raw) - data_at - ECPUBSIZE
    if extra > 0:
        hashable = hashable[:-extra]
    return hashlib.sha256(hashable).digest()[:LINK_ID_LEN]


class _Lazy:
    """torch and reticulum_amd.device, imported at first use: importing the
    package does not import torch (link_id_from_lr_packet needs neither)."""

    def __init__(self, name, package=None):
        self._name, self._package, self._mod = name, package, None

    def __getattr__(self, attr):
        if self._mod is None:
            import importlib
            self._mod = importlib.import_module(self._name, self._package)
        return getattr(self._mod, attr)


torch = _Lazy("torch")
_dev = _Lazy(".device", __package__)


def _torch_device(dev):
    if dev is None:
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device("cuda", dev) if isinstance(dev, int) else torch.device(dev)
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _rows(x, width, dev, name):
    """(n, width) uint8 rows on ``dev`` from a device tensor, a numpy array or
    a sequence of ``width``-byte strings."""
    if isinstance(x, torch.Tensor):
        t = x
    elif isinstance(x, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint8))
    else:
        rows = [bytes(r) for r in x]
        if any(len(r) != width for r in rows):
            raise ValueError(f"{name} must be {width} bytes each")
        t = torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).copy()).view(len(rows), width)
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"{name} must be (n, {width}) uint8 rows")
    return t.to(dev).contiguous()


class LinkTable:
    """A device-resident map from 16-byte link id to an int (the index of the
    link's key in a :class:`KeySet`) for at most ``max_links`` links.

    ``insert``, ``remove`` and ``lookup`` take a batch of ids ((n, 16) uint8
    device tensor, numpy array, or a sequence of 16-byte strings), enqueue on
    ``stream`` (default: the current stream of the table's GPU) and return
    device tensors without synchronising; ``len()`` reads the count back."""

    def __init__(self, max_links, device=None):
        max_links = int(max_links)
        if not 1 <= max_links <= 1 << 29:
            raise ValueError("max_links must be 1 .. 2**29")
        self.device = _torch_device(device)
        self.max_links = max_links
        self._lib = _native.load()
        self._ptr = self._lib.rt_linktable_create(_native.context(self.device.index), max_links)
        if not self._ptr:
            raise _native.NativeError(-1, _native.last_error())
        self.capacity = int(self._lib.rt_linktable_capacity(self._ptr))

    @property
    def handle(self):
        return self._ptr

    def __del__(self):
        p = getattr(self, "_ptr", None)
        if p:
            try:
                self._lib.rt_linktable_destroy(p)
            except Exception:
                pass
            self._ptr = None

    def _values(self, values, n):
        if isinstance(values, torch.Tensor):
            v = values
        else:
            v = np.asarray(values)
            if v.size and (v.min() < 0 or v.max() > 0x7FFFFFFF):
                raise ValueError("values must be 0 .. 2**31 - 1")
            v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32))
        if v.dtype != torch.int32 or v.numel() != n:
            raise ValueError(f"values must be ({n},) int32")
        return v.to(self.device).contiguous()

    def insert(self, ids, values, stream=None):
        """Enter ids[i] -> values[i].  Returns the (n,) int32 status:
        device.LINK_OK, LINK_DUPLICATE (the id is present, or comes earlier in
        this batch: the earlier one stays) or LINK_FULL."""
        ids = _rows(ids, LINK_ID_LEN, self.device, "link ids")
        n = ids.shape[0]
        values = self._values(values, n)
        with _on(stream):
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        _dev._order_after_current(stream, ids, values)
        _dev.linktable_insert(self._ptr, ids, values, status, stream=stream)
        return status

    def remove(self, ids, stream=None):
        """Remove ids[i].  Returns the (n,) int32 status: LINK_OK or LINK_MISSING."""
        ids = _rows(ids, LINK_ID_LEN, self.device, "link ids")
        with _on(stream):
            status = torch.empty(ids.shape[0], dtype=torch.int32, device=self.device)
        _dev._order_after_current(stream, ids)
        _dev.linktable_remove(self._ptr, ids, status, stream=stream)
        return status

    def lookup(self, ids, stream=None):
        """(values, found): (n,) int32 values (-1 on a miss) and (n,) bool."""
        ids = _rows(ids, LINK_ID_LEN, self.device, "link ids")
        n = ids.shape[0]
        with _on(stream):
            values = torch.empty(n, dtype=torch.int32, device=self.device)
            found = torch.empty(n, dtype=torch.uint8, device=self.device)
        _dev._order_after_current(stream, ids)
        _dev.linktable_lookup(self._ptr, ids, values, found, stream=stream)
        with _on(stream):
            return values, found.bool()

    def __len__(self):
        """Entries present (waits for the table's queued work)."""
        count = torch.empty(1, dtype=torch.int32, device=self.device)
        _dev.linktable_count(self._ptr, count)
        return int(count.item())


def _on(stream):
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def derive_link_keys(privates, peer_publics, link_ids, mode=MODE_AES256_CBC, device=None):
    """The handshake keys of a batch of links (Link.handshake, Link.py:348-361)
    as a :class:`KeySet`: key i is Token(hkdf(L, X25519(privates[i],
    peer_publics[i]), salt=link_ids[i], context=None)) with L = 64 for
    MODE_AES256_CBC and 32 for MODE_AES128_CBC, in one call; neither the
    shared secrets nor the derived keys leave the device.  ``privates`` and
    ``peer_publics`` are (n, 32) and ``link_ids`` (n, 16) uint8 rows (device
    tensors, numpy arrays or sequences of byte strings)."""
    if mode == MODE_AES128_CBC:
        key_len = 32
    elif mode == MODE_AES256_CBC:
        key_len = 64
    else:
        raise TypeError(f"Invalid link mode {mode}")
    dev = privates.device if isinstance(privates, torch.Tensor) and privates.is_cuda else _torch_device(device)
    prv = _rows(privates, 32, dev, "privates")
    pub = _rows(peer_publics, 32, dev, "peer_publics")
    ids = _rows(link_ids, LINK_ID_LEN, dev, "link_ids")
    n = prv.shape[0]
    if n < 1 or pub.shape[0] != n or ids.shape[0] != n:
        raise ValueError("privates, peer_publics and link_ids must hold one row per link (at least one)")
    return _dev.derive_keyset_x25519(prv, pub, salt=ids, context=None, key_len=key_len, n=n)


class LinkDestinations:
    """The node's own SINGLE destinations on the device, for the link request
    stage: a :class:`LinkTable` from 16-byte destination hash to row, and per
    row the identity's Ed25519 signing seed, its public key (derived once,
    device.ed25519_public) and a flags byte: ACCEPTS (accept_link_requests,
    Destination.py:432) and PROVE_ALL | HAS_CHANNEL, which become the flags of
    a new link's :class:`reticulum_amd.proof.LinkSigners` row (a destination
    that proves by callback, PROVE_APP, gets neither).

    ``hashes`` (n, 16), ``seeds`` (n, 32) and ``flags`` (n,) may be device
    tensors, numpy arrays or sequences (of byte strings; flags: of ints).
    Nothing of it leaves the device."""

    def __init__(self, hashes, seeds, flags, device=None):
        dev = _torch_device(device)
        self.device = dev
        self.hashes = _rows(hashes, LINK_ID_LEN, dev, "destination hashes")
        self.n = int(self.hashes.shape[0])
        if self.n < 1:
            raise ValueError("at least one destination")
        self.seeds = _rows(seeds, 32, dev, "seeds")
        if self.seeds.shape[0] != self.n:
            raise ValueError("seeds must hold one row per destination")
        if isinstance(flags, torch.Tensor):
            fl = flags
        else:
            fl = np.asarray(flags)
            if fl.size and (fl.min() < 0 or fl.max() > ACCEPTS | PROVE_ALL | HAS_CHANNEL):
                raise ValueError("flags are ACCEPTS | PROVE_ALL | HAS_CHANNEL")
            fl = torch.from_numpy(np.ascontiguousarray(fl, dtype=np.uint8))
        if fl.dtype != torch.uint8 or fl.numel() != self.n:
            raise ValueError(f"flags must be ({self.n},) uint8")
        self.flags = fl.to(dev).contiguous().view(self.n)
        self.publics = torch.empty_like(self.seeds)
        _dev.ed25519_public(self.seeds, self.publics)
        self.table = LinkTable(self.n, device=dev)
        status = self.table.insert(self.hashes, torch.arange(self.n, dtype=torch.int32, device=dev))
        if bool((status != 0).any()):                   # once, at construction: reads the status back
            raise ValueError("destination hashes must be distinct: a repeated one could never reach its row")


def accept_requests_batch(raws, ks, links, destinations, transport_identity, slots, ephemeral_privates, nh_mtu=MTU,
                          signers=None):
    """The link request stage for callers without torch tensors: ``raws`` is a
    sequence of raw packets (byte strings, as the interface handed them on),
    ``transport_identity`` 16 bytes, ``slots`` a sequence of free slots and
    ``ephemeral_privates`` as many 32-byte strings of fresh randomness
    (os.urandom, as X25519PrivateKey.generate draws it).  Unpacks the packets
    and runs device.link_accept over them against ``ks``, ``links``
    (:class:`LinkTable`), ``destinations`` (:class:`LinkDestinations`) and
    optional ``signers``.  Returns one dict per packet: ``status`` (LINKREQ_*),
    ``slot`` (or -1), ``link_id`` and ``mtu`` (for a valid request, else None)
    and ``lrproof`` (the 118-byte packet to send, or None)."""
    dev = links.device
    raws = [bytes(r) for r in raws]
    n = len(raws)
    if n == 0:
        return []
    off = np.zeros(n, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])[:-1]
    pkt = torch.from_numpy(np.frombuffer(b"".join(raws) + b"\0", dtype=np.uint8).copy()).to(dev)
    pkt_off = torch.from_numpy(off).to(dev)
    pkt_len = torch.tensor([len(r) for r in raws], dtype=torch.int32, device=dev)
    fields = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    _dev.packet_unpack(pkt, pkt_off, pkt_len, fields)
    slots = torch.as_tensor(np.asarray(list(slots), dtype=np.int32)).to(dev)
    m = slots.numel()
    eph = _rows(ephemeral_privates, 32, dev, "ephemeral_privates") if m else \
        torch.empty((0, 32), dtype=torch.uint8, device=dev)
    tid = torch.from_numpy(np.frombuffer(bytes(transport_identity), dtype=np.uint8).copy()).to(dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    accepted = torch.empty(n, dtype=torch.int32, device=dev)
    mtu = torch.empty(n, dtype=torch.int32, device=dev)
    plen = torch.empty(n, dtype=torch.int32, device=dev)
    ids = torch.empty((n, LINK_ID_LEN), dtype=torch.uint8, device=dev)
    proofs = torch.zeros((n, 128), dtype=torch.uint8, device=dev)
    _dev.link_accept(ks, links, destinations, tid, pkt, pkt_off, fields, slots, eph, status, accepted, ids, mtu,
                     proofs, plen, nh_mtu=nh_mtu, signers=signers)
    status, accepted, mtu, plen = (t.cpu().numpy() for t in (status, accepted, mtu, plen))
    ids, proofs = ids.cpu().numpy(), proofs.cpu().numpy()
    valid = (LINKREQ_ACCEPTED, LINKREQ_DUPLICATE, LINKREQ_NO_SLOT)
    return [{"status": int(status[i]), "slot": int(accepted[i]),
             "link_id": ids[i].tobytes() if status[i] in valid else None,
             "mtu": int(mtu[i]) if status[i] in valid else None,
             "lrproof": proofs[i, :LRPROOF_LEN].tobytes() if plen[i] == LRPROOF_LEN else None} for i in range(n)]


# Link request proofs: the initiator side (lrproof_kernels.hip).  A link's
# state is the reference's (Link.PENDING, HANDSHAKE, ACTIVE, CLOSED), and what
# became of a record RT_LRPROOF_* (include/rnstok.h).
PENDING, HANDSHAKE, ACTIVE, CLOSED = 0x00, 0x01, 0x02, 0x04
LRPROOF_ACTIVATED, LRPROOF_NOT_LRPROOF, LRPROOF_NO_LINK, LRPROOF_NOT_PENDING = 0, 1, 2, 3
LRPROOF_HOPS, LRPROOF_BAD_SIZE, LRPROOF_BAD_MODE, LRPROOF_BAD_SIGNATURE, LRPROOF_NO_SLOT = 4, 6, 7, 8, 9
CONTEXT_LRRTT = 0xFE                                  # Packet.LRRTT
MTU_BYTEMASK = 0x1FFFFF                               # Link.MTU_BYTEMASK


def signalling_bytes(mtu, mode=MODE_AES256_CBC):
    """Link.signalling_bytes (Link.py:148-151) for the one enabled mode."""
    if mode != MODE_AES256_CBC:
        raise TypeError(f"Requested link mode {mode} not enabled")
    return ((mtu & MTU_BYTEMASK) + (((mode << 5) & 0xE0) << 16)).to_bytes(3, "big")


def pack_rtt(rtt):
    """The LRRTT packet's plaintext (Link.py:435): umsgpack.packb of a float,
    0xcb and the big-endian double, 9 bytes.  The caller sends it on the new
    link with ``outbound(..., key_idx=slot, context=CONTEXT_LRRTT)``; the RTT is
    host time and the token's IV fresh randomness, both the caller's."""
    import struct
    return b"\xcb" + struct.pack(">d", float(rtt))


class PendingLinks:
    """The links this node has requested and that wait for their proof
    (Transport.pending_links), on the device: a :class:`LinkTable` from the
    16-byte link id to a row, and per row the initiator's ephemeral X25519
    private key, the destination identity's Ed25519 public key, the link's own
    Ed25519 seed (its ``sig_prv``) and public key, the flags of its
    :class:`reticulum_amd.proof.LinkSigners` row, the slot it is to take in
    ``links`` / ``ks`` / ``signers``, and its state as the reference keeps it:
    ``expected_hops``, ``rebalanced``, ``state`` (PENDING, HANDSHAKE, ACTIVE,
    CLOSED) and ``mtu`` (written on activation).  The slots of the pending
    links are distinct, as a free list gives them: two rows with one slot
    would both come up and write the same key record and signer row.
    ``pipeline.inbound(..., establish=pending)`` / ``device.link_establish``
    validate the LRPROOFs of a read against it.

    ``add`` and ``remove`` are batched and enqueue on ``stream`` without
    synchronising; which row an id has is kept on the host, so the ids are host
    data (bytes, or anything ``bytes()`` takes).  ``state()`` and ``hops()``
    read back for the caller's bookkeeping (the path table's rebalance,
    callbacks, the LRRTT).  Nothing private leaves the device."""

    def __init__(self, max_pending, device=None):
        self.table = LinkTable(max_pending, device=device)
        dev = self.device = self.table.device
        n = self.max_pending = self.table.max_links
        z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)     # noqa: E731
        self.privates, self.dest_publics, self.sig_seeds, self.sig_publics = (z8(n, 32) for _ in range(4))
        self.flags, self.rebalanced = z8(n), z8(n)
        self.row_state = torch.full((n,), CLOSED, dtype=torch.uint8, device=dev)
        self.slots = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.expected_hops = torch.zeros(n, dtype=torch.int32, device=dev)
        self.mtu = torch.zeros(n, dtype=torch.int32, device=dev)
        self._row = {}                                  # link id -> row
        self._free = list(range(n - 1, -1, -1))

    def __len__(self):
        return len(self._row)

    def row_of(self, link_id):
        """The row of a pending link, or None."""
        return self._row.get(bytes(link_id))

    def add(self, link_ids, privates, dest_sig_publics, sig_seeds, flags, slots, expected_hops, stream=None):
        """Enter links.  Returns the (n,) int32 numpy status: device.LINK_OK,
        LINK_DUPLICATE (the id is pending, or comes earlier in this batch: the
        earlier one stays) or LINK_FULL (no free row)."""
        ids = [bytes(i) for i in link_ids]
        n = len(ids)
        if any(len(i) != LINK_ID_LEN for i in ids):
            raise ValueError("link ids are 16 bytes each")
        dev = self.device

        def rows_of(x, width, name):
            t = _rows(x, width, dev, name)
            if t.shape[0] != n:
                raise ValueError(f"{name} must hold one row per link")
            return t

        def ints(x, dtype, name):
            t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype)
            if t.numel() != n:
                raise ValueError(f"{name} must hold one value per link")
            return t.to(dev, dtype).view(n)

        # every input is checked before a row is taken: a call that raises leaves the links as they were
        with _on(stream):
            prv, pub = rows_of(privates, 32, "privates"), rows_of(dest_sig_publics, 32, "dest_sig_publics")
            seeds = rows_of(sig_seeds, 32, "sig_seeds")
            fl, sl = ints(flags, torch.uint8, "flags"), ints(slots, torch.int32, "slots")
            hops = ints(expected_hops, torch.int32, "expected_hops")
        status = np.zeros(n, dtype=np.int32)
        rows, take, taken = [], [], set()
        free = len(self._free)
        for k, i in enumerate(ids):
            if i in self._row or i in taken:
                status[k] = 1
            elif len(take) == free:
                status[k] = 2
            else:
                taken.add(i)
                take.append(k)
        if not take:
            return status
        for k in take:
            self._row[ids[k]] = self._free.pop()
            rows.append(self._row[ids[k]])
        with _on(stream):
            pick = torch.as_tensor(take, dtype=torch.int64).to(dev)
            r = torch.as_tensor(rows, dtype=torch.int64).to(dev)
            seeds = seeds[pick].contiguous()
            publics = torch.empty_like(seeds)
        _dev.ed25519_public(seeds, publics, stream=stream)
        with _on(stream):
            self.privates[r] = prv[pick]
            self.dest_publics[r] = pub[pick]
            self.sig_seeds[r] = seeds
            self.sig_publics[r] = publics
            self.flags[r] = fl[pick]
            self.slots[r] = sl[pick]
            self.expected_hops[r] = hops[pick]
            self.rebalanced[r] = 0
            self.mtu[r] = 0
            self.row_state[r] = PENDING
        # the table holds max_pending ids and the host gives out no more rows than that, with distinct ids: the
        # insert cannot answer DUPLICATE or FULL, and reading its status back would wait for the stream
        self.table.insert([ids[k] for k in take], np.asarray(rows, dtype=np.int32), stream=stream)
        return status

    def remove(self, link_ids, stream=None):
        """Remove links (the watchdog's timeout, or after an ACTIVE state was
        read back) and free their rows; the rows' private bytes are cleared.
        Returns the (n,) int32 numpy status: device.LINK_OK or LINK_MISSING."""
        ids = [bytes(i) for i in link_ids]
        status = np.full(len(ids), 3, dtype=np.int32)
        rows, gone = [], []
        for k, i in enumerate(ids):
            row = self._row.pop(i, None)
            if row is not None:
                status[k] = 0
                rows.append(row)
                gone.append(i)
        if not rows:
            return status
        self.table.remove(gone, stream=stream)
        with _on(stream):
            r = torch.as_tensor(rows, dtype=torch.int64).to(self.device)
            self.privates[r] = 0
            self.sig_seeds[r] = 0
            self.row_state[r] = CLOSED
        self._free.extend(rows)
        return status

    def _read(self, t, link_ids):
        rows = [self._row[bytes(i)] for i in link_ids]
        return t.cpu().numpy()[rows] if rows else np.zeros(0, dtype=t.cpu().numpy().dtype)

    def state(self, link_ids):
        """(n,) uint8 numpy: the links' states (waits for the queued work)."""
        return self._read(self.row_state, link_ids)

    def hops(self, link_ids):
        """(expected_hops, rebalanced, mtu) of the links as numpy arrays (waits
        for the queued work)."""
        return (self._read(self.expected_hops, link_ids), self._read(self.rebalanced, link_ids),
                self._read(self.mtu, link_ids))


def _unpack_raws(raws, dev):
    off = np.zeros(len(raws), dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])[:-1]
    pkt = torch.from_numpy(np.frombuffer(b"".join(raws) + b"\0", dtype=np.uint8).copy()).to(dev)
    pkt_off = torch.from_numpy(off).to(dev)
    pkt_len = torch.tensor([len(r) for r in raws], dtype=torch.int32, device=dev)
    fields = torch.empty((len(raws), 96), dtype=torch.uint8, device=dev)
    _dev.packet_unpack(pkt, pkt_off, pkt_len, fields)
    return pkt, pkt_off, fields


def establish_batch(raws, ks, links, pending, signers=None, seen=None):
    """The link request proof stage for callers without torch tensors:
    ``raws`` is a sequence of raw packets as the interface handed them on.
    Unpacks them and runs device.link_establish against ``ks``, ``links``
    (:class:`LinkTable`), ``pending`` (:class:`PendingLinks`) and optional
    ``signers`` and ``seen``.  Returns one dict per packet: ``status``
    (LRPROOF_*), ``slot`` (or -1) and ``mtu`` (of an activated link, else None)."""
    dev = links.device
    raws = [bytes(r) for r in raws]
    n = len(raws)
    if n == 0:
        return []
    pkt, pkt_off, fields = _unpack_raws(raws, dev)
    status, slot, mtu = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    _dev.link_establish(ks, links, pending, pkt, pkt_off, fields, status, slot, mtu, signers=signers, seen=seen)
    status, slot, mtu = (t.cpu().numpy() for t in (status, slot, mtu))
    return [{"status": int(status[i]), "slot": int(slot[i]),
             "mtu": int(mtu[i]) if status[i] == LRPROOF_ACTIVATED else None} for i in range(n)]


def pack_link_request(destination_hash, pub, sig_pub, mtu=MTU):
    """The raw LINKREQUEST packet (Link.py:304-316, Packet.pack): flags 0x02
    (HEADER_1, broadcast, SINGLE, LINKREQUEST), hops 0, the destination hash,
    context 0, then the two public keys and, unless ``mtu`` is None, the three
    signalling bytes."""
    destination_hash, pub, sig_pub = bytes(destination_hash), bytes(pub), bytes(sig_pub)
    if len(destination_hash) != LINK_ID_LEN or len(pub) != 32 or len(sig_pub) != 32:
        raise ValueError("a 16-byte destination hash and two 32-byte public keys")
    return b"\x02\x00" + destination_hash + b"\x00" + pub + sig_pub + (b"" if mtu is None else signalling_bytes(mtu))


def open_requests_batch(destination_hashes, dest_sig_publics, ephemeral_privates, sig_seeds, slots, expected_hops,
                        mtu=MTU, flags=None, pending=None, device=None):
    """The initiator's other end: the LINKREQUEST packets that open links to
    ``destination_hashes`` (16 bytes each), from ``ephemeral_privates`` and
    ``sig_seeds`` (32 bytes of fresh randomness each, as
    X25519PrivateKey.generate and Ed25519PrivateKey.generate draw them).  The
    public keys come from device.x25519 on the base point and
    device.ed25519_public; ``mtu`` is the next hop's HW_MTU to signal (None:
    no signalling bytes).  With ``pending`` the links are entered there, with
    ``dest_sig_publics`` (the destinations' Ed25519 public keys), ``slots``
    (distinct, as a free list gives them), ``expected_hops`` and ``flags``
    (signer flags, default 0); where ``pending`` cannot take them all, none is
    entered and ValueError is raised.  Returns (raws, link_ids)."""
    dev = pending.device if pending is not None else _torch_device(device)
    prv = _rows(ephemeral_privates, 32, dev, "ephemeral_privates")
    seeds = _rows(sig_seeds, 32, dev, "sig_seeds")
    hashes = [bytes(h) for h in destination_hashes]
    n = len(hashes)
    if prv.shape[0] != n or seeds.shape[0] != n:
        raise ValueError("one ephemeral private key and one seed per destination")
    if n == 0:
        return [], []
    pubs, sig_pubs = torch.empty_like(prv), torch.empty_like(seeds)
    _dev.x25519(prv, None, pubs)
    _dev.ed25519_public(seeds, sig_pubs)
    pubs, sig_pubs = pubs.cpu().numpy(), sig_pubs.cpu().numpy()
    raws = [pack_link_request(hashes[i], pubs[i].tobytes(), sig_pubs[i].tobytes(), mtu) for i in range(n)]
    ids = [link_id_from_lr_packet(r) for r in raws]
    if pending is not None:
        st = pending.add(ids, prv, dest_sig_publics, seeds, [0] * n if flags is None else flags, slots, expected_hops)
        if st.any():
            # nothing half-registered: a request that is sent must have its row, or its proof reads NO_LINK
            pending.remove([i for i, s in zip(ids, st) if s == 0])
            raise ValueError("pending has no room for %d of the links, and %d of their ids are pending already"
                             % (int((st == 2).sum()), int((st == 1).sum())))
    return raws, ids
