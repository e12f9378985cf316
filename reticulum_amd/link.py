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
