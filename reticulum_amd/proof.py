"""Packet proofs on links, on the device: proving what a link received and
settling the proofs that come back.

A link whose destination proves all packets answers every DATA packet it could
decrypt with ``packet_hash ‖ sign(packet_hash)`` (Link.receive, Link.py:943-955;
Link.prove_packet, Link.py:378-389), a link with a channel every CHANNEL packet
(Link.py:1140-1145); and every proof that comes back is matched against the
outstanding receipts and verified under the key of the link it arrived on
(Transport.py:2326-2363; PacketReceipt.validate_link_proof, Packet.py:434-459).
:class:`LinkSigners` keeps the links' signing rows and :class:`ReceiptTable` the
receipts in device memory; ``pipeline.inbound(..., links=table, signers=s,
receipts=t)`` runs both inside the read, and ``device.link_prove`` /
``device.proof_settle`` are the stages alone.

The proofs for packets sent to SINGLE destinations come back on no link and are
verified under the key of the identity the packet went to
(PacketReceipt.validate_proof, Packet.py:480-524): :class:`DestinationReceipts`
keeps those receipts with their keys, ``pipeline.inbound(...,
destination_receipts=t)`` settles them inside the read and
``device.destination_proof_settle`` is the stage alone.

Row l of the signers belongs to the link whose :class:`LinkTable` value is l,
which is also the index of its key in the :class:`KeySet`; keeping the three in
step is the caller's part.
"""
import numpy as np

from . import _native
from .link import LinkTable, _Lazy, _on, _rows, _torch_device

PROVE_ALL, HAS_CHANNEL = 1, 2           # RT_LINK_PROVE_ALL, RT_LINK_HAS_CHANNEL (include/rnstok.h)
HASH_LEN = 32                           # Identity.HASHLENGTH // 8: a receipt is held by the full packet hash
MAX_RECEIPTS = 1024                     # Transport.MAX_RECEIPTS

torch = _Lazy("torch")
_dev = _Lazy(".device", __package__)


class LinkSigners:
    """Per-link signing rows on the device, indexed by the link table's value.

    ``seeds``: the links' ``sig_prv`` seeds, (n_links, 32), or one row for all
    (responder links of one destination sign with their owner's key);
    ``peer_publics``: the links' ``peer_sig_pub``, (n_links, 32); ``flags``:
    (n_links,) of PROVE_ALL | HAS_CHANNEL (a link whose destination proves by
    callback, PROVE_APP, gets neither).  Each may be a device tensor, a numpy
    array or a sequence of byte strings (flags: of ints).  ``publics`` is
    derived once from the seeds (device.ed25519_public).  Nothing of it leaves
    the device."""

    def __init__(self, seeds, peer_publics, flags, device=None):
        dev = _torch_device(device)
        self.device = dev
        self.peer_publics = _rows(peer_publics, 32, dev, "peer_publics")
        self.n_links = int(self.peer_publics.shape[0])
        if self.n_links < 1:
            raise ValueError("at least one link")
        self.seeds = _rows(seeds, 32, dev, "seeds")
        if self.seeds.shape[0] not in (1, self.n_links):
            raise ValueError("seeds must hold one row per link, or one row for all")
        if isinstance(flags, torch.Tensor):
            fl = flags
        else:
            fl = np.asarray(flags)
            if fl.size and (fl.min() < 0 or fl.max() > PROVE_ALL | HAS_CHANNEL):
                raise ValueError("flags are PROVE_ALL | HAS_CHANNEL")
            fl = torch.from_numpy(np.ascontiguousarray(fl, dtype=np.uint8))
        if fl.dtype != torch.uint8 or fl.numel() != self.n_links:
            raise ValueError(f"flags must be ({self.n_links},) uint8")
        self.flags = fl.to(dev).contiguous().view(self.n_links)
        self.publics = torch.empty_like(self.seeds)
        _dev.ed25519_public(self.seeds, self.publics)


class ReceiptTable:
    """Transport.receipts on the device: packet hash -> receipt id, for at most
    ``max_receipts`` outstanding receipts (the reference caps its list at
    MAX_RECEIPTS = 1024).  A :class:`LinkTable` over the truncated hash,
    hash[:16], whose value is the id, beside ``hashes`` (max_receipts x 32),
    the full hash by id: a proof is matched on all 32 bytes, as the reference
    compares them.  The caller chooses the ids, 0 .. max_receipts - 1, and
    keeps what belongs to a receipt (callbacks, timeouts) under them; timeouts
    and culling (Transport.py:569-587) go through :meth:`remove`.

    ``add`` and ``remove`` take (n, 32) hashes (device tensor, numpy array or a
    sequence of 32-byte strings), enqueue on ``stream`` and return device
    tensors without synchronising; ``len()`` reads the count back."""

    def __init__(self, max_receipts=MAX_RECEIPTS, device=None):
        self.table = LinkTable(max_receipts, device=device)
        self.device = self.table.device
        self.max_receipts = self.table.max_links
        self.hashes = torch.zeros((self.max_receipts, HASH_LEN), dtype=torch.uint8, device=self.device)

    @property
    def handle(self):
        return self.table.handle

    def add(self, hashes, ids, stream=None):
        """Enter hashes[i] -> ids[i].  Returns the (n,) int32 status, as
        LinkTable.insert: LINK_OK, LINK_DUPLICATE (a receipt with the same
        first 16 bytes is present, or comes earlier in this batch: the earlier
        one and its hash stay untouched) or LINK_FULL."""
        hashes = _rows(hashes, HASH_LEN, self.device, "packet hashes")
        n = hashes.shape[0]
        if not isinstance(ids, torch.Tensor):
            v = np.asarray(ids)
            if v.size and (v.min() < 0 or v.max() >= self.max_receipts):
                raise ValueError(f"receipt ids must be 0 .. {self.max_receipts - 1}")
        ids = self.table._values(ids, n)
        _dev._order_after_current(stream, hashes, ids)
        with _on(stream):
            short = hashes[:, :16].contiguous()
        status = self.table.insert(short, ids, stream=stream)
        _dev.receipt_store(self, hashes, ids, status, stream=stream)
        return status

    def remove(self, hashes, stream=None):
        """Remove the receipts of hashes[i].  Returns the (n,) int32 status:
        LINK_OK or LINK_MISSING."""
        hashes = _rows(hashes, HASH_LEN, self.device, "packet hashes")
        _dev._order_after_current(stream, hashes)
        with _on(stream):
            short = hashes[:, :16].contiguous()
        return self.table.remove(short, stream=stream)

    def __len__(self):
        """Receipts present (waits for the table's queued work)."""
        return len(self.table)


class DestinationReceipts:
    """The receipts of packets sent to SINGLE destinations, with the key each
    proof is verified under: a :class:`ReceiptTable`'s table and ``hashes``,
    and beside them ``keys`` (max_receipts x 32), the Ed25519 public key of the
    destination's identity (``Identity.get_public_key()[32:64]``), and ``keyed``
    (max_receipts bytes), 0 for a receipt without an identity (one sent on a
    link), which no proof of this kind delivers.  The caller chooses the ids,
    0 .. max_receipts - 1; timeouts and culling go through :meth:`remove`.

    ``scan_trials`` (default 4 x max_receipts) bounds what implicit proofs that
    are not addressed to the receipt they prove can cost in one call: each is
    tried against every live keyed receipt, a frame of that many
    verifications, and only whole frames inside the budget are run
    (device.destination_proof_settle).  The object owns the stage's work lists,
    which grow with the largest read it has served.  Nothing of it leaves the
    device."""

    def __init__(self, max_receipts=MAX_RECEIPTS, scan_trials=None, device=None):
        self.table = LinkTable(max_receipts, device=device)
        self.device = self.table.device
        self.max_receipts = self.table.max_links
        self.scan_trials = 4 * self.max_receipts if scan_trials is None else int(scan_trials)
        if not 0 <= self.scan_trials <= (1 << 30) - 2:
            raise ValueError("scan_trials is 0 .. 2**30 - 2")
        z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=self.device)     # noqa: E731
        self.hashes, self.keys, self.keyed = z(self.max_receipts, HASH_LEN), z(self.max_receipts, 32), z(self.max_receipts)
        self.work = None

    @property
    def handle(self):
        return self.table.handle

    def work_bytes(self, n):
        """The bytes of work lists a call of ``n`` records needs."""
        return int(_native.load().rt_destination_proof_workspace_bytes(int(n), self.max_receipts))

    def work_for(self, n, stream=None):
        """The work lists for a call of ``n`` records on ``stream``: the
        object's own where they are large enough, else new and larger ones."""
        need = self.work_bytes(n)
        if self.work is None or self.work.numel() < need:
            with _on(stream):
                self.work = torch.empty(max(need, 2 * (0 if self.work is None else self.work.numel())),
                                        dtype=torch.uint8, device=self.device)
        if stream is not None:
            self.work.record_stream(stream)
        return self.work

    def add(self, hashes, ids, keys=None, stream=None):
        """Enter hashes[i] -> ids[i] with keys[i] ((n, 32): the destination
        identity's signing key; None: receipts without an identity, keyed 0).
        Returns the (n,) int32 status, as ReceiptTable.add: a duplicate leaves
        the earlier entry, its hash and its key untouched."""
        hashes = _rows(hashes, HASH_LEN, self.device, "packet hashes")
        n = hashes.shape[0]
        if keys is not None:
            keys = _rows(keys, 32, self.device, "keys")
            if keys.shape[0] != n:
                raise ValueError("keys must hold one 32-byte row per hash")
        if not isinstance(ids, torch.Tensor):
            v = np.asarray(ids)
            if v.size and (v.min() < 0 or v.max() >= self.max_receipts):
                raise ValueError(f"receipt ids must be 0 .. {self.max_receipts - 1}")
        ids = self.table._values(ids, n)
        _dev._order_after_current(stream, hashes, ids, keys)
        with _on(stream):
            short = hashes[:, :16].contiguous()
        status = self.table.insert(short, ids, stream=stream)
        _dev.receipt_store_keyed(self, hashes, keys, ids, status, stream=stream)
        return status

    remove = ReceiptTable.remove
    __len__ = ReceiptTable.__len__


__all__ = ["LinkSigners", "ReceiptTable", "DestinationReceipts", "PROVE_ALL", "HAS_CHANNEL", "MAX_RECEIPTS"]
