"""The node's own SINGLE destinations on the device: packets addressed to
them are opened and proved inside the read.

Transport.inbound hands a DATA packet whose destination hash is one of the
node's registered destinations to Destination.receive (Transport.py:2188-2202):
Identity.decrypt tries the destination's ratchets in order and then the
identity's own key on the token behind the packet's ephemeral X25519 key
(Identity.py:848-898, Destination.py:622-654), and a PROVE_ALL destination
answers with a PROOF packet signed by the identity (Packet.py:327-381,
Identity.py:942-953).  :class:`SingleDestinations` keeps what that needs in
device memory, ``pipeline.inbound(..., deliver=destinations)`` /
``device.destination_deliver`` run it over the frames of a read, and
:func:`deliver_batch` is the form for callers without tensors.
:func:`settle_destination_proofs_batch` is that form for the other end: the
proofs that come back for packets this node sent to SINGLE destinations
(reticulum_amd.proof.DestinationReceipts).
"""
import numpy as np

from . import _native
from .link import LINK_ID_LEN, LinkTable, _Lazy, _on, _rows, _torch_device, _unpack_raws

# what became of a record: RT_DELIVER_* (include/rnstok.h)
DELIVER_DELIVERED, DELIVER_NOT_DATA, DELIVER_NO_DESTINATION, DELIVER_TYPE_MISMATCH = 0, 1, 2, 3
DELIVER_SHORT, DELIVER_NOT_OPENED, DELIVER_DEFERRED = 4, 5, 6
# a destination's flags: RT_LINK_PROVE_ALL and RT_DEST_ENFORCE_RATCHETS
PROVE_ALL, ENFORCE_RATCHETS = 1, 8
PROOF_IMPLICIT_LEN, PROOF_EXPLICIT_LEN = 83, 115      # header (19) ‖ [packet hash (32)] ‖ signature (64)

torch = _Lazy("torch")
_dev = _Lazy(".device", __package__)


class SingleDestinations:
    """The node's SINGLE destinations for the delivery stage: a
    :class:`reticulum_amd.link.LinkTable` from 16-byte destination hash to row
    (distinct hashes, checked once at construction), and per row the identity's
    X25519 private key, its 16-byte hash (the HKDF salt of Identity.get_salt),
    its Ed25519 signing seed and public key (derived once,
    device.ed25519_public), a flags byte (PROVE_ALL, ENFORCE_RATCHETS; a
    PROVE_APP or PROVE_NONE destination has no proof flag) and its ratchet
    private keys, newest first as Destination.ratchets is ordered, as a CSR:
    ``ratchet_off`` (n + 1,) int32 and ``ratchets`` (capacity, 32) uint8.

    ``hashes`` (n, 16), ``privates`` (n, 32), ``identity_hashes`` (n, 16),
    ``seeds`` (n, 32) and ``flags`` (n,) may be device tensors, numpy arrays or
    sequences (of byte strings; flags: of ints); ``ratchets`` is a sequence of n
    lists of 32-byte strings (None: no destination has ratchets).  The object
    owns the stage's scratch, sized at construction: a key set of 64-byte keys
    with ``max_frames + retry_trials`` records (one per frame of a read for the
    first candidate, ``retry_trials`` for the remaining candidates of the
    frames the first did not open) and the work lists; a call takes at most
    ``max_frames`` frames.  ``ratchet_capacity`` (default: what ``ratchets``
    holds) is the number of ratchet keys :meth:`set_ratchets` can lay out
    without a new allocation.  Nothing of it leaves the device."""

    def __init__(self, hashes, privates, identity_hashes, seeds, flags, ratchets=None, max_frames=1024,
                 retry_trials=1024, ratchet_capacity=None, device=None):
        dev = _torch_device(device)
        self.device = dev
        self.hashes = _rows(hashes, LINK_ID_LEN, dev, "destination hashes")
        n = self.n = int(self.hashes.shape[0])
        if n < 1:
            raise ValueError("at least one destination")
        self.privates = _rows(privates, 32, dev, "privates")
        self.identity_hashes = _rows(identity_hashes, 16, dev, "identity hashes")
        self.seeds = _rows(seeds, 32, dev, "seeds")
        if self.privates.shape[0] != n or self.identity_hashes.shape[0] != n or self.seeds.shape[0] != n:
            raise ValueError("privates, identity_hashes and seeds must hold one row per destination")
        if isinstance(flags, torch.Tensor):
            fl = flags
        else:
            fl = np.asarray(flags)
            if fl.size and (fl.min() < 0 or (fl & ~(PROVE_ALL | ENFORCE_RATCHETS)).any()):
                raise ValueError("flags are PROVE_ALL | ENFORCE_RATCHETS")
            fl = torch.from_numpy(np.ascontiguousarray(fl, dtype=np.uint8))
        if fl.dtype != torch.uint8 or fl.numel() != n:
            raise ValueError(f"flags must be ({n},) uint8")
        self.flags = fl.to(dev).contiguous().view(n)
        self.max_frames, self.retry_trials = int(max_frames), int(retry_trials)
        if not 1 <= self.max_frames <= (1 << 30) - 2 or not 0 <= self.retry_trials <= (1 << 30) - 2:
            raise ValueError("max_frames is 1 .. 2**30 - 2 and retry_trials 0 .. 2**30 - 2")
        self.publics = torch.empty_like(self.seeds)
        _dev.ed25519_public(self.seeds, self.publics)
        lists = [[] for _ in range(n)] if ratchets is None else [list(r) for r in ratchets]
        if len(lists) != n:
            raise ValueError("ratchets must hold one list per destination")
        self._counts = np.zeros(n, dtype=np.int64)
        total = sum(len(r) for r in lists)
        self.ratchet_capacity = max(int(ratchet_capacity) if ratchet_capacity is not None else total, total, 1)
        self.ratchets = torch.zeros((self.ratchet_capacity, 32), dtype=torch.uint8, device=dev)
        self.ratchet_off = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        self.set_ratchets(range(n), lists)
        # the scratch: key records and work lists
        self.scratch = _dev.keyset(torch.zeros((self.max_frames + self.retry_trials, 64), dtype=torch.uint8, device=dev))
        lib = _native.load()
        self.work_bytes = int(lib.rt_destination_deliver_workspace_bytes(self.max_frames, self.retry_trials))
        self.work = torch.empty(self.work_bytes, dtype=torch.uint8, device=dev)
        self.table = LinkTable(n, device=dev)
        status = self.table.insert(self.hashes, torch.arange(n, dtype=torch.int32, device=dev))
        if bool((status != 0).any()):                   # once, at construction: reads the status back
            raise ValueError("destination hashes must be distinct: a repeated one could never reach its row")

    def set_ratchets(self, rows, lists, stream=None):
        """Replaces the ratchet lists of ``rows`` with ``lists`` (one list of
        32-byte private keys per row, newest first).  Enqueued on ``stream``
        (default: the current stream) without synchronising; the CSR is laid
        out again on the device, and ``ratchets`` / ``ratchet_off`` keep their
        memory as long as the total fits ``ratchet_capacity``.  How many
        ratchets a row has is kept on the host; the keys are not."""
        rows = [int(r) for r in rows]
        lists = [[bytes(k) for k in r] for r in lists]
        if len(rows) != len(lists) or len(set(rows)) != len(rows) or any(not 0 <= r < self.n for r in rows):
            raise ValueError("rows are distinct destination rows, with one list each")
        if any(len(k) != 32 for r in lists for k in r):
            raise ValueError("ratchet private keys are 32 bytes each")
        old_off = np.zeros(self.n + 1, dtype=np.int64)
        old_off[1:] = np.cumsum(self._counts)
        counts = self._counts.copy()
        for r, keys in zip(rows, lists):
            counts[r] = len(keys)
        new_off = np.zeros(self.n + 1, dtype=np.int64)
        new_off[1:] = np.cumsum(counts)
        total, old_total = int(new_off[-1]), int(old_off[-1])
        # where each new row of the CSR comes from: an old row, or a row of the upload behind the old ones
        src = np.empty(total, dtype=np.int64)
        new_keys, at = [], old_total
        given = dict(zip(rows, lists))
        for d in range(self.n):
            lo, hi = int(new_off[d]), int(new_off[d + 1])
            if d in given:
                src[lo:hi] = np.arange(at, at + hi - lo)
                new_keys.extend(given[d])
                at += hi - lo
            else:
                src[lo:hi] = np.arange(int(old_off[d]), int(old_off[d + 1]))
        dev = self.device
        with _on(stream):
            if total:
                up = torch.from_numpy(np.frombuffer(b"".join(new_keys), dtype=np.uint8).copy()).view(-1, 32).to(dev) \
                    if new_keys else torch.empty((0, 32), dtype=torch.uint8, device=dev)
                laid = torch.cat([self.ratchets[:old_total], up])[torch.from_numpy(src).to(dev)]
                if total > self.ratchet_capacity:
                    self.ratchet_capacity = total
                    self.ratchets = torch.zeros((total, 32), dtype=torch.uint8, device=dev)
                self.ratchets[:total].copy_(laid)
            if total < old_total:
                self.ratchets[total:old_total].zero_()  # keys that left the lists
            self.ratchet_off.copy_(torch.from_numpy(new_off.astype(np.int32)).to(dev))
        self._counts = counts

    def ratchet_counts(self):
        """How many ratchets each destination has (host bookkeeping)."""
        return self._counts.copy()


def deliver_batch(raws, destinations, implicit_proof=True):
    """The delivery stage for callers without torch tensors: ``raws`` is a
    sequence of raw packets (byte strings, as the interface handed them on, at
    most ``destinations.max_frames``).  Unpacks them and runs
    device.destination_deliver against ``destinations``
    (:class:`SingleDestinations`).  Returns ``(plaintexts, status, destination,
    ratchet, proofs)``: per packet the plaintext (bytes) of a DELIVERED packet
    or None; the (n,) int32 numpy arrays DELIVER_*, the destination's row or -1
    and the rank of the ratchet that opened the packet (-1: the identity's key,
    or nothing); and the PROOF packet to send (bytes) or None."""
    dev = destinations.device
    raws = [bytes(r) for r in raws]
    n = len(raws)
    if n == 0:
        z = np.zeros(0, dtype=np.int32)
        return [], z, z.copy(), z.copy(), []
    pkt, pkt_off, fields = _unpack_raws(raws, dev)
    pt = torch.zeros_like(pkt)
    pt_off = torch.zeros(n, dtype=torch.int64, device=dev)
    pt_len, status, dstatus, dest, ratchet, plen = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(6))
    proofs = torch.zeros((n, 128), dtype=torch.uint8, device=dev)
    _dev.destination_deliver(destinations, pkt, pkt_off, fields, pt, pt_off, pt_len, status, dstatus, dest, ratchet,
                             proofs, plen, implicit_proof=implicit_proof)
    pt, pt_off, pt_len, dstatus, dest, ratchet, plen, proofs = (
        t.cpu().numpy() for t in (pt, pt_off, pt_len, dstatus, dest, ratchet, plen, proofs))
    plain = [pt[pt_off[i]:pt_off[i] + pt_len[i]].tobytes() if dstatus[i] == DELIVER_DELIVERED else None
             for i in range(n)]
    out_proofs = [proofs[i, :plen[i]].tobytes() if plen[i] else None for i in range(n)]
    return plain, dstatus, dest, ratchet, out_proofs


def settle_destination_proofs_batch(raws, receipts):
    """The proofs for packets sent to SINGLE destinations, for callers without
    torch tensors: ``raws`` is a sequence of raw packets (byte strings, as the
    interface handed them on) and ``receipts`` a
    :class:`reticulum_amd.proof.DestinationReceipts`.  Unpacks them and runs
    device.destination_proof_settle with no link active.  Returns ``(status,
    receipt)``, (n,) int32 numpy arrays: device.DPROOF_* and the delivered
    receipt's id (which has left the table) or -1."""
    dev = receipts.device
    raws = [bytes(r) for r in raws]
    n = len(raws)
    if n == 0:
        z = np.zeros(0, dtype=np.int32)
        return z, z.copy()
    pkt, pkt_off, fields = _unpack_raws(raws, dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    receipt = torch.zeros(n, dtype=torch.int32, device=dev)
    _dev.destination_proof_settle(pkt, pkt_off, fields, receipts, status, receipt)
    return status.cpu().numpy(), receipt.cpu().numpy()
