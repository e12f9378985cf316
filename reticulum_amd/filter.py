"""Replay protection on the device: Transport's packet hash list.

Transport.inbound hands a packet on only when Transport.packet_filter lets it
pass (Transport.py:1377-1427): a packet for another transport node, a PLAIN or
GROUP packet from further than one hop and a packet whose hash is in
``packet_hashlist`` or ``packet_hashlist_prev`` are dropped, and a packet that
passes is remembered (Transport.py:1525-1545).  :class:`PacketHashlist` keeps
the two sets in device memory, ``pipeline.inbound(..., seen=list,
transport_identity=...)`` runs the filter between unpack and dispatch, and
:meth:`PacketHashlist.cull` is the job loop's step (Transport.py:656-658).

What stays with the caller is listed in INTEGRATION.md §7: calling ``cull``,
saving and reloading the list, the hashes whose remembering the reference
defers, and the removal of a link packet's hash that came in on the wrong
interface (Transport.py:2186-2187).
"""
from . import _native
from .link import _Lazy, _on, _rows, _torch_device

torch = _Lazy("torch")
_dev = _Lazy(".device", __package__)

HASH_LEN = 32                     # a full packet hash, Packet.get_hash (Packet.py:342-353)
HASHLIST_MAXSIZE = 1000000        # Transport.hashlist_maxsize (Transport.py:107)


class PacketHashlist:
    """Two generations, current and previous, of a set of 32-byte packet
    hashes in device memory; each holds at most ``max_hashes`` entries.

    ``add``, ``remove`` and ``contains`` take a batch of hashes ((n, 32) uint8
    device tensor, numpy array, or a sequence of 32-byte strings), enqueue on
    ``stream`` (default: the current stream of the list's GPU) and return
    device tensors without synchronising; ``counts()`` reads the counts back."""

    def __init__(self, max_hashes=HASHLIST_MAXSIZE, device=None):
        max_hashes = int(max_hashes)
        if not 1 <= max_hashes <= 1 << 29:
            raise ValueError("max_hashes must be 1 .. 2**29")
        self.device = _torch_device(device)
        self.max_hashes = max_hashes
        self._lib = _native.load()
        self._ptr = self._lib.rt_hashlist_create(_native.context(self.device.index), max_hashes)
        if not self._ptr:
            raise _native.NativeError(-1, _native.last_error())
        self.capacity = int(self._lib.rt_hashlist_capacity(self._ptr))

    @property
    def handle(self):
        return self._ptr

    def __del__(self):
        p = getattr(self, "_ptr", None)
        if p:
            try:
                self._lib.rt_hashlist_destroy(p)
            except Exception:
                pass
            self._ptr = None

    def filter(self, fields, transport_identity, transit=None, stream=None):
        """Transport.packet_filter and the remember step over packet_unpack's
        records ``fields`` ((n, 96) uint8 on the device), in index order.
        Returns the (n,) int32 status (device.FILTER_*); a dropped packet's
        ``ok`` is cleared in ``fields``.  ``transit`` is a LinkTable standing
        for Transport.link_table, or None."""
        tid = _rows([transport_identity], 16, self.device, "transport_identity") \
            if isinstance(transport_identity, (bytes, bytearray)) else transport_identity
        with _on(stream):
            status = torch.empty(fields.shape[0], dtype=torch.int32, device=self.device)
        _dev._order_after_current(stream, fields, tid)
        _dev.packet_filter(self._ptr, fields, tid, status, transit=transit.handle if transit is not None else None,
                           stream=stream)
        return status

    def cull(self, stream=None):
        """The job loop's step: when the current generation holds more than
        ``max_hashes // 2`` entries it becomes the previous one and the
        current one becomes empty.  Decided on the device; nothing is read back."""
        _dev.hashlist_cull(self._ptr, self.device, stream=stream)

    def add(self, hashes, stream=None):
        """Enter hashes into the current generation (Transport.add_packet_hash)."""
        hashes = _rows(hashes, HASH_LEN, self.device, "packet hashes")
        _dev._order_after_current(stream, hashes)
        _dev.hashlist_add(self._ptr, hashes, stream=stream)

    def remove(self, hashes, stream=None):
        """Remove hashes from the current generation.  Returns the (n,) int32
        status: device.LINK_OK or LINK_MISSING."""
        hashes = _rows(hashes, HASH_LEN, self.device, "packet hashes")
        with _on(stream):
            status = torch.empty(hashes.shape[0], dtype=torch.int32, device=self.device)
        _dev._order_after_current(stream, hashes)
        _dev.hashlist_remove(self._ptr, hashes, status, stream=stream)
        return status

    def contains(self, hashes, stream=None):
        """(n,) uint8: 0 absent, 1 in the current generation, 2 in the
        previous one only."""
        hashes = _rows(hashes, HASH_LEN, self.device, "packet hashes")
        with _on(stream):
            found = torch.empty(hashes.shape[0], dtype=torch.uint8, device=self.device)
        _dev._order_after_current(stream, hashes)
        _dev.hashlist_contains(self._ptr, hashes, found, stream=stream)
        return found

    def counts(self):
        """(current, previous, overflow): entries in each generation and the
        packets that passed without being remembered because the current
        generation was full (waits for the list's queued work)."""
        out = torch.empty(3, dtype=torch.int32, device=self.device)
        _dev.hashlist_counts(self._ptr, out)
        return tuple(int(x) for x in out.cpu().tolist())

    def __len__(self):
        """Entries in the current generation (waits for the list's queued work)."""
        return self.counts()[0]
