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

Keeping ``KeySet`` and ``LinkTable`` in step is the caller's part: value v of
the table means key v of the key set the batch is decrypted with
(INTEGRATION.md §6).
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
