"""reticulum_amd — MI355X-native engine for Reticulum's encrypted-token path.

Drop-in for ``RNS.Cryptography.Token`` (AES-256/128-CBC + PKCS7 +
HMAC-SHA256), computed by hand-written gfx950 HIP kernels in librnstok.so.

    from reticulum_amd import Token
    t = Token(Token.generate_key())
    assert t.decrypt(t.encrypt(b"hello")) == b"hello"

Batch use: ``KeySet.encrypt_batch`` / ``decrypt_batch`` over host buffers,
``reticulum_amd.device`` over device-resident (torch) buffers, and
``reticulum_amd.shard`` for one-process-per-GPU sharding.  Key derivation:
``hkdf`` (drop-in for RNS.Cryptography.hkdf), ``hkdf_batch`` and
``derive_keyset`` (Identity's per-packet keys, derived and expanded on the
device).  X25519: ``exchange_batch`` / ``public_keys_batch`` / ``exchange`` /
``public_key`` (``reticulum_amd.x25519``, X25519.py:49-93); Identity.encrypt /
decrypt for a batch, from the exchange to the token: ``encrypt_batch`` /
``decrypt_batch`` (``reticulum_amd.identity``, Identity.py:803-904); their
device-tensor forms are ``device.x25519`` and ``device.derive_keyset_x25519``.
Ed25519 (``reticulum_amd.ed25519``: ``verify_batch`` / ``sign_batch`` /
``public_keys_batch`` and the single forms, as the reference's internal
provider decides); ``Identity.validate`` / ``sign`` / ``validate_announce``
for a batch: ``validate_batch`` / ``sign_batch`` / ``validate_announces_batch``;
device-tensor forms ``device.ed25519_verify`` / ``ed25519_sign`` / ``ed25519_public``.
Resource hashmaps: ``resource_hashmap`` / ``build_hashmap`` /
``get_map_hash`` (Resource.py:426-468, 505-506); integrity hash and proof:
``resource_hashes`` / ``verify_resource`` / ``validate_proof`` /
``prepare_resource`` (Resource.py:436-439, 698-699, 759-760, 787-790).  Wire-side neighbours
(HDLC framing, IFAC masking, packet header unpack/pack): ``reticulum_amd.wire``.
Links (``reticulum_amd.link``): ``LinkTable`` (link id -> key index on the
device; ``pipeline.inbound(..., links=table)`` finds each packet's link and
key, Transport.py:2161-2176, Link.py:941-1148), ``derive_link_keys`` (the
handshake keys of a batch of links, Link.py:348-361) and
``link_id_from_lr_packet`` (Link.py:336-342).
Replay protection (``reticulum_amd.filter``): ``PacketHashlist``, Transport's
packet hash list on the device; ``pipeline.inbound(..., seen=list)`` runs
Transport.packet_filter between unpack and dispatch (Transport.py:1377-1427,
1525-1545) and ``cull()`` is the job loop's step (Transport.py:656-658).
Announces: ``pipeline.inbound(..., announces=True)`` validates every announce
of a read inside its packet (Identity.validate_announce, Identity.py:505-606;
``device.announce_validate`` is the stage alone).
Packet proofs on links (``reticulum_amd.proof``): ``LinkSigners`` (the links'
signing rows) and ``ReceiptTable`` (Transport.receipts on the device);
``pipeline.inbound(..., links=table, signers=s, receipts=t)`` proves the packets
a link proves (Link.py:943-955, 1140-1145, 378-389) and settles the proofs that
come back (Transport.py:2326-2363, Packet.py:434-459); ``device.link_prove`` and
``device.proof_settle`` are the stages alone.
Packets for the node's own SINGLE destinations (``reticulum_amd.destination``):
``SingleDestinations`` (keys, ratchets and flags on the device);
``pipeline.inbound(..., links=table, deliver=destinations)`` opens them (ratchets
in order, then the identity's key) and proves them for PROVE_ALL destinations
(Transport.py:2188-2202, Identity.py:848-898, 942-953); ``device.destination_deliver``
is the stage alone and ``deliver_batch`` the form without tensors.
The proofs that come back for packets sent to SINGLE destinations
(``reticulum_amd.proof.DestinationReceipts``: the receipts with the recipient
identities' keys): ``pipeline.inbound(..., destination_receipts=t)`` settles
explicit and implicit proofs (Transport.py:2326-2363, Packet.py:480-524);
``device.destination_proof_settle`` is the stage alone and
``settle_destination_proofs_batch`` the form without tensors.
What a read has to send (``pipeline.reply``, or ``pipeline.inbound(...,
reply=True)``): the link request proofs, link proofs and destination proofs of
the read gathered in frame order, signed and masked for the interface and
HDLC-framed, as the byte stream for the socket the read came from
(Transport.py:1069-1104, 1199-1356); ``device.reply_gather`` and
``device.hdlc_frame_counted`` are the stages alone and ``reply_batch`` the form
without tensors.

``available()`` tells whether the library and a gfx950 device are usable;
``reticulum_amd.dropin`` is the import for the reference's one-line swap,
which raises ImportError when they are not.
"""
from ._native import NativeError, NativeUnavailable, LIB_PATH, available  # noqa: F401
from ._native import RT_ST_OK, RT_ST_TOO_SHORT, RT_ST_BAD_HMAC, RT_ST_BAD_CT_LEN, RT_ST_BAD_PAD  # noqa: F401
from .hkdf import derive_keyset, hkdf, hkdf_batch  # noqa: F401
from . import ed25519, identity, x25519  # noqa: F401
from .identity import decrypt_batch, encrypt_batch  # noqa: F401
from .identity import sign_batch, validate_announces_batch, validate_batch  # noqa: F401
from .x25519 import exchange, exchange_batch, public_key, public_keys_batch  # noqa: F401
from .resource import build_hashmap, get_map_hash, resource_hashmap  # noqa: F401
from .resource import prepare_resource, resource_hashes, validate_proof, verify_resource  # noqa: F401
from . import wire  # noqa: F401
from .wire import reply_batch  # noqa: F401
from . import link  # noqa: F401
from .link import LinkDestinations, LinkTable, accept_requests_batch, derive_link_keys, link_id_from_lr_packet  # noqa: F401
from .link import PendingLinks, establish_batch, open_requests_batch, pack_rtt  # noqa: F401
from . import destination  # noqa: F401
from .destination import SingleDestinations, deliver_batch, settle_destination_proofs_batch  # noqa: F401
from . import filter  # noqa: F401
from .filter import PacketHashlist  # noqa: F401
from . import proof  # noqa: F401
from .proof import DestinationReceipts, LinkSigners, ReceiptTable  # noqa: F401
from .token import AES, AES_128_CBC, AES_256_CBC, KeySet, Packed, Token, TOKEN_OVERHEAD, token_len  # noqa: F401

__version__ = "0.1.0"
