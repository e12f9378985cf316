"""Resource hashmap on the GPU (RNS/Resource.py:426-468, 505-506).

A Resource's encrypted stream is cut into SDU-sized parts; each part is
advertised by ``SHA-256(part || random_hash)[:4]`` and the sender draws a new
random_hash while any map hash repeats one of the previous
COLLISION_GUARD_SIZE map hashes.  ``build_hashmap`` is that loop with the
map hashes and the collision scan computed by librnstok's k_map_hashes /
k_map_collisions; ``get_map_hash`` is the single-part form used by the
receiver (receive_part, Resource.py:865-866).  The integrity hash and proof
(Resource.py:436-439, 698-699, 759-760) are ``resource_hashes`` (sender),
``verify_resource`` (receiver) and ``prepare_resource`` (the sender's loop
with both); ``validate_proof`` is the sender's check of the answer.  No CPU
fallback.
"""
import ctypes
import os

import numpy as np

from . import _native

SDU = 464                    # Resource.SDU = Packet.MDU for the default MTU
MAPHASH_LEN = 4              # Resource.MAPHASH_LEN
RANDOM_HASH_SIZE = 4         # Resource.RANDOM_HASH_SIZE
COLLISION_GUARD_SIZE = 224   # ResourceAdvertisement.COLLISION_GUARD_SIZE = 2*WINDOW_MAX + HASHMAP_MAX_LEN
_NONE = 0xFFFFFFFF


def _bytes(x, what):
    if not isinstance(x, (bytes, bytearray, memoryview)):
        raise TypeError(f"{what} must be bytes")
    return bytes(x)


def resource_hashmap(stream, random_hash, sdu=SDU, guard=COLLISION_GUARD_SIZE, device=None):
    """Map hashes of every part of ``stream`` and the index of the first part
    whose map hash repeats one of the previous ``guard`` ones (None if the
    hashmap would be accepted).  Returns (hashmap_bytes, first_collision)."""
    stream = _bytes(stream, "stream")
    random_hash = _bytes(random_hash, "random_hash")
    if sdu < 1:
        raise ValueError("sdu must be positive")
    parts = -(-len(stream) // sdu)
    if parts == 0:
        return b"", None
    lib = _native.load()
    ctx = _native.context(device)
    data = np.frombuffer(stream, np.uint8)
    rh = np.frombuffer(random_hash, np.uint8) if random_hash else None
    out = np.zeros(4 * parts, np.uint8)
    col = ctypes.c_uint32(_NONE)
    _native.check(lib.rt_resource_hashmap_host(ctx, data.ctypes.data_as(ctypes.c_void_p), len(stream), sdu,
                                               None if rh is None else rh.ctypes.data_as(ctypes.c_void_p),
                                               len(random_hash), guard, out.ctypes.data_as(ctypes.c_void_p),
                                               ctypes.byref(col)))
    return out.tobytes(), (None if col.value == _NONE else int(col.value))


def build_hashmap(stream, sdu=SDU, guard=COLLISION_GUARD_SIZE, random_hash=None, device=None, max_rounds=64):
    """The sender's loop (Resource.py:431-468): draw random_hash
    (Identity.get_random_hash()[:4], i.e. os.urandom-backed) until no map hash
    collides inside the guard window.  Returns (random_hash, hashmap).
    ``random_hash`` may be a callable returning the next candidate (tests)."""
    draw = random_hash if callable(random_hash) else (lambda: os.urandom(RANDOM_HASH_SIZE))
    for _ in range(max_rounds):
        rh = draw()
        hashmap, col = resource_hashmap(stream, rh, sdu, guard, device)
        if col is None:
            return rh, hashmap
    raise RuntimeError("resource hashmap kept colliding (repeated parts inside the guard window)")


def get_map_hash(data, random_hash, device=None):
    """Resource.get_map_hash (Resource.py:505-506) for one part:
    SHA-256(data || random_hash)[:4]."""
    data = _bytes(data, "data")
    random_hash = _bytes(random_hash, "random_hash")
    if data:
        return resource_hashmap(data, random_hash, sdu=len(data), guard=0, device=device)[0]
    if random_hash:      # SHA-256(b"" || rh) is the one-part hash of rh with an empty salt
        return resource_hashmap(random_hash, b"", sdu=len(random_hash), guard=0, device=device)[0]
    raise ValueError("get_map_hash of an empty part with an empty random_hash")


# ------------------------------------------------ integrity hash and proof --
# Resource.py:436-439 (sender), :698-699 and :759-760 (receiver), :787-790
# (the sender's check of the proof), computed by librnstok's
# k_resource_hashes / k_resource_hashes_split in one pass over the data.

HASH_LEN = 32                # Identity.HASHLENGTH // 8
TRUNCATED_HASH_LEN = 16      # Identity.TRUNCATED_HASHLENGTH // 8


def _hashes(data, random_hash, expect, device):
    lib = _native.load()
    ctx = _native.context(device)
    vp = ctypes.c_void_p
    d = np.frombuffer(data, np.uint8) if data else None
    rh = np.frombuffer(random_hash, np.uint8) if random_hash else None
    ex = np.frombuffer(expect, np.uint8) if expect is not None else None
    out = np.zeros(2 * HASH_LEN, np.uint8)
    st = ctypes.c_int32(0)
    _native.check(lib.rt_resource_hashes_host(
        ctx, None if d is None else d.ctypes.data_as(vp), len(data), None if rh is None else rh.ctypes.data_as(vp),
        len(random_hash), None if ex is None else ex.ctypes.data_as(vp), out.ctypes.data_as(vp),
        out[HASH_LEN:].ctypes.data_as(vp), ctypes.byref(st)))
    return out[:HASH_LEN].tobytes(), out[HASH_LEN:].tobytes(), st.value


def _rh(random_hash):
    random_hash = _bytes(random_hash, "random_hash")
    if len(random_hash) > HASH_LEN:
        raise ValueError("random_hash is at most 32 bytes")
    return random_hash


def resource_hashes(data, random_hash, device=None):
    """The sender's hashes (Resource.py:437-439) of ``data`` (metadata ||
    resource data, :330): hash = SHA-256(data || random_hash), truncated_hash
    = hash[:16], expected_proof = SHA-256(data || hash).  Returns (hash,
    truncated_hash, expected_proof)."""
    data = _bytes(data, "data")
    h, proof, _ = _hashes(data, _rh(random_hash), None, device)
    return h, h[:TRUNCATED_HASH_LEN], proof


def verify_resource(data, random_hash, expected_hash, device=None):
    """The receiver's check and answer (Resource.py:698-699, 759-760) for an
    assembled (decrypted, random-hash stripped, decompressed) segment:
    recompute SHA-256(data || random_hash); if it equals the advertised
    ``expected_hash`` return the proof packet's data hash || SHA-256(data ||
    hash), else None (Resource.CORRUPT: nothing is proved)."""
    data = _bytes(data, "data")
    random_hash = _rh(random_hash)
    expected_hash = _bytes(expected_hash, "expected_hash")
    if len(expected_hash) != HASH_LEN:
        return None                       # no 32-byte digest equals it
    _, proof, status = _hashes(data, random_hash, expected_hash, device)
    return None if status else expected_hash + proof


def validate_proof(proof_data, expected_proof):
    """Resource.validate_proof's test (Resource.py:789-790): the proof packet
    is hash || proof, 64 bytes, and its second half equals expected_proof.
    Host only."""
    proof_data = _bytes(proof_data, "proof_data")
    expected_proof = _bytes(expected_proof, "expected_proof")
    return len(proof_data) == 2 * HASH_LEN and proof_data[HASH_LEN:] == expected_proof


def prepare_resource(data, stream, sdu=SDU, guard=COLLISION_GUARD_SIZE, random_hash=None, device=None, max_rounds=64,
                     rehash_segment=False):
    """The sender's whole loop (Resource.py:431-468): draw random_hash, hash
    ``data`` (the plaintext segment, metadata || resource data) for the
    integrity hash and the expected proof, build the hashmap of ``stream``
    (the encrypted data the parts are cut from), and start over with a new
    draw while a map hash collides inside the guard window.  Returns
    (random_hash, hash, expected_proof, hashmap).  ``random_hash`` may be a
    callable returning the next candidate, as for ``build_hashmap``.

    Parity with a reference quirk: the reference's loop rebinds the name
    ``data`` to each part it cuts (:450), so after a collision the retry at
    :437-439 hashes the colliding *encrypted part*, not the segment.  This
    function does the same by default, because the project's contract is
    parity; the hash and proof the reference (and this function) produce after
    a retry cannot be verified by any receiver, which hashes the segment.
    ``rehash_segment=True`` hashes the real segment on every round instead."""
    data = _bytes(data, "data")
    stream = _bytes(stream, "stream")
    if sdu < 1:
        raise ValueError("sdu must be positive")
    draw = random_hash if callable(random_hash) else (lambda: os.urandom(RANDOM_HASH_SIZE))
    hashed = data
    for _ in range(max_rounds):
        rh = draw()
        h, _, proof = resource_hashes(hashed, rh, device)
        hashmap, col = resource_hashmap(stream, rh, sdu, guard, device)
        if col is None:
            return rh, h, proof, hashmap
        if not rehash_segment:
            hashed = stream[col * sdu:(col + 1) * sdu]       # what `data` names when the reference loops (:450)
    raise RuntimeError("resource hashmap kept colliding (repeated parts inside the guard window)")
