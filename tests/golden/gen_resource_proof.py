"""Generate tests/golden/resource_proof_vectors.json from the reference Resource.

Runs only in the build container (imports the reference checkout).  Fixtures
for the Resource integrity hash and proof (RNS/Resource.py:436-439, 698-699,
759-760), all from real RNS.Resource(data, link, advertise=False,
auto_compress=False) constructions over the stub link and stand-in Packet
that gen_resource.py uses:

* sizes on every tail-block boundary of SHA-256(data || 4-byte random_hash)
  and SHA-256(data || 32-byte hash): data, random_hash, hash, truncated_hash,
  expected_proof;
* one construction with metadata=: the bytes hashed are metadata || data (:330);
* one forced collision retry: get_map_hash is wrapped so that, under the
  first drawn random_hash only, two parts inside the guard window get the
  same map hash.  The reference then loops and, at :437-439, hashes the name
  ``data`` as rebound at :450: the colliding encrypted part.  The generator
  asserts exactly that, so the quirk is what is pinned.  The stream is an
  input we make (a stub encrypt returning tests_helpers.collision_stream), so
  only its seed and length are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_resource_proof.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/ (tests_helpers)
REF = os.environ.get("RNS_REFERENCE", "/root/reference")

SIZES = (0, 1, 23, 24, 51, 52, 55, 56, 63, 64, 65, 200, 1000, 5000)


def sha(x):
    return hashlib.sha256(x).digest()


def main():
    sys.path.insert(0, REF)
    import RNS
    from RNS.Cryptography.Token import Token
    from RNS.vendor import umsgpack
    from tests_helpers import collision_stream

    rng = np.random.Generator(np.random.PCG64(759))
    tok = Token(rng.integers(0, 256, 64, dtype=np.uint8).tobytes())

    class StubLink:
        mtu = None
        mdu = None
        rtt = 0.5
        traffic_timeout_factor = 6
        link_id = bytes(16)

        def __init__(self, fixed_stream=None):
            self.streams = []
            self.fixed_stream = fixed_stream

        def encrypt(self, plaintext):
            ct = self.fixed_stream if self.fixed_stream is not None else tok.encrypt(plaintext)
            self.streams.append(ct)
            return ct

    class StubPacket:
        RESOURCE = RNS.Packet.RESOURCE

        def __init__(self, link, data, context=None):
            self.data = data

        def pack(self):
            pass

    out = {"reference": "RNS/Resource.py:330,436-439,446-462,698-699,759-760",
           "generator": "tests/golden/gen_resource_proof.py", "resources": [], "skipped_sizes": []}
    real_packet = RNS.Packet
    RNS.Packet = StubPacket
    try:
        for size in SIZES:
            data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
            try:
                res = RNS.Resource(data, StubLink(), advertise=False, auto_compress=False)
            except Exception as e:                   # size 0, if the reference refuses it
                out["skipped_sizes"].append({"size": size, "error": type(e).__name__})
                continue
            assert res.hash == sha(data + res.random_hash) and res.truncated_hash == res.hash[:16]
            assert res.expected_proof == sha(data + res.hash)
            out["resources"].append({"size": size, "data": data.hex(), "random_hash": res.random_hash.hex(),
                                     "hash": res.hash.hex(), "truncated_hash": res.truncated_hash.hex(),
                                     "expected_proof": res.expected_proof.hex()})

        # metadata: the hashes cover metadata || data (:330)
        data = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
        metadata = {"name": "fixture", "n": 7}
        res = RNS.Resource(data, StubLink(), metadata=metadata, advertise=False, auto_compress=False)
        packed = umsgpack.packb(metadata)
        hashed = len(packed).to_bytes(3, "big") + packed + data
        assert res.hash == sha(hashed + res.random_hash) and res.expected_proof == sha(hashed + res.hash)
        out["metadata"] = {"data": data.hex(), "metadata_msgpack": packed.hex(), "hashed": hashed.hex(),
                           "random_hash": res.random_hash.hex(), "hash": res.hash.hex(),
                           "truncated_hash": res.truncated_hash.hex(), "expected_proof": res.expected_proof.hex()}

        # forced collision retry
        sdu, seed, n_parts = RNS.Resource.SDU, 7590, 12
        stream = collision_stream(seed, n_parts * sdu - 30, None, sdu)
        first_part, col = 3, 9                      # part 9 gets part 3's map hash under the first draw
        draws, first_draw = [], []
        real_get_map_hash = RNS.Resource.get_map_hash
        real_random_hash = RNS.Identity.get_random_hash

        def recording_random_hash():
            # the constructor draws once for the stream's prefix (:408), then once per loop round (:436)
            h = real_random_hash()
            draws.append(h)
            if len(draws) == 2:
                first_draw.append(h[:RNS.Resource.RANDOM_HASH_SIZE])
            return h

        def colliding_get_map_hash(self, part):
            if self.random_hash == first_draw[0] and part == stream[col * sdu:(col + 1) * sdu]:
                part = stream[first_part * sdu:(first_part + 1) * sdu]
            return real_get_map_hash(self, part)

        data = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
        RNS.Identity.get_random_hash = staticmethod(recording_random_hash)
        RNS.Resource.get_map_hash = colliding_get_map_hash
        try:
            res = RNS.Resource(data, StubLink(fixed_stream=stream), advertise=False, auto_compress=False)
        finally:
            RNS.Resource.get_map_hash = real_get_map_hash
            RNS.Identity.get_random_hash = real_random_hash
        loop_draws = [d[:RNS.Resource.RANDOM_HASH_SIZE] for d in draws[1:]]
        assert len(loop_draws) == 2 and res.random_hash == loop_draws[1], len(loop_draws)
        part = stream[col * sdu:(col + 1) * sdu]
        # the quirk: after the retry the reference hashed the colliding encrypted part
        assert res.hash == sha(part + res.random_hash) and res.expected_proof == sha(part + res.hash)
        assert res.hash != sha(data + res.random_hash)
        assert len(res.hashmap) == 4 * n_parts
        out["collision_retry"] = {"seed": seed, "stream_len": len(stream), "sdu": sdu, "data": data.hex(),
                                  "draws": [d.hex() for d in loop_draws], "forced_same": [first_part, col],
                                  "colliding_index": col, "random_hash": res.random_hash.hex(),
                                  "hash": res.hash.hex(), "expected_proof": res.expected_proof.hex(),
                                  "hashmap": res.hashmap.hex()}
    finally:
        RNS.Packet = real_packet

    path = os.path.join(HERE, "resource_proof_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes; skipped", out["skipped_sizes"])


if __name__ == "__main__":
    main()
