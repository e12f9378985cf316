"""Small helpers shared by the test modules."""
import ctypes
import functools

import numpy as np


def b(h):
    return bytes.fromhex(h)


def u8(data, *shape):
    return np.frombuffer(bytes(data), np.uint8).reshape(*shape).copy()


def pack(msgs):
    """A list of bytes -> (flat uint8 array, uint64 offsets, uint32 lengths)."""
    lens = np.array([len(m) for m in msgs], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return u8(b"".join(msgs) or b"\x00", -1), offs, lens


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def lib_ctx():
    from reticulum_amd import _native
    return _native.load(), _native.context(0)


# ---- plain models of the Identity layer (RNS/Identity.py), built from the
# tests' integer references and the C oracle's token alone

@functools.lru_cache(maxsize=None)
def _ladder(scalar, point):
    import x25519_ref
    return x25519_ref.ladder(scalar, point)


def identity_decrypt_ref(private, salt, token, ratchets, enforce):
    """``Identity.decrypt`` (Identity.py:857-902) for one token: ``(plaintext |
    None, which)``.  A token of 32 bytes or fewer gives ``(None, None)``;
    otherwise every ratchet in order and then the identity's key (left out under
    ``enforce``) derives a token key from its exchange with token[:32], and the
    first that opens token[32:] wins: ``which`` is that ratchet's index, or -1
    for the identity's key."""
    import x25519_ref
    from oracle import ctoken
    token = bytes(token)
    if len(token) <= 32:
        return None, None
    tried = [(bytes(r), i) for i, r in enumerate(ratchets or [])]
    if not enforce:
        tried.append((bytes(private), -1))
    for scalar, which in tried:
        key = x25519_ref.hkdf(64, _ladder(scalar, token[:32]), salt)
        status, pt = ctoken.decrypt(key, token[32:])
        if status == 0:
            return pt, which
    return None, None


def identity_encrypt_ref(target_public, salt, pt, eph, iv):
    """``Identity.encrypt`` (Identity.py:811-833) with the ephemeral private key
    and the IV given: ephemeral_pub ‖ iv ‖ ct ‖ tag."""
    import x25519_ref
    from oracle import ctoken
    key = x25519_ref.hkdf(64, _ladder(bytes(eph), bytes(target_public)), salt)
    return _ladder(bytes(eph), x25519_ref.BASE) + ctoken.encrypt(key, bytes(iv), bytes(pt))


def announce_valid_ref(destination_hash, context_flag, data, only_validate_signature=False):
    """``Identity.validate_announce`` (Identity.py:511-606) for one announce."""
    import ed25519_ref
    return ed25519_ref.validate_announce(bytes(destination_hash), context_flag, bytes(data), only_validate_signature)


def trial_case(seed, n_tok=40, n_keys=12):
    """Tokens under random keys of a key set and candidate lists in which the
    right key sits at a random rank, is missing, or appears twice; plus
    malformed and too-short tokens that no key opens."""
    import numpy as np
    from oracle import ctoken
    rng = np.random.Generator(np.random.PCG64(seed))
    keys = rng.integers(0, 256, (n_keys, 64), dtype=np.uint8)
    toks, cands, expect = [], [], []
    for t in range(n_tok):
        k = int(rng.integers(0, n_keys))
        pt = rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()
        tok = ctoken.encrypt(keys[k].tobytes(), rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), pt)
        others = [i for i in rng.permutation(n_keys).tolist() if i != k][: int(rng.integers(0, 6))]
        mode = t % 5
        if mode == 0:                      # right key missing
            cand, exp = others, -1
        elif mode == 1:                    # right key twice
            cand = others + [k, k]
            exp = k
        elif mode == 2:                    # malformed: ciphertext not whole blocks
            tok, cand, exp = tok[:-33] + tok[-32:], others + [k], -1
        elif mode == 3:                    # too short
            tok, cand, exp = tok[:32], [k], -1
        else:
            pos = int(rng.integers(0, len(others) + 1))
            cand = others[:pos] + [k] + others[pos:]
            exp = k
        toks.append(tok)
        cands.append(cand)
        expect.append(exp)
    return keys, toks, cands, np.array(expect)


def collision_stream(seed, length, dup, sdu=464):
    """The input stream of a Resource collision-guard fixture
    (tests/golden/gen_resource.py): `length` seeded random bytes with part
    dup[1] overwritten by a copy of part dup[0] (no copy when dup is None or
    names one part)."""
    import numpy as np
    stream = bytearray(np.random.Generator(np.random.PCG64(seed)).integers(0, 256, length, dtype=np.uint8).tobytes())
    if dup and dup[0] != dup[1]:
        a, c = dup
        stream[c * sdu:(c + 1) * sdu] = stream[a * sdu:(a + 1) * sdu]
    return bytes(stream)


# ---- Resource hashmap edge cases (tests/test_resource_edges.py builds them
# against the oracle, tests/test_resource_edges_gpu.py runs them on the device)

EDGE_SDU = 8                  # tiny parts: thousands of them cost kilobytes
EDGE_PARTS = 6000             # 23 whole collision tiles and one of 112 parts
EDGE_TILE = 256               # COLL_TILE, the collision kernels' workgroup
EDGE_LDS_GUARD_MAX = 4096     # COLL_LDS_GUARD_MAX: larger guards run k_map_collisions
EDGE_GUARDS = (1, 2, 224, 255, 256, 257, 600, 4096, 4097, 5000)


@functools.lru_cache(maxsize=None)
def edge_base(seed=7101):
    """(stream, salt): 6000 parts of 8 bytes, the last one short, whose map
    hashes under `salt` are all distinct (tests/test_resource_edges.py checks
    it), so the only repeats in a case are the planted ones."""
    rng = np.random.Generator(np.random.PCG64(seed))
    stream = rng.integers(0, 256, EDGE_PARTS * EDGE_SDU - 3, dtype=np.uint8).tobytes()
    return stream, rng.integers(0, 256, 4, dtype=np.uint8).tobytes()


def edge_part(i):
    """Part i of the base stream."""
    return edge_base()[0][i * EDGE_SDU:(i + 1) * EDGE_SDU]


def plant_repeats(stream, pairs, sdu=EDGE_SDU):
    """`stream` with part a copied over part c for every (a, c) of `pairs`, in
    order (collision_stream's way, for several pairs).  A copy over a short
    last part makes that part whole."""
    s = bytearray(stream)
    for a, c in pairs:
        s[c * sdu:(c + 1) * sdu] = s[a * sdu:(a + 1) * sdu]
    return bytes(s)


def sha_map_hashes(parts, salt):
    """SHA-256(part || salt)[:4] of every part, by hashlib."""
    import hashlib
    return b"".join(hashlib.sha256(bytes(p) + bytes(salt)).digest()[:4] for p in parts)


def cut(stream, sdu=EDGE_SDU):
    return [stream[i:i + sdu] for i in range(0, len(stream), sdu)]


def edge_later_parts(guard):
    """The later parts c of the window-edge cases: the first, second and last
    lane of a tile >= 1 (tile 21), the last part of the launch (lane 111 of
    the partial tile 23), and the last lane of tile 0 where the guard leaves
    room for a part guard + 1 before it."""
    return (5376, 5377, 5631, EDGE_PARTS - 1) + ((EDGE_TILE - 1,) if guard + 1 < EDGE_TILE else ())


def edge_cases(guard):
    """(a, c, expected) for every later part c: a copy of part c - guard sits
    on the window's oldest place and breaks at c; a copy of part
    c - guard - 1 is one place too old and is accepted."""
    out = []
    for c in edge_later_parts(guard):
        out += [(c - guard, c, c), (c - guard - 1, c, None)]
    return out


@functools.lru_cache(maxsize=None)
def edge_single(guard, a, c):
    """One case as a single resource over the whole base stream: (stream,
    salt, map hashes by hashlib, the oracle's first collision of them)."""
    from oracle import ctoken
    stream, salt = edge_base()
    stream = plant_repeats(stream, [(a, c)])
    hm = sha_map_hashes(cut(stream), salt)
    return stream, salt, hm, ctoken.first_collision(hm, guard)


class Layout:
    """Parts of several resources for one explicit-form launch: the packed
    data, each part's offset, length and resource, each resource's first
    global part index, and per resource the map hashes (hashlib) and the
    oracle's first collision as the device reports it: start[r] + col, or -1."""

    def __init__(self, resources, salts, guard):
        from oracle import ctoken
        self.guard, self.salts = guard, [bytes(s) for s in salts]
        self.parts = [p for r in resources for p in r]
        self.res = [r for r, ps in enumerate(resources) for _ in ps]
        self.len = [len(p) for p in self.parts]
        self.off = [0] * len(self.parts)
        for j in range(1, len(self.parts)):
            self.off[j] = self.off[j - 1] + self.len[j - 1]
        self.data = b"".join(self.parts)
        self.start, self.hashes, self.first = [], [], []
        pos = 0
        for r, ps in enumerate(resources):
            hm = sha_map_hashes(ps, self.salts[r])
            col = ctoken.first_collision(hm, guard)
            self.start.append(pos)
            self.hashes.append(hm)
            self.first.append(-1 if col is None else pos + col)
            pos += len(ps)
        self.n_parts, self.n_res = pos, len(resources)

    def mixed_window(self, j):
        """Does the LDS kernel's window of part j's tile (the tile's parts and
        the `guard` before them) hold parts of more than one resource?"""
        j0 = j - j % EDGE_TILE
        return self.res[max(0, j0 - self.guard)] != self.res[min(j0 + EDGE_TILE, self.n_parts) - 1]


@functools.lru_cache(maxsize=None)
def edge_batched(guard):
    """The window-edge cases as resources of their own in one launch: (layout,
    cases) with cases = [(resource, global later part, hit)].  A case resource
    is parts 0 .. guard + 1 of the base stream and three more, with part
    guard + 1 overwritten by a copy of part 1 (distance guard: breaks there)
    or of part 0, the resource's first (guard + 1: accepted).  A filler
    resource before it moves the later part to the wanted lane of its tile:
    first, second, last, and lane 100 for the case that ends the launch.
    Every window so sits in its resource, while the tile's LDS window holds a
    boundary: behind the later part for lanes 0 and 1, before its window for
    the others."""
    _, salt = edge_base()
    resources, cases, pos = [], [], 0
    for lane in (0, 1, EDGE_TILE - 1, 100):
        for hit in (True, False):
            fill = (lane - (pos + guard + 1)) % EDGE_TILE
            if fill:
                resources.append([edge_part(5300 + i) for i in range(fill)])
            last = lane == 100 and not hit
            ps = [edge_part(i) for i in range(guard + 2 + (0 if last else 3))]
            ps[guard + 1] = ps[1 if hit else 0]
            cases.append((len(resources), pos + fill + guard + 1, hit))
            resources.append(ps)
            pos += fill + len(ps)
    return Layout(resources, [salt] * len(resources), guard), cases


# (a, c) repeats in tiles 23, 21 and 22 of one resource, every one inside a
# window of 224; the earliest later part (5400) is neither planted first nor
# in the first or last workgroup to run
SEVERAL = ((5800, 5900), (5390, 5400), (5500, 5640))


@functools.lru_cache(maxsize=None)
def several_two_resources(guard):
    """Two resources of 3000 parts in one launch.  The first repeats at its
    parts 2900 and 2600; the second at 2980, 2950 and 2999, all three in the
    launch's last tile.  Each resource reports its own earliest."""
    _, salt = edge_base()
    A = [edge_part(i) for i in range(3000)]
    B = [edge_part(3000 + i) for i in range(3000)]
    for ps, pairs in ((A, ((2800, 2900), (2500, 2600))), (B, ((2960, 2980), (2900, 2950), (2990, 2999)))):
        for a, c in pairs:
            ps[c] = ps[a]
    return Layout([A, B], [salt, salt], guard)


@functools.lru_cache(maxsize=None)
def edge_boundaries(guard):
    """Resource boundaries with equal parts on both sides, all resources under
    one salt (tests/test_resource_edges.py states what each must give):
    (layout, names) with names = {name: resource index}.
      A | B   boundary inside a tile; B's first guard // 2 + 1 parts copy A's last
      C | D   the same with the boundary on a tile boundary
      one * 300   one-part resources of identical content
      E | F   F starts inside a tile with a copy of E's last part, and its part
              `guard` repeats its own first part
    """
    _, salt = edge_base()
    pool = iter(range(EDGE_PARTS - 1))
    fresh = lambda n: [edge_part(next(pool)) for _ in range(n)]
    half = guard // 2 + 1
    A = fresh(guard + 50)
    B = A[-half:] + fresh(guard + 50 - half)
    C = fresh(guard + EDGE_TILE - (2 * (guard + 50) + guard) % EDGE_TILE)
    D = C[-half:] + fresh(guard + 50 - half)
    ones = [fresh(1)] * 300
    E = fresh(100)
    F = [E[-1]] + fresh(guard + 9)
    F[guard] = F[0]
    resources = [A, B, C, D] + ones + [E, F]
    names = {"A": 0, "B": 1, "C": 2, "D": 3, "ones": range(4, 304), "E": 304, "F": 305}
    return Layout(resources, [salt] * len(resources), guard), names
