"""The index maps of the Identity layer on the GPU (reticulum_amd/identity.py):
decrypt_batch's m x (R+1) key set with its way back through `live` and
`key_used - j*C`, encrypt_batch's per-packet keys, and the `keep` lists of
validate_batch and validate_announces_batch, in batches large and mixed enough
that a wrong index returns a valid answer for the wrong packet.  Expected
values are the plain models of tests_helpers.py, which tests/test_identity_edges.py
ties to the reference's recorded cases; every comparison is exact."""
import functools
import hashlib

import numpy as np
import pytest

import ed25519_ref
import x25519_ref as ref
from oracle import ctoken
from tests_helpers import announce_valid_ref, b, identity_decrypt_ref, identity_encrypt_ref

pytestmark = pytest.mark.gpu

PT_LENGTHS = (0, 15, 16, 17, 383)
MISSHAPED = (33, 64, 80, 81, 32 + 48 + 8)       # live, but no token: nothing, 32 B, iv ‖ tag, 1 and 8 bytes of ciphertext
DEAD = (0, 1, 32)


class Gen:
    def __init__(self, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))

    def __call__(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def public(prv):
    return ref.ladder(prv, ref.BASE)


def token_key(eph, target_pub, salt):
    return ref.hkdf(64, ref.ladder(eph, target_pub), salt)


def flip(data, at, bit):
    return data[:at] + bytes([data[at] ^ bit]) + data[at + 1:]


@functools.lru_cache(maxsize=None)
def batch(R, n):
    """n live tokens for an identity with R ratchets, and dead ones among them.

    Live token k is, in rotation, good / misshaped / good / damaged.  Good and
    damaged ones go in turn to the identity's key and to every ratchet, with
    plaintext lengths from PT_LENGTHS; the damage is one bit of the tag, of
    the ciphertext or of the ephemeral key; the misshaped ones have the total
    lengths of MISSHAPED behind a real ephemeral key, every other one with a
    tag that is right for its bytes, so that only the token's shape refuses
    it.  Dead tokens (lengths 0, 1, 32) stand first, last, in the middle and
    after every 16th live one.  n counts the live ones: they are what the key
    set is built over.  Returns (private, salt, ratchets, tokens, labels, sent)
    with sent[i] = (plaintext, target) for a good token, target -1 being the
    identity's key."""
    rnd = Gen(1000 * R + n)
    prv, salt = rnd(32), rnd(16)
    ratchets = [rnd(32) for _ in range(R)]
    targets = [(-1, public(prv))] + [(r, public(ratchets[r])) for r in range(R)]
    live, good, damaged, misshaped = [], (4 if n == 1 else 0), 0, 0       # a single token goes to ratchet 3
    for k in range(n):
        kind = ("good", "misshaped", "good", "damaged")[k % 4] if n > 1 else "good"
        eph = rnd(32)
        if kind == "misshaped":
            which, target_pub = targets[misshaped % len(targets)]
            total = MISSHAPED[misshaped % 5]
            body = rnd(total - 32)
            if total >= 80 and (misshaped // 5) % 2:
                body = body[:-32] + ctoken.hmac_sha256(token_key(eph, target_pub, salt)[:32], body[:-32])
            live.append((public(eph) + body, "misshaped %d" % total, None))
            misshaped += 1
            continue
        count = good if kind == "good" else damaged // 3
        which, target_pub = targets[count % len(targets)]
        pt = rnd(PT_LENGTHS[(good if kind == "good" else damaged) % 5])
        tok = identity_encrypt_ref(target_pub, salt, pt, eph, rnd(16))
        if kind == "good":
            label = "to the identity" if which < 0 else "to ratchet %d" % which
            live.append((tok, label + ", %d B" % len(pt), (pt, which)))
            good += 1
        else:
            what = ("tag", "ciphertext", "ephemeral key")[damaged % 3]
            at = {"tag": len(tok) - 1 - damaged % 32, "ciphertext": 48 + damaged % 16, "ephemeral key": damaged % 31}[what]
            live.append((flip(tok, at, 1 << (damaged % 8)), "damaged " + what, None))
            damaged += 1
    dead = 0

    def a_dead_one():
        nonlocal dead
        dead += 1
        return (rnd(DEAD[(dead - 1) % 3]), "dead", None)
    items = [a_dead_one()]
    for k, it in enumerate(live):
        items.append(it)
        if k % 16 == 15 or (n > 1 and k == n // 2):
            items.append(a_dead_one())
    if items[-1][1] != "dead":
        items.append(a_dead_one())
    assert sum(1 for it in items if len(it[0]) > 32) == n
    return prv, salt, ratchets, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items]


@functools.lru_cache(maxsize=None)
def modelled(R, n, enforce):
    prv, salt, ratchets, toks, labels, sent = batch(R, n)
    return [identity_decrypt_ref(prv, salt, t, ratchets, enforce) for t in toks]


def assert_items(got, want, labels):
    pts, which = got
    assert len(pts) == len(which) == len(want)
    for i, (w, label) in enumerate(zip(want, labels)):
        assert (pts[i], which[i]) == w, "item %d (%s)" % (i, label)


# ---- a. decrypt_batch against the model

@pytest.mark.parametrize("enforce", [False, True])
@pytest.mark.parametrize("R,n", [(0, 65), (1, 130), (2, 86), (5, 43), (5, 1)])
def test_decrypt_batch_against_the_model(R, n, enforce):
    """m * C = 65, 260, 258, 258 and 6 keys: on or across 64, 256 and 258."""
    import reticulum_amd as rt
    prv, salt, ratchets, toks, labels, sent = batch(R, n)
    want = modelled(R, n, enforce)
    # the model's output holds what the batch was built to hold
    seen = {}
    for (pt, which), label, s in zip(want, labels, sent):
        if s is None:
            assert (pt, which) == (None, None), label
        elif enforce and s[1] < 0:
            assert (pt, which) == (None, None), label
        else:
            assert (pt, which) == s, label
        for part in label.split(", "):
            seen[part] = seen.get(part, 0) + 1
    opened_by = {w for _, w in want if w is not None}
    if n > 1:
        assert opened_by == set(range(R)) | (set() if enforce else {-1})
        classes = (["to the identity", "dead", "damaged tag", "damaged ciphertext", "damaged ephemeral key"] +
                   ["to ratchet %d" % r for r in range(R)] + ["%d B" % L for L in PT_LENGTHS] +
                   ["misshaped %d" % L for L in MISSHAPED])
        assert all(seen.get(c, 0) >= 2 for c in classes), seen
        assert labels[0] == labels[-1] == "dead" and {len(t) for t, la in zip(toks, labels) if la == "dead"} == set(DEAD)
    else:
        assert labels == ["dead", "to ratchet 3, 383 B", "dead"] and opened_by == {3}
    assert_items(rt.identity.decrypt_batch(prv, salt, toks, ratchets=ratchets, enforce_ratchets=enforce), want, labels)


# ---- b. ratchet-list edges

def test_ratchet_list_edges():
    import reticulum_amd as rt
    prv, salt, (ra, rb), toks, labels, sent = batch(2, 65)
    to = [None if s is None else s[1] for s in sent]
    assert min(to.count(w) for w in (-1, 0, 1)) >= 8

    def run(ratchets, enforce=False):
        want = [identity_decrypt_ref(prv, salt, t, ratchets, enforce) for t in toks]
        assert_items(rt.identity.decrypt_batch(prv, salt, toks, ratchets=ratchets, enforce_ratchets=enforce), want, labels)
        return [w for _, w in want]
    # the same ratchet twice: the first index wins
    which = run([ra, ra, rb])
    assert all(which[i] == {-1: -1, 0: 0, 1: 2}[t] for i, t in enumerate(to) if t is not None)
    which = run([rb, ra, ra, rb], enforce=True)
    assert all(which[i] == {-1: None, 0: 1, 1: 0}[t] for i, t in enumerate(to) if t is not None)
    # a ratchet that is the identity's own key: its index, not -1
    for enforce in (False, True):
        which = run([rb, prv], enforce)
        assert all(which[i] == {-1: 1, 0: None, 1: 0}[t] for i, t in enumerate(to) if t is not None)
    # ratchets enforced and none given: nothing opens
    for ratchets in ([], None):
        got = rt.identity.decrypt_batch(prv, salt, toks, ratchets=ratchets, enforce_ratchets=True)
        assert got == ([None] * len(toks), [None] * len(toks))
    assert set(run([], enforce=True)) == {None}


# ---- c. low-order ephemeral keys

def test_low_order_ephemeral_keys_open_under_any_key():
    """An ephemeral key of low order makes the shared secret 32 zero bytes
    whatever the private key (the reference does not raise there:
    tests/test_x25519.py::test_low_order_points_give_zero_without_error), so
    a token made under hkdf(zeros) opens under the first key tried."""
    import reticulum_amd as rt
    rnd = Gen(8)
    prv, salt, ratchet = rnd(32), rnd(16), rnd(32)
    notes = ("point 0", "point order 8 (a)", "point order 8 (b)", "point 1", "point p", "point p+1")
    points = [next(b(e["point"]) for e in ref.vectors()["exchanges"] if e["note"] == note) for note in notes]
    assert points[0] == bytes(32)
    zero_key = ref.hkdf(64, bytes(32), salt)
    toks, labels, low = [], [], []
    for i in range(24):
        pt = rnd(PT_LENGTHS[i % 5])
        if i % 2:
            target = (public(prv), public(ratchet))[(i // 2) % 2]
            tok = identity_encrypt_ref(target, salt, pt, rnd(32), rnd(16))
            if i % 8 == 7:                               # bit 255 of the ephemeral key is ignored: the token still opens
                tok = flip(tok, 31, 0x80)
            labels.append("ordinary")
        else:
            tok = points[(i // 2) % len(points)] + ctoken.encrypt(zero_key, rnd(16), pt)
            labels.append("low order: " + notes[(i // 2) % len(points)])
            low.append(i)
        toks.append(tok)
    # of the 12 ordinary tokens 6 go to the identity's key and 6 to the ratchet
    for ratchets, enforce, first, opened in (([], False, -1, 18), ([ratchet], False, 0, 24), ([ratchet], True, 0, 18)):
        want = [identity_decrypt_ref(prv, salt, t, ratchets, enforce) for t in toks]
        assert all(want[i][0] is not None and want[i][1] == first for i in low)
        assert sum(w[0] is not None for w in want) == opened
        assert_items(rt.identity.decrypt_batch(prv, salt, toks, ratchets=ratchets, enforce_ratchets=enforce), want, labels)
    # and under a key that has nothing to do with the sender
    stranger = rnd(32)
    pts, which = rt.identity.decrypt_batch(stranger, salt, toks)
    assert [i for i, p in enumerate(pts) if p is not None] == low and {which[i] for i in low} == {-1}
    assert all((pts[i], which[i]) == identity_decrypt_ref(stranger, salt, toks[i], [], False) for i in range(24))


# ---- d. encrypt_batch with given ephemerals and IVs

@pytest.fixture(scope="module")
def outgoing():
    rnd = Gen(9)
    prv, salt, ratchet = rnd(32), rnd(16), rnd(32)
    lengths = [0, 400, 15, 16, 17, 383, 1] + [int(x) for x in rnd.rng.integers(0, 401, 250)]
    pts = [rnd(L) for L in lengths]
    ephs = [rnd(32) for _ in pts]
    ivs = np.frombuffer(rnd(16 * len(pts)), np.uint8).reshape(-1, 16)
    assert len(pts) == 257 and len(set(ephs)) == 257
    want = [identity_encrypt_ref(public(prv), salt, p, e, iv.tobytes()) for p, e, iv in zip(pts, ephs, ivs)]
    return prv, salt, ratchet, pts, ephs, ivs, want


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_encrypt_batch_equals_the_model(outgoing, n):
    import reticulum_amd as rt
    prv, salt, ratchet, pts, ephs, ivs, want = outgoing
    got = rt.identity.encrypt_batch(public(prv), salt, pts[:n], ephemeral_privates=ephs[:n], ivs=ivs[:n])
    assert len(got) == n
    for i in range(n):
        assert got[i] == want[i], "item %d (%d B)" % (i, len(pts[i]))


def test_encrypt_batch_to_a_ratchet_equals_the_model(outgoing):
    import reticulum_amd as rt
    prv, salt, ratchet, pts, ephs, ivs, to_identity = outgoing
    want = [identity_encrypt_ref(public(ratchet), salt, p, e, iv.tobytes()) for p, e, iv in zip(pts, ephs, ivs)]
    got = rt.identity.encrypt_batch(public(ratchet), salt, pts, ephemeral_privates=ephs, ivs=ivs)
    for i in range(257):
        assert got[i] == want[i] and got[i] != to_identity[i], "item %d (%d B)" % (i, len(pts[i]))
    back = rt.identity.decrypt_batch(prv, salt, got, ratchets=[ratchet])
    assert back == (pts, [0] * 257)


# ---- e. validate_batch

@pytest.fixture(scope="module")
def signed():
    """130 messages signed under ten keys in rotation and all of them under
    the first; every fifth signature damaged, every seventh 63 or 65 bytes."""
    rnd = Gen(10)
    seeds = [rnd(32) for _ in range(10)]
    pubs = [ed25519_ref.public_key(s) for s in seeds]
    msgs = [rnd((i * 29) % 211) for i in range(130)]

    def spoil(sigs):
        out = []
        for i, s in enumerate(sigs):
            if i % 5 == 0:
                s = flip(s, (i * 3) % 64, 1 << (i % 8))
            if i % 7 == 0:
                s = s[:63] if i % 14 else s + b"\x00"
            out.append(s)
        return out
    keys = [pubs[i % 10] for i in range(130)]
    per_item = spoil([ed25519_ref.sign(seeds[i % 10], m, keys[i]) for i, m in enumerate(msgs)])
    one_key = spoil([ed25519_ref.sign(seeds[0], m, pubs[0]) for m in msgs])

    def expect(ks, sigs):
        return [len(s) == 64 and ed25519_ref.verify(k, s, m) for k, s, m in zip(ks, sigs, msgs)]
    want_per_item, want_one_key = expect(keys, per_item), expect([pubs[0]] * 130, one_key)
    for want in (want_per_item, want_one_key):
        assert want == [i % 5 != 0 and i % 7 != 0 for i in range(130)]
    return keys, msgs, per_item, want_per_item, one_key, want_one_key


def test_validate_batch_with_wrong_lengths_and_damage(signed):
    import reticulum_amd as rt
    keys, msgs, per_item, want_per_item, one_key, want_one_key = signed
    assert {len(s) for s in per_item} == {63, 64, 65}
    assert rt.validate_batch(keys, per_item, msgs) == want_per_item
    assert rt.validate_batch(keys[0], one_key, msgs) == want_one_key


# ---- f. validate_announces_batch

KINDS = ("good", "one byte short", "wrong destination hash", "signed for another destination",
         "valid signature, destination hash not of this identity", "tampered")


@pytest.fixture(scope="module")
def announces():
    """130 announces laid out as tests/golden/gen_ed25519.py lays them out
    (the X25519 half of the public key is only hashed, so it is random here)."""
    rnd = Gen(11)
    seeds = [rnd(32) for _ in range(10)]
    pubs = [rnd(32) + ed25519_ref.public_key(s) for s in seeds]
    items, notes = [], []
    for i in range(130):
        flag, app, kind = i % 2, (b"", rnd(11), rnd(40))[i % 3], KINDS[(i // 6) % 6]
        seed, pub = seeds[i % 10], pubs[i % 10]
        name_hash, random_hash, ratchet = rnd(10), rnd(10), (rnd(32) if flag else b"")
        dest = hashlib.sha256(name_hash + hashlib.sha256(pub).digest()[:16]).digest()[:16]
        signed_for = dest
        if kind == "signed for another destination":
            signed_for = hashlib.sha256(rnd(10) + hashlib.sha256(pub).digest()[:16]).digest()[:16]
        elif kind == "valid signature, destination hash not of this identity":
            signed_for = dest = rnd(16)
        sig = ed25519_ref.sign(seed, signed_for + pub + name_hash + random_hash + ratchet + app, pub[32:])
        head = pub + name_hash + random_hash + ratchet
        data = head + sig + app
        if kind == "one byte short":
            data = data[:len(head) + 63]
        elif kind == "wrong destination hash":
            dest = flip(dest, i % 16, 1 << (i % 8))
        elif kind == "tampered":                         # the app data where there is some, else the name hash
            data = flip(data, len(data) - 1, 1) if app else flip(data, 64 + i % 10, 1)
        items.append((dest, flag, data))
        notes.append("%s, flag %d, %d B app data" % (kind, flag, len(app)))
    want = [announce_valid_ref(*it) for it in items]
    want_sig = [announce_valid_ref(*it, only_validate_signature=True) for it in items]
    return items, notes, want, want_sig


def test_validate_announces_batch_mixed(announces):
    import reticulum_amd as rt
    items, notes, want, want_sig = announces
    assert {True, False} == set(want) == set(want_sig) and want != want_sig
    for i, note in enumerate(notes):                     # each kind gives what it was built to give
        kind = KINDS[(i // 6) % 6]
        assert (want[i], want_sig[i]) == {"good": (True, True),
                                          "valid signature, destination hash not of this identity": (False, True)
                                          }.get(kind, (False, False)), note
    assert {(n.split(", ", 1)[1]) for n, w in zip(notes, want) if w} == {
        "flag %d, %d B app data" % (f, a) for f in (0, 1) for a in (0, 11, 40)}
    got = rt.validate_announces_batch(items)
    got_sig = rt.validate_announces_batch(items, only_validate_signature=True)
    for i, note in enumerate(notes):
        assert (got[i], got_sig[i]) == (want[i], want_sig[i]), "item %d (%s)" % (i, note)
