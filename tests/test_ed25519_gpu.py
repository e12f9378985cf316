"""k_ed25519_verify / _sign / _public on the GPU through the C-ABI's host and
device forms and the Python layers, against the reference's fixtures
(tests/golden/ed25519_vectors.json) and the tests' own integer implementation
(tests/ed25519_ref.py)."""
import ctypes

import numpy as np
import pytest

import ed25519_ref as ref
from tests_helpers import b, lib_ctx, pack, ptr, u8

pytestmark = pytest.mark.gpu

RT_E_INVAL = -1


def fixture_cases():
    """Every verification the fixtures hold: (pk, sig, msg, ok, note)."""
    v = ref.vectors()
    cases = [(b(s["public"]), b(s["sig"]), b(s["msg"]), True, "signature") for s in v["signatures"] + [v["selftest"]]]
    cases += [(b(c["pk"]), b(c["sig"]), b(c["msg"]), c["ok"], c["note"]) for c in v["verify"]]
    for a in v["announces"]:
        pub, name_hash, random_hash, ratchet, sig, app = ref.announce_fields(b(a["data"]), a["context_flag"])
        if len(pub) == 64 and len(sig) == 64:
            signed = b(a["destination_hash"]) + pub + name_hash + random_hash + ratchet + app
            cases.append((pub[32:], sig, signed, a["ok_signature_only"], a["note"]))
    return cases


@pytest.fixture(scope="module")
def mixed():
    """257 items whose neighbours differ in message length (0-300 bytes, so in
    SHA-512 block count) and in outcome: honest signatures, single-bit damage in
    the signature, the key or the message, and the fixtures' edge cases, lane
    by lane.  Expected results from the integer reference, computed once."""
    rng = np.random.Generator(np.random.PCG64(25519))
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(8)]
    pubs = [ref.public_key(s) for s in seeds]
    edges = [c for c in fixture_cases() if not c[4].startswith(("signature", "ratchet"))]
    pks, sigs, msgs = [], [], []
    for i in range(257):
        if i % 6 == 5:
            pk, sig, msg = edges[(i // 6) % len(edges)][:3]
        else:
            msg = rng.integers(0, 256, (i * 37) % 301, dtype=np.uint8).tobytes()
            pk, sig = pubs[i % 8], ref.sign(seeds[i % 8], msg, pubs[i % 8])
            kind = i % 6
            if kind == 1:
                sig = bytes([sig[0] ^ 1]) + sig[1:]
            elif kind == 2:
                sig = sig[:40] + bytes([sig[40] ^ 0x10]) + sig[41:]
            elif kind == 3 and msg:
                msg = msg[:-1] + bytes([msg[-1] ^ 0x80])
            elif kind == 4 and i % 12 == 4:
                pk = pubs[(i + 1) % 8]
        pks.append(pk), sigs.append(sig), msgs.append(msg)
    want = np.array([ref.verify(p, s, m) for p, s, m in zip(pks, sigs, msgs)])
    assert 60 < want.sum() < 200
    return pks, sigs, msgs, want


def device_verify(pks, sigs, msgs):
    import torch
    from reticulum_amd import device
    n = len(msgs)
    flat, offs, lens = pack(msgs)
    ok = torch.full((n + 3,), 0xEE, dtype=torch.uint8, device="cuda")
    device.ed25519_verify(torch.from_numpy(u8(b"".join(pks), n, 32)).cuda(), torch.from_numpy(u8(b"".join(sigs), n, 64)).cuda(),
                          torch.from_numpy(flat).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(),
                          torch.from_numpy(lens.astype(np.int32)).cuda(), ok[:n])
    out = ok.cpu().numpy()
    assert (out[n:] == 0xEE).all()                       # nothing written past item n - 1
    assert set(out[:n].tolist()) <= {0, 1}
    return out[:n].astype(bool)


def test_every_fixture_host_and_device():
    from reticulum_amd import ed25519 as ed
    cases = fixture_cases()
    assert len(cases) > 90
    pks, sigs, msgs = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    want = np.array([c[3] for c in cases])
    got = ed.verify_batch(pks, sigs, msgs)
    for c, g in zip(cases, got):
        assert bool(g) == c[3], c[4]
    assert np.array_equal(device_verify(pks, sigs, msgs), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_with_interleaved_outcomes_and_lengths(mixed, n):
    from reticulum_amd import ed25519 as ed
    pks, sigs, msgs, want = mixed
    assert np.array_equal(ed.verify_batch(pks[:n], sigs[:n], msgs[:n]), want[:n])
    if n in (65, 257):
        assert np.array_equal(device_verify(pks[:n], sigs[:n], msgs[:n]), want[:n])


def test_stride0_key_against_70_signatures():
    import torch
    from reticulum_amd import device, ed25519 as ed
    s = ref.vectors()["signatures"][3]
    seed, pk = b(s["seed"]), b(s["public"])
    msgs = [bytes([i]) * (i % 40) for i in range(70)]
    sigs = ed.sign_batch(seed, msgs, public_keys=pk)
    assert sigs[5].tobytes() == ref.sign(seed, msgs[5]) and sigs[69].tobytes() == ref.sign(seed, msgs[69])
    bad = sigs.copy()
    bad[::7, 33] ^= 4
    want = np.ones(70, bool)
    want[::7] = False
    assert ed.verify_batch(pk, sigs, msgs).all()
    assert np.array_equal(ed.verify_batch(pk, bad, msgs), want)
    flat, offs, lens = pack(msgs)
    ok = torch.zeros(70, dtype=torch.uint8, device="cuda")
    one = torch.from_numpy(u8(pk, 1, 32)).cuda()
    args = (torch.from_numpy(bad).cuda(), torch.from_numpy(flat).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(),
            torch.from_numpy(lens.astype(np.int32)).cuda(), ok)
    device.ed25519_verify(one, *args)
    assert np.array_equal(ok.cpu().numpy().astype(bool), want)
    ok.zero_()
    device.ed25519_verify(one.expand(70, 32), *args)
    assert np.array_equal(ok.cpu().numpy().astype(bool), want)


def test_message_offsets_at_every_phase_out_of_order_and_shared():
    lib, ctx = lib_ctx()
    sg = ref.vectors()["signatures"]
    picks = [sg[2], sg[5], sg[8], sg[9], sg[5], sg[0]]          # lengths 31, 48, 65, 111, 48 again, 0
    blob = bytearray(b"\xA5" * 400)
    spots = [301, 2, 107, 188]                                    # offsets = 1, 2, 3, 0 mod 4, not ascending
    assert sorted(o % 4 for o in spots) == [0, 1, 2, 3]
    offs = []
    for s, o in zip(picks[:4], spots):
        m = b(s["msg"])
        blob[o:o + len(m)] = m
        offs.append(o)
    offs += [offs[1], 399]                                        # one offset used twice; an empty message at the end
    offs = np.array(offs, np.uint64)
    lens = np.array([len(b(s["msg"])) for s in picks], np.uint32)
    flat = u8(blob, -1)
    pks = u8(b"".join(b(s["public"]) for s in picks), 6, 32)
    sigs = u8(b"".join(b(s["sig"]) for s in picks), 6, 64)
    ok = np.full(6, 0xEE, np.uint8)
    assert lib.rt_ed25519_verify_host(ctx, ptr(pks), 32, ptr(sigs), 64, ptr(flat), ptr(offs), ptr(lens), ptr(ok), 6) == 0
    assert ok.tolist() == [1] * 6
    flat[offs[2]] ^= 1                                           # damage one message in place
    assert lib.rt_ed25519_verify_host(ctx, ptr(pks), 32, ptr(sigs), 64, ptr(flat), ptr(offs), ptr(lens), ptr(ok), 6) == 0
    assert ok.tolist() == [1, 1, 0, 1, 1, 1]
    # signing reads the same spans
    seeds = u8(b"".join(b(s["seed"]) for s in picks), 6, 32)
    flat[offs[2]] ^= 1
    out = np.full((6, 64), 0xEE, np.uint8)
    assert lib.rt_ed25519_sign_host(ctx, ptr(seeds), 32, None, 0, ptr(flat), ptr(offs), ptr(lens), ptr(out), 64, 6) == 0
    assert np.array_equal(out, sigs)


def test_odd_strides_leave_guard_bytes_untouched():
    import torch
    from reticulum_amd import device
    lib, ctx = lib_ctx()
    sg = ref.vectors()["signatures"][:5]
    n = len(sg)
    msgs = [b(s["msg"]) for s in sg]
    flat, offs, lens = pack(msgs)
    SS, KS, OS = 67, 35, 71
    sigs = np.full((n, SS), 0xEE, np.uint8)
    pks = np.full((n, KS), 0xEE, np.uint8)
    seeds = np.full((n, KS), 0xEE, np.uint8)
    for i, s in enumerate(sg):
        sigs[i, :64], pks[i, :32], seeds[i, :32] = u8(b(s["sig"]), 64), u8(b(s["public"]), 32), u8(b(s["seed"]), 32)
    ok = np.full(n + 4, 0xEE, np.uint8)
    assert lib.rt_ed25519_verify_host(ctx, ptr(pks), KS, ptr(sigs), SS, ptr(flat), ptr(offs), ptr(lens), ptr(ok), n) == 0
    assert ok.tolist() == [1] * n + [0xEE] * 4
    out = np.full((n, OS), 0xEE, np.uint8)
    assert lib.rt_ed25519_sign_host(ctx, ptr(seeds), KS, ptr(pks), KS, ptr(flat), ptr(offs), ptr(lens), ptr(out), OS, n) == 0
    assert np.array_equal(out[:, :64], sigs[:, :64]) and (out[:, 64:] == 0xEE).all()
    pub = np.full((n, KS), 0xEE, np.uint8)
    assert lib.rt_ed25519_public_host(ctx, ptr(seeds), KS, ptr(pub), KS, n) == 0
    assert np.array_equal(pub[:, :32], pks[:, :32]) and (pub[:, 32:] == 0xEE).all()
    # the device forms at the same strides
    d_out = torch.full((n, OS), 0xEE, dtype=torch.uint8, device="cuda")
    d_msg = (torch.from_numpy(flat).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(),
             torch.from_numpy(lens.astype(np.int32)).cuda())
    d_seeds = torch.from_numpy(seeds).cuda()
    device.ed25519_sign(d_seeds[:, :32], *d_msg, d_out[:, :64])
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:, :64], sigs[:, :64]) and (got[:, 64:] == 0xEE).all()
    d_pub = torch.full((n, KS), 0xEE, dtype=torch.uint8, device="cuda")
    device.ed25519_public(d_seeds[:, :32], d_pub[:, :32])
    got = d_pub.cpu().numpy()
    assert np.array_equal(got[:, :32], pks[:, :32]) and (got[:, 32:] == 0xEE).all()
    d_ok = torch.full((n + 4,), 0xEE, dtype=torch.uint8, device="cuda")
    device.ed25519_verify(d_pub[:, :32], torch.from_numpy(sigs).cuda()[:, :64], *d_msg, d_ok[:n])
    assert d_ok.cpu().numpy().tolist() == [1] * n + [0xEE] * 4


def test_sign_and_public_keys_equal_the_fixtures():
    from reticulum_amd import ed25519 as ed
    v = ref.vectors()
    sg = v["signatures"] + [v["selftest"]]
    seeds, msgs = [b(s["seed"]) for s in sg], [b(s["msg"]) for s in sg]
    want = u8(b"".join(b(s["sig"]) for s in sg), len(sg), 64)
    derived = ed.sign_batch(seeds, msgs)
    given = ed.sign_batch(seeds, msgs, public_keys=[b(s["public"]) for s in sg])
    for i, s in enumerate(sg):
        assert derived[i].tobytes().hex() == s["sig"], len(msgs[i])
    assert np.array_equal(given, want)
    assert ed.verify_batch([b(s["public"]) for s in sg], derived, msgs).all()
    pk = v["public_keys"]
    got = ed.public_keys_batch([b(k["seed"]) for k in pk])
    assert [g.tobytes().hex() for g in got] == [k["public"] for k in pk]
    s = v["selftest"]
    assert ed.public_key(b(s["seed"])).hex() == s["public"]
    assert ed.sign(b(s["seed"]), b(s["msg"])).hex() == s["sig"]
    assert ed.verify(b(s["public"]), b(s["sig"]), b(s["msg"])) is True
    assert ed.verify(b(s["public"]), b(s["sig"]), b(s["msg"]) + b"!") is False


def test_argument_errors():
    import torch
    lib, ctx = lib_ctx()
    from reticulum_amd import _native
    n = 2
    pks, sigs, seeds = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8), np.zeros((n, 32), np.uint8)
    flat, offs, lens = np.zeros(8, np.uint8), np.zeros(n, np.uint64), np.array([4, 4], np.uint32)
    ok, out, pub = np.zeros(n, np.uint8), np.zeros((n, 64), np.uint8), np.zeros((n, 32), np.uint8)
    P = ptr

    def v(ctx=ctx, pk=pks, ps=32, sg=sigs, ss=64, m=flat, o=offs, ln=lens, okk=ok, n=n):
        return lib.rt_ed25519_verify_host(ctx, P(pk), ps, P(sg), ss, P(m), P(o), P(ln), P(okk), n)

    def s(ctx=ctx, sd=seeds, sds=32, pk=None, ps=0, m=flat, o=offs, ln=lens, o_=out, os_=64, n=n):
        return lib.rt_ed25519_sign_host(ctx, P(sd), sds, P(pk), ps, P(m), P(o), P(ln), P(o_), os_, n)

    def p(ctx=ctx, sd=seeds, sds=32, o_=pub, os_=32, n=n):
        return lib.rt_ed25519_public_host(ctx, P(sd), sds, P(o_), os_, n)
    bad = [v(ctx=None), v(pk=None), v(sg=None), v(okk=None), v(o=None), v(ln=None), v(ps=31), v(ss=63), v(ss=0), v(m=None),
           s(ctx=None), s(sd=None), s(o_=None), s(o=None), s(ln=None), s(sds=16), s(pk=pks, ps=8), s(os_=63), s(m=None),
           p(ctx=None), p(sd=None), p(o_=None), p(sds=31), p(os_=31)]
    assert bad == [RT_E_INVAL] * len(bad)
    assert v(m=None) == RT_E_INVAL and "null messages" in _native.last_error()
    # n == 0 is RT_OK whatever else is null; msgs NULL is fine when every length is 0
    assert v(pk=None, sg=None, okk=None, n=0) == 0 and s(sd=None, o_=None, n=0) == 0 and p(sd=None, o_=None, n=0) == 0
    zero = np.zeros(n, np.uint32)
    assert v(m=None, ln=zero) == 0 and s(m=None, ln=zero) == 0
    # one item: any stride
    assert v(ss=0, n=1) == 0 and s(os_=0, n=1) == 0 and p(os_=0, n=1) == 0
    # the device forms refuse the same
    d = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dp = ctypes.c_void_p(d.data_ptr())
    assert lib.rt_ed25519_verify(ctx, None, 32, dp, 64, dp, dp, dp, dp, n, None) == RT_E_INVAL
    assert lib.rt_ed25519_verify(ctx, dp, 32, dp, 63, dp, dp, dp, dp, n, None) == RT_E_INVAL
    assert lib.rt_ed25519_verify(ctx, dp, 16, dp, 64, dp, dp, dp, dp, n, None) == RT_E_INVAL
    assert lib.rt_ed25519_verify(ctx, dp, 32, dp, 64, dp, None, dp, dp, n, None) == RT_E_INVAL
    assert lib.rt_ed25519_sign(ctx, dp, 32, None, 0, dp, dp, dp, None, 64, n, None) == RT_E_INVAL
    assert lib.rt_ed25519_sign(ctx, dp, 32, None, 0, dp, dp, dp, dp, 32, n, None) == RT_E_INVAL
    assert lib.rt_ed25519_public(ctx, None, 32, dp, 32, n, None) == RT_E_INVAL
    assert lib.rt_ed25519_public(ctx, dp, 32, dp, 16, n, None) == RT_E_INVAL
    assert lib.rt_ed25519_verify(ctx, None, 0, None, 0, None, None, None, None, 0, None) == 0


def test_identity_layer():
    import reticulum_amd as rt
    v = ref.vectors()
    s = v["signatures"][6]
    seed, pk = b(s["seed"]), b(s["public"])
    msgs = [b"proof %d" % i for i in range(9)] + [b""]
    sigs = rt.sign_batch(seed, msgs)
    assert sigs == [ref.sign(seed, m) for m in msgs]
    assert rt.validate_batch(pk, sigs, msgs) == [True] * 10
    damaged = list(sigs)
    damaged[2] = sigs[2][:63]                                   # 63 bytes: False, no exception
    damaged[4] = sigs[5]
    damaged[7] = sigs[7] + b"\x00"
    assert rt.validate_batch(pk, damaged, msgs) == [True, True, False, True, False, True, True, False, True, True]
    assert rt.validate_batch([pk] * 10, damaged, msgs)[2:5] == [False, True, False]
    ann = v["announces"]
    items = [(b(a["destination_hash"]), a["context_flag"], b(a["data"])) for a in ann]
    got = rt.validate_announces_batch(items)
    got_sig = rt.validate_announces_batch(items, only_validate_signature=True)
    for a, g, gs in zip(ann, got, got_sig):
        assert (g, gs) == (a["ok"], a["ok_signature_only"]), a["note"]
