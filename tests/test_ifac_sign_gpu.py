"""The interface access code on the device: k_ifac_sign in both modes through
device.ifac_sign / ifac_check, wire.transmit_batch / receive_batch and the
pipeline, bit-exact against the fixture recorded from the reference
(tests/golden/ifac_vectors.json) and the tests' big-integer model
(ed25519_ref.sign, tied to the reference by tests/test_ifac_sign.py).  Every
signature of the model is computed once per run (ifac_helpers.signature)."""
import numpy as np
import pytest

import ifac_helpers as ih
from oracle import ctoken
from oracle import wire as ow

pytestmark = pytest.mark.gpu

KEY = bytes((i * 37 + 11) & 0xFF for i in range(64))          # the ifac_key of the tests that need no fixture
GUARD = 0xA5


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _identity(ifac_key):
    """(seed, public key) tensors from the model's own public key."""
    seed = ih.seed_of(ifac_key)
    return _t(np.frombuffer(seed, np.uint8)), _t(np.frombuffer(ih.public_of(seed), np.uint8))


def _layout(msgs, lead=0):
    """Packets end to end after `lead` bytes: (buffer, int64 offsets, int32 lengths)."""
    lens = np.array([len(m) for m in msgs], np.int32)
    off = lead + np.concatenate(([0], np.cumsum(lens[:-1], dtype=np.int64))).astype(np.int64)
    buf = np.frombuffer(bytes(lead) + b"".join(msgs) + b"\x00", np.uint8)
    return buf, off, lens


def _sign(ifac_key, msgs, isz, lead=0):
    """device.ifac_sign over msgs: the (n, isz) codes and the guard row after them."""
    import torch
    from reticulum_amd import device
    seed, pub = _identity(ifac_key)
    buf, off, lens = _layout(msgs, lead)
    n = len(msgs)
    out = torch.full((n + 1, isz), GUARD, dtype=torch.uint8, device=_dev())
    device.ifac_sign(seed, pub, _t(buf), _t(off), _t(lens), out[:n])
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:n], o[n]


def _packets(n, length=86, seed=86):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, 256, length, dtype=np.uint8).tobytes() for _ in range(n)]


# ------------------------------------------------------------ fixture rows --

def test_fixture_rows_sign_transmit_and_receive():
    from reticulum_amd import wire
    v = ih.vectors()
    for isz in (1, 8, 16, 32, 33, 64):
        cases = [c for c in v["cases"] if c["ifac_size"] == isz]
        dropped = [d for d in v["dropped"] if d["ifac_size"] == isz]
        key = bytes.fromhex(cases[0]["ifac_key"])
        raws = [bytes.fromhex(c["raw"]) for c in cases]
        codes, guard = _sign(key, raws, isz)
        assert [codes[i].tobytes().hex() for i in range(len(raws))] == [c["ifac"] for c in cases], isz
        assert (guard == GUARD).all()
        assert [m.hex() for m in wire.transmit_batch(raws, isz, key)] == [c["masked"] for c in cases], isz
        received = [bytes.fromhex(c["masked"]) for c in cases] + [bytes.fromhex(d["received"]) for d in dropped]
        want = [c["inbound_passed"] for c in cases] + [d["inbound_passed"] for d in dropped]
        got = wire.receive_batch(received, isz, key)
        assert [None if g is None else g.hex() for g in got] == want, isz
        assert sum(w is not None for w in want) == 7 and want[len(cases):] == [None] * 4


# ----------------------------------------------------------------- lengths --

@pytest.mark.parametrize("isz", [16, 64])
def test_every_length_and_byte_phase_in_one_launch(isz):
    """Lengths 2..600 end to end: every byte phase, and neighbouring lanes on
    both sides of every SHA-512 block step of r (32 + len: 79|80, 207|208, ...)
    and of h (64 + len: 47|48, 175|176, ...)."""
    rng = np.random.Generator(np.random.PCG64(600))
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in range(2, 601)]
    lens = [len(m) for m in msgs]
    for a in (79, 207, 335, 463, 47, 175, 303, 431, 559):
        assert lens[a - 2] == a and lens[a - 1] == a + 1
    codes, guard = _sign(KEY, msgs, isz, lead=3)
    assert (guard == GUARD).all()
    for i, m in enumerate(msgs):
        assert codes[i].tobytes() == ih.code(KEY, m, isz), len(m)


# ------------------------------------------------------------- batch edges --

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_batch_edges(n):
    msgs = _packets(513)[:n]
    codes, guard = _sign(KEY, msgs, 16)
    assert (guard == GUARD).all()
    for i, m in enumerate(msgs):
        assert codes[i].tobytes() == ih.code(KEY, m, 16), i


@pytest.mark.parametrize("isz", [1, 8, 31, 32, 33, 64])
def test_every_code_width_at_65_packets(isz):
    msgs = _packets(513)[:65]
    codes, guard = _sign(KEY, msgs, isz)
    assert (guard == GUARD).all()
    for i, m in enumerate(msgs):
        assert codes[i].tobytes() == ih.code(KEY, m, isz), i


def test_zero_length_items_are_skipped_and_zeroed():
    """Offsets of empty items point far past the buffer: never dereferenced."""
    import torch
    from reticulum_amd import device
    msgs = _packets(513)[:70]
    buf, off, lens = _layout(msgs)
    empty = np.arange(70) % 5 == 2
    lens = np.where(empty, 0, lens).astype(np.int32)
    off = np.where(empty, 1 << 40, off).astype(np.int64)
    seed, pub = _identity(KEY)
    out = torch.full((71, 16), GUARD, dtype=torch.uint8, device=_dev())
    device.ifac_sign(seed, pub, _t(buf), _t(off), _t(lens), out[:70])
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    for i, m in enumerate(msgs):
        assert o[i].tobytes() == (bytes(16) if empty[i] else ih.code(KEY, m, 16)), i
    assert (o[70] == GUARD).all()


# -------------------------------------------------------------- check mode --

def _check(msgs, codes, lens, off, status, isz, buf):
    import torch
    from reticulum_amd import device
    seed, pub = _identity(KEY)
    t_len, t_st = _t(lens.astype(np.int32)), _t(status.astype(np.int32))
    device.ifac_check(seed, pub, _t(buf), _t(off), t_len, _t(codes), t_st)
    torch.cuda.synchronize()
    return t_len.cpu().numpy(), t_st.cpu().numpy()


@pytest.mark.parametrize("isz", [16, 33])
def test_check_marks_exactly_the_mismatches(isz):
    n = 260
    msgs = _packets(513)[:n]
    buf, off, lens = _layout(msgs)
    buf = buf.copy()
    codes = np.stack([np.frombuffer(ih.code(KEY, m, isz), np.uint8) for m in msgs]).copy()
    status = np.zeros(n, np.int32)
    want_bad = np.zeros(n, bool)
    for i in range(n):
        kind = i % 8
        if kind == 1:
            codes[i, -1] ^= 0x01                                # wrong last byte (in S)
            want_bad[i] = True
        elif kind == 2:
            codes[i, 0] ^= 0x80                                 # wrong first byte (in R where isz is 33)
            want_bad[i] = True
        elif kind == 3:
            buf[off[i] + 40] ^= 0x04                            # body changed after signing
            want_bad[i] = True
        elif kind == 4:
            status[i] = 1                                       # dropped earlier: left alone, code wrong or not
            codes[i, 0] ^= 0xFF
        elif kind == 5:
            lens[i] = 0                                         # no packet: offset far past the buffer
            off[i] = 1 << 40
    got_len, got_st = _check(msgs, codes, lens, off, status, isz, buf)
    assert (got_st == np.where(want_bad, 2, status)).all()
    assert (got_len == np.where(want_bad, 0, lens)).all()
    assert want_bad.sum() >= 90 and (~want_bad).sum() >= 90


@pytest.mark.parametrize("outcome", ["match", "mismatch", "skipped"])
def test_check_whole_waves_of_one_outcome(outcome):
    n, isz = 128, 16
    msgs = _packets(513)[:n]
    buf, off, lens = _layout(msgs)
    codes = np.stack([np.frombuffer(ih.code(KEY, m, isz), np.uint8) for m in msgs]).copy()
    status = np.zeros(n, np.int32)
    if outcome == "mismatch":
        codes[:, 7] ^= 0x20
    elif outcome == "skipped":
        status[:] = 1
        codes[:] = 0
    got_len, got_st = _check(msgs, codes, lens, off, status, isz, buf)
    assert (got_st == (2 if outcome == "mismatch" else status)).all()
    assert (got_len == (0 if outcome == "mismatch" else lens)).all()


# ---------------------------------------------------------------- pipeline --

L = 35                                            # plaintext bytes: a 19 + 96 = 115-byte packet


def _traffic(n, seed=300):
    rng = np.random.Generator(np.random.PCG64(seed))
    key = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    arrs = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, L), (n, 16), (n, 16), (n,))]
    return key, arrs


def _raw_packets(key, arrs):
    pt, iv, dh, ctx = arrs
    return [ow.pack_header(0, 0, dh[i].tobytes(), int(ctx[i])) + ctoken.encrypt(key, iv[i].tobytes(), pt[i].tobytes())
            for i in range(len(pt))]


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", [1, 65, 300])
def test_outbound_makes_the_codes_the_model_makes(n, aligned):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    key, arrs = _traffic(300)
    arrs = [a[:n] for a in arrs]
    raws = _raw_packets(key, arrs)
    assert len(raws[0]) == 115
    codes = np.stack([np.frombuffer(ih.code(KEY, r, 16), np.uint8) for r in raws])
    ks = rt.KeySet(key, device=0)
    ik = _t(np.frombuffer(KEY, np.uint8))
    args = [_t(a) for a in arrs]
    a_s, a_o = pipeline.outbound(ks, *args, _t(codes), ik, aligned=aligned)
    b_s, b_o = pipeline.outbound(ks, *args, ifac_key=ik, ifac_size=16, aligned=aligned)
    torch.cuda.synchronize()
    assert torch.equal(a_o, b_o)
    end = int(a_o[-1])
    assert torch.equal(a_s[:end], b_s[:end])
    assert a_s[:end].cpu().numpy().tobytes() == b"".join(ow.hdlc_frame(ow.ifac_mask(r, c.tobytes(), KEY))
                                                         for r, c in zip(raws, codes))
    with pytest.raises(ValueError, match="64-byte ifac_key"):
        pipeline.outbound(ks, *args, ifac_key=ik[:32], ifac_size=16)


def _forged_stream(n, isz):
    """n honest frames; after every 7th comes a forgery by someone who holds
    the link key and the mask key but not the interface identity: alternately
    the honest packet under a wrong code, and another well-formed packet under
    the honest packet's code.  Both unmask, unpack and decrypt where the code
    is not checked.  Returns (stream, is_forged per frame, key, the plaintext
    each frame carries)."""
    key, arrs = _traffic(n, seed=77)
    raws = _raw_packets(key, arrs)
    _, others = _traffic(n, seed=78)
    other_raws = _raw_packets(key, others)
    parts, forged, pts = [], [], []
    for i, r in enumerate(raws):
        code = ih.code(KEY, r, isz)
        parts.append(ow.hdlc_frame(ow.ifac_mask(r, code, KEY)))
        forged.append(False)
        pts.append(arrs[0][i].tobytes())
        if i % 7 == 3:
            if (i // 7) % 2:
                bad = bytearray(code)
                bad[i % isz] ^= 0x08
                parts.append(ow.hdlc_frame(ow.ifac_mask(r, bytes(bad), KEY)))
                pts.append(arrs[0][i].tobytes())
            else:
                parts.append(ow.hdlc_frame(ow.ifac_mask(other_raws[i], code, KEY)))
                pts.append(others[0][i].tobytes())
            forged.append(True)
    return b"".join(parts), np.array(forged), key, pts


def _same_read(a, b, nf):
    """Two inbound results over the same read agree in everything they define:
    the per-pair arrays up to the pairs found, the per-frame arrays (those past
    the nf frames are empty: status and lengths only) and every plaintext."""
    import torch
    assert set(a) == set(b)
    pairs = int(a["counts"][0])
    assert torch.equal(a["counts"], b["counts"]) and int(a["n_frames"]) == int(b["n_frames"]) == nf
    assert torch.equal(a["frame_status"], b["frame_status"])
    assert torch.equal(a["frame_len"][:pairs], b["frame_len"][:pairs])
    for k in ("ifac_status", "status", "pt_len"):
        assert torch.equal(a[k], b[k]), k
    for k in ("ifac", "fields", "frame_pair", "pt_off"):
        assert torch.equal(a[k][:nf], b[k][:nf]), k
    pa, pb = a["pt"].cpu().numpy(), b["pt"].cpu().numpy()
    po, pl = a["pt_off"].cpu().numpy(), a["pt_len"].cpu().numpy()
    for i in range(nf):
        assert pa[po[i]:po[i] + pl[i]].tobytes() == pb[po[i]:po[i] + pl[i]].tobytes(), i


@pytest.mark.parametrize("aligned", [True, False])
def test_inbound_drops_forged_packets_before_the_token(aligned):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    isz = 16
    stream, forged, key, pts = _forged_stream(100, isz)
    ks = rt.KeySet(key, device=0)
    ik = _t(np.frombuffer(KEY, np.uint8))
    buf = _t(np.frombuffer(stream, np.uint8))
    mp = 2 * len(forged) + 2
    off = pipeline.inbound(ks, buf, ik, isz, mp, aligned=aligned)
    off2 = pipeline.inbound(ks, buf, ik, isz, mp, aligned=aligned, check_ifac=False)
    on = pipeline.inbound(ks, buf, ik, isz, mp, aligned=aligned, check_ifac=True)
    torch.cuda.synchronize()
    nf = len(forged)
    assert int(on["n_frames"]) == int(off["n_frames"]) == nf and forged.sum() == 14
    assert set(off) == set(on) == set(off2)
    # without the check: today's results, forged packets unmasked and handed to the token stage
    assert (off["ifac_status"][:nf] == 0).all() and (off["ifac_status"][nf:] == 1).all()
    assert (off["status"][:nf] == 0).all()
    pt0, po0 = off["pt"].cpu().numpy(), off["pt_off"].cpu().numpy()
    assert all(pt0[po0[i]:po0[i] + L].tobytes() == pts[i] for i in range(nf))
    _same_read(off, off2, nf)
    ist, tst = on["ifac_status"].cpu().numpy(), on["status"].cpu().numpy()
    ok = on["fields"].cpu().numpy()[:, 0]
    assert (ist[:nf] == np.where(forged, 2, 0)).all() and (ist[nf:] == 1).all()
    assert (ok[:nf] == np.where(forged, 0, 1)).all()
    assert (tst[:nf][forged] != 0).all() and (tst[:nf][~forged] == 0).all()
    pt, po, pl = on["pt"].cpu().numpy(), on["pt_off"].cpu().numpy(), on["pt_len"].cpu().numpy()
    for i in range(nf):
        if forged[i]:
            # nothing of a forged packet is decrypted: no length, and where the
            # unchecked run puts this frame's plaintext the checked run has none
            assert pl[i] == 0
            assert pt[po0[i]:po0[i] + L].tobytes() != pts[i], i
        else:
            assert pl[i] == L and pt[po[i]:po[i] + L].tobytes() == pts[i], i
    honest = _t(np.flatnonzero(~forged))
    for k in ("ifac", "fields", "status", "pt_len", "pt_off"):
        assert torch.equal(on[k][honest], off[k][honest]), k


def test_inbound_without_ifac_and_empty_read_ignore_the_check():
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    key, arrs = _traffic(20, seed=5)
    ks = rt.KeySet(key, device=0)
    ik = _t(np.frombuffer(KEY, np.uint8))
    framed, foff = pipeline.outbound(ks, *[_t(a) for a in arrs], None, ik)
    stream = framed[:int(foff[-1])]
    a = pipeline.inbound(ks, stream, ik, 0, 50, check_ifac=True)
    b = pipeline.inbound(ks, stream, ik, 0, 50)
    torch.cuda.synchronize()
    _same_read(a, b, 20)
    assert int(a["n_frames"]) == 20 and (a["status"][:20] == 0).all()
    for isz in (0, 16):
        e = pipeline.inbound(ks, torch.empty(0, dtype=torch.uint8, device=_dev()), ik, isz, 4, check_ifac=True)
        torch.cuda.synchronize()
        assert int(e["n_frames"]) == 0 and (e["ifac_status"].cpu() == 1).all() and (e["status"].cpu() == 1).all()
        assert (e["pt_len"].cpu() == 0).all()


def test_device_calls_check_their_arguments():
    import torch
    from reticulum_amd import device
    seed, pub = _identity(KEY)
    buf, off, lens = _layout(_packets(513)[:4])
    good = dict(pkt=_t(buf), pkt_off=_t(off), pkt_len=_t(lens))
    out = torch.zeros((4, 16), dtype=torch.uint8, device=_dev())
    with pytest.raises(ValueError):
        device.ifac_sign(seed[:31], pub, ifac_out=out, **good)
    with pytest.raises(ValueError):
        device.ifac_sign(seed, pub, ifac_out=torch.zeros((4, 65), dtype=torch.uint8, device=_dev()), **good)
    with pytest.raises(ValueError):
        device.ifac_sign(seed, pub, ifac_out=out[:3], **good)
    with pytest.raises(ValueError):
        device.ifac_sign(seed, pub, ifac_out=out, pkt=good["pkt"], pkt_off=good["pkt_off"],
                         pkt_len=good["pkt_len"].to(torch.int64))
    with pytest.raises(ValueError):
        device.ifac_check(seed, pub, good["pkt"], good["pkt_off"], good["pkt_len"], out,
                          torch.zeros(3, dtype=torch.int32, device=_dev()))
