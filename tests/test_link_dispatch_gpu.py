"""Link dispatch on the device: rt_link_spans (k_link_spans) against the route
rule of tests/link_helpers.py for every (packet type, destination type) pair,
every context 0..255, hits and misses, failed unpacks and HEADER_2 packets at
the batch edges; pipeline.inbound(links=table) over one stream of five
interleaved links against the model plus the C oracle's decrypt under each
link's key; derive_link_keys against the reference's recorded handshakes."""
import numpy as np
import pytest

import link_helpers as lh
from oracle import ctoken
from oracle import wire as ow

pytestmark = pytest.mark.gpu

BATCHES = (0, 1, 63, 64, 65, 255, 256, 257)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ------------------------------------------------------------- link_spans --

@pytest.fixture(scope="module")
def span_case():
    """A table of 5 links and a shuffled list of packets that covers the
    route rule; unpacked once on the device."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    rng = np.random.Generator(np.random.PCG64(2161))
    link_ids = [_rb(rng, 16) for _ in range(5)]
    values = [3, 0, 4, 1, 2]
    tab = rt.LinkTable(32, device=0)
    assert tab.insert(link_ids, values).cpu().tolist() == [lh.OK] * 5
    table = dict(zip(link_ids, values))
    raws = []
    for ptype in range(4):
        for dtype in range(4):
            for ctx in (0x00, 0x01, 0xFA):
                for known in (True, False):
                    dh = link_ids[len(raws) % 5] if known else _rb(rng, 16)
                    raws.append(ow.pack_header(dtype << 2 | ptype, 1, dh, ctx) + _rb(rng, 80))
    for ctx in range(256):
        for known in (True, False):
            dh = link_ids[ctx % 5] if known else _rb(rng, 16)
            raws.append(ow.pack_header(lh.LINK << 2 | lh.DATA, ctx % 128, dh, ctx) + _rb(rng, 64 + ctx % 3))
        raws.append(ow.pack_header(lh.LINK << 2 | lh.PROOF, 0, link_ids[ctx % 5], ctx) + _rb(rng, 64))
    for i in range(24):                  # HEADER_2: the destination follows the transport id
        ctx = (0x00, 0x0E, 0xFC, 0x01, 0x0B, 0xFD)[i % 6]
        dh = link_ids[i % 5] if i % 4 else _rb(rng, 16)
        raws.append(ow.pack_header(0x40 | 0x10 | lh.LINK << 2 | (lh.PROOF if i % 7 == 6 else lh.DATA), 2, dh, ctx,
                                   transport_id=_rb(rng, 16)) + _rb(rng, 70))
    for i in range(8):                   # failed unpacks: too short for the header, hop count too high
        head = ow.pack_header(lh.LINK << 2, 0, link_ids[i % 5], 0)
        raws += [b"", head[:1], head[:18], bytes([head[0], 128 + i]) + head[2:] + _rb(rng, 64),
                 (ow.pack_header(0x40 | lh.LINK << 2, 0, link_ids[0], 0, transport_id=_rb(rng, 16)))[:34]]
    order = rng.permutation(len(raws))
    raws = [raws[k] for k in order]
    off = np.cumsum([0] + [len(r) + 5 for r in raws])[:-1].astype(np.int64)
    flat = np.zeros(int(off[-1]) + len(raws[-1]) + 5, dtype=np.uint8)
    for o, r in zip(off, raws):
        flat[o:o + len(r)] = np.frombuffer(r, np.uint8)
    n = len(raws)
    fields = torch.empty((n, 96), dtype=torch.uint8, device="cuda:0")
    device.packet_unpack(_t(flat), _t(off), _t(np.array([len(r) for r in raws], np.int32)), fields)
    want = []
    for o, r in zip(off, raws):
        f = ow.unpack(r)
        value = table.get(f["destination_hash"]) if f else None
        route, link, dec = lh.route(f is not None, f and f["destination_type"], f and f["packet_type"],
                                    f and f["context"], value, n_keys=5)
        want.append((route, link, int(o) + (f["data_offset"] if dec else 0), len(f["data"]) if dec else 0,
                     link if dec else 0))
    assert {w[0] for w in want} == {0, 1, 2, 3}
    return tab, fields, _t(off), want


@pytest.mark.parametrize("n", BATCHES)
def test_link_spans_follow_the_route_rule(span_case, n):
    import torch
    from reticulum_amd import device
    tab, fields, off, want = span_case
    total = len(want)
    # the first n packets and the last n of the shuffled list
    for lo in (0, total - n):
        tok_off = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
        tok_len, key_idx, link = (torch.full((n,), -7, dtype=torch.int32, device="cuda:0") for _ in range(3))
        route = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
        device.link_spans(tab.handle, fields[lo:lo + n], off[lo:lo + n], 5, tok_off, tok_len, key_idx, link, route)
        got = list(zip(route.cpu().tolist(), link.cpu().tolist(), tok_off.cpu().tolist(), tok_len.cpu().tolist(),
                       key_idx.cpu().tolist()))
        assert got == want[lo:lo + n]


def test_link_spans_whole_list_and_the_key_bound(span_case):
    import torch
    from reticulum_amd import device
    tab, fields, off, want = span_case
    n = len(want)
    outs = [torch.empty(n, dtype=torch.int64, device="cuda:0")] + \
           [torch.empty(n, dtype=torch.int32, device="cuda:0") for _ in range(3)] + \
           [torch.empty(n, dtype=torch.uint8, device="cuda:0")]
    device.link_spans(tab.handle, fields, off, 5, *outs)
    got = list(zip(outs[4].cpu().tolist(), outs[3].cpu().tolist(), outs[0].cpu().tolist(), outs[1].cpu().tolist(),
                   outs[2].cpu().tolist()))
    assert got == want
    # a key set of 3 keys: links 3 and 4 are found but never decrypted
    device.link_spans(tab.handle, fields, off, 3, *outs)
    route, link, key = outs[4].cpu().numpy(), outs[3].cpu().numpy(), outs[2].cpu().numpy()
    w = np.array([x[0] for x in want])
    assert ((route == w) | ((w == 3) & (link >= 3) & (route == 2))).all() and (key < 3).all()
    assert ((route == 2) & (w == 3)).any() and (outs[1].cpu().numpy()[(w == 3) & (link >= 3)] == 0).all()
    with pytest.raises(ValueError):
        device.link_spans(tab.handle, fields, off[:5], 5, *outs)
    with pytest.raises(ValueError):
        device.link_spans(tab.handle, fields, off, 5, outs[0], outs[1], outs[2], outs[3].long(), outs[4])


# ------------------------------------------------------- pipeline.inbound --

L, ISZ = 100, 16


@pytest.fixture(scope="module")
def stream_case():
    """One byte stream of about 300 frames on 5 links, most of it from
    pipeline.outbound(key_idx=...), the rest packed by hand."""
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    rng = np.random.Generator(np.random.PCG64(941))
    keys = rng.integers(0, 256, (5, 64), dtype=np.uint8)
    link_ids = [_rb(rng, 16) for _ in range(5)]
    values = [2, 4, 0, 3, 1]                      # link j decrypts under key values[j]
    ifac_key = _rb(rng, 64)
    ks = rt.KeySet(keys, device=0)
    tab = rt.LinkTable(8, device=0)
    assert tab.insert(link_ids, values).cpu().tolist() == [lh.OK] * 5

    n = 290
    pt = rng.integers(0, 256, (n, L), dtype=np.uint8)
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ifac = rng.integers(0, 256, (n, ISZ), dtype=np.uint8)
    which = np.arange(n) % 5                      # links interleaved
    rng.shuffle(which[100:])
    ctxs = np.array(sorted(lh.DECRYPTED), dtype=np.uint8)[rng.integers(0, 12, n)]
    flags = np.full(n, lh.LINK << 2 | lh.DATA, dtype=np.uint8)
    dh = np.stack([np.frombuffer(link_ids[j], np.uint8) for j in which]).copy()
    key_idx = np.array([values[j] for j in which], dtype=np.int32)
    dh[17] = np.frombuffer(_rb(rng, 16), np.uint8)          # an unknown link id
    flags[40] = lh.SINGLE << 2 | lh.DATA                    # a SINGLE-destination packet
    ctxs[63], ctxs[64] = lh.KEEPALIVE, lh.RESOURCE          # contexts Link.receive does not decrypt
    ctxs[65], ctxs[128] = 0x0B, lh.CACHE_REQUEST
    # a valid token sent under another link's id: the key follows the id, so its tag fails
    key_idx[90] = values[(which[90] + 1) % 5]
    key_idx[255] = values[(which[255] + 3) % 5]
    framed, foff = pipeline.outbound(ks, _t(pt), _t(iv), _t(dh), _t(ctxs), _t(ifac),
                                     _t(np.frombuffer(ifac_key, np.uint8)), flags=_t(flags), key_idx=_t(key_idx))
    fo = foff.cpu().numpy()
    wire = framed[:int(fo[-1])].cpu().numpy().tobytes()
    frames = [wire[fo[i]:fo[i + 1]] for i in range(n)]
    raws = [ow.pack_header(int(flags[i]), 0, dh[i].tobytes(), int(ctxs[i])) +
            ctoken.encrypt(keys[key_idx[i]].tobytes(), iv[i].tobytes(), pt[i].tobytes()) for i in range(n)]

    def by_hand(raw):
        return raw, ow.hdlc_frame(ow.ifac_mask(raw, _rb(rng, ISZ), ifac_key))

    def token(j, plain):
        return ctoken.encrypt(keys[values[j]].tobytes(), _rb(rng, 16), plain)

    link_data = lh.LINK << 2 | lh.DATA
    tampered = bytearray(token(3, _rb(rng, 77)))
    tampered[30] ^= 0x40
    hand = [
        ow.pack_header(link_data, 0, link_ids[1], lh.KEEPALIVE) + b"\xFF",
        ow.pack_header(link_data, 0, link_ids[2], lh.RESOURCE) + _rb(rng, 200),
        ow.pack_header(lh.LINK << 2 | lh.PROOF, 0, link_ids[0], lh.RESOURCE_PRF) + _rb(rng, 64),
        ow.pack_header(link_data, 0, link_ids[3], lh.NONE) + bytes(tampered),
        ow.pack_header(link_data, 3, link_ids[4], lh.CHANNEL) + token(4, b""),
        ow.pack_header(0x40 | 0x10 | link_data, 5, link_ids[0], lh.REQUEST, transport_id=_rb(rng, 16)) +
        token(0, _rb(rng, 383)),
        ow.pack_header(link_data, 0, link_ids[2], lh.LINKCLOSE) + token(2, link_ids[2])[:-1],      # a byte short
    ]
    for k, raw in enumerate(hand):             # spread through the stream
        raw, frame = by_hand(raw)
        at = 11 + 43 * k
        raws.insert(at, raw)
        frames.insert(at, frame)
    table = dict(zip(link_ids, values))
    return ks, tab, keys, table, ifac_key, raws, b"".join(frames)


@pytest.mark.parametrize("aligned", [True, False])
def test_inbound_dispatches_every_packet_to_its_link(stream_case, aligned):
    import torch
    from reticulum_amd import pipeline
    ks, tab, keys, table, ifac_key, raws, wire = stream_case
    n = len(raws)
    assert n == 297
    buf = torch.frombuffer(bytearray(wire), dtype=torch.uint8).to("cuda:0")
    ik = _t(np.frombuffer(ifac_key, np.uint8))
    res = pipeline.inbound(ks, buf, ik, ISZ, 2 * n, aligned=aligned, links=tab)
    torch.cuda.synchronize()
    assert int(res["n_frames"]) == n
    route, link, key_idx = (res[k].cpu().numpy() for k in ("route", "link", "key_idx"))
    status, pt_len, pt_off = (res[k].cpu().numpy() for k in ("status", "pt_len", "pt_off"))
    pt = res["pt"].cpu().numpy()
    seen = set()
    for i, raw in enumerate(raws):
        f = ow.unpack(raw)
        r, lk, dec = lh.route(True, f["destination_type"], f["packet_type"], f["context"],
                              table.get(f["destination_hash"]), n_keys=5)
        assert (route[i], link[i], key_idx[i]) == (r, lk, lk if dec else 0), i
        if dec:
            st, plain = ctoken.decrypt(keys[lk].tobytes(), f["data"])
            plain = plain or b""
        else:
            st, plain = 1, b""                   # RT_ST_TOO_SHORT: never decrypted
        assert status[i] == st, (i, r, status[i], st)
        assert pt_len[i] == len(plain) and pt[pt_off[i]:pt_off[i] + len(plain)].tobytes() == plain, i
        seen.add((r, int(st)))
    # every kind of packet the stream was built to hold is there
    assert {(0, 1), (1, 1), (2, 1), (3, 0), (3, 2)} <= seen
    assert (route[n:] == 0).all() and (link[n:] == -1).all() and (status[n:] == 1).all()

    # the same stream without a table: today's result, every packet under key 0
    old = pipeline.inbound(ks, buf, ik, ISZ, 2 * n, aligned=aligned)
    assert set(old) == set(res) - {"route", "link", "key_idx"}
    o_status, o_len, o_off = (old[k].cpu().numpy() for k in ("status", "pt_len", "pt_off"))
    o_pt = old["pt"].cpu().numpy()
    for i, raw in enumerate(raws):
        st, plain = ctoken.decrypt(keys[0].tobytes(), ow.unpack(raw)["data"])
        assert o_status[i] == st and o_len[i] == len(plain or b""), i
        if st == 0:
            assert o_pt[o_off[i]:o_off[i] + len(plain)].tobytes() == plain
    for k in ("fields", "ifac", "ifac_status", "frame_pair"):          # per frame; `ifac` is unwritten past them
        assert torch.equal(old[k][:n], res[k][:n]), k
    pairs = int(res["counts"][0])
    assert pairs == 2 * n - 1 and torch.equal(old["counts"], res["counts"])
    for k in ("frame_status", "frame_len"):                            # per flag pair found
        assert torch.equal(old[k][:pairs], res[k][:pairs]), k


# ------------------------------------------------------- derive_link_keys --

@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_derive_link_keys_gives_the_references_handshake_keys(mode, n):
    import reticulum_amd as rt
    hs = [h for h in lh.vectors()["handshakes"] if h["mode"] == mode]
    assert len(hs) >= 3
    rows = [hs[(i * 2 + i // len(hs)) % len(hs)] for i in range(n)]
    ks = rt.derive_link_keys([bytes.fromhex(h["private"]) for h in rows],
                             [bytes.fromhex(h["peer_public"]) for h in rows],
                             [bytes.fromhex(h["link_id"]) for h in rows], mode=mode, device=0)
    assert ks.n_keys == n and ks.key_len == (64 if mode == 1 else 32)
    rng = np.random.Generator(np.random.PCG64(n + mode))
    pts = [_rb(rng, int(rng.integers(0, 200))) for _ in range(n)]
    ivs = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    toks = ks.encrypt_batch(pts, ivs=ivs, key_idx=np.arange(n, dtype=np.uint32))
    for i, h in enumerate(rows):
        assert toks[i] == ctoken.encrypt(bytes.fromhex(h["derived_key"]), ivs[i].tobytes(), pts[i]), i
