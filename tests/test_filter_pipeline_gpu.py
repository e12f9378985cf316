"""pipeline.inbound(seen=list): Transport's packet filter between unpack and
dispatch.  One byte stream over five links in which every packet comes twice
with a copy for another transport node in between; the same stream read a
second time; the path without a list against today's; and an interface with
the access-code check on, where forged packets never reach the list."""
import numpy as np
import pytest

import filter_helpers as fh
import ifac_helpers as ih
import link_helpers as lh
from oracle import ctoken
from oracle import wire as ow

pytestmark = pytest.mark.gpu

ISZ = 16
OWN = bytes(range(7, 23))
TOO_SHORT = 1          # RT_ST_TOO_SHORT


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def stream_case():
    """40 link packets; on the wire: the packet, a HEADER_2 copy for a foreign
    transport node, the packet again, and now and then the HEADER_2 copy
    addressed to this node."""
    import reticulum_amd as rt
    rng = np.random.Generator(np.random.PCG64(1525))
    keys = rng.integers(0, 256, (5, 64), dtype=np.uint8)
    link_ids = [_rb(rng, 16) for _ in range(5)]
    values = [2, 4, 0, 3, 1]
    ifac_key = _rb(rng, 64)
    ks = rt.KeySet(keys, device=0)
    tab = rt.LinkTable(8, device=0)
    assert tab.insert(link_ids, values).cpu().tolist() == [lh.OK] * 5
    link_data = lh.LINK << 2 | lh.DATA
    raws, kinds = [], []
    for k in range(40):
        j = k % 5
        ctx = (lh.NONE, lh.REQUEST, lh.CHANNEL, lh.KEEPALIVE)[k % 4 if k % 8 else 0]
        data = b"\xFF" if ctx == lh.KEEPALIVE else \
            ctoken.encrypt(keys[values[j]].tobytes(), _rb(rng, 16), _rb(rng, 20 + 9 * k))
        body = link_ids[j] + bytes([ctx]) + data
        plain = bytes([link_data, 0]) + body
        foreign = bytes([0x40 | 0x10 | link_data, 2]) + _rb(rng, 16) + body
        mine = bytes([0x40 | 0x10 | link_data, 1]) + OWN + body
        for kind, raw in (("first", plain), ("foreign", foreign), ("second", plain)) + \
                ((("relayed", mine),) if k % 7 == 3 else ()):
            raws.append(raw)
            kinds.append(kind)
    wire = b"".join(ow.hdlc_frame(ow.ifac_mask(raw, _rb(rng, ISZ), ifac_key)) for raw in raws)
    return ks, tab, keys, dict(zip(link_ids, values)), ifac_key, raws, kinds, wire


def _model_packet(raw):
    f = ow.unpack(raw)
    return f, fh.packet(f["packet_hash"], f["packet_type"], f["destination_type"], f["context"], f["hops"],
                        f["header_type"], f.get("transport_id") or b"", f["destination_hash"])


@pytest.mark.parametrize("aligned", [True, False])
def test_replayed_packets_are_dropped_before_dispatch(stream_case, aligned):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    ks, tab, keys, table, ifac_key, raws, kinds, wire = stream_case
    n = len(raws)
    buf = torch.frombuffer(bytearray(wire), dtype=torch.uint8).to("cuda:0")
    ik, own = _t(np.frombuffer(ifac_key, np.uint8)), _t(np.frombuffer(OWN, np.uint8))
    seen = rt.PacketHashlist(4096, device=0)
    model = fh.ListModel(4096, OWN)
    res = pipeline.inbound(ks, buf, ik, ISZ, 2 * n, aligned=aligned, links=tab, seen=seen, transport_identity=own)
    torch.cuda.synchronize()
    assert int(res["n_frames"]) == n
    fstat, status, ok = (res[k].cpu().numpy() for k in ("filter_status", "status", "fields"))
    ok = ok[:, 0]
    route, pt_len, pt_off, pt = (res[k].cpu().numpy() for k in ("route", "pt_len", "pt_off", "pt"))
    want = []
    for i, raw in enumerate(raws):
        f, p = _model_packet(raw)
        assert f["packet_hash"] == bytes(res["fields"][i, 52:84].cpu().numpy())
        st = model.packet(p)[0]
        want.append(st)
        assert fstat[i] == st and ok[i] == (st == fh.PASS), (i, kinds[i], fstat[i], st)
        if st != fh.PASS:
            # dropped like every other dropped packet: no link, an empty span, nothing decrypted
            assert (route[i], status[i], pt_len[i]) == (lh.NOT_LINK, TOO_SHORT, 0), (i, kinds[i])
            continue
        r, lk, dec = lh.route(True, f["destination_type"], f["packet_type"], f["context"],
                              table.get(f["destination_hash"]), n_keys=5)
        assert route[i] == r
        if dec:
            st_tok, plain = ctoken.decrypt(keys[lk].tobytes(), f["data"])
            assert st_tok == 0 and status[i] == 0 and pt[pt_off[i]:pt_off[i] + pt_len[i]].tobytes() == plain, i
        else:
            assert status[i] == TOO_SHORT and pt_len[i] == 0
    # KEEPALIVE and CHANNEL never consult the list, so their copies pass; every other copy is a duplicate
    free = [ow.unpack(raw)["context"] in fh.ALWAYS for raw in raws]
    for w, kind, fr in zip(want, kinds, free):
        assert w == {"first": fh.PASS, "foreign": fh.OTHER_TRANSPORT}.get(kind, fh.PASS if fr else fh.DUPLICATE)
    copies = sum(1 for kind, fr in zip(kinds, free) if kind in ("second", "relayed") and not fr)
    assert want.count(fh.DUPLICATE) == copies > 20 and any(free)
    assert (fstat[n:] == fh.NO_PACKET).all() and (status[n:] == TOO_SHORT).all()
    # every hash was remembered once (the keepalives of one link are one packet, so one hash)
    assert seen.counts() == model.counts() == (len({ow.unpack(raw)["packet_hash"] for raw in raws}), 0, 0)

    # the same stream read a second time is dropped whole (but for the packets that never consult the list)
    res2 = pipeline.inbound(ks, buf, ik, ISZ, 2 * n, aligned=aligned, links=tab, seen=seen, transport_identity=own)
    torch.cuda.synchronize()
    want2 = [model.packet(_model_packet(raw)[1])[0] for raw in raws]
    assert res2["filter_status"].cpu().tolist()[:n] == want2
    assert all(w == (fh.OTHER_TRANSPORT if kind == "foreign" else fh.PASS if fr else fh.DUPLICATE)
               for w, kind, fr in zip(want2, kinds, free))
    st2, len2 = res2["status"].cpu().numpy(), res2["pt_len"].cpu().numpy()
    gone = np.array(want2) != fh.PASS
    assert (st2[:n][gone] == TOO_SHORT).all() and (len2[:n][gone] == 0).all() and (st2[n:] == TOO_SHORT).all()
    assert seen.counts() == model.counts()

    # without links: the filter feeds token_spans the same way
    seen3 = rt.PacketHashlist(64, device=0)
    res3 = pipeline.inbound(ks, buf, ik, ISZ, 2 * n, aligned=aligned, seen=seen3, transport_identity=own)
    assert res3["filter_status"].cpu().tolist()[:n] == want
    dropped = np.array(want) != fh.PASS
    assert (res3["status"].cpu().numpy()[:n][dropped] == TOO_SHORT).all()
    assert (res3["pt_len"].cpu().numpy()[:n][~dropped] >= 0).all() and "route" not in res3


def test_without_a_list_the_path_is_the_parents(stream_case):
    """seen=None takes none of the new code: same keys in the result, same
    tensors as a second run of the same call, and the statuses a list-less
    model gives (every copy decrypts)."""
    import torch
    from reticulum_amd import pipeline
    ks, tab, keys, table, ifac_key, raws, kinds, wire = stream_case
    n = len(raws)
    buf = torch.frombuffer(bytearray(wire), dtype=torch.uint8).to("cuda:0")
    ik = _t(np.frombuffer(ifac_key, np.uint8))
    a = pipeline.inbound(ks, buf, ik, ISZ, 2 * n, links=tab)
    b = pipeline.inbound(ks, buf, ik, ISZ, 2 * n, links=tab, seen=None, transport_identity=None, transit=None)
    assert set(a) == set(b) == {"pt", "pt_off", "pt_len", "status", "ifac", "ifac_status", "fields", "frame_pair",
                                "n_frames", "frame_status", "frame_len", "counts", "route", "link", "key_idx"}
    for k in ("pt_off", "pt_len", "status", "fields", "route", "link", "key_idx", "frame_pair"):
        assert torch.equal(a[k][:n], b[k][:n]), k
    assert torch.equal(a["counts"], b["counts"]) and int(a["n_frames"]) == int(b["n_frames"]) == n
    status, route, ok = a["status"].cpu().numpy(), a["route"].cpu().numpy(), a["fields"].cpu().numpy()[:, 0]
    for i, raw in enumerate(raws):
        f = ow.unpack(raw)
        r, lk, dec = lh.route(True, f["destination_type"], f["packet_type"], f["context"],
                              table.get(f["destination_hash"]), n_keys=5)
        assert ok[i] == 1 and route[i] == r and status[i] == (0 if dec else TOO_SHORT), (i, kinds[i])


def test_forged_packets_never_reach_the_list():
    """check_ifac on: a packet whose access code is not the interface's
    signature is dropped before unpack, so its hash is not remembered and the
    genuine packet that follows is not a duplicate."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    rng = np.random.Generator(np.random.PCG64(1470))
    ifac_key = _rb(rng, 64)
    key = rng.integers(0, 256, (1, 64), dtype=np.uint8)
    ks = rt.KeySet(key, device=0)
    raws, forged, codes = [], [], []
    for k in range(6):
        raw = ow.pack_header(lh.SINGLE << 2 | lh.DATA, 0, _rb(rng, 16), 0) + \
            ctoken.encrypt(key[0].tobytes(), _rb(rng, 16), _rb(rng, 30 + k))
        code = ih.code(ifac_key, raw, ISZ)
        bad = bytes([code[0] ^ 1]) + code[1:]
        # forged first, then the genuine packet, then the genuine packet replayed
        for c in (bad, code, code) if k % 2 == 0 else (code, bad, code):
            raws.append(raw)
            forged.append(c is bad)
            codes.append(c)
    wire = b"".join(ow.hdlc_frame(ow.ifac_mask(raw, c, ifac_key)) for raw, c in zip(raws, codes))
    n = len(raws)
    buf = torch.frombuffer(bytearray(wire), dtype=torch.uint8).to("cuda:0")
    seen = rt.PacketHashlist(64, device=0)
    res = pipeline.inbound(ks, buf, _t(np.frombuffer(ifac_key, np.uint8)), ISZ, 2 * n, check_ifac=True, seen=seen,
                           transport_identity=_t(np.frombuffer(OWN, np.uint8)))
    torch.cuda.synchronize()
    assert int(res["n_frames"]) == n
    model = fh.ListModel(64, OWN)
    want = [fh.NO_PACKET if f else model.packet(_model_packet(raw)[1])[0] for raw, f in zip(raws, forged)]
    assert res["filter_status"].cpu().tolist()[:n] == want
    assert res["ifac_status"].cpu().tolist()[:n] == [2 if f else 0 for f in forged]
    assert want.count(fh.PASS) == 6 and want.count(fh.DUPLICATE) == 6 and want.count(fh.NO_PACKET) == 6
    assert res["status"].cpu().tolist()[:n] == [0 if w == fh.PASS else TOO_SHORT for w in want]
    assert seen.counts() == (6, 0, 0)
    # without the check the forged copy comes first into the list and the genuine one is the duplicate
    seen2 = rt.PacketHashlist(64, device=0)
    res = pipeline.inbound(ks, buf, _t(np.frombuffer(ifac_key, np.uint8)), ISZ, 2 * n, seen=seen2,
                           transport_identity=_t(np.frombuffer(OWN, np.uint8)))
    assert res["filter_status"].cpu().tolist()[:n] == [fh.PASS, fh.DUPLICATE, fh.DUPLICATE] * 6
