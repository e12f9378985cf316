"""pipeline.inbound(links, signers, receipts): packet proofs inside the read.

One framed stream of about 300 packets over five links: DATA packets built by
pipeline.outbound(key_idx=...) with contexts NONE, CHANNEL and KEEPALIVE, some
under another link's key (a forged token), interleaved with proofs for
receipts added beforehand, good ones and every kind of bad one.  The read is
held to the model of tests/proof_helpers.py, which test_proof.py ties to the
reference; the same stream is read twice through a packet hash list; and the
call without the new arguments is compared with the same call beside it."""
import numpy as np
import pytest

import ed25519_ref as ed
import filter_helpers as fh
import link_helpers as lh
import proof_helpers as ph
from oracle import ctoken
from oracle import wire as ow

pytestmark = pytest.mark.gpu

OWN = bytes(range(11, 27))
VALUES = [2, 4, 0, 3, 1]                 # link j -> the row of its key and of its signing rows
FLAGS = [ph.PROVE_ALL | ph.HAS_CHANNEL, ph.PROVE_ALL, 0, ph.HAS_CHANNEL, ph.PROVE_ALL]     # by row
N_DATA, PT_LEN, N_RECEIPTS = 240, 37, 32


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def case():
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    rng = np.random.Generator(np.random.PCG64(943))
    keys = rng.integers(0, 256, (5, 64), dtype=np.uint8)
    link_ids = [_rb(rng, 16) for _ in range(5)]
    seeds = [_rb(rng, 32) for _ in range(5)]                    # by row
    peer_seeds = [_rb(rng, 32) for _ in range(5)]
    ks = rt.KeySet(keys, device=0)
    tab = rt.LinkTable(8, device=0)
    assert tab.insert(link_ids, VALUES).cpu().tolist() == [lh.OK] * 5
    peers = [ph.public_key(s) for s in peer_seeds]
    signers = rt.LinkSigners(seeds, peers, FLAGS, device=0)
    model = ph.Signers(seeds, peers, FLAGS)

    # the DATA packets, sent on five links in one call; every eighth under the next link's key
    j = np.arange(N_DATA) % 5
    context = np.array([(lh.NONE, lh.CHANNEL, lh.NONE, lh.KEEPALIVE, lh.CHANNEL, lh.NONE)[i % 6] for i in range(N_DATA)],
                       np.uint8)
    forged = np.arange(N_DATA) % 8 == 5
    key_idx = np.where(forged, np.array(VALUES)[(j + 1) % 5], np.array(VALUES)[j]).astype(np.int32)
    framed, frame_off = pipeline.outbound(
        ks, _t(rng.integers(0, 256, (N_DATA, PT_LEN), dtype=np.uint8)),
        _t(rng.integers(0, 256, (N_DATA, 16), dtype=np.uint8)),
        _t(np.frombuffer(b"".join(link_ids[k] for k in j), np.uint8).reshape(N_DATA, 16)), _t(context),
        flags=_t(np.full(N_DATA, lh.LINK << 2 | lh.DATA, np.uint8)), key_idx=_t(key_idx))
    torch.cuda.synchronize()
    off = frame_off.cpu().numpy()
    wire = framed.cpu().numpy().tobytes()
    data_frames = [wire[off[i]:off[i + 1]] for i in range(N_DATA)]

    # the proofs that come back: receipt r was sent on link r % 5
    hashes = [_rb(rng, 32) for _ in range(N_RECEIPTS)]

    def proof(r, signer=None, h=None, context=lh.NONE, tail=b""):
        k = r % 5
        h = hashes[r] if h is None else h
        sig = ph.sign(peer_seeds[VALUES[k] if signer is None else signer], h)
        return bytes([lh.LINK << 2 | lh.PROOF, 0]) + link_ids[k] + bytes([context]) + h + sig + tail

    proofs = []
    for r in range(N_RECEIPTS - 4):          # the last four receipts stay outstanding
        kind = r % 7
        if kind == 3:
            proofs.append(proof(r, signer=(VALUES[r % 5] + 1) % 5))                # a bad signature first
        if kind == 4:
            proofs.append(proof(r, h=hashes[r][:16] + _rb(rng, 16)))               # 16 bytes agree
        if kind == 5:
            proofs.append(proof(r, context=ph.LRPROOF))
        proofs.append(proof(r, tail=_rb(rng, r % 3)))
        if kind == 6:
            proofs.append(proofs[-1])                                              # the same proof again
    proofs.append(proof(3, h=_rb(rng, 32)))                                        # a hash no receipt holds
    proofs.append(proof(2)[:19 + 90])                                              # short
    frames, at = [], 0
    for i, f in enumerate(data_frames):
        frames.append(f)
        if i % 5 == 2 and at < len(proofs):
            frames.append(ow.hdlc_frame(proofs[at]))
            at += 1
    assert at == len(proofs) and 280 <= len(frames) <= 320
    raws = [ow.hdlc_unescape(f[1:-1]) for f in frames]
    table = dict(zip(link_ids, VALUES))
    return dict(ks=ks, tab=tab, signers=signers, model=model, keys=keys, table=table, hashes=hashes, raws=raws,
                seeds=seeds, wire=b"".join(frames))


def _receipts(hashes):
    import reticulum_amd as rt
    t, m = rt.ReceiptTable(64, device=0), ph.Receipts(64)
    ids = list(range(10, 10 + len(hashes)))
    assert t.add(hashes, ids).cpu().tolist() == m.add(hashes, ids) == [lh.OK] * len(hashes)
    return t, m


def _expect(c, receipts, passed=None):
    """The model over the stream: (proofs or None, (proof status, receipt))."""
    fields = [ow.unpack(r) if passed is None or passed[i] else None for i, r in enumerate(c["raws"])]
    routes = [ph.link_of(f, c["table"]) for f in fields]
    proved = []
    for f, (route, link) in zip(fields, routes):
        tstat = ctoken.decrypt(c["keys"][link].tobytes(), f["data"])[0] if route == lh.LINK_DECRYPT else 1
        proved.append(ph.prove(f, route, link, tstat, c["model"]))
    return proved, ph.settle(fields, [link for _, link in routes], c["model"], receipts), routes


def _check(res, n, proved, settled):
    rows, ln = res["proofs"].cpu().numpy(), res["proof_len"].cpu().numpy()
    st, rc = res["proof_status"].cpu().numpy(), res["receipt"].cpu().numpy()
    assert rows.shape == (ln.size, 128) and ln.size == st.size == rc.size
    assert ln[:n].tolist() == [ph.PROOF_LEN if p is not None else 0 for p in proved]
    for i, p in enumerate(proved):
        if p is not None:
            assert rows[i, :ph.PROOF_LEN].tobytes() == p, i
    assert st[:n].tolist() == [s for s, _ in settled] and rc[:n].tolist() == [r for _, r in settled]
    # past the frames of the read there is no packet
    assert not ln[n:].any() and (st[n:] == ph.NOT_PROOF).all() and (rc[n:] == -1).all()


def test_a_read_proves_and_settles(case):
    import torch
    from reticulum_amd import pipeline
    c = case
    n = len(c["raws"])
    buf = torch.frombuffer(bytearray(c["wire"]), dtype=torch.uint8).to("cuda:0")
    nokey = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    table, receipts = _receipts(c["hashes"])
    proved, settled, routes = _expect(c, receipts)
    res = pipeline.inbound(c["ks"], buf, nokey, 0, 2 * n, links=c["tab"], signers=c["signers"], receipts=table)
    torch.cuda.synchronize()
    assert int(res["n_frames"]) == n
    _check(res, n, proved, settled)
    # every proof verifies under its link's key, by the tests' own Ed25519
    for p, (_, link) in zip(proved, routes):
        if p is not None:
            assert ed.verify(ed.public_key(c["seeds"][link]), p[51:], p[19:51])
    kinds = [s for s, _ in settled]
    assert set(kinds) == {ph.DELIVERED, ph.NOT_PROOF, ph.SHORT, ph.NO_RECEIPT, ph.BAD_SIGNATURE}
    assert kinds.count(ph.DELIVERED) == N_RECEIPTS - 4 and len(table) == len(receipts) == 4
    contexts = {(ow.unpack(r)["context"], p is not None) for r, p in zip(c["raws"], proved)
                if ow.unpack(r)["packet_type"] == lh.DATA}
    assert contexts == {(lh.NONE, True), (lh.NONE, False), (lh.CHANNEL, True), (lh.CHANNEL, False),
                        (lh.KEEPALIVE, False)}

    # signers alone: the same proofs and no settling; and the call without either
    # is the call as it was, key for key and byte for byte
    only = pipeline.inbound(c["ks"], buf, nokey, 0, 2 * n, links=c["tab"], signers=c["signers"])
    plain = pipeline.inbound(c["ks"], buf, nokey, 0, 2 * n, links=c["tab"])
    torch.cuda.synchronize()
    assert set(only) == set(plain) | {"proofs", "proof_len"}
    assert set(res) == set(only) | {"proof_status", "receipt"}
    assert torch.equal(only["proof_len"], res["proof_len"])
    live = only["proof_len"] > 0
    assert torch.equal(only["proofs"][live][:, :ph.PROOF_LEN], res["proofs"][live][:, :ph.PROOF_LEN])
    for k, v in plain.items():
        if k in ("n_frames", "frame_status", "counts"):
            assert torch.equal(v, res[k]), k
        elif k not in ("pt", "frame_len"):
            assert torch.equal(v[:n], res[k][:n]), k
    pairs = int(plain["counts"][0])
    assert torch.equal(plain["frame_len"][:pairs], res["frame_len"][:pairs])
    pt_a, pt_b = plain["pt"].cpu().numpy(), res["pt"].cpu().numpy()
    off, ln = plain["pt_off"].cpu().numpy(), plain["pt_len"].cpu().numpy()
    assert sum(ln[:n] > 0) > N_DATA // 2
    for i in range(n):
        assert pt_a[off[i]:off[i] + ln[i]].tobytes() == pt_b[off[i]:off[i] + ln[i]].tobytes(), i


def test_a_replayed_read_settles_nothing_and_proves_only_what_passes_the_filter(case):
    """The read twice through a packet hash list.  The second time every
    packet the list remembers is dropped before the link dispatch: no proof
    is settled and no packet with context NONE is proved.  CHANNEL and
    KEEPALIVE packets never consult the list (Transport.py:1388-1396), so the
    reference hands a replayed CHANNEL packet to Link.receive, which proves it
    again; so does the read."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    c = case
    n = len(c["raws"])
    buf = torch.frombuffer(bytearray(c["wire"]), dtype=torch.uint8).to("cuda:0")
    nokey = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    own = _t(np.frombuffer(OWN, np.uint8))
    table, receipts = _receipts(c["hashes"])
    seen, listed = rt.PacketHashlist(4096, device=0), fh.ListModel(4096, OWN)
    fields = [ow.unpack(r) for r in c["raws"]]
    for read in range(2):
        passed = [listed.packet(fh.packet(f["packet_hash"], f["packet_type"], f["destination_type"], f["context"],
                                          f["hops"], f["header_type"], b"", f["destination_hash"]))[0] == fh.PASS
                  for f in fields]
        proved, settled, _ = _expect(c, receipts, passed)
        res = pipeline.inbound(c["ks"], buf, nokey, 0, 2 * n, links=c["tab"], signers=c["signers"], receipts=table,
                               seen=seen, transport_identity=own)
        torch.cuda.synchronize()
        assert res["filter_status"].cpu()[:n].tolist() == [fh.PASS if p else fh.DUPLICATE for p in passed]
        _check(res, n, proved, settled)
        delivered = sum(s == ph.DELIVERED for s, _ in settled)
        if read == 0:
            assert delivered == N_RECEIPTS - 4 and not all(passed)      # the proof that comes twice
        else:
            assert delivered == 0 and {s for s, _ in settled} == {ph.NOT_PROOF}
            assert all(f["context"] == lh.CHANNEL for f, p in zip(fields, proved) if p is not None)
            assert any(p is not None for p in proved) and not any(
                pas for f, pas in zip(fields, passed) if f["context"] == lh.NONE)
        assert len(table) == len(receipts) == 4


def test_signers_and_receipts_need_links(case):
    import torch
    from reticulum_amd import pipeline
    c = case
    buf = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    table, _ = _receipts(c["hashes"][:2])
    with pytest.raises(ValueError, match="links"):
        pipeline.inbound(c["ks"], buf, buf[:1], 0, 4, signers=c["signers"])
    with pytest.raises(ValueError, match="links"):
        pipeline.inbound(c["ks"], buf, buf[:1], 0, 4, receipts=table)
    with pytest.raises(ValueError, match="signers"):
        pipeline.inbound(c["ks"], buf, buf[:1], 0, 4, links=c["tab"], receipts=table)
