"""pipeline.inbound(destination_receipts=...): the proofs for packets sent to
SINGLE destinations settled inside the read, beside the link proofs.

One framed stream of about 90 packets: DATA packets on three links built by
pipeline.outbound, link proofs for a ReceiptTable (rt_proof_settle's) and
proofs for a DestinationReceipts, explicit, implicit, stray and bad, one of
them of destination type LINK for a link that is not in the table.  Each stage
settles its own: the read is held to tests/proof_helpers.py and
tests/destination_proof_helpers.py, which the CPU tests tie to the reference;
the same stream is read twice through a packet hash list; and the call without
the new argument is compared with the same call beside it."""
import numpy as np
import pytest

import destination_proof_helpers as dp
import filter_helpers as fh
import link_helpers as lh
import proof_helpers as ph
from oracle import wire as ow

pytestmark = pytest.mark.gpu

OWN = bytes(range(11, 27))
VALUES = [1, 2, 0]                       # link j -> the row of its key and of its signing rows
N_DATA, PT_LEN = 60, 21


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
    rng = np.random.Generator(np.random.PCG64(2363))
    keys = rng.integers(0, 256, (3, 64), dtype=np.uint8)
    link_ids = [_rb(rng, 16) for _ in range(3)]
    seeds, peer_seeds = [_rb(rng, 32) for _ in range(3)], [_rb(rng, 32) for _ in range(3)]
    ks = rt.KeySet(keys, device=0)
    tab = rt.LinkTable(8, device=0)
    assert tab.insert(link_ids, VALUES).cpu().tolist() == [lh.OK] * 3
    peers = [ph.public_key(s) for s in peer_seeds]
    signers = rt.LinkSigners(seeds, peers, [0, 0, 0], device=0)
    model = ph.Signers(seeds, peers, [0, 0, 0])
    j = np.arange(N_DATA) % 3
    framed, frame_off = pipeline.outbound(
        ks, _t(rng.integers(0, 256, (N_DATA, PT_LEN), dtype=np.uint8)),
        _t(rng.integers(0, 256, (N_DATA, 16), dtype=np.uint8)),
        _t(np.frombuffer(b"".join(link_ids[k] for k in j), np.uint8).reshape(N_DATA, 16)),
        _t(np.zeros(N_DATA, np.uint8)), flags=_t(np.full(N_DATA, lh.LINK << 2 | lh.DATA, np.uint8)),
        key_idx=_t(np.array(VALUES)[j].astype(np.int32)))
    torch.cuda.synchronize()
    off, wire = frame_off.cpu().numpy(), framed.cpu().numpy().tobytes()
    data_frames = [wire[off[i]:off[i + 1]] for i in range(N_DATA)]

    # link receipts (sent on link r % 3) and destination receipts (recipient r & 1)
    link_hashes = [_rb(rng, 32) for _ in range(6)]
    dest_seeds = [_rb(rng, 32) for _ in range(2)]
    dest_hashes = [_rb(rng, 32) for _ in range(12)]

    def link_proof(r, good=True):
        k = r % 3
        sig = ph.sign(peer_seeds[VALUES[k] if good else (VALUES[k] + 1) % 3], link_hashes[r])
        return bytes([lh.LINK << 2 | lh.PROOF, 0]) + link_ids[k] + bytes([lh.NONE]) + link_hashes[r] + sig

    def dest_proof(r, implicit, **kw):
        return dp.proof_packet(dest_hashes[r], dest_seeds[r & 1], implicit, **kw)

    elsewhere = _rb(rng, 16)
    proofs = [link_proof(0), dest_proof(0, False), dest_proof(1, True), link_proof(1, good=False), link_proof(1),
              dest_proof(2, True, address=elsewhere),                                   # a stray that validates
              dest_proof(3, False)[:-1], dest_proof(3, False), dest_proof(3, False),    # short; twice
              dp.proof_packet(dest_hashes[4], dest_seeds[1], False),                    # the other recipient's key
              dest_proof(4, False), link_proof(2), dest_proof(5, True, dtype=lh.LINK),  # LINK, no such link
              dest_proof(6, True, address=link_ids[0], dtype=lh.LINK),                  # LINK on an active link
              dest_proof(6, True, context=ph.LRPROOF), dest_proof(6, True),
              dp.proof_packet(_rb(rng, 32), dest_seeds[0], True),                       # a stray that finds nothing
              link_proof(3), dest_proof(7, False, dtype=lh.PLAIN), dest_proof(8, True), dest_proof(8, True),
              dest_proof(9, False)]
    # link receipts 4, 5 and destination receipts 10, 11 stay outstanding
    frames, at = [], 0
    for i, f in enumerate(data_frames):
        frames.append(f)
        if i % 2 == 1 and at < len(proofs):
            frames.append(ow.hdlc_frame(proofs[at]))
            at += 1
    assert at == len(proofs)
    raws = [ow.hdlc_unescape(f[1:-1]) for f in frames]
    return dict(ks=ks, tab=tab, signers=signers, model=model, table=dict(zip(link_ids, VALUES)), raws=raws,
                wire=b"".join(frames), link_hashes=link_hashes, dest_hashes=dest_hashes,
                dest_keys=[dp.public_key(dest_seeds[r & 1]) for r in range(12)])


def _receipts(c):
    import reticulum_amd as rt
    t, m = rt.ReceiptTable(16, device=0), ph.Receipts(16)
    ids = list(range(3, 3 + len(c["link_hashes"])))
    assert t.add(c["link_hashes"], ids).cpu().tolist() == m.add(c["link_hashes"], ids) == [lh.OK] * len(ids)
    d, dm = rt.DestinationReceipts(16, device=0), dp.Receipts(16)
    ids = list(range(len(c["dest_hashes"])))
    assert d.add(c["dest_hashes"], ids, keys=c["dest_keys"]).cpu().tolist() == \
        dm.add(c["dest_hashes"], ids, c["dest_keys"]) == [lh.OK] * len(ids)
    return t, m, d, dm


def _expect(c, m, dm, passed=None):
    fields = [ow.unpack(r) if passed is None or passed[i] else None for i, r in enumerate(c["raws"])]
    links = [ph.link_of(f, c["table"])[1] for f in fields]
    return (ph.settle(fields, links, c["model"], m),
            dp.settle(fields, dm, dm.max_receipts * 4, links=links, n_links=c["model"].n_links))


def _check(res, n, settled, dsettled):
    for key, idk, want, idle in (("proof_status", "receipt", settled, ph.NOT_PROOF),
                                 ("dproof_status", "dproof_receipt", dsettled, dp.NOT_PROOF)):
        st, rc = res[key].cpu().numpy(), res[idk].cpu().numpy()
        assert st[:n].tolist() == [s for s, _ in want], key
        assert rc[:n].tolist() == [r for _, r in want], idk
        assert (st[n:] == idle).all() and (rc[n:] == -1).all()      # past the frames of the read there is no packet


def test_each_stage_settles_its_own_proofs(case):
    import torch
    from reticulum_amd import pipeline
    c = case
    n = len(c["raws"])
    buf = torch.frombuffer(bytearray(c["wire"]), dtype=torch.uint8).to("cuda:0")
    nokey = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    t, m, d, dm = _receipts(c)
    settled, dsettled = _expect(c, m, dm)
    res = pipeline.inbound(c["ks"], buf, nokey, 0, 2 * n, links=c["tab"], signers=c["signers"], receipts=t,
                           destination_receipts=d)
    torch.cuda.synchronize()
    assert int(res["n_frames"]) == n
    _check(res, n, settled, dsettled)
    kinds = [s for s, _ in dsettled]
    assert set(kinds) == {dp.DELIVERED, dp.NOT_PROOF, dp.ON_LINK, dp.BAD_LENGTH, dp.NO_RECEIPT, dp.BAD_SIGNATURE}
    assert kinds.count(dp.DELIVERED) == 10 and len(d) == len(dm) == 2
    assert [s for s, _ in settled].count(ph.DELIVERED) == 4 and len(t) == len(m) == 2
    # no proof is settled by both, and a link proof on an active link is the link stage's alone
    for (s, _), (ds, _) in zip(settled, dsettled):
        assert not (s == ph.DELIVERED and ds == dp.DELIVERED)
        if s in (ph.DELIVERED, ph.BAD_SIGNATURE, ph.NO_RECEIPT, ph.SHORT):
            assert ds == dp.ON_LINK

    # without links no link is active: the LINK proof on a table link is settled here too
    t2, m2, d2, dm2 = _receipts(c)
    fields = [ow.unpack(r) for r in c["raws"]]
    alone = pipeline.inbound(c["ks"], buf, nokey, 0, 2 * n, destination_receipts=d2)
    torch.cuda.synchronize()
    want = dp.settle(fields, dm2, dm2.max_receipts * 4)
    assert alone["dproof_status"].cpu()[:n].tolist() == [s for s, _ in want]
    assert alone["dproof_receipt"].cpu()[:n].tolist() == [r for _, r in want]
    assert dp.ON_LINK not in [s for s, _ in want] and len(d2) == len(dm2)

    # with the argument None the call is the call as it was, key for key and byte for byte
    t3, _, _, _ = _receipts(c)
    plain = pipeline.inbound(c["ks"], buf, nokey, 0, 2 * n, links=c["tab"], signers=c["signers"], receipts=t3,
                             destination_receipts=None)
    torch.cuda.synchronize()
    assert set(res) == set(plain) | {"dproof_status", "dproof_receipt"}
    for k, v in plain.items():
        if k in ("n_frames", "frame_status", "counts"):
            assert torch.equal(v, res[k]), k
        elif k == "proofs":
            live = plain["proof_len"] > 0
            assert torch.equal(v[live][:, :ph.PROOF_LEN], res[k][live][:, :ph.PROOF_LEN])
        elif k not in ("pt", "frame_len"):
            assert torch.equal(v[:n], res[k][:n]), k
    pairs = int(plain["counts"][0])
    assert torch.equal(plain["frame_len"][:pairs], res["frame_len"][:pairs])
    pt_a, pt_b = plain["pt"].cpu().numpy(), res["pt"].cpu().numpy()
    off, ln = plain["pt_off"].cpu().numpy(), plain["pt_len"].cpu().numpy()
    assert sum(ln[:n] > 0) >= N_DATA
    for i in range(n):
        assert pt_a[off[i]:off[i] + ln[i]].tobytes() == pt_b[off[i]:off[i] + ln[i]].tobytes(), i


def test_a_replayed_read_settles_nothing(case):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    c = case
    n = len(c["raws"])
    buf = torch.frombuffer(bytearray(c["wire"]), dtype=torch.uint8).to("cuda:0")
    nokey = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    own = _t(np.frombuffer(OWN, np.uint8))
    t, m, d, dm = _receipts(c)
    seen, listed = rt.PacketHashlist(1024, device=0), fh.ListModel(1024, OWN)
    fields = [ow.unpack(r) for r in c["raws"]]
    for read in range(2):
        passed = [listed.packet(fh.packet(f["packet_hash"], f["packet_type"], f["destination_type"], f["context"],
                                          f["hops"], f["header_type"], b"", f["destination_hash"]))[0] == fh.PASS
                  for f in fields]
        settled, dsettled = _expect(c, m, dm, passed)
        res = pipeline.inbound(c["ks"], buf, nokey, 0, 2 * n, links=c["tab"], signers=c["signers"], receipts=t,
                               destination_receipts=d, seen=seen, transport_identity=own)
        torch.cuda.synchronize()
        assert res["filter_status"].cpu()[:n].tolist() == [fh.PASS if p else fh.DUPLICATE for p in passed]
        _check(res, n, settled, dsettled)
        delivered = sum(s == dp.DELIVERED for s, _ in dsettled)
        if read == 0:
            assert delivered == 10 and not all(passed)              # the proofs that come twice are dropped as replays
        else:
            # a PLAIN packet never consults the list (Transport.py:1395-1401): that proof comes
            # through again and finds its receipt gone
            again = [i for i, (s, _) in enumerate(dsettled) if s != dp.NOT_PROOF]
            assert delivered == 0 and [dsettled[i][0] for i in again] == [dp.NO_RECEIPT]
            assert fields[again[0]]["destination_type"] == lh.PLAIN
        assert len(d) == len(dm) == 2 and len(t) == len(m) == 2
