"""pipeline.inbound(reply=True): what a read has to send, and the loop it closes.

One framed stream with access codes mixes DATA packets on two PROVE_ALL links,
a link request to one of the node's destinations, SINGLE packets for a
PROVE_ALL destination and noise.  The node reads it with ``signers``, ``accept``
and ``deliver`` and ``reply=True``: the reply stream is held to the model of
tests/reply_helpers.py over the rows of the same result.  That stream then goes
to a second read standing for the peer, which settles the link proofs and the
destination proofs under its receipts and finds the link established; and the
node, reading its own stream back, drops every frame as a replay."""
import numpy as np
import pytest

import destination_deliver_helpers as dd
import ed25519_ref as ed
import ifac_helpers as ih
import link_accept_helpers as la
import link_helpers as lh
import mixed_read_helpers as mr
import proof_helpers as ph
import reply_helpers as rh
from oracle import wire as ow

pytestmark = pytest.mark.gpu

ISZ = 16
N_KEYS = 8
SLOT, PEER_SLOT = 4, 6
DUPLICATE = 5


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _wire(ifac_key, raws):
    return b"".join(ow.hdlc_frame(ow.ifac_mask(r, ih.code(ifac_key, r, ISZ), ifac_key)) for r in raws)


def _keyset(keys):
    import reticulum_amd as rt
    return rt.KeySet(np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 64), device=0)


@pytest.fixture(scope="module")
def world():
    """The node, its peer, and the read the peer sent: made on the host
    (mixed_read_helpers.reply_world, the link request included), so that the
    composed model reads the same world; the peer's pending link is entered
    from the host-made request."""
    import reticulum_amd as rt
    w = mr.reply_world()
    o = w["opened"]
    pending = rt.PendingLinks(8, device=0)
    assert pending.add([o.link_id], [o.prv], [o.dest_public], [o.sig_seed], [o.flags], [o.slot],
                       [o.expected_hops]).tolist() == [0]
    w["pending"] = pending
    return w


def _node_read(w, seen, reply, buf=None):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    d, frames = w["dests"], w["frames"]
    tab = rt.LinkTable(32, device=0)
    assert tab.insert(w["link_ids"], [0, 1]).cpu().tolist() == [lh.OK] * 2
    signers = rt.LinkSigners(w["seeds"], w["peer_publics"], w["flags"], device=0)
    accept = dict(destinations=rt.LinkDestinations([x.hash for x in d], [x.seed for x in d], [la.F_ACCEPTS] * len(d),
                                                   device=0),
                  slots=_t(np.array([SLOT, SLOT + 1], np.int32)), nh_mtu=500,
                  ephemeral_privates=_t(np.frombuffer(b"".join(w["ephemerals"]), np.uint8).reshape(2, 32)))
    deliver = rt.SingleDestinations([x.hash for x in d], [x.prv for x in d], [x.identity_hash for x in d],
                                    [x.seed for x in d], [x.flags for x in d], [x.ratchets for x in d],
                                    max_frames=64, retry_trials=32, device=0)
    kw = dict(check_ifac=True, links=tab, signers=signers, accept=accept, deliver=deliver,
              transport_identity=_t(np.frombuffer(w["tid"], np.uint8)))
    if seen is not None:
        kw["seen"] = seen
    if reply is not None:
        kw["reply"] = reply
    if buf is None:
        buf = torch.frombuffer(bytearray(_wire(w["ifac_key"], [raw for _, raw in frames])), dtype=torch.uint8)
    res = pipeline.inbound(_keyset(w["keys"]), buf.to("cuda:0"), _t(np.frombuffer(w["ifac_key"], np.uint8)), ISZ, 32,
                           **kw)
    torch.cuda.synchronize()
    return res


def _model_over(res, cap=None):
    """The model's replies over the rows of the result itself."""
    from reticulum_amd import pipeline
    sources = []
    for rows, ln in pipeline.REPLY_SOURCES:
        r, n = res[rows].cpu().numpy(), res[ln].cpu().numpy()
        sources.append(([bytes(x) for x in r], n))
    return rh.gather_model(sources, cap)


def test_one_mixed_read_and_the_loop_it_closes(world):
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    w = world
    names = [name for name, _ in w["frames"]]
    at = {name: i for i, name in enumerate(names)}
    seen = rt.PacketHashlist(1024, device=0)
    res = _node_read(w, seen, True)
    assert int(res["n_frames"]) == len(names)
    # what the stages wrote: a proof per link packet, the LRPROOF, a proof per SINGLE packet
    assert res["proof_len"][:8].cpu().tolist() == [115, 0, 0, 0, 115, 0, 0, 115]
    assert res["lr_proof_len"][:8].cpu().tolist() == [0, 0, 0, 118, 0, 0, 0, 0]
    assert res["dest_proof_len"][:8].cpu().tolist() == [0, 0, 83, 0, 0, 83, 0, 0]
    # and all of it as the composed model has it, row for row: nothing of the device's enters this expectation
    model = mr.compose(mr.reply_node(w), mr.reply_wire(w), ISZ, 32)
    for rows, ln in pipeline.REPLY_SOURCES:
        assert res[ln].cpu().tolist() == mr.lengths(model[rows]), ln
        for i, row in enumerate(model[rows]):
            assert row is None or res[rows][i, :len(row)].cpu().numpy().tobytes() == row, (rows, i)
    rep = res["reply"]
    assert [(k, s) for k, s, _ in model["replies"]] == list(zip(rep["reply_frame"][:6].cpu().tolist(),
                                                                 rep["reply_source"][:6].cpu().tolist()))
    assert bytes(rep["stream"][:int(rep["frame_off"][32])].cpu().numpy()) == b"".join(model["reply_frames"])
    assert set(rep) == {"stream", "frame_off", "reply_counts", "reply_frame", "reply_source", "reply_len", "packets"}
    replies, found = _model_over(res)
    assert found == 6 and rep["reply_counts"].cpu().tolist() == [6, 6]
    want = rh.reply_stream_model(replies, w["ifac_key"], ISZ)
    foff = rep["frame_off"].cpu().numpy()
    assert foff.shape == (33,) and foff[:7].tolist() == np.cumsum([0] + [len(f) for f in want]).tolist()
    assert (foff[6:] == foff[32]).all()
    stream = bytes(rep["stream"][:int(foff[32])].cpu().numpy())
    assert stream == b"".join(want)
    # the replies name the right frames, in frame order, each by its stage
    assert rep["reply_frame"][:6].cpu().tolist() == [at[x] for x in ("link 0", "single 0", "request", "link 1",
                                                                    "single 1", "link 0 again")]
    P, D, L = device.REPLY_LINK_PROOF, device.REPLY_DEST_PROOF, device.REPLY_LRPROOF
    assert rep["reply_source"][:6].cpu().tolist() == [P, D, L, P, D, P]
    assert rep["reply_len"][:6].cpu().tolist() == [115, 83, 118, 115, 83, 115]
    assert rep["reply_frame"][6:].cpu().tolist() == [-1] * 26 and not rep["reply_len"][6:].any()

    # ---- the peer reads the stream: its receipts are delivered, its link comes up
    raws = dict(w["frames"])
    peer_tab = rt.LinkTable(32, device=0)
    assert peer_tab.insert(w["link_ids"], [0, 1]).cpu().tolist() == [lh.OK] * 2
    node_publics = [ed.public_key(s) for s in w["seeds"]]
    peer_signers = rt.LinkSigners([_rb(w["rng"], 32) for _ in range(N_KEYS)], node_publics, [0] * N_KEYS, device=0)
    receipts = rt.ReceiptTable(64, device=0)
    sent_on_links = ["link 0", "link 1", "link 0 again"]
    assert receipts.add([dd.packet_hash(raws[x]) for x in sent_on_links], [10, 11, 12]).cpu().tolist() == [lh.OK] * 3
    dest_receipts = rt.DestinationReceipts(64, device=0)
    assert dest_receipts.add([dd.packet_hash(raws["single 0"]), dd.packet_hash(raws["single 1"])], [20, 21],
                             keys=[ed.public_key(w["dests"][0].seed), ed.public_key(w["dests"][1].seed)]
                             ).cpu().tolist() == [lh.OK] * 2
    buf = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
    peer = pipeline.inbound(_keyset([_rb(w["rng"], 64) for _ in range(N_KEYS)]), buf,
                            _t(np.frombuffer(w["ifac_key"], np.uint8)), ISZ, 16, check_ifac=True, links=peer_tab,
                            signers=peer_signers, receipts=receipts, destination_receipts=dest_receipts,
                            establish=w["pending"], transport_identity=_t(np.frombuffer(w["peer_tid"], np.uint8)))
    torch.cuda.synchronize()
    assert int(peer["n_frames"]) == 6 and peer["ifac_status"][:6].cpu().tolist() == [0] * 6
    assert [peer["proof_status"][j].item() for j in (0, 3, 5)] == [ph.DELIVERED] * 3
    assert [peer["receipt"][j].item() for j in (0, 3, 5)] == [10, 11, 12]
    assert [peer["dproof_status"][j].item() for j in (1, 4)] == [device.DPROOF_DELIVERED] * 2
    assert [peer["dproof_receipt"][j].item() for j in (1, 4)] == [20, 21]
    assert peer["lrproof_status"][2].item() == 0 and peer["established_link"][2].item() == PEER_SLOT       # activated
    assert peer["established_link"][:6].cpu().tolist() == [-1, -1, PEER_SLOT, -1, -1, -1]
    assert w["pending"].state([w["link_id"]]).tolist() == [2]                                               # ACTIVE
    assert len(receipts.table) == 0 and len(dest_receipts.table) == 0

    # ---- the node hears its own replies on a shared medium: every frame is a replay
    hashes = [rh.packet_hash(r) for _, _, r in replies]
    assert seen.contains(hashes).cpu().tolist() == [1] * 6
    echo = _node_read(w, seen, None, buf=torch.frombuffer(bytearray(stream), dtype=torch.uint8))
    assert int(echo["n_frames"]) == 6
    assert echo["filter_status"][:6].cpu().tolist() == [DUPLICATE] * 6
    assert not echo["fields"][:6, 0].any()                                                                  # ok = 0
    assert not echo["proof_len"].any() and not echo["lr_proof_len"].any() and not echo["dest_proof_len"].any()


def test_max_replies_cuts_the_stream(world):
    w = world
    res = _node_read(w, None, {"max_replies": 4})
    rep = res["reply"]
    replies, found = _model_over(res, 4)
    assert found == 6 and rep["reply_counts"].cpu().tolist() == [4, 6]
    total = int(rep["frame_off"][4])
    assert bytes(rep["stream"][:total].cpu().numpy()) == b"".join(rh.reply_stream_model(replies, w["ifac_key"], ISZ))
    assert rep["packets"].shape == (4, 128)


def test_a_read_without_reply_is_the_read_it_was(world):
    import torch
    w = world
    on, off = _node_read(w, None, True), _node_read(w, None, None)
    assert "reply" not in off and set(on) == set(off) | {"reply"}
    n = int(off["n_frames"])
    for k, b in off.items():
        a = on[k]
        if k in ("n_frames", "frame_status", "counts"):
            assert torch.equal(a, b), k
        elif k == "pt":
            for i in range(n):
                lo, ln = int(off["pt_off"][i]), int(off["pt_len"][i])
                assert torch.equal(a[lo:lo + ln], b[lo:lo + ln]), (k, i)
        elif k in ("proofs", "lr_proofs", "dest_proofs"):
            ln = {"proofs": "proof_len", "lr_proofs": "lr_proof_len", "dest_proofs": "dest_proof_len"}[k]
            for i in range(n):
                assert torch.equal(a[i, :int(on[ln][i])], b[i, :int(off[ln][i])]), (k, i)
        elif k == "frame_len":
            assert torch.equal(a[:int(on["counts"][0])], b[:int(off["counts"][0])]), k
        else:
            assert torch.equal(a[:n], b[:n]), k
