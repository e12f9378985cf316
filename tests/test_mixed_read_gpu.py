"""One mixed read of real size through pipeline.inbound with every stage on,
held column by column and frame by frame to the composed host model of
tests/mixed_read_helpers.py (no device result enters the expectation; what
of a column is compared, and what inbound leaves unwritten, is in ``check``).

N = 577 frames (two workgroups, a wave and a lone lane of the 256-thread stages)
in four layouts, and N = 1025 (one 1024-frame block of the scans and the reply
gather, and a lone frame) in layout 0; with and without access codes, with and
without slots.  Then: the state the read leaves in the tables, a stage alone
against the stage in the full read, and the loop the reply stream closes at
this size.

``max_frames`` of SingleDestinations cannot cap a read through inbound (it
refuses max_pairs above it, checked below): the delivery cap of layout 3 is
``retry_trials``, beside ``scan_trials`` and ``max_replies``."""
import numpy as np
import pytest

import link_helpers as lh
import link_proof_helpers as lp
import mixed_read_helpers as mr
import proof_helpers as ph
import destination_proof_helpers as dp
import filter_helpers as fh
import reply_helpers as rh

pytestmark = pytest.mark.gpu

CASES = [(0, mr.N), (1, mr.N), (2, mr.N), (3, mr.N), (0, mr.N_SCAN)]
GUARD = 256


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _u8(b, *shape):
    return np.frombuffer(bytes(b), np.uint8).reshape(*shape) if shape else np.frombuffer(bytes(b), np.uint8)


@pytest.fixture(scope="module")
def world():
    return mr.World()


@pytest.fixture(scope="module")
def models(world):
    """(layout, n, ifac_size) -> (frames, wire, model), made once."""
    made = {}

    def get(layout, n, isz):
        if (layout, n, isz) not in made:
            frames = mr.build(world, layout, n)
            wire = mr.wire_of(world, frames, isz)
            caps = layout == 3
            made[layout, n, isz] = (frames, wire, mr.compose(
                world.node(caps), wire, isz, 2 * n, max_replies=mr.CAPS["max_replies"] if caps else None))
        return made[layout, n, isz]
    return get


class DeviceNode:
    """The device objects of a mr.Node, stage for stage."""

    def __init__(self, nd, max_pairs):
        import reticulum_amd as rt
        self.nd = nd
        self.ks = rt.KeySet(_u8(b"".join(nd.keys), len(nd.keys), 64), device=0)
        self.tab = rt.LinkTable(1024, device=0)
        if nd.table:
            assert self.tab.insert(list(nd.table), list(nd.table.values())).cpu().tolist() == [lh.OK] * len(nd.table)
        self.kw = dict(links=self.tab, transport_identity=_t(_u8(nd.tid)), announces=nd.announces)
        if nd.signers is not None:
            s = nd.signers
            self.kw["signers"] = rt.LinkSigners(s.seeds, s.peer_publics, s.flags, device=0)
        if nd.accept is not None:
            a = nd.accept
            self.kw["accept"] = dict(
                destinations=rt.LinkDestinations([d.hash for d in a["dests"]], [d.seed for d in a["dests"]],
                                                 [d.flags for d in a["dests"]], device=0),
                slots=_t(np.array(a["slots"], np.int32)), nh_mtu=a["nh_mtu"],
                ephemeral_privates=_t(_u8(b"".join(a["ephemerals"]), len(a["ephemerals"]), 32)))
        if nd.pending is not None:
            self.pending = rt.PendingLinks(max(8, len(nd.pending)), device=0)
            p = list(nd.pending.values())
            if p:
                assert self.pending.add([x.link_id for x in p], [x.prv for x in p], [x.dest_public for x in p],
                                        [x.sig_seed for x in p], [x.flags for x in p], [x.slot for x in p],
                                        [x.expected_hops for x in p]).tolist() == [0] * len(p)
            self.kw["establish"] = self.pending
        if nd.deliver is not None:
            d = nd.deliver["dests"]
            self.kw["deliver"] = rt.SingleDestinations(
                [x.hash for x in d], [x.prv for x in d], [x.identity_hash for x in d], [x.seed for x in d],
                [x.flags for x in d], [x.ratchets for x in d], max_frames=max_pairs,
                retry_trials=nd.deliver["retry_trials"], device=0)
            self.kw["implicit_proof"] = nd.deliver["implicit"]
        if nd.receipts is not None:
            self.receipts = self.kw["receipts"] = rt.ReceiptTable(nd.max_receipts, device=0)
            ids = sorted(nd.receipts.hashes)
            if ids:
                assert self.receipts.add([nd.receipts.hashes[i] for i in ids], ids).cpu().tolist() == [lh.OK] * len(ids)
        if nd.dest_receipts is not None:
            r = nd.dest_receipts
            self.dest_receipts = self.kw["destination_receipts"] = rt.DestinationReceipts(
                nd.max_receipts, scan_trials=nd.scan_trials, device=0)
            ids = sorted(r.hashes)
            if ids:
                assert self.dest_receipts.add([r.hashes[i] for i in ids], ids,
                                              keys=[r.keys[i] for i in ids]).cpu().tolist() == [lh.OK] * len(ids)
        if nd.seen is not None:
            self.seen = self.kw["seen"] = rt.PacketHashlist(nd.seen.max, device=0)

    def read(self, wire, isz, max_pairs, aligned=None, reply=True, check_ifac=True):
        """The read, with guard bytes behind the one buffer the caller owns."""
        import torch
        from reticulum_amd import pipeline
        held = torch.full((len(wire) + GUARD,), 0xA5, dtype=torch.uint8)
        held[:len(wire)] = torch.frombuffer(bytearray(wire), dtype=torch.uint8)
        held = held.to("cuda:0")
        kw = dict(self.kw)
        if reply is not None and reply is not False:
            kw["reply"] = reply
        res = pipeline.inbound(self.ks, held[:len(wire)], _t(_u8(self.nd.ifac_key)), isz, max_pairs, aligned=aligned,
                               check_ifac=bool(isz) and check_ifac, **kw)
        torch.cuda.synchronize()
        back = held.cpu().numpy()
        assert back[:len(wire)].tobytes() == wire and (back[len(wire):] == 0xA5).all()      # the input and its guard
        return res


def _col(res, k):
    return res[k].cpu().numpy()


def _rows(res, rows, ln, want, what):
    """A sparse row output against the model's packets (None: nothing)."""
    got_len = _col(res, ln)
    assert got_len.tolist() == mr.lengths(want), what
    got = _col(res, rows)
    for i, w in enumerate(want):
        if w:
            assert got[i, :len(w)].tobytes() == w, (what, i)


def check(res, m, isz, what=""):
    """Every column inbound returned against the model: every entry of the
    per-frame columns the stages write for all max_pairs entries, the entries
    past n_frames included; ``frame_len`` up to the pairs found and
    ``frame_pair`` and ``ifac`` up to n_frames (past them they are not
    written); of ``fields`` the ok byte everywhere and the record where ok is
    set."""
    n, mp = m["n_frames"], len(m["status"])
    assert int(res["n_frames"]) == n, what
    assert _col(res, "counts").tolist() == m["counts"], what
    pairs = m["counts"][0]
    assert _col(res, "frame_status").tolist() == m["frame_status"], what
    assert _col(res, "frame_len")[:pairs].tolist() == m["frame_len"], what
    assert _col(res, "frame_pair")[:n].tolist() == m["frame_pair"], what
    assert _col(res, "ifac_status").tolist() == m["ifac_status"], what
    if isz:
        # the code as it came: of every frame the unmask took, matched or not (ifac_status 0 and 2); the rows of
        # frames dropped before it and past n_frames are not written
        got = _col(res, "ifac")
        for i in range(n):
            assert (m["ifac"][i] is not None) == (m["ifac_status"][i] != 1), (what, i)
            if m["ifac"][i] is not None:
                assert got[i].tobytes() == m["ifac"][i], (what, i)
    fields = _col(res, "fields")
    assert fields[:, 0].tolist() == m["ok"], what
    for i, f in enumerate(m["unpacked"]):                  # the rest of a record counts where ok is set
        if f is not None:
            r = fields[i]
            assert (r[1], r[2], r[3], r[6], r[7], r[8]) == (f["flags"], f["hops"], f["header_type"], f["destination_type"],
                                                            f["packet_type"], f["context"]), (what, "fields", i)
            assert r[36:52].tobytes() == f["destination_hash"] and r[52:84].tobytes() == f["packet_hash"], (what, i)
            assert f["transport_id"] is None or r[20:36].tobytes() == f["transport_id"], (what, i)
    plain = ["filter_status", "announce_status", "linkreq_status", "accepted_link", "link_mtu", "lrproof_status",
             "established_link", "route", "link", "key_idx", "proof_status", "receipt", "dproof_status",
             "dproof_receipt", "status", "deliver_status", "destination", "ratchet"]
    for k in plain:
        assert (k in res) == (k in m), (what, k)
        if k in m:
            got, want = _col(res, k).astype(np.int64), np.array(m[k], np.int64)
            bad = np.nonzero(got != want)[0]
            assert not bad.size, (what, k, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    for k in ("announce_identity", "link_id"):
        if k in m:
            assert _col(res, k).tobytes() == b"".join(m[k]), (what, k)
    for rows, ln in (("lr_proofs", "lr_proof_len"), ("proofs", "proof_len"), ("dest_proofs", "dest_proof_len")):
        assert (rows in res) == (rows in m), (what, rows)
        if rows in m:
            _rows(res, rows, ln, m[rows], (what, rows))
    pt, off, ln = _col(res, "pt"), _col(res, "pt_off"), _col(res, "pt_len")
    for i in range(mp):
        if m["status"][i] == 0:
            assert pt[off[i]:off[i] + ln[i]].tobytes() == m["pt"][i], (what, "pt", i)
        elif m["status"][i] in (1, 2):
            assert ln[i] == 0, (what, "pt_len", i)
    if "replies" in m:
        check_reply(res["reply"], m, isz, what)


def check_reply(rep, m, isz, what=""):
    replies, (written, found) = m["replies"], m["reply_counts"]
    assert _col(rep, "reply_counts").tolist() == [written, found], what
    cap = rep["packets"].shape[0]
    foff = _col(rep, "frame_off")
    want_off = np.cumsum([0] + [len(x) for x in m["reply_frames"]])
    assert foff.shape == (cap + 1,) and foff[:written + 1].tolist() == want_off.tolist(), what
    assert (foff[written:] == foff[cap]).all(), what
    assert _col(rep, "stream")[:int(foff[cap])].tobytes() == b"".join(m["reply_frames"]), what
    assert _col(rep, "reply_frame").tolist() == [k for k, _, _ in replies] + [rh.NONE_FRAME] * (cap - written), what
    assert _col(rep, "reply_source").tolist() == [s for _, s, _ in replies] + [rh.NONE_SOURCE] * (cap - written), what
    assert _col(rep, "reply_len").tolist() == [len(r) for _, _, r in replies] + [rh.NONE_LEN] * (cap - written), what
    assert _col(rep, "packets")[:written].tobytes() == b"".join(r.ljust(rh.ROW, b"\0") for _, _, r in replies), what


def check_state(dev, after, world, frames):
    """What the read left in the tables, through their lookup and contains calls."""
    ids = sorted(set(after.table) | set(dev.nd.table) | set(after.pending or {}))
    values, found = dev.tab.lookup(ids)
    assert found.cpu().tolist() == [int(i in after.table) for i in ids]
    assert [v for v, f in zip(values.cpu().tolist(), found.cpu().tolist()) if f] == [after.table[i] for i in ids
                                                                                     if i in after.table]
    assert len(dev.tab) == len(after.table)
    if after.seen is not None:
        assert dev.seen.counts() == after.seen.counts()
        hashes = sorted(after.seen.current) + [rh.packet_hash(raw) for _, raw in frames if len(raw) > 19]
        assert dev.seen.contains(hashes).cpu().tolist() == after.seen.contains(hashes)
    for name, model in (("receipts", after.receipts), ("dest_receipts", after.dest_receipts)):
        if model is not None:
            table = getattr(dev, name)
            assert len(table) == len(model)
            ids = sorted(model.hashes)
            hs = [model.hashes[i][:16] for i in ids]
            values, found = table.table.lookup(hs)
            values, found = values.cpu().tolist(), found.cpu().tolist()
            assert found == [int(h in model.table.entries) for h in hs], name
            assert [v for v, f in zip(values, found) if f] == [model.table.entries[h] for h in hs
                                                                if h in model.table.entries], name
            assert [i for i, f in zip(ids, found) if f] == [v for v, f in zip(values, found) if f], name
    if after.pending:
        ids = list(after.pending)
        assert dev.pending.state(ids).tolist() == [after.pending[i].state for i in ids]
        hops, rebalanced, mtu = dev.pending.hops(ids)
        assert hops.tolist() == [after.pending[i].expected_hops for i in ids]
        assert rebalanced.tolist() == [int(after.pending[i].rebalanced) for i in ids]
        assert mtu.tolist() == [after.pending[i].mtu for i in ids]


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("isz", [mr.ISZ, 0])
@pytest.mark.parametrize("layout,n", CASES)
def test_the_read_is_the_composed_model(world, models, layout, n, isz, aligned):
    frames, wire, m = models(layout, n, isz)
    caps = layout == 3
    dev = DeviceNode(world.node(caps), 2 * n)
    res = dev.read(wire, isz, 2 * n, aligned=aligned, reply={"max_replies": mr.CAPS["max_replies"]} if caps else True)
    check(res, m, isz, (layout, n, isz, aligned))
    if caps:
        written, found = m["reply_counts"]
        assert found > written == mr.CAPS["max_replies"] and res["reply"]["packets"].shape == (written, 128)
        assert 6 in m["deliver_status"] and dp.DEFERRED in m["dproof_status"]
    check_state(dev, m["node"], world, frames)


def test_inbound_refuses_a_read_larger_than_max_frames(world):
    import reticulum_amd as rt
    import torch
    from reticulum_amd import pipeline
    d = world.dests
    small = rt.SingleDestinations([x.hash for x in d], [x.prv for x in d], [x.identity_hash for x in d],
                                  [x.seed for x in d], [x.flags for x in d], [x.ratchets for x in d], max_frames=8,
                                  device=0)
    with pytest.raises(ValueError, match="max_pairs <= deliver.max_frames"):
        pipeline.inbound(rt.KeySet(_u8(world.keys[0], 1, 64), device=0), torch.zeros(64, dtype=torch.uint8, device="cuda:0"),
                         _t(_u8(world.ifac_key)), 0, 16, links=rt.LinkTable(8, device=0), deliver=small)


@pytest.mark.parametrize("stage,rows,ln", [("signers", "proofs", "proof_len"), ("accept", "lr_proofs", "lr_proof_len"),
                                           ("deliver", "dest_proofs", "dest_proof_len")])
def test_a_stage_alone_writes_the_rows_it_writes_in_the_full_read(world, models, stage, rows, ln):
    frames, wire, m = models(0, mr.N, mr.ISZ)
    full = DeviceNode(world.node(), 2 * mr.N).read(wire, mr.ISZ, 2 * mr.N)
    nd = world.node().only(stage)
    alone_model = mr.compose(nd, wire, mr.ISZ, 2 * mr.N)
    alone = DeviceNode(nd, 2 * mr.N).read(wire, mr.ISZ, 2 * mr.N)
    check(alone, alone_model, mr.ISZ, stage)
    a, b = _col(alone, rows), _col(full, rows)
    la_, lb = _col(alone, ln), _col(full, ln)
    # the kind's frames: what the full read answered, but for DATA on links that only the full read's accept brings up
    mine = [i for i in range(mr.N) if lb[i] and not (stage == "signers" and m["link"][i] >= mr.PRE_LINKS)]
    assert len(mine) >= 40
    for i in mine:
        assert la_[i] == lb[i] and a[i, :la_[i]].tobytes() == b[i, :lb[i]].tobytes() == m[rows][i], (stage, i)


@pytest.mark.parametrize("layout", [0, 3])
def test_the_loop_closes_at_this_size(world, models, layout):
    import torch
    frames, wire, m = models(layout, mr.N, mr.ISZ)
    caps = layout == 3
    dev = DeviceNode(world.node(caps), 2 * mr.N)
    res = dev.read(wire, mr.ISZ, 2 * mr.N, reply={"max_replies": mr.CAPS["max_replies"]} if caps else True)
    rep = res["reply"]
    written = m["reply_counts"][0]
    stream = _col(rep, "stream")[:int(rep["frame_off"][-1])].tobytes()
    assert stream == b"".join(m["reply_frames"])
    # ---- the peers read the stream: their receipts are delivered, their links come up
    peer = mr.peer_node(world, frames)
    pm = mr.compose(peer, stream, mr.ISZ, 2 * written, reply=False)
    pdev = DeviceNode(peer, 2 * written)
    pres = pdev.read(stream, mr.ISZ, 2 * written, reply=None)
    check(pres, pm, mr.ISZ, "peer")
    check_state(pdev, pm["node"], world, [])
    by_source = [[k for k, s, _ in m["replies"] if s == src] for src in range(3)]
    assert pm["n_frames"] == written and pm["ifac_status"][:written] == [0] * written
    assert pm["lrproof_status"].count(lp.ACTIVATED) == len(by_source[0]) > 0
    assert pm["proof_status"].count(ph.DELIVERED) == len(by_source[1]) > 0
    assert pm["dproof_status"].count(dp.DELIVERED) == len(by_source[2]) > 0
    after = pm["node"]
    assert [p.state for p in after.pending.values()].count(lp.ACTIVE) == len(by_source[0])
    # ---- the node hears its own replies on a shared medium: every frame is a replay
    hashes = [rh.packet_hash(r) for _, _, r in m["replies"]]
    assert dev.seen.contains(hashes).cpu().tolist() == [1] * written
    echo = dev.read(stream, mr.ISZ, 2 * written, reply=None)
    assert int(echo["n_frames"]) == written
    assert _col(echo, "filter_status")[:written].tolist() == [fh.DUPLICATE] * written
    assert not _col(echo, "fields")[:, 0].any()
    assert not any(_col(echo, k).any() for k in ("proof_len", "lr_proof_len", "dest_proof_len"))
    torch.cuda.synchronize()
