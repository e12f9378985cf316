"""The mixed read's builder and composed model (tests/mixed_read_helpers.py), on the host:
the placement rule holds for every layout, the model reproduces what
tests/test_reply_pipeline_gpu.py expects of its 8-frame world, and its token
stage agrees with the fake back end of tests/fake_native.py."""
import ctypes

import numpy as np
import pytest

import destination_deliver_helpers as dd
import destination_proof_helpers as dp
import fake_native
import filter_helpers as fh
import link_accept_helpers as la
import link_helpers as lh
import link_proof_helpers as lp
import mixed_read_helpers as mr
import proof_helpers as ph

LR, P, D = 0, 1, 2                       # device.REPLY_LRPROOF, REPLY_LINK_PROOF, REPLY_DEST_PROOF


@pytest.fixture(scope="module")
def world():
    return mr.World()


@pytest.fixture(scope="module")
def reads(world):
    """Layout -> (frames, model) with access codes, N = 577."""
    out = {}
    for layout in range(mr.LAYOUTS):
        frames = mr.build(world, layout)
        caps = layout == 3
        out[layout] = (frames, mr.compose(world.node(caps), mr.wire_of(world, frames, mr.ISZ), mr.ISZ, 2 * mr.N,
                                          max_replies=mr.CAPS["max_replies"] if caps else None))
    return out


def test_placement_holds_for_every_layout(world):
    edges = [e for e in mr.EDGES if e < mr.N]
    assert edges == [0, 63, 64, 255, 256, 511, 512, 575, 576] and mr.N == 2 * 256 + 64 + 1
    on_every_edge = set()
    for n in (mr.N, mr.N_SCAN):
        for layout in range(mr.LAYOUTS):
            kinds = mr.kinds_of(layout, n)
            assert len(kinds) == n
            for kind in mr.REPLY_KINDS:
                if all(kinds[e] == kind for e in mr.EDGES if e < n):
                    on_every_edge.add((n, kind))
            assert all(kinds[i] == mr.NOISE for i in mr.NOISE_WAVE)                  # a whole wave of noise
            assert len({kinds[i] for i in mr.REPLY_WAVE}) == 1 and kinds[mr.REPLY_WAVE[0]] in mr.REPLY_KINDS
            assert mr.NOISE_WAVE[0] % 64 == 0 and len(mr.NOISE_WAVE) == 64
            assert mr.REPLY_WAVE[0] % 64 == 0 and len(mr.REPLY_WAVE) == 64
            # the meetings sit in different workgroups of every 256-thread stage
            for a, b in ((mr.DATA_A, mr.DATA_B), (mr.SINGLE_A, mr.SINGLE_B), (mr.REQUEST_A, mr.REQUEST_B),
                         (mr.PROOF_A, mr.PROOF_B)):
                assert a // 256 != b // 256 and kinds[a] == kinds[b] == mr.MEETING
            assert set(mr.CYCLE) <= set(kinds)
        kinds = mr.kinds_of(3, n)
        assert kinds.count(mr.LRPROOF) == 1 and kinds[n - 1] == mr.LRPROOF           # once, at the last frame
    assert on_every_edge == {(n, k) for n in (mr.N, mr.N_SCAN) for k in mr.REPLY_KINDS}
    assert mr.N_SCAN == 1024 + 1                                                     # SCAN_BLOCK and RG_BLOCK frames, and one


def test_the_frames_are_what_their_kind_says(world, reads):
    for layout, (frames, m) in reads.items():
        kinds = mr.kinds_of(layout)
        n = mr.N
        assert m["n_frames"] == n and m["counts"][0] == 2 * n - 1
        lr, pr, dpf = mr.lengths(m["lr_proofs"]), mr.lengths(m["proofs"]), mr.lengths(m["dest_proofs"])
        for i, kind in enumerate(kinds):
            if kind == mr.BAD_CODE:
                assert m["ifac_status"][i] == 2 and not m["ok"][i]
            elif kind == mr.LINK_PROVED:
                assert pr[i] == 115 and m["status"][i] == 0 and m["route"][i] == lh.LINK_DECRYPT
            elif kind == mr.REQUEST:
                assert m["linkreq_status"][i] == la.ACCEPTED and lr[i] == 118
            elif kind == mr.OTHER_TRANSPORT:
                assert m["filter_status"][i] == fh.OTHER_TRANSPORT
            elif kind == mr.NOISE:
                assert lr[i] == pr[i] == dpf[i] == 0 and m["status"][i] != 0
            elif kind == mr.LINK_PLAIN:
                assert pr[i] == 0 and m["link"][i] in (2, 3)
            elif kind == mr.LRPROOF:
                assert m["lrproof_status"][i] == lp.ACTIVATED and m["established_link"][i] == mr.PENDING_SLOT
        if layout != 3:
            for i, kind in enumerate(kinds):
                if kind == mr.SINGLE_PROVED:
                    assert m["deliver_status"][i] == dd.DELIVERED and dpf[i] == 83
                elif kind == mr.SINGLE_PLAIN:
                    assert m["deliver_status"][i] == dd.DELIVERED and dpf[i] == 0
            assert dd.DEFERRED not in m["deliver_status"] and dp.DEFERRED not in m["dproof_status"]
            assert m["reply_counts"][0] == m["reply_counts"][1]
        # the meetings: the lower index wins
        assert m["filter_status"][mr.DATA_A] == fh.PASS and m["filter_status"][mr.DATA_B] == fh.DUPLICATE
        assert m["filter_status"][mr.SINGLE_A] == fh.PASS and m["filter_status"][mr.SINGLE_B] == fh.DUPLICATE
        assert pr[mr.DATA_A] == 115 and pr[mr.DATA_B] == 0 and dpf[mr.SINGLE_A] == 83 and dpf[mr.SINGLE_B] == 0
        assert m["linkreq_status"][mr.REQUEST_A] == la.ACCEPTED and m["linkreq_status"][mr.REQUEST_B] == la.DUPLICATE
        assert m["link_id"][mr.REQUEST_A] == m["link_id"][mr.REQUEST_B] != bytes(16)
        assert m["proof_status"][mr.PROOF_A] == ph.DELIVERED and m["proof_status"][mr.PROOF_B] == ph.NO_RECEIPT
        assert m["receipt"][mr.PROOF_A] == mr.POOL - 1
        # same-read ordering: DATA behind its request is decrypted and proved, as the reference's loop does it; DATA
        # ahead of it too (pipeline.inbound's docstring, "One difference: a link packet that precedes its request in
        # the same read is dispatched too"), exactly once in the read
        slot = m["accepted_link"][mr.REQUEST_A]
        for i, text in ((mr.LATE_DATA, b"behind its request"), (mr.EARLY_DATA, b"ahead of its request")):
            assert m["link"][i] == m["key_idx"][i] == slot and m["status"][i] == 0 and m["pt"][i] == text and pr[i] == 115
        early = [i for i in range(n) if m["link"][i] >= mr.FIRST_SLOT
                 and i < m["accepted_link"].index(m["link"][i])]
        assert early == [mr.EARLY_DATA]
        # every status a stage can give for these kinds turns up
        assert {dp.DELIVERED, dp.NOT_PROOF, dp.ON_LINK, dp.BAD_SIGNATURE} <= set(m["dproof_status"])
        assert {ph.DELIVERED, ph.NO_RECEIPT, ph.BAD_SIGNATURE} <= set(m["proof_status"])
        assert {0, 3} <= set(m["announce_status"][:n])


def test_the_caps_defer_whole_frames_in_frame_order(world, reads):
    frames, m = reads[3]
    free = mr.compose(world.node(False), mr.wire_of(world, frames, mr.ISZ), mr.ISZ, 2 * mr.N)
    # delivery: a frame that asks for more than is left of retry_trials is DEFERRED with every undecided frame behind it
    st, full = m["deliver_status"], free["deliver_status"]
    deferred = [i for i, s in enumerate(st) if s == dd.DEFERRED]
    assert deferred and all(full[i] == dd.DELIVERED for i in deferred)
    second_pass = [i for i in range(mr.N) if full[i] == dd.DELIVERED and
                   free["ratchet"][i] != 0 and len(world.dests[free["destination"][i]].candidates()) > 1]
    asks = [len(world.dests[free["destination"][i]].candidates()) - 1 for i in second_pass]
    fit = sum(1 for k in range(len(asks)) if sum(asks[:k + 1]) <= mr.CAPS["retry_trials"])
    assert deferred == second_pass[fit:] and [st[i] for i in second_pass[:fit]] == [dd.DELIVERED] * fit
    assert all(m["dest_proofs"][i] is None and m["pt"][i] == b"" for i in deferred)
    # destination proofs: stray r is tried when (r + 1) * L <= scan_trials
    strays = [i for i, s in enumerate(m["dproof_status"]) if s == dp.DEFERRED]
    # (the first stray fits and is delivered; of the two behind it one would have been, one proves nothing known)
    assert [free["dproof_status"][i] for i in strays] == [dp.DELIVERED, dp.NO_RECEIPT]
    first = next(i for i, (_, raw) in enumerate(frames) if raw == world.instance(mr.DEST_PROOF, 5))
    assert first < strays[0] and m["dproof_status"][first] == free["dproof_status"][first] == dp.DELIVERED
    # replies: [written, found], found > written, and the written ones are the first in frame order
    written, found = m["reply_counts"]
    assert written == mr.CAPS["max_replies"] < found == free["reply_counts"][1] - \
        sum(1 for i in deferred if free["dest_proofs"][i])
    uncapped = [r for r in free["replies"] if r[0] not in deferred]
    assert m["replies"] == uncapped[:written]


def test_the_model_reproduces_the_reply_tests_expectations():
    w = mr.reply_world()
    m = mr.compose(mr.reply_node(w), mr.reply_wire(w), mr.ISZ, 32)
    at = {name: i for i, (name, _) in enumerate(w["frames"])}
    assert m["n_frames"] == 8
    assert mr.lengths(m["proofs"])[:8] == [115, 0, 0, 0, 115, 0, 0, 115]
    assert mr.lengths(m["lr_proofs"])[:8] == [0, 0, 0, 118, 0, 0, 0, 0]
    assert mr.lengths(m["dest_proofs"])[:8] == [0, 0, 83, 0, 0, 83, 0, 0]
    assert m["reply_counts"] == [6, 6]
    assert [k for k, _, _ in m["replies"]] == [at[x] for x in ("link 0", "single 0", "request", "link 1", "single 1",
                                                              "link 0 again")]
    assert [s for _, s, _ in m["replies"]] == [P, D, LR, P, D, P]
    assert [len(r) for _, _, r in m["replies"]] == [115, 83, 118, 115, 83, 115]
    assert not any(sum(mr.lengths(m[k])[8:]) for k in ("proofs", "lr_proofs", "dest_proofs"))
    capped = mr.compose(mr.reply_node(w, seen=False), mr.reply_wire(w), mr.ISZ, 32, max_replies=4)
    assert capped["reply_counts"] == [4, 6] and capped["replies"] == m["replies"][:4]
    # the node's own replies are in its list afterwards: an echo is a replay
    assert m["node"].seen.contains([mr.rh.packet_hash(r) for _, _, r in m["replies"]]) == [1] * 6
    echo = mr.compose(m["node"], b"".join(m["reply_frames"]), mr.ISZ, 32, reply=False)
    assert echo["filter_status"][:6] == [fh.DUPLICATE] * 6 and not any(echo["ok"])


def test_the_read_reaches_what_a_wrong_rank_or_order_would_break(world, reads):
    """Where a select kernel's wave-level append or the gather's order could be
    wrong, the read has frames that would show it: candidates of every stage in
    the last lane of a wave with more candidates behind them, waves with none,
    and replies whose frame order is not their source order."""
    last_lane = {k: set() for k in ("proofs", "lr_proofs", "dest_proofs", "filter", "settle", "dsettle")}
    for layout, (frames, m) in reads.items():
        cand = {k: [i for i in range(mr.N) if m[k][i]] for k in ("proofs", "lr_proofs", "dest_proofs")}
        cand["filter"] = [i for i in range(mr.N) if m["filter_status"][i] == fh.PASS]
        cand["settle"] = [i for i in range(mr.N) if m["proof_status"][i] in (ph.DELIVERED, ph.NO_RECEIPT, ph.BAD_SIGNATURE)]
        cand["dsettle"] = [i for i in range(mr.N) if m["dproof_status"][i] in (dp.DELIVERED, dp.NO_RECEIPT,
                                                                                dp.BAD_SIGNATURE, dp.DEFERRED)]
        for k, c in cand.items():
            waves = {i // 64 for i in c}
            last_lane[k] |= {i for i in c if i % 64 == 63 and len([j for j in c if j // 64 == i // 64]) > 1
                             and any(j > i for j in c)}
            if k != "filter":
                assert mr.NOISE_WAVE[0] // 64 not in waves, (layout, k)         # an empty ballot in every select kernel
        # the gather: frame-major order is not source-major order, inside what max_replies leaves too, and some
        # 128-byte line's worth of consecutive replies holds all three sources
        replies = [(k, s) for k, s, _ in m["replies"]]
        assert replies == sorted(replies) != sorted(replies, key=lambda r: (r[1], r[0]))
        assert any({s for _, s in replies[j:j + 8]} == {LR, P, D} for j in range(len(replies) - 8))
        assert [r for r in replies if r[0] in (63, 64, 255, 256, 511, 512)]
    assert all(last_lane.values()), {k: sorted(v) for k, v in last_lane.items()}


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_the_token_stage_agrees_with_the_fake_back_end(world, reads):
    """Of the stages of a read, fake_native implements the token's: decrypt
    (rt_decrypt_host), the tag check (rt_verify_host) and the key derivation
    (rt_hkdf_host).  The model's key_idx, status and plaintext per frame, and
    the records the accepted links' keys were derived into, against them."""
    frames, m = reads[0]
    keys = m["node"].keys                                       # after the read: the accepted links' records are in
    fake = fake_native.FakeLib()
    ks = fake.rt_keyset_create(1, np.frombuffer(b"".join(keys), np.uint8).ctypes.data, 64, len(keys))
    idx = [i for i in range(mr.N) if m["route"][i] == lh.LINK_DECRYPT]
    assert len(idx) > 100 and any(m["key_idx"][i] >= mr.FIRST_SLOT for i in idx)
    toks = [frames[i][1][19:] for i in idx]
    n = len(idx)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum([len(t) for t in toks])[:-1]
    ln = np.array([len(t) for t in toks], np.uint32)
    tok = np.frombuffer(b"".join(toks), np.uint8).copy()
    pt, pt_len, status = np.zeros(tok.size, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.int32)
    ki = np.array([m["key_idx"][i] for i in idx], np.uint32)
    ptr = _ptr
    assert fake.rt_decrypt_host(ks, ptr(tok), ptr(off), ptr(ln), ptr(ki), ptr(pt), ptr(off), ptr(pt_len), ptr(status),
                                n) == 0
    assert status.tolist() == [m["status"][i] for i in idx] and 2 in status
    for j, i in enumerate(idx):
        if status[j] == 0:
            assert pt[int(off[j]):int(off[j]) + int(pt_len[j])].tobytes() == m["pt"][i], i
    verified = np.zeros(n, np.int32)
    assert fake.rt_verify_host(ks, ptr(tok), ptr(off), ptr(ln), ptr(ki), ptr(verified), n) == 0
    assert verified.tolist() == [m["status"][i] for i in idx]                 # no token here verifies and then fails
    # the key record of every link the read accepted: hkdf(64, X25519(ephemeral of its rank, the request's key), link id)
    acc = [i for i in range(mr.N) if m["linkreq_status"][i] == la.ACCEPTED]
    assert len(acc) >= 40
    ikm = np.frombuffer(b"".join(la.x25519(world.ephemerals[m["accepted_link"][i] - mr.FIRST_SLOT], frames[i][1][19:51])
                                 for i in acc), np.uint8).copy()
    salt = np.frombuffer(b"".join(m["link_id"][i] for i in acc), np.uint8).copy()
    out = np.zeros(64 * len(acc), np.uint8)
    assert fake.rt_hkdf_host(1, ptr(ikm), 32, 32, ptr(salt), 16, 16, None, 0, ptr(out), 64, 64, len(acc)) == 0
    assert out.tobytes() == b"".join(keys[m["accepted_link"][i]] for i in acc)
