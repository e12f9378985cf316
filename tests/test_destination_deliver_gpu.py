"""device.destination_deliver: the delivery stage alone, against the model of
tests/destination_deliver_helpers.py (which test_destination_deliver.py ties to
the reference).

Every call is checked in full (_check): deliver_status, destination, ratchet,
and for DELIVERED / NOT_OPENED frames the token status, pt_len and the
plaintext where pt_off points; status, pt_len and pt_off keep their sentinels
elsewhere; the PROOF packet with the sentinel bytes behind it, whole sentinel
rows where nothing was proved, and guard rows past n.  In every test that is
not about the retry budget the budget is the model's own count and no frame
may read DEFERRED."""
import numpy as np
import pytest

import destination_deliver_helpers as dd

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 3                       # rows past n that must stay untouched
I32_SENTINEL = -0x5A5A5A5B      # 0xA5A5A5A5 as int32


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def device_dests(model, max_frames, retry_trials, capacity=None):
    import reticulum_amd as rt
    d = rt.SingleDestinations([m.hash for m in model], [m.prv for m in model], [m.identity_hash for m in model],
                              [m.seed for m in model], [m.flags for m in model], [m.ratchets for m in model],
                              max_frames=max_frames, retry_trials=retry_trials, ratchet_capacity=capacity, device=0)
    assert d.publics.cpu().numpy().tobytes() == b"".join(m.public for m in model)
    return d


def stage(dests, raws, implicit=True, pt_shift=0):
    """Runs the stage over ``raws`` with sentinel-filled outputs and GUARD rows
    behind them; returns numpy arrays."""
    import torch
    from reticulum_amd import device
    n = len(raws)
    off = np.zeros(n, np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])[:-1]
    pkt = _t(np.frombuffer(b"".join(raws) + b"\0" * 16, np.uint8).copy())
    pkt_off = _t(off)
    pkt_len = _t(np.array([len(r) for r in raws], np.int32))
    fields = torch.empty((n, 96), dtype=torch.uint8, device="cuda:0")
    if n:
        device.packet_unpack(pkt, pkt_off, pkt_len, fields)
    full = n + GUARD
    i32 = lambda: torch.full((full,), I32_SENTINEL, dtype=torch.int32, device="cuda:0")      # noqa: E731
    pt = torch.full_like(pkt, SENTINEL)
    pt_off = torch.full((full,), -7, dtype=torch.int64, device="cuda:0")
    pt_len, status, dstatus, dest, ratchet, plen = (i32() for _ in range(6))
    proofs = torch.full((full, 128), SENTINEL, dtype=torch.uint8, device="cuda:0")
    device.destination_deliver(dests, pkt, pkt_off, fields, pt, pt_off[:n], pt_len[:n], status[:n], dstatus[:n],
                               dest[:n], ratchet[:n], proofs[:n], plen[:n], implicit_proof=implicit,
                               pt_shift=pt_shift)
    torch.cuda.synchronize()
    return dict(off=off, pt=pt.cpu().numpy(), pt_off=pt_off.cpu().numpy(), pt_len=pt_len.cpu().numpy(),
                status=status.cpu().numpy(), dstatus=dstatus.cpu().numpy(), dest=dest.cpu().numpy(),
                ratchet=ratchet.cpu().numpy(), plen=plen.cpu().numpy(), proofs=proofs.cpu().numpy())


def _check(raws, model, got, want, implicit=True, pt_shift=0):
    n = len(raws)
    for i, (raw, w) in enumerate(zip(raws, want)):
        tag = (i, w["status"])
        assert got["dstatus"][i] == w["status"], tag
        assert got["dest"][i] == w["dest"], tag
        assert got["ratchet"][i] == w["ratchet"], tag
        if w["status"] in (dd.DELIVERED, dd.NOT_OPENED):
            at = 35 if raw[0] & 0x40 else 19
            assert got["status"][i] == w["token_status"], tag
            assert got["pt_off"][i] == got["off"][i] + at + 32 + pt_shift, tag
            if w["status"] == dd.DELIVERED:
                p = w["plaintext"]
                assert got["pt_len"][i] == len(p), tag
                assert got["pt"][got["pt_off"][i]:got["pt_off"][i] + len(p)].tobytes() == p, tag
            elif w["token_status"] != dd.ST_BAD_PAD:
                assert got["pt_len"][i] == 0, tag
        else:
            # nothing but deliver_status, destination, ratchet and proof_len is written
            assert got["status"][i] == I32_SENTINEL and got["pt_len"][i] == I32_SENTINEL and got["pt_off"][i] == -7, tag
        if w["proof"] is not None:
            k = len(w["proof"])
            assert k == (83 if implicit else 115) and got["plen"][i] == k, tag
            assert got["proofs"][i, :k].tobytes() == w["proof"], tag
            assert (got["proofs"][i, k:] == SENTINEL).all(), tag
        else:
            assert got["plen"][i] == 0 and (got["proofs"][i] == SENTINEL).all(), tag
    # guard rows
    for name in ("pt_len", "status", "dstatus", "dest", "ratchet", "plen"):
        assert (got[name][n:] == I32_SENTINEL).all(), name
    assert (got["pt_off"][n:] == -7).all() and (got["proofs"][n:] == SENTINEL).all()
    # plaintext bytes only inside the delivered (or rejected) tokens' spans
    touched = np.zeros(len(got["pt"]), bool)
    for i, (raw, w) in enumerate(zip(raws, want)):
        if w["status"] in (dd.DELIVERED, dd.NOT_OPENED):
            at = 35 if raw[0] & 0x40 else 19
            touched[got["off"][i] + at + 32:got["off"][i] + len(raw)] = True
    assert (got["pt"][~touched] == SENTINEL).all()


def run(model, raws, retry=None, implicit=True, dests=None, pt_shift=0, allow_deferred=False):
    budget = dd.second_pass_pairs(raws, model) if retry is None else retry
    if dests is None:
        dests = device_dests(model, max(len(raws), 1), budget)
    want = dd.deliver(raws, model, dests.retry_trials, implicit=implicit)
    if not allow_deferred:
        assert all(w["status"] != dd.DEFERRED for w in want)
    got = stage(dests, raws, implicit=implicit, pt_shift=pt_shift)
    _check(raws, model, got, want, implicit=implicit, pt_shift=pt_shift)
    return got, want, dests


@pytest.fixture(scope="module")
def world():
    """Destinations with 0, 1, 2 and 5 ratchets (and enforcing ones), a pool of
    ephemeral keys, and a maker of frames by outcome."""
    rng = np.random.Generator(np.random.PCG64(2188))
    model = [dd.make_dest(rng, 0, dd.F_PROVE_ALL), dd.make_dest(rng, 1, 0), dd.make_dest(rng, 2, dd.F_PROVE_ALL),
             dd.make_dest(rng, 5, dd.F_PROVE_ALL), dd.make_dest(rng, 2, dd.F_PROVE_ALL | dd.F_ENFORCE),
             dd.make_dest(rng, 0, dd.F_ENFORCE)]
    pool = [_rb(rng, 32) for _ in range(6)]

    def frame(k, rank, pt_len=None, header2=None, context=0):
        """A packet for destination k sealed for ratchet `rank` (None: the
        identity's key; "none": a key it does not hold)."""
        pt = _rb(rng, int(rng.integers(0, 70)) if pt_len is None else pt_len)
        eph = pool[int(rng.integers(len(pool)))]
        if rank == "none":
            other = dd.make_dest(rng, 0, 0)
            data = dd.seal(dd.Dest(b"", other.prv + other.seed, model[k].identity_hash, [], 0), None, pt, eph, _rb(rng, 16))
        else:
            data = dd.seal(model[k], rank, pt, eph, _rb(rng, 16))
        return dd.packet(data, model[k].hash, header2=header2, context=context)

    def junk():
        return bytes([dd.LINK << 2, 0]) + _rb(rng, 16) + b"\x00" + _rb(rng, int(rng.integers(1, 90)))

    return dict(rng=rng, model=model, frame=frame, junk=junk)


def test_fixture_cases():
    vec = dd.vectors()
    model = dd.fixture_dests(vec)
    for implicit in (True, False):
        cases = [c for c in vec["cases"] if c["implicit_proof"] == implicit]
        raws = [c["raw"] for c in cases]
        got, want, _ = run(model, raws, implicit=implicit)
        for i, c in enumerate(cases):
            assert got["dstatus"][i] == dd.STATUS[c["expect"]], c["note"]
            assert got["ratchet"][i] == c["ratchet"], c["note"]
            if c["proof"] is not None:
                assert got["proofs"][i, :len(c["proof"])].tobytes() == c["proof"], c["note"]
            if c["plaintext"] is not None:
                o = got["pt_off"][i]
                assert got["pt"][o:o + got["pt_len"][i]].tobytes() == c["plaintext"], c["note"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_sizes_and_lane_positions(world, n):
    """Delivered frames on the first and last lane of a wave and of a
    workgroup, every winning rank (none included) and every ratchet count mixed
    in one batch."""
    f, junk, model = world["frame"], world["junk"], world["model"]
    ranks = {0: [None, "none"], 1: [0, None, "none"], 2: [0, 1, None, "none"], 3: [0, 1, 2, 3, 4, None, "none"],
             4: [0, 1, None], 5: [None]}
    kinds = [(k, r) for k in ranks for r in ranks[k]]
    raws = []
    for i in range(n):
        if i in (0, 63, 64, 255, 256, n - 1):
            raws.append(f(3, 4 if i % 2 else 0))                # delivered, first and last lanes
        elif i % 5 == 4:
            raws.append(junk())
        else:
            k, r = kinds[i % len(kinds)]
            raws.append(f(k, r))
    got, want, _ = run(model, raws)
    if n >= 63:
        assert {w["status"] for w in want} >= {dd.DELIVERED, dd.NOT_OPENED, dd.NOT_DATA}
        assert {w["ratchet"] for w in want} >= {-1, 0, 1, 2, 3, 4}


@pytest.mark.parametrize("kind", ["delivered0", "second_pass", "not_opened", "junk"])
def test_whole_waves_of_one_outcome(world, kind):
    f, junk, model = world["frame"], world["junk"], world["model"]
    make = {"delivered0": lambda: f(2, 0), "second_pass": lambda: f(2, None), "not_opened": lambda: f(2, "none"),
            "junk": junk}[kind]
    other = junk if kind != "junk" else (lambda: f(0, None))
    raws = [make() for _ in range(128)] + [other() for _ in range(64)] + [make() for _ in range(64)]
    run(model, raws)


def test_retry_budget(world):
    f, model = world["frame"], world["model"]
    # frames 0..5: the identity's key behind 1, 2, 5, 2, 1 ratchets, and a first-candidate winner in between
    raws = [f(1, None), f(2, None), f(2, 0), f(3, None), f(2, 1), f(1, None)]
    asks = [1, 2, 0, 5, 2, 1]
    total = sum(asks)
    assert dd.second_pass_pairs(raws, model) == total
    # nothing: every second-pass frame is deferred, the others are as ever
    got, want, _ = run(model, raws, retry=0, allow_deferred=True)
    assert [w["status"] == dd.DEFERRED for w in want] == [a > 0 for a in asks]
    # exactly enough
    got, want, _ = run(model, raws, retry=total)
    assert all(w["status"] == dd.DELIVERED for w in want)
    # one row short: the last undecided frame and only it
    got, want, _ = run(model, raws, retry=total - 1, allow_deferred=True)
    assert [w["status"] == dd.DEFERRED for w in want] == [False] * 5 + [True]
    # a frame whose candidates alone exceed the budget, followed by one that would fit: both
    got, want, _ = run(model, [f(3, None), f(1, None), f(2, 0)], retry=4, allow_deferred=True)
    assert [w["status"] for w in want] == [dd.DEFERRED, dd.DEFERRED, dd.DELIVERED]
    # deferred frames across a workgroup edge
    many = [f(2, None) for _ in range(300)]
    got, want, _ = run(model, many, retry=2 * 257, allow_deferred=True)
    assert [w["status"] == dd.DEFERRED for w in want] == [False] * 257 + [True] * 43


def test_twice_on_one_object_and_set_ratchets(world):
    rng, f, model = world["rng"], world["frame"], world["model"]
    raws = [f(2, 0), f(2, 1), f(2, None), f(3, 3), f(1, 0), f(0, None), f(2, "none")]
    dests = device_dests(model, 16, 32, capacity=24)
    a, want, _ = run(model, raws, dests=dests)
    b, _, _ = run(model, raws, dests=dests)                     # the scratch is reused
    for k in a:
        assert (a[k] == b[k]).all(), k
    # a new ratchet in front of destination 2's list: what was rank 0 is rank 1 now, with no new memory
    ptrs = (dests.ratchets.data_ptr(), dests.ratchet_off.data_ptr())
    fresh = _rb(rng, 32)
    old = list(model[2].ratchets)
    model[2].ratchets = [fresh] + old
    try:
        dests.set_ratchets([2], [model[2].ratchets])
        assert ptrs == (dests.ratchets.data_ptr(), dests.ratchet_off.data_ptr())
        got, want, _ = run(model, raws + [f(2, 0)], dests=dests)
        assert [w["ratchet"] for w in want[:3]] == [1, 2, -1] and want[-1]["ratchet"] == 0
        # and dropping to one ratchet: the packet for the dropped key is not opened any more
        model[2].ratchets = [fresh]
        dests.set_ratchets([2], [model[2].ratchets])
        got, want, _ = run(model, raws, dests=dests)
        assert [w["status"] for w in want[:3]] == [dd.NOT_OPENED, dd.NOT_OPENED, dd.DELIVERED]
    finally:
        model[2].ratchets = old


@pytest.mark.parametrize("pt_len", [0, 15, 16, 31, 32, 47, 48, 63, 64])
def test_token_lengths_round_the_hash_tail(world, pt_len):
    """Tokens of 64 .. 128 bytes: both sides of each step of the SHA-256 tail
    block of the tag (iv ‖ ct of 32, 48, 64, 80, 96 bytes), first and second pass."""
    f, model = world["frame"], world["model"]
    raws = [f(2, 0, pt_len), f(2, 1, pt_len), f(2, None, pt_len), f(0, None, pt_len), f(2, "none", pt_len)]
    run(model, raws, implicit=pt_len % 32 == 0, pt_shift=16 if pt_len % 2 else 0)


def test_header_2_contexts_and_explicit_proofs(world):
    rng, f, model = world["rng"], world["frame"], world["model"]
    tid = _rb(rng, 16)
    raws = [f(2, 0, header2=tid), f(0, None, header2=tid, context=0x0E), f(3, 2, context=0xFE), f(1, None, context=1)]
    run(model, raws, implicit=False)


def test_deliver_batch_host_form(world):
    import reticulum_amd as rt
    f, junk, model = world["frame"], world["junk"], world["model"]
    raws = [f(2, 1), junk(), f(0, None), f(1, "none")]
    dests = device_dests(model, 8, 16)
    want = dd.deliver(raws, model, 16)
    plain, status, dest, ratchet, proofs = rt.deliver_batch(raws, dests)
    assert plain == [w["plaintext"] for w in want] and proofs == [w["proof"] for w in want]
    assert list(status) == [w["status"] for w in want] and list(dest) == [w["dest"] for w in want]
    assert list(ratchet) == [w["ratchet"] for w in want]
    assert rt.deliver_batch([], dests)[0] == []
    with pytest.raises(ValueError):
        rt.deliver_batch(raws * 3, dests)                       # more frames than the scratch serves
