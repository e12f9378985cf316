"""Link request proofs on the inbound path (rt_link_establish), timed with
device events on device-resident buffers.

    python tools/link_proof_rate.py [--steps 5] [--warmup 1] [--runs 5] [--log2 20] [--links-log2 16]
                                    [--out profiles/link_proof_rate.json]

Prints one JSON line (also written to --out):

* "stage": device.link_establish alone over n = 2^log2 LRPROOFs (118-byte
  HEADER_1 packets with signalling bytes, signed by four destination
  identities, one per pending link, every one activated into an empty link
  table, a key set and signers of n rows) and over one proof against the same
  n pending links; every timed call gets an empty table and rows that are
  PENDING again (made before it, untimed);
* "composed": what the same work costs as the separate calls that exist
  without the stage, in the same run: device.ed25519_verify over the 83 signed
  bytes, link.derive_link_keys (exchange, HKDF, key setup) and
  LinkTable.insert; their sum is the yardstick of "stage".  The host round
  trips between them (the signed bytes are put together and the length, mode
  and hop rules applied on the host today) are not in it;
* "inbound": pipeline.inbound per read of n frames with 16-byte access codes
  over 2^links-log2 links (451-byte link DATA packets, the stream of
  tools/link_accept_rate.py) and as many pending links, without ``establish``
  and with it: with no proof in the read, with one frame in 64 a proof, and
  with every frame one (the k-th proof of a read proves pending link k mod
  2^links-log2: the first of each activates, the others find the link decided).

Every figure is --runs medians of --steps timed calls; "spread" is (max - min)
/ median of those medians.  Outputs are checked: every proof activated, the
link table holds them, a token encrypted under the composed key set's key
decrypts under the stage's record, the signers' rows carry the destinations'
keys.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LRPROOF_LEN, SIGNED_LEN, N_DESTS = 19 + 99, 83, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--links-log2", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_proof_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(2270)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    def i32(n, fill=None):
        return torch.empty(n, dtype=torch.int32, device=dev) if fill is None else \
            torch.full((n,), fill, dtype=torch.int32, device=dev)

    n, n_links, plain, isz = 1 << args.log2, 1 << args.links_log2, 383, 16
    n_pend = min(n, n_links)
    result = {"tool": "tools/link_proof_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "runs": args.runs, "n": n, "links": n_links, "pending_in_reads": n_pend,
              "lrproof_bytes": LRPROOF_LEN, "destinations": N_DESTS, "ifac_size": isz, "ok": True}

    def check(cond):
        result["ok"] = result["ok"] and bool(cond)

    med = lambda v: sorted(v)[len(v) // 2]           # noqa: E731

    def timed(fn, prepare=None):
        """--runs medians of --steps event-timed calls of fn; prepare runs before each, untimed."""
        out = []
        for _ in range(args.runs):
            ms = []
            for k in range(args.warmup + args.steps):
                if prepare is not None:
                    prepare()
                    torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ms.append(a.elapsed_time(b))
            out.append(med(ms))
        m = med(out)
        return {"ms": out, "median_ms": m, "spread": (max(out) - min(out)) / m}

    # ---- n pending links to four destinations, and the proof each destination sends back
    dest_seeds = rand(N_DESTS, 32)
    dest_publics = torch.empty_like(dest_seeds)
    device.ed25519_public(dest_seeds, dest_publics)
    which_dest = torch.arange(n, device=dev) % N_DESTS
    ids, prv, sig_seeds, peer = rand(n, 16), rand(n, 32), rand(n, 32), rand(n, 32)
    peer[:, 31] &= 0x7F         # peer_pub below 2^255: the stage and derive_link_keys then mean the same point
    pk = dest_publics[which_dest].contiguous()
    signalling = torch.tensor([0x20, 0x01, 0xF4], dtype=torch.uint8, device=dev).expand(n, 3)   # signalling_bytes(500, 1)
    signed = torch.cat([ids, peer, pk, signalling], dim=1).contiguous()
    s_off = torch.arange(n, dtype=torch.int64, device=dev) * SIGNED_LEN
    s_len = i32(n, SIGNED_LEN)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    device.ed25519_sign(dest_seeds[which_dest].contiguous(), signed.view(-1), s_off, s_len, sig, public_keys=pk)
    proof = torch.zeros((n, LRPROOF_LEN), dtype=torch.uint8, device=dev)
    proof[:, 0] = 0x0F                                                             # HEADER_1, LINK, PROOF
    proof[:, 2:18] = ids
    proof[:, 18] = 0xFF                                                            # LRPROOF
    proof[:, 19:83], proof[:, 83:115], proof[:, 115:118] = sig, peer, signalling
    p_flat = proof.view(-1)
    p_off = torch.arange(n, dtype=torch.int64, device=dev) * LRPROOF_LEN
    p_fields = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    device.packet_unpack(p_flat, p_off, i32(n, LRPROOF_LEN), p_fields)
    slots = torch.arange(n, dtype=torch.int32, device=dev)
    ids_host = ids.cpu().numpy()

    def pending_of(count, first_slot):
        p = rt.PendingLinks(count, device=0)
        st = p.add(ids_host[:count], prv[:count], pk[:count], sig_seeds[:count],
                   torch.full((count,), rt.link.PROVE_ALL, dtype=torch.uint8), slots[:count] + first_slot,
                   torch.ones(count, dtype=torch.int32))
        check(not st.any())
        return p

    def reset(p):
        p.row_state.zero_()
        p.rebalanced.zero_()
        p.mtu.zero_()

    # ---- the stage alone
    pending = pending_of(n, 0)
    ks = device.keyset(rand(n, 64))
    signers = rt.LinkSigners(rand(n, 32), rand(n, 32), torch.zeros(n, dtype=torch.uint8, device=dev), device=0)
    out = dict(status=i32(n), slot=i32(n), mtu=i32(n))
    holder = {}

    def fresh(size):
        def make():
            holder["tab"] = rt.LinkTable(size, device=0)
            reset(pending)
        return make

    def establish(m):
        device.link_establish(ks, holder["tab"], pending, p_flat, p_off[:m], p_fields[:m], out["status"][:m],
                              out["slot"][:m], out["mtu"][:m], signers=signers)

    result["stage"] = {}
    for m in (n, 1):
        entry = timed(lambda: establish(m), prepare=fresh(m))
        check(bool((out["status"][:m] == 0).all()) and torch.equal(out["slot"][:m], slots[:m]))
        check(bool((out["mtu"][:m] == 500).all()) and len(holder["tab"]) == m)
        check(bool((pending.row_state[:m] == rt.link.ACTIVE).all()))
        entry.update(n=m, proofs_per_s=m / (entry["median_ms"] * 1e-3))
        result["stage"]["n_%d" % m] = entry
    fresh(n)()
    establish(n)
    # the key: the record of slot i opens what the composed key set's key i sealed; and the signers' rows
    composed_ks = rt.derive_link_keys(prv, peer, ids)
    pt, iv = rand(n, 48), rand(n, 16)
    tok = torch.empty((n, rt.token_len(48)), dtype=torch.uint8, device=dev)
    device.encrypt_uniform(composed_ks, pt, 48, iv, tok, key_idx=slots)
    back, blen, bst = torch.empty((n, 64), dtype=torch.uint8, device=dev), i32(n), i32(n)
    device.decrypt_uniform(ks, tok, tok.shape[1], back, blen, bst, key_idx=slots)
    check(bool((bst == 0).all()) and torch.equal(back[:, :48], pt))
    check(torch.equal(signers.peer_publics, pk) and torch.equal(signers.seeds, sig_seeds))
    check(bool((signers.flags == rt.link.PROVE_ALL).all()))

    # ---- the same work as the separate calls
    ok8 = torch.empty(n, dtype=torch.uint8, device=dev)
    comp = {
        "ed25519_verify": timed(lambda: device.ed25519_verify(pk, sig, signed.view(-1), s_off, s_len, ok8)),
        "derive_link_keys": timed(lambda: rt.derive_link_keys(prv, peer, ids)),
        "linktable_insert": timed(lambda: holder["tab"].insert(ids, slots), prepare=fresh(n)),
    }
    check(bool((ok8 == 1).all()))
    total = sum(v["median_ms"] for v in comp.values())
    comp.update(n=n, sum_ms=total)
    result["composed"] = comp
    result["stage"]["ratio_to_composed"] = result["stage"]["n_%d" % n]["median_ms"] / total
    del ks, signers, composed_ks, tok, back, pt, iv, sig, ok8, out, holder["tab"], pending
    torch.cuda.empty_cache()

    # ---- inside the read: n frames over n_links links, n_pend links pending
    pl = 19 + rt.token_len(plain)
    ifac_key, tid = rand(64), rand(16)
    ks = device.keyset(rand(n_links + n_pend, 64))               # the links that exist, and room for the pending ones
    link_ids = rand(n_links, 16)
    which = torch.randperm(n, device=dev, generator=g) % n_links
    links_flat = torch.zeros(n * pl, dtype=torch.uint8, device=dev)
    rows = links_flat.view(n, pl)
    device.encrypt_uniform(ks, rand(n, plain), plain, rand(n, 16), rows[:, 19:], key_idx=which.to(torch.int32))
    off = torch.arange(n, dtype=torch.int64, device=dev) * pl
    device.pack_headers(torch.full((n,), 3 << 2, dtype=torch.uint8, device=dev),
                        torch.zeros(n, dtype=torch.uint8, device=dev), link_ids[which].contiguous(),
                        torch.zeros(n, dtype=torch.uint8, device=dev), links_flat, off)
    ifac = rand(n, isz)
    max_pairs = 2 * n + 1
    pending = pending_of(n_pend, n_links)

    def make_stream(every):
        is_proof = torch.zeros(n, dtype=torch.bool, device=dev)
        if every:
            is_proof[every // 2::every] = True
        flat = links_flat.clone()
        if every:
            # the k-th proof of the read proves pending link k mod n_pend
            flat.view(n, pl)[is_proof, :LRPROOF_LEN] = proof[torch.arange(int(is_proof.sum()), device=dev) % n_pend]
        p_len = torch.where(is_proof, LRPROOF_LEN, pl).to(torch.int32)
        ml = pl + isz
        masked = torch.empty(n * ml, dtype=torch.uint8, device=dev)
        mo = torch.arange(n, dtype=torch.int64, device=dev) * ml
        device.ifac_mask(flat, off, p_len, ifac, ifac_key, masked, mo)
        framed = torch.empty(n * (2 * ml + 2), dtype=torch.uint8, device=dev)
        frame_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        device.hdlc_frame(masked, mo, p_len + isz, framed, frame_off)
        torch.cuda.synchronize()
        return framed[:int(frame_off[-1])].clone(), is_proof

    def fresh_links():
        holder["tab"] = rt.LinkTable(n_links + n_pend, device=0)
        holder["tab"].insert(link_ids, torch.arange(n_links, dtype=torch.int32, device=dev))
        reset(pending)

    result["inbound"] = {}
    for name, every in (("no_proof", 0), ("one_in_64", 64), ("all", 1)):
        stream, is_proof = make_stream(every)
        m = int(is_proof.sum())
        # the distinct links the read's proofs name: each comes up once
        up = min(m, n_pend)

        def read(**kw):
            return pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, links=holder["tab"], transport_identity=tid,
                                    **kw)

        fresh_links()
        res = read(establish=pending)
        check(int(res["n_frames"]) == n)
        st = res["lrproof_status"][:n]
        check(int((st == 0).sum()) == up and int((st == 3).sum()) == m - up and int((st == 1).sum()) == n - m)
        check(bool((res["status"][:n][~is_proof] == 0).all()) and len(holder["tab"]) == n_links + up)
        del res
        entry = {"proofs": m, "activated": up, "stream_bytes": stream.numel(),
                 "without_establish": timed(lambda: read(), prepare=fresh_links),
                 "with_establish": timed(lambda: read(establish=pending), prepare=fresh_links)}
        entry["added_ms"] = entry["with_establish"]["median_ms"] - entry["without_establish"]["median_ms"]
        result["inbound"][name] = entry
        del stream

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not result["ok"]:
        raise SystemExit("an output check failed")


if __name__ == "__main__":
    main()
