"""Link requests on the inbound path (rt_link_accept), timed with device events
on device-resident buffers.

    python tools/link_accept_rate.py [--steps 5] [--warmup 1] [--runs 5] [--log2 20] [--links-log2 16]
                                     [--out profiles/link_accept_rate.json]

Prints one JSON line (also written to --out):

* "stage": device.link_accept alone over n = 2^log2 link requests (86-byte
  HEADER_1 packets with signalling bytes, to four destinations, every one
  accepted into an empty link table, a key set and signers of n rows) and over
  one request; every timed call gets an empty table (made before it, untimed);
* "composed": what the same work costs as the separate calls that exist
  without the stage, in the same run: device.x25519 on the base point (the
  public keys), link.derive_link_keys (exchange, HKDF, key setup),
  device.ed25519_sign with the public keys given over the 83 signed bytes, and
  LinkTable.insert; their sum is the yardstick of "stage".  The host round
  trips between them (the link ids, the signed bytes and the packets are put
  together on the host today) are not in it;
* "inbound": pipeline.inbound per read of n frames with 16-byte access codes
  over 2^links-log2 links (451-byte link DATA packets, the stream of
  tools/proof_rate.py) without ``accept``, with ``accept`` and no request in
  the read, with ``announces=True`` and no announce (another select pass, for
  comparison), with one frame in 64 a request, and with every frame one.

Every figure is --runs medians of --steps timed calls; "spread" is (max - min)
/ median of those medians.  Outputs are checked: every request accepted, each
packet's signature verified by device.ed25519_verify under its destination's
key, a token encrypted under nothing but the stage's record decrypts.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LRPROOF_LEN, REQ_LEN, N_DESTS = 118, 19 + 67, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--links-log2", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_accept_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(2127)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    def i32(n, fill=None):
        return torch.empty(n, dtype=torch.int32, device=dev) if fill is None else \
            torch.full((n,), fill, dtype=torch.int32, device=dev)

    n, n_links, plain, isz = 1 << args.log2, 1 << args.links_log2, 383, 16
    result = {"tool": "tools/link_accept_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "runs": args.runs, "n": n, "links": n_links, "request_bytes": REQ_LEN,
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

    # ---- the node's destinations and n requests to them
    tid = rand(16)
    dest_hashes, dest_seeds = rand(N_DESTS, 16), rand(N_DESTS, 32)
    flags = torch.full((N_DESTS,), rt.link.ACCEPTS | rt.link.PROVE_ALL, dtype=torch.uint8, device=dev)
    dests = rt.LinkDestinations(dest_hashes, dest_seeds, flags, device=0)
    which_dest = torch.arange(n, device=dev) % N_DESTS
    req = torch.zeros((n, REQ_LEN), dtype=torch.uint8, device=dev)
    req[:, 0] = 2                                                                  # HEADER_1, SINGLE, LINKREQUEST
    req[:, 2:18] = dest_hashes[which_dest]
    req[:, 19:83] = rand(n, 64)
    req[:, 50] &= 0x7F          # peer_pub below 2^255: the stage and derive_link_keys then mean the same point
    req[:, 83:86] = torch.tensor([0x20, 0x01, 0xF4], dtype=torch.uint8, device=dev)     # signalling_bytes(500, 1)
    req_flat = req.view(-1)
    req_off = torch.arange(n, dtype=torch.int64, device=dev) * REQ_LEN
    req_fields = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    device.packet_unpack(req_flat, req_off, i32(n, REQ_LEN), req_fields)
    eph = rand(n, 32)
    slots = torch.arange(n, dtype=torch.int32, device=dev)

    # ---- the stage alone
    ks = device.keyset(rand(n, 64))
    signers = rt.LinkSigners(rand(n, 32), rand(n, 32), torch.zeros(n, dtype=torch.uint8, device=dev), device=0)
    out = dict(status=i32(n), accepted=i32(n), link_id=torch.empty((n, 16), dtype=torch.uint8, device=dev),
               mtu=i32(n), proofs=torch.empty((n, 128), dtype=torch.uint8, device=dev), plen=i32(n))
    holder = {}

    def fresh(size):
        def make():
            holder["tab"] = rt.LinkTable(size, device=0)
        return make

    def accept(m):
        device.link_accept(ks, holder["tab"], dests, tid, req_flat, req_off[:m], req_fields[:m], slots[:m], eph[:m],
                           out["status"][:m], out["accepted"][:m], out["link_id"][:m], out["mtu"][:m],
                           out["proofs"][:m], out["plen"][:m], nh_mtu=500, signers=signers)

    result["stage"] = {}
    for m in (n, 1):
        entry = timed(lambda: accept(m), prepare=fresh(m))
        check(bool((out["status"][:m] == 0).all()) and torch.equal(out["accepted"][:m], slots[:m]))
        check(bool((out["plen"][:m] == LRPROOF_LEN).all()) and len(holder["tab"]) == m)
        entry.update(n=m, requests_per_s=m / (entry["median_ms"] * 1e-3))
        result["stage"]["n_%d" % m] = entry
    # each packet's signature, under its destination's key, over link id ‖ pub ‖ that key ‖ signalling
    pk = dests.publics[which_dest].contiguous()
    signed = torch.cat([out["link_id"], out["proofs"][:, 83:115], pk, out["proofs"][:, 115:118]], dim=1).contiguous()
    s_off = torch.arange(n, dtype=torch.int64, device=dev) * 83
    s_len = i32(n, 83)
    ok8 = torch.empty(n, dtype=torch.uint8, device=dev)
    device.ed25519_verify(pk, out["proofs"][:, 19:83].contiguous(), signed.view(-1), s_off, s_len, ok8)
    check(bool((ok8 == 1).all()))
    # and the key: the record of slot i opens what the composed key set's key i sealed
    composed_ks = rt.derive_link_keys(eph, req[:, 19:51].contiguous(), out["link_id"])
    pt, iv = rand(n, 48), rand(n, 16)
    tok = torch.empty((n, rt.token_len(48)), dtype=torch.uint8, device=dev)
    device.encrypt_uniform(composed_ks, pt, 48, iv, tok, key_idx=slots)
    back, blen, bst = torch.empty((n, 64), dtype=torch.uint8, device=dev), i32(n), i32(n)
    device.decrypt_uniform(ks, tok, tok.shape[1], back, blen, bst, key_idx=slots)
    check(bool((bst == 0).all()) and torch.equal(back[:, :48], pt))

    # ---- the same work as the separate calls
    pub = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    ids, peer = out["link_id"].clone(), req[:, 19:51].contiguous()
    sd = dest_seeds[which_dest].contiguous()
    comp = {
        "x25519_public": timed(lambda: device.x25519(eph, None, pub)),
        "derive_link_keys": timed(lambda: rt.derive_link_keys(eph, peer, ids)),
        "ed25519_sign": timed(lambda: device.ed25519_sign(sd, signed.view(-1), s_off, s_len, sig, public_keys=pk)),
        "linktable_insert": timed(lambda: holder["tab"].insert(ids, slots), prepare=fresh(n)),
    }
    check(torch.equal(pub, out["proofs"][:, 83:115]) and torch.equal(sig, out["proofs"][:, 19:83]))
    total = sum(v["median_ms"] for v in comp.values())
    comp.update(n=n, sum_ms=total)
    result["composed"] = comp
    result["stage"]["ratio_to_composed"] = result["stage"]["n_%d" % n]["median_ms"] / total
    del ks, signers, composed_ks, tok, back, pt, iv, signed, sig, pub, out, holder["tab"]
    torch.cuda.empty_cache()

    # ---- inside the read: n frames over n_links links
    pl = 19 + rt.token_len(plain)
    ifac_key = rand(64)
    ks = device.keyset(rand(2 * n_links, 64))                    # the links that exist, and room for as many again
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

    def make_stream(every):
        is_req = torch.zeros(n, dtype=torch.bool, device=dev)
        if every:
            is_req[every // 2::every] = True
        flat = links_flat.clone()
        if every:
            flat.view(n, pl)[is_req, :REQ_LEN] = req[is_req]
        p_len = torch.where(is_req, REQ_LEN, pl).to(torch.int32)
        ml = pl + isz
        masked = torch.empty(n * ml, dtype=torch.uint8, device=dev)
        mo = torch.arange(n, dtype=torch.int64, device=dev) * ml
        device.ifac_mask(flat, off, p_len, ifac, ifac_key, masked, mo)
        framed = torch.empty(n * (2 * ml + 2), dtype=torch.uint8, device=dev)
        frame_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        device.hdlc_frame(masked, mo, p_len + isz, framed, frame_off)
        torch.cuda.synchronize()
        return framed[:int(frame_off[-1])].clone(), is_req

    def fresh_links(extra):
        def make():
            holder["tab"] = rt.LinkTable(n_links + max(extra, 1), device=0)
            holder["tab"].insert(link_ids, torch.arange(n_links, dtype=torch.int32, device=dev))
        return make

    result["inbound"] = {}
    for name, every in (("no_request", 0), ("one_in_64", 64), ("all", 1)):
        stream, is_req = make_stream(every)
        m = int(is_req.sum())
        # free slots behind the links that exist; a read of nothing but requests has more requests than slots
        free = min(max(m, 1), n_links)
        acc = dict(destinations=dests, nh_mtu=500, ephemeral_privates=eph[:free],
                   slots=torch.arange(n_links, n_links + free, dtype=torch.int32, device=dev))

        def read(**kw):
            return pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, links=holder["tab"], transport_identity=tid,
                                    **kw)

        fresh_links(free)()
        res = read(accept=acc)
        check(int(res["n_frames"]) == n)
        st = res["linkreq_status"][:n]
        check(int((st == 0).sum()) == min(m, free) and int((st == 9).sum()) == m - min(m, free))
        check(bool((res["status"][:n][~is_req] == 0).all()))
        del res
        entry = {"requests": m, "accepted": min(m, free), "stream_bytes": stream.numel(),
                 "without_accept": timed(lambda: read(), prepare=fresh_links(free)),
                 "with_accept": timed(lambda: read(accept=acc), prepare=fresh_links(free))}
        entry["added_ms"] = entry["with_accept"]["median_ms"] - entry["without_accept"]["median_ms"]
        if not every:
            entry["with_announces"] = timed(lambda: read(announces=True), prepare=fresh_links(free))
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
