"""Packet proofs on the inbound path (rt_link_prove, rt_proof_settle), timed
with device events on device-resident buffers.

    python tools/proof_rate.py [--steps 5] [--warmup 1] [--runs 3] [--log2 20] [--links-log2 16]
                               [--out profiles/proof_rate.json]

Shape: n = 2^log2 frames with 16-byte access codes: link DATA packets with
context NONE and 383-byte plaintexts (451-byte packets) over 2^links-log2
links, the stream of tools/link_dispatch_rate.py and tools/announce_rate.py.
Every link has a signing seed of its own and a peer key of its own.  In the
second stream one frame in 64, spread evenly, is a 115-byte proof, signed on
the device by the peer of the link it arrives on, for a receipt added before
each read (adding them is not timed); in the third every frame is one.
Prints one JSON line (also written to --out):

* "inbound": pipeline.inbound(links=table) per read, with signers and receipts
  off (the baseline of the same run), with PROVE_ALL on every link (n
  signatures per read), and over the second stream with the receipts settled
  and nothing proved;
* "prove": device.link_prove alone over the records of the first stream, and
  device.ed25519_sign with the public keys given over as many 32-byte messages;
* "settle": device.proof_settle alone over the records of the second and the
  third stream, and device.ed25519_verify over as many 32-byte messages.

Outputs are checked: every packet proved and every proof row accepted by
device.ed25519_verify under its link's public key, every proof delivered under
its receipt's id and the table empty afterwards, the link packets decrypted.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROOF_LEN = 115


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--links-log2", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proof_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(2326)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    n, n_links, plain, isz = 1 << args.log2, 1 << args.links_log2, 383, 16
    pl = 19 + rt.token_len(plain)
    result = {"tool": "tools/proof_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "runs": args.runs, "n": n, "links": n_links, "plaintext_bytes": plain,
              "packet_bytes": pl, "proof_bytes": PROOF_LEN, "ifac_size": isz, "ok": True}

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
        return {"ms": out, "median_ms": med(out)}

    # ---- the link packets, in slots of one packet's length
    ifac_key = rand(64)
    keys = rand(n_links, 64)
    ks = device.keyset(keys)
    link_ids = rand(n_links, 16)
    tab = rt.LinkTable(n_links, device=0)
    check(bool((tab.insert(link_ids, torch.arange(n_links, dtype=torch.int32, device=dev)) == 0).all()))
    which = torch.randperm(n, device=dev, generator=g) % n_links
    links_flat = torch.empty(n * pl, dtype=torch.uint8, device=dev)
    rows = links_flat.view(n, pl)
    device.encrypt_uniform(ks, rand(n, plain), plain, rand(n, 16), rows[:, 19:], key_idx=which.to(torch.int32))
    off = torch.arange(n, dtype=torch.int64, device=dev) * pl
    device.pack_headers(torch.full((n,), 3 << 2, dtype=torch.uint8, device=dev),      # LINK destination, DATA
                        torch.zeros(n, dtype=torch.uint8, device=dev), link_ids[which].contiguous(),
                        torch.zeros(n, dtype=torch.uint8, device=dev), links_flat, off)

    # ---- the links' signing rows; one set proves everything, the other nothing
    seeds, peer_seeds = rand(n_links, 32), rand(n_links, 32)
    peer_pub = torch.empty((n_links, 32), dtype=torch.uint8, device=dev)
    device.ed25519_public(peer_seeds, peer_pub)
    prove_all = rt.LinkSigners(seeds, peer_pub, torch.full((n_links,), rt.proof.PROVE_ALL, dtype=torch.uint8,
                                                            device=dev), device=0)
    prove_none = rt.LinkSigners(seeds, peer_pub, torch.zeros(n_links, dtype=torch.uint8, device=dev), device=0)

    # ---- n proofs, one per frame: for receipt i, arriving on link which[i], signed by that link's peer
    hashes = rand(n, 32)
    h_off = torch.arange(n, dtype=torch.int64, device=dev) * 32
    h_len = torch.full((n,), 32, dtype=torch.int32, device=dev)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    device.ed25519_sign(peer_seeds[which].contiguous(), hashes.view(-1), h_off, h_len, sig,
                        public_keys=peer_pub[which].contiguous())
    head = torch.zeros((n, 19), dtype=torch.uint8, device=dev)
    head[:, 0] = 0x0F                                                              # HEADER_1, LINK, PROOF
    head[:, 2:18] = link_ids[which]
    proofs = torch.cat([head, hashes, sig], dim=1).contiguous()
    check(proofs.shape == (n, PROOF_LEN))
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    del head

    max_pairs = 2 * n + 1
    ifac = rand(n, isz)

    def unframed(every):
        is_prf = torch.zeros(n, dtype=torch.bool, device=dev)
        if every:
            is_prf[every // 2::every] = True
        flat = links_flat.clone()
        if every:
            flat.view(n, pl)[is_prf, :PROOF_LEN] = proofs[is_prf]
        return flat, torch.where(is_prf, PROOF_LEN, pl).to(torch.int32), is_prf

    def make_stream(every):
        flat, p_len, is_prf = unframed(every)
        ml = pl + isz
        masked = torch.empty(n * ml, dtype=torch.uint8, device=dev)
        mo = torch.arange(n, dtype=torch.int64, device=dev) * ml
        device.ifac_mask(flat, off, p_len, ifac, ifac_key, masked, mo)
        framed = torch.empty(n * (2 * ml + 2), dtype=torch.uint8, device=dev)
        frame_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        device.hdlc_frame(masked, mo, p_len + isz, framed, frame_off)
        torch.cuda.synchronize()
        return framed[:int(frame_off[-1])].clone(), is_prf

    def read(stream, **kw):
        return pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, links=tab, **kw)

    result["inbound"], result["prove"], result["settle"] = {}, {}, {}

    # ---- the first stream: proving
    stream, _ = make_stream(0)
    res = read(stream, signers=prove_all)
    check(int(res["n_frames"]) == n and bool((res["status"][:n] == 0).all()))
    check(bool((res["proof_len"][:n] == PROOF_LEN).all()) and not bool(res["proof_len"][n:].any()))
    ok8 = torch.empty(n, dtype=torch.uint8, device=dev)
    device.ed25519_verify(prove_all.publics[which].contiguous(), res["proofs"][:n, 51:PROOF_LEN],
                          res["proofs"].view(-1), torch.arange(n, dtype=torch.int64, device=dev) * 128 + 19, h_len, ok8)
    check(bool((ok8 == 1).all()))
    base = timed(lambda: read(stream))
    proving = timed(lambda: read(stream, signers=prove_all))
    result["inbound"]["baseline"] = dict(base, stream_bytes=stream.numel())
    result["inbound"]["prove_all"] = dict(proving, signatures=n, added_ms=proving["median_ms"] - base["median_ms"])
    fields, route, link, status = res["fields"], res["route"], res["link"], res["status"]
    rows_out = torch.empty((max_pairs, 128), dtype=torch.uint8, device=dev)
    ln_out = torch.empty(max_pairs, dtype=torch.int32, device=dev)
    call = timed(lambda: device.link_prove(fields, route, link, status, prove_all, rows_out, ln_out))
    check(bool((ln_out[:n] == PROOF_LEN).all()) and torch.equal(rows_out[:n, :PROOF_LEN], res["proofs"][:n, :PROOF_LEN]))
    msgs = fields[:n, 52:84].contiguous()
    sd, pk = seeds[which].contiguous(), prove_all.publics[which].contiguous()
    sig_out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    plain_sign = timed(lambda: device.ed25519_sign(sd, msgs.view(-1), h_off, h_len, sig_out, public_keys=pk))
    check(torch.equal(sig_out, rows_out[:n, 51:PROOF_LEN]))
    result["prove"] = {"n": n, "link_prove": call, "ed25519_sign": plain_sign,
                       "signatures_per_s": n / (call["median_ms"] * 1e-3),
                       "ratio_to_ed25519_sign": call["median_ms"] / plain_sign["median_ms"]}
    del res, stream, fields, route, link, status, rows_out, msgs, sd, pk, sig_out

    # ---- the second and third stream: settling
    for name, every in (("one_in_64", 64), ("all", 1)):
        flat, p_len, is_prf = unframed(every)
        m = int(is_prf.sum())
        receipts = rt.ReceiptTable(m, device=0)
        mine, mine_ids = hashes[is_prf].contiguous(), ids[:m].contiguous()

        def refill():
            check(bool((receipts.add(mine, mine_ids) == 0).all()))

        entry = {"n": n, "proofs": m}
        if every == 64:
            stream, _ = make_stream(every)
            refill()
            res = read(stream, signers=prove_none, receipts=receipts)
            check(int(res["n_frames"]) == n and bool((res["proof_status"][:n][is_prf] == 0).all()))
            check(torch.equal(res["receipt"][:n][is_prf], mine_ids) and bool((res["receipt"][:n][~is_prf] == -1).all()))
            check(bool((res["status"][:n][~is_prf] == 0).all()) and not bool(res["proof_len"].any()))
            check(len(receipts) == 0)
            del res
            base = timed(lambda: read(stream))
            settling = timed(lambda: read(stream, signers=prove_none, receipts=receipts), prepare=refill)
            result["inbound"]["settle_one_in_64"] = dict(settling, proofs=m, baseline_same_stream=base,
                                                         added_ms=settling["median_ms"] - base["median_ms"])
            del stream
        rec = torch.empty((n, 96), dtype=torch.uint8, device=dev)
        device.packet_unpack(flat, off, p_len, rec)
        link = which.to(torch.int32)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        rc = torch.empty(n, dtype=torch.int32, device=dev)
        entry["proof_settle"] = timed(lambda: device.proof_settle(flat, off, rec, link, prove_none, receipts, st, rc),
                                      prepare=refill)
        check(bool((st[is_prf] == 0).all()) and torch.equal(rc[is_prf], mine_ids) and bool((st[~is_prf] == 1).all()))
        check(len(receipts) == 0)
        keys_m, sig_m = peer_pub[which[is_prf]].contiguous(), sig[is_prf].contiguous()
        entry["ed25519_verify"] = timed(lambda: device.ed25519_verify(keys_m, sig_m, mine.view(-1), h_off[:m].contiguous(),
                                                                      h_len[:m].contiguous(), ok8[:m]))
        check(bool((ok8[:m] == 1).all()))
        entry["proofs_per_s"] = m / (entry["proof_settle"]["median_ms"] * 1e-3)
        entry["ratio_to_ed25519_verify"] = entry["proof_settle"]["median_ms"] / entry["ed25519_verify"]["median_ms"]
        result["settle"][name] = entry
        del flat, rec, receipts, keys_m, sig_m, mine

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not result["ok"]:
        raise SystemExit("an output check failed")


if __name__ == "__main__":
    main()
