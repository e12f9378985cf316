"""Proofs for packets sent to SINGLE destinations on the inbound path
(rt_destination_proof_settle), timed with device events on device-resident
buffers.

    python tools/destination_proof_rate.py [--steps 5] [--warmup 1] [--runs 3] [--log2 20] [--links-log2 16]
                                           [--out profiles/destination_proof_rate.json]

Shape: n = 2^log2 frames with 16-byte access codes: link DATA packets with
context NONE and 383-byte plaintexts (451-byte packets) over 2^links-log2
links, the stream of tools/proof_rate.py.  The receipts belong to 4096
recipient identities; every proof is signed on the device.  Prints one JSON
line (also written to --out):

* "settle": device.destination_proof_settle alone over n explicit proofs (115
  bytes) and over n addressed implicit proofs (83 bytes), each for a receipt of
  its own added before the call (adding is not timed), and
  device.ed25519_verify over as many contiguous 32-byte messages;
* "stray": the call alone over 1024 addressed implicit proofs against a full
  table of 1024 receipts plus k = 0, 1, 2, 4 strays that validate nothing (a
  full scan each), and the added time per stray;
* "inbound": pipeline.inbound(links=table) per read without and with
  destination_receipts, in the same run: over the link frames alone; with one
  frame in 64 an addressed implicit proof for a receipt of its own; and with
  one frame in 64 a proof against a full table of 1024 (1024 addressed
  implicit proofs, the others explicit proofs of packets no longer
  outstanding), without and with 4 strays.

Outputs are checked: every proof delivered under its receipt's id and the table
empty afterwards, the strays NO_RECEIPT, the link packets decrypted.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMPLICIT_LEN, EXPLICIT_LEN = 83, 115
DELIVERED, NOT_PROOF, NO_RECEIPT = 0, 1, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--links-log2", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "destination_proof_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(2349)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    n, n_links, plain, isz, n_keys, table = 1 << args.log2, 1 << args.links_log2, 383, 16, 4096, 1024
    pl = 19 + rt.token_len(plain)
    result = {"tool": "tools/destination_proof_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "runs": args.runs, "n": n, "links": n_links, "recipients": n_keys,
              "packet_bytes": pl, "ifac_size": isz, "ok": True}

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
        return {"ms": out, "median_ms": med(out), "spread_ms": max(out) - min(out)}

    # ---- the link packets, in slots of one packet's length
    ifac_key = rand(64)
    ks = device.keyset(rand(n_links, 64))
    link_ids = rand(n_links, 16)
    tab = rt.LinkTable(n_links, device=0)
    check(bool((tab.insert(link_ids, torch.arange(n_links, dtype=torch.int32, device=dev)) == 0).all()))
    which = torch.randperm(n, device=dev, generator=g) % n_links
    links_flat = torch.empty(n * pl, dtype=torch.uint8, device=dev)
    device.encrypt_uniform(ks, rand(n, plain), plain, rand(n, 16), links_flat.view(n, pl)[:, 19:],
                           key_idx=which.to(torch.int32))
    off = torch.arange(n, dtype=torch.int64, device=dev) * pl
    device.pack_headers(torch.full((n,), 3 << 2, dtype=torch.uint8, device=dev),      # LINK destination, DATA
                        torch.zeros(n, dtype=torch.uint8, device=dev), link_ids[which].contiguous(),
                        torch.zeros(n, dtype=torch.uint8, device=dev), links_flat, off)

    # ---- n receipts, receipt i under recipient i % n_keys, and both proofs of each
    seeds = rand(n_keys, 32)
    pub = torch.empty((n_keys, 32), dtype=torch.uint8, device=dev)
    device.ed25519_public(seeds, pub)
    owner = torch.arange(n, device=dev) % n_keys
    keys = pub[owner].contiguous()
    hashes = rand(n, 32)
    h_off = torch.arange(n, dtype=torch.int64, device=dev) * 32
    h_len = torch.full((n,), 32, dtype=torch.int32, device=dev)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    device.ed25519_sign(seeds[owner].contiguous(), hashes.view(-1), h_off, h_len, sig, public_keys=keys)
    head = torch.zeros((n, 19), dtype=torch.uint8, device=dev)
    head[:, 0] = 0x03                                                              # HEADER_1, SINGLE, PROOF
    head[:, 2:18] = hashes[:, :16]
    implicit = torch.cat([head, sig], dim=1).contiguous()
    explicit = torch.cat([head, hashes, sig], dim=1).contiguous()
    check(implicit.shape == (n, IMPLICIT_LEN) and explicit.shape == (n, EXPLICIT_LEN))
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    ok8 = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    del head

    def records(rows):
        """(flat, off, fields) of the packets in ``rows`` (m, width), end to end."""
        m, width = rows.shape
        flat = torch.cat([rows.reshape(-1), torch.zeros(1, dtype=torch.uint8, device=dev)])
        o = torch.arange(m, dtype=torch.int64, device=dev) * width
        rec = torch.empty((m, 96), dtype=torch.uint8, device=dev)
        device.packet_unpack(flat, o, torch.full((m,), width, dtype=torch.int32, device=dev), rec)
        return flat, o, rec

    # ---- the call alone at full density
    result["settle"] = {}
    receipts = rt.DestinationReceipts(n, scan_trials=0, device=0)

    def refill():
        check(bool((receipts.add(hashes, ids, keys=keys) == 0).all()))

    verify = timed(lambda: device.ed25519_verify(keys, sig, hashes.view(-1), h_off, h_len, ok8))
    check(bool((ok8 == 1).all()))
    st = torch.empty(n, dtype=torch.int32, device=dev)
    rc = torch.empty(n, dtype=torch.int32, device=dev)
    for name, rows in (("explicit", explicit), ("implicit", implicit)):
        flat, o, rec = records(rows)
        call = timed(lambda: device.destination_proof_settle(flat, o, rec, receipts, st, rc), prepare=refill)
        check(bool((st == DELIVERED).all()) and torch.equal(rc, ids) and len(receipts) == 0)
        result["settle"][name] = {"n": n, "destination_proof_settle": call, "ed25519_verify": verify,
                                  "proofs_per_s": n / (call["median_ms"] * 1e-3),
                                  "ratio_to_ed25519_verify": call["median_ms"] / verify["median_ms"]}
        del flat, o, rec
    del receipts, st, rc

    # ---- the price of one stray at L = 1024: implicit proofs of receipts that are not in the table
    small = rt.DestinationReceipts(table, device=0)
    result["stray"] = {"receipts": table, "scan_trials": small.scan_trials, "strays": {}}

    def refill_small():
        small.remove(hashes[:table])
        check(bool((small.add(hashes[:table], ids[:table], keys=keys[:table]) == 0).all()))

    for k in (0, 1, 2, 4):
        flat, o, rec = records(torch.cat([implicit[:table], implicit[2 * table:2 * table + k]]))
        st = torch.empty(table + k, dtype=torch.int32, device=dev)
        rc = torch.empty(table + k, dtype=torch.int32, device=dev)
        call = timed(lambda: device.destination_proof_settle(flat, o, rec, small, st, rc), prepare=refill_small)
        check(bool((st[:table] == DELIVERED).all()) and bool((st[table:] == NO_RECEIPT).all()) and len(small) == 0)
        result["stray"]["strays"][str(k)] = call
    t0 = result["stray"]["strays"]["0"]["median_ms"]
    result["stray"]["added_ms_per_stray"] = {str(k): (result["stray"]["strays"][str(k)]["median_ms"] - t0) / k
                                             for k in (1, 2, 4)}

    # ---- reads
    max_pairs = 2 * n + 1
    ifac = rand(n, isz)

    def make_stream(flat, p_len):
        ml = pl + isz
        masked = torch.empty(n * ml, dtype=torch.uint8, device=dev)
        mo = torch.arange(n, dtype=torch.int64, device=dev) * ml
        device.ifac_mask(flat, off, p_len, ifac, ifac_key, masked, mo)
        framed = torch.empty(n * (2 * ml + 2), dtype=torch.uint8, device=dev)
        frame_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        device.hdlc_frame(masked, mo, p_len + isz, framed, frame_off)
        torch.cuda.synchronize()
        return framed[:int(frame_off[-1])].clone()

    def read(stream, **kw):
        return pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, links=tab, **kw)

    result["inbound"] = {}
    full_len = torch.full((n,), pl, dtype=torch.int32, device=dev)

    # no proof in the read
    stream = make_stream(links_flat, full_len)
    without = timed(lambda: read(stream))
    res = read(stream, destination_receipts=small)
    check(int(res["n_frames"]) == n and bool((res["status"][:n] == 0).all()))
    check(bool((res["dproof_status"][:n] == NOT_PROOF).all()))
    del res
    with_ = timed(lambda: read(stream, destination_receipts=small))
    result["inbound"]["no_proofs"] = {"without": without, "with": with_, "stream_bytes": stream.numel(),
                                      "added_ms": with_["median_ms"] - without["median_ms"]}
    del stream

    # one frame in 64 an addressed implicit proof for a receipt of its own
    is_prf = torch.zeros(n, dtype=torch.bool, device=dev)
    is_prf[32::64] = True
    m = int(is_prf.sum())
    flat = links_flat.clone()
    flat.view(n, pl)[is_prf, :IMPLICIT_LEN] = implicit[:m]
    stream = make_stream(flat, torch.where(is_prf, IMPLICIT_LEN, pl).to(torch.int32))
    mid = rt.DestinationReceipts(m, device=0)

    def refill_mid():
        check(bool((mid.add(hashes[:m], ids[:m], keys=keys[:m]) == 0).all()))

    refill_mid()
    res = read(stream, destination_receipts=mid)
    check(int(res["n_frames"]) == n and bool((res["dproof_status"][:n][is_prf] == DELIVERED).all()))
    check(torch.equal(res["dproof_receipt"][:n][is_prf], ids[:m]) and bool((res["status"][:n][~is_prf] == 0).all()))
    check(len(mid) == 0)
    del res
    without = timed(lambda: read(stream))
    with_ = timed(lambda: read(stream, destination_receipts=mid), prepare=refill_mid)
    result["inbound"]["one_in_64"] = {"proofs": m, "without": without, "with": with_,
                                      "added_ms": with_["median_ms"] - without["median_ms"]}
    del stream, mid

    # one frame in 64 a proof against a full table of 1024: 1024 addressed implicit proofs, the
    # others explicit proofs of packets no longer outstanding; then the same read with 4 strays
    spots = torch.nonzero(is_prf).view(-1)
    for name, strays in (("table_1024", 0), ("table_1024_4_strays", 4)):
        flat = links_flat.clone()
        v = flat.view(n, pl)
        v[spots[:table], :IMPLICIT_LEN] = implicit[:table]
        v[spots[table:], :EXPLICIT_LEN] = explicit[table:m]
        p_len = torch.full((n,), pl, dtype=torch.int32, device=dev)
        p_len[spots[:table]] = IMPLICIT_LEN
        p_len[spots[table:]] = EXPLICIT_LEN
        at = spots[table + 7:table + 7 + strays]
        v[at, :IMPLICIT_LEN] = implicit[m:m + strays]
        p_len[at] = IMPLICIT_LEN
        stream = make_stream(flat, p_len)
        refill_small()
        res = read(stream, destination_receipts=small)
        check(int(res["n_frames"]) == n and bool((res["dproof_status"][:n][spots[:table]] == DELIVERED).all()))
        check(bool((res["dproof_status"][:n][spots[table:]] == NO_RECEIPT).all()) and len(small) == 0)
        del res
        with_ = timed(lambda: read(stream, destination_receipts=small), prepare=refill_small)
        result["inbound"][name] = {"proofs": m, "receipts": table, "strays": strays, "with": with_}
        del stream, flat, v
    result["inbound"]["added_ms_per_stray_in_a_read"] = (
        result["inbound"]["table_1024_4_strays"]["with"]["median_ms"]
        - result["inbound"]["table_1024"]["with"]["median_ms"]) / 4

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not result["ok"]:
        raise SystemExit("an output check failed")


if __name__ == "__main__":
    main()
