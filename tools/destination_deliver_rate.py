"""Destination delivery on the inbound path (rt_destination_deliver), timed with
device events on device-resident buffers.

    python tools/destination_deliver_rate.py [--steps 5] [--warmup 1] [--runs 5] [--log2 20] [--links-log2 16]
                                             [--out profiles/destination_deliver_rate.json]

Prints one JSON line (also written to --out):

* "stage": device.destination_deliver alone over n = 2^log2 HEADER_1 packets
  of 383-byte plaintexts to one destination without ratchets, every one opening
  on candidate 0 (the identity's key), with PROVE_ALL and without;
* "composed": what the same work costs as the separate device calls it
  replaces, in the same run: device.derive_keyset_x25519 with ``point_off``
  (exchange, HKDF, key setup), device.decrypt with ``key_idx`` and, for
  PROVE_ALL, device.ed25519_sign over the packet hashes.  The host round trips
  between them are not in it; "ratio_to_composed" and whether it is beyond the
  spreads follow;
* "second_pass": the same packets opening on rank 1 of 2 ratchets, and on the
  identity's key after 4 ratchets (retry_trials n and 4n), without proofs;
* "inbound": pipeline.inbound per read of n frames with 16-byte access codes
  over 2^links-log2 links (451-byte link DATA packets) with ``deliver=None`` and
  with ``deliver``: no SINGLE packet in the read, one frame in 64, every frame.

Every figure is --runs medians of --steps timed calls; "spread" is (max - min)
/ median of those medians.  Outputs are checked: every packet DELIVERED with
its plaintext, the composed path's plaintexts and signatures equal the stage's.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN = 383


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--links-log2", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "destination_deliver_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(2188)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    def i32(n, fill=None):
        return torch.empty(n, dtype=torch.int32, device=dev) if fill is None else \
            torch.full((n,), fill, dtype=torch.int32, device=dev)

    n, n_links, isz = 1 << args.log2, 1 << args.links_log2, 16
    tl = rt.token_len(PLAIN)
    pl = 19 + 32 + tl                                   # a SINGLE packet: header, ephemeral key, token
    result = {"tool": "tools/destination_deliver_rate.py", "device": torch.cuda.get_device_name(0),
              "steps": args.steps, "warmup": args.warmup, "runs": args.runs, "n": n, "links": n_links,
              "plaintext_bytes": PLAIN, "packet_bytes": pl, "ifac_size": isz, "ok": True}
    try:
        result["sclk_mhz"] = torch.cuda.clock_rate()
    except Exception:
        result["sclk_mhz"] = None

    def check(cond):
        result["ok"] = result["ok"] and bool(cond)

    med = lambda v: sorted(v)[len(v) // 2]           # noqa: E731

    def timed(fn):
        out = []
        for _ in range(args.runs):
            ms = []
            for k in range(args.warmup + args.steps):
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

    # ---- one identity, its ratchets, and n packets sealed for a chosen candidate
    prv, seed, id_hash, dest_hash = rand(1, 32), rand(1, 32), rand(1, 16), rand(1, 16)
    ratchets = rand(4, 32)
    plain = rand(n, PLAIN)
    off = torch.arange(n, dtype=torch.int64, device=dev) * pl
    p_len = i32(n, pl)

    def packets(target_prv):
        """(flat, fields) of n packets whose tokens open under target_prv."""
        eph = rand(n, 32)
        flat = torch.zeros(n * pl, dtype=torch.uint8, device=dev)
        rows = flat.view(n, pl)
        target_pub = torch.empty((1, 32), dtype=torch.uint8, device=dev)
        device.x25519(target_prv, None, target_pub)
        device.x25519(eph, None, rows[:, 19:51])                                    # the ephemeral public keys
        sender = device.derive_keyset_x25519(eph, target_pub, salt=id_hash.expand(n, 16), n=n)
        device.encrypt_uniform(sender, plain, PLAIN, rand(n, 16), rows[:, 51:],
                               key_idx=torch.arange(n, dtype=torch.int32, device=dev))
        z = torch.zeros(n, dtype=torch.uint8, device=dev)
        device.pack_headers(z, z, dest_hash.expand(n, 16).contiguous(), z, flat, off)
        fields = torch.empty((n, 96), dtype=torch.uint8, device=dev)
        device.packet_unpack(flat, off, p_len, fields)
        torch.cuda.synchronize()
        del sender
        return flat, fields

    out = dict(pt_off=torch.zeros(n, dtype=torch.int64, device=dev), pt_len=i32(n), status=i32(n), dstatus=i32(n),
               dest=i32(n), ratchet=i32(n), proofs=torch.empty((n, 128), dtype=torch.uint8, device=dev), plen=i32(n))

    def destinations(n_ratchets, flags, retry):
        return rt.SingleDestinations(dest_hash, prv, id_hash, seed, [flags], [[bytes(r.tolist()) for r in
                                                                               ratchets[:n_ratchets].cpu()]],
                                     max_frames=n, retry_trials=retry, device=0)

    def stage(d, flat, fields, pt):
        device.destination_deliver(d, flat, off, fields, pt, out["pt_off"], out["pt_len"], out["status"],
                                   out["dstatus"], out["dest"], out["ratchet"], out["proofs"], out["plen"])

    def delivered(pt, want_ratchet):
        check(bool((out["dstatus"] == 0).all()) and bool((out["ratchet"] == want_ratchet).all()))
        check(bool((out["pt_len"] == PLAIN).all()) and torch.equal(pt.view(n, pl)[:, 51:51 + PLAIN], plain))

    flat, fields = packets(prv)
    pt = torch.zeros_like(flat)
    result["stage"] = {}
    for name, flags in (("prove_all", rt.destination.PROVE_ALL), ("no_proof", 0)):
        d = destinations(0, flags, 0)
        entry = timed(lambda: stage(d, flat, fields, pt))
        delivered(pt, -1)
        check(bool((out["plen"] == (83 if flags else 0)).all()))
        entry.update(packets_per_s=n / (entry["median_ms"] * 1e-3))
        result["stage"][name] = entry
        if flags:
            stage_sig = out["proofs"][:, 19:83].clone()
        del d
    # ---- the same work as the separate calls
    tok_off, tok_len = off + 51, i32(n, tl)
    pt2, st2, len2 = torch.zeros_like(flat), i32(n), i32(n)
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    hashes = fields[:, 52:84].contiguous()             # rt_packet_fields.packet_hash
    h_off, h_len = torch.arange(n, dtype=torch.int64, device=dev) * 32, i32(n, 32)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    pub = torch.empty((1, 32), dtype=torch.uint8, device=dev)
    device.ed25519_public(seed, pub)
    holder = {}

    def derive():
        holder["ks"] = device.derive_keyset_x25519(prv, flat, salt=id_hash.expand(n, 16), point_off=off + 19, n=n)

    derive()
    comp = {
        "derive_keyset_x25519": timed(derive),
        "decrypt": timed(lambda: device.decrypt(holder["ks"], flat, tok_off, tok_len, pt2, tok_off, len2, st2,
                                                key_idx=idx)),
        "ed25519_sign": timed(lambda: device.ed25519_sign(seed.expand(n, 32), hashes.view(-1), h_off, h_len, sig,
                                                          public_keys=pub.expand(n, 32))),
    }
    check(bool((st2 == 0).all()) and torch.equal(pt2.view(n, pl)[:, 51:51 + PLAIN], plain))
    check(torch.equal(sig, stage_sig))
    with_sign = sum(v["median_ms"] for v in comp.values())
    without = with_sign - comp["ed25519_sign"]["median_ms"]
    comp.update(n=n, sum_ms_prove_all=with_sign, sum_ms_no_proof=without)
    result["composed"] = comp
    for name, total in (("prove_all", with_sign), ("no_proof", without)):
        e = result["stage"][name]
        e["ratio_to_composed"] = e["median_ms"] / total
        spread = max(e["spread"], max(v["spread"] for k, v in comp.items() if isinstance(v, dict)))
        e["beyond_spread"] = abs(e["ratio_to_composed"] - 1.0) > spread
    del holder["ks"], pt2, sig
    torch.cuda.empty_cache()

    # ---- the second pass
    result["second_pass"] = {}
    for name, n_ratchets, target, want in (("rank_1_of_2", 2, ratchets[1:2], 1), ("identity_after_4", 4, prv, -1)):
        f2, fld2 = packets(target)
        d = destinations(n_ratchets, 0, n * n_ratchets)
        entry = timed(lambda: stage(d, f2, fld2, pt))
        delivered(pt, want)
        entry.update(candidates_tried=(want + 1 if want >= 0 else n_ratchets + 1),
                     packets_per_s=n / (entry["median_ms"] * 1e-3))
        result["second_pass"][name] = entry
        del d, f2, fld2
        torch.cuda.empty_cache()

    # ---- inside the read: n frames over n_links links, some of them SINGLE packets
    lpl = 19 + tl
    ifac_key = rand(64)
    ks = device.keyset(rand(n_links, 64))
    link_ids = rand(n_links, 16)
    which = torch.randperm(n, device=dev, generator=g) % n_links
    links_flat = torch.zeros(n * pl, dtype=torch.uint8, device=dev)
    rows = links_flat.view(n, pl)
    device.encrypt_uniform(ks, plain, PLAIN, rand(n, 16), rows[:, 19:19 + tl], key_idx=which.to(torch.int32))
    z = torch.zeros(n, dtype=torch.uint8, device=dev)
    device.pack_headers(torch.full((n,), 3 << 2, dtype=torch.uint8, device=dev), z, link_ids[which].contiguous(), z,
                        links_flat, off)
    ifac = rand(n, isz)
    max_pairs = 2 * n + 1
    tab = rt.LinkTable(n_links, device=0)
    tab.insert(link_ids, torch.arange(n_links, dtype=torch.int32, device=dev))
    d = destinations(0, rt.destination.PROVE_ALL, 0)
    d_big = rt.SingleDestinations(dest_hash, prv, id_hash, seed, [rt.destination.PROVE_ALL], max_frames=max_pairs,
                                  retry_trials=0, device=0)
    del d

    def make_stream(every):
        single = torch.zeros(n, dtype=torch.bool, device=dev)
        if every:
            single[every // 2::every] = True
        mixed = links_flat.clone()
        if every:
            mixed.view(n, pl)[single] = flat.view(n, pl)[single]
        length = torch.where(single, pl, lpl).to(torch.int32)
        ml = pl + isz
        masked = torch.empty(n * ml, dtype=torch.uint8, device=dev)
        mo = torch.arange(n, dtype=torch.int64, device=dev) * ml
        device.ifac_mask(mixed, off, length, ifac, ifac_key, masked, mo)
        framed = torch.empty(n * (2 * ml + 2), dtype=torch.uint8, device=dev)
        frame_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        device.hdlc_frame(masked, mo, length + isz, framed, frame_off)
        torch.cuda.synchronize()
        return framed[:int(frame_off[-1])].clone(), single

    result["inbound"] = {}
    for name, every in (("no_single", 0), ("one_in_64", 64), ("all", 1)):
        stream, single = make_stream(every)
        m = int(single.sum())

        def read(**kw):
            return pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, links=tab, **kw)

        res = read(deliver=d_big)
        check(int(res["n_frames"]) == n)
        check(int((res["deliver_status"][:n] == 0).sum()) == m and bool((res["status"][:n] == 0).all()))
        check(int((res["dest_proof_len"][:n] == 83).sum()) == m)
        del res
        entry = {"single_packets": m, "stream_bytes": stream.numel(),
                 "without_deliver": timed(lambda: read()), "with_deliver": timed(lambda: read(deliver=d_big))}
        entry["added_ms"] = entry["with_deliver"]["median_ms"] - entry["without_deliver"]["median_ms"]
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
