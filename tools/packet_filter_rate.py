"""Transport's packet filter on the inbound path (rt_packet_filter,
rt_hashlist_*), timed with device events on device-resident buffers.

    python tools/packet_filter_rate.py [--steps 5] [--warmup 1] [--runs 3] [--log2 20] [--links-log2 16]
                                       [--preload 500000] [--out profiles/packet_filter_rate.json]

Shape: n = 2^log2 link DATA packets with 383-byte plaintexts (a 451-byte
packet) and 16-byte access codes over 2^links-log2 links, the stream of
tools/link_dispatch_rate.py.  The hash list is made for 2n hashes and
preloaded with --preload others.  Prints one JSON line (also written to --out):

* "inbound": pipeline.inbound(links=table) with and without seen=list, --runs
  sustained stretches each, a path's stretches back to back.
  Without the list it is the parent's path.  With it, the first timed read
  enters n new hashes and every later one finds n duplicates, so each step
  starts from a list rebuilt outside the timed span ("new": every packet
  passes, is remembered and is decrypted) or reads the stream a second time
  ("replayed": every packet is dropped before the decrypt);
* "filter": the filter call alone over the unpacked records, all new hashes
  (a fresh list per step, made outside the timed span) and all duplicates;
* "list": add of n hashes, contains (hits and misses) and the cull that rotates.

Outputs are checked: every packet of the first read passes and decrypts, every
packet of the second is RT_FILTER_DUPLICATE, and the counts are as entered.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--links-log2", type=int, default=16)
    ap.add_argument("--preload", type=int, default=500000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packet_filter_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1377)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    n, n_links, plain, isz = 1 << args.log2, 1 << args.links_log2, 383, 16
    max_hashes = 2 * n
    result = {"tool": "tools/packet_filter_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "runs": args.runs, "n": n, "links": n_links, "plaintext_bytes": plain,
              "packet_bytes": 19 + rt.token_len(plain), "ifac_size": isz, "max_hashes": max_hashes,
              "preload": args.preload, "ok": True}

    def check(cond):
        result["ok"] = result["ok"] and bool(cond)

    med = lambda v: sorted(v)[len(v) // 2]           # noqa: E731

    def timed(fn, before=None):
        """--runs medians of --steps event-timed calls of fn; `before` runs ahead of each, outside the span."""
        out = []
        for _ in range(args.runs):
            ms = []
            for k in range(args.warmup + args.steps):
                if before:
                    before()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ms.append(a.elapsed_time(b))
            out.append(med(ms))
        return out

    # ---- the stream of the many links
    ifac_key, own = rand(64), rand(16)
    keys = rand(n_links, 64)
    ks = device.keyset(keys)
    link_ids = rand(n_links, 16)
    tab = rt.LinkTable(n_links, device=0)
    check(bool((tab.insert(link_ids, torch.arange(n_links, dtype=torch.int32, device=dev)) == 0).all()))
    which = torch.randperm(n, device=dev, generator=g) % n_links
    pt, iv, ifac = rand(n, plain), rand(n, 16), rand(n, isz)
    ctx = torch.zeros(n, dtype=torch.uint8, device=dev)
    flags = torch.full((n,), 3 << 2, dtype=torch.uint8, device=dev)          # LINK destination, DATA
    framed, foff = pipeline.outbound(ks, pt, iv, link_ids[which].contiguous(), ctx, ifac, ifac_key, flags=flags,
                                     key_idx=which.to(torch.int32))
    torch.cuda.synchronize()
    stream = framed[:int(foff[-1])].clone()
    del framed, pt, iv, ifac
    max_pairs = 2 * n + 1
    preload = rand(args.preload, 32)
    seen = [None]

    def fresh():
        seen[0] = rt.PacketHashlist(max_hashes, device=0)
        seen[0].add(preload)

    def read(with_seen):
        return pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, links=tab,
                                **(dict(seen=seen[0], transport_identity=own) if with_seen else {}))

    fresh()
    res = read(True)
    check(int(res["n_frames"]) == n and bool((res["filter_status"][:n] == 0).all()) and
          bool((res["status"][:n] == 0).all()) and bool((res["filter_status"][n:] == 1).all()))
    check(seen[0].counts() == (args.preload + n, 0, 0))
    res = read(True)
    check(bool((res["filter_status"][:n] == 5).all()) and bool((res["status"] == 1).all()))
    check(seen[0].counts() == (args.preload + n, 0, 0))
    del res
    res = read(False)
    fields_new = res["fields"].clone()
    del res

    base = timed(lambda: read(False))
    new = timed(lambda: read(True), before=fresh)
    fresh()
    read(True)
    rep = timed(lambda: read(True))
    result["inbound"] = {"n": n, "stream_bytes": stream.numel(),
                         "links_only": {"ms": base, "median_ms": med(base)},
                         "seen_new": {"ms": new, "median_ms": med(new)},
                         "seen_replayed": {"ms": rep, "median_ms": med(rep)},
                         "added_ms_new": med(new) - med(base)}

    # ---- the filter call alone
    status = torch.empty(max_pairs, dtype=torch.int32, device=dev)
    work = torch.empty_like(fields_new)

    def reset():
        fresh()
        work.copy_(fields_new)

    a = timed(lambda: device.packet_filter(seen[0].handle, work, own, status), before=reset)
    check(bool((status[:n] == 0).all()))
    b = timed(lambda: device.packet_filter(seen[0].handle, work, own, status), before=lambda: work.copy_(fields_new))
    check(bool((status[:n] == 5).all()))
    result["filter"] = {"n": max_pairs, "all_new_ms": a, "all_duplicates_ms": b}

    # ---- the list alone
    hashes, miss = rand(n, 32), rand(n, 32)
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    add = timed(lambda: seen[0].add(hashes), before=fresh)
    hit = timed(lambda: device.hashlist_contains(seen[0].handle, hashes, found))
    check(bool((found == 1).all()))
    mis = timed(lambda: device.hashlist_contains(seen[0].handle, miss, found))
    check(not bool(found.any()))
    small = [None]

    def half_full():
        small[0] = rt.PacketHashlist(n, device=0)
        small[0].add(hashes[:n // 2 + 1])

    cull = timed(lambda: small[0].cull(), before=half_full)
    check(small[0].counts() == (0, n // 2 + 1, 0))
    result["list"] = {"n": n, "capacity": seen[0].capacity, "add_ms": add, "contains_hits_ms": hit,
                      "contains_misses_ms": mis, "cull_rotating_ms": cull, "cull_capacity": small[0].capacity}

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not result["ok"]:
        raise SystemExit("an output check failed")


if __name__ == "__main__":
    main()
