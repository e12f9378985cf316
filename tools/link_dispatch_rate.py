"""The link table and the dispatch of inbound link packets (rt_linktable_*,
rt_link_spans), timed with device events on device-resident buffers.

    python tools/link_dispatch_rate.py [--steps 5] [--warmup 1] [--runs 3] [--log2 20] [--links-log2 16]
                                       [--out profiles/link_dispatch_rate.json]

Shape: n = 2^log2 DATA packets with 383-byte plaintexts (a 432-byte token, a
451-byte packet) and 16-byte access codes, spread evenly over 2^links-log2
links, each with its own key.  Prints one JSON line (also written to --out):

* "inbound": pipeline.inbound(links=table) over the stream of the many links
  against pipeline.inbound with one key over a one-key stream of the same
  shape (the path as it was before the table), --runs sustained stretches each,
  a path's stretches back to back and the two paths never alternated launch by
  launch; "clock_ghz" is the shader clock the decrypt
  launches of each path's stretches held (device.LaunchClock);
* "spans": k_link_spans alone against k_token_spans alone on the unpacked
  fields of the many-link stream;
* "table": n inserts of fresh ids into a table made for n links (each timed
  step makes its own table, so the zeroing of the slots is in the figure), n
  lookups that all hit and n that all miss.

Outputs are checked: every packet of the many-link read decrypts under its own
link's key to the plaintext sent, every insert reports RT_LINK_OK, every lookup
the value entered.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ed25519_rate import median_ms      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--links-log2", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_dispatch_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(2161)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    n, n_links, plain, isz = 1 << args.log2, 1 << args.links_log2, 383, 16
    result = {"tool": "tools/link_dispatch_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "runs": args.runs, "n": n, "links": n_links, "plaintext_bytes": plain,
              "packet_bytes": 19 + rt.token_len(plain), "ifac_size": isz, "ok": True}

    def check(cond):
        result["ok"] = result["ok"] and bool(cond)

    def stretches(fn):
        return [median_ms(fn, args.steps, args.warmup) for _ in range(args.runs)]

    med = lambda v: sorted(v)[len(v) // 2]           # noqa: E731

    # ---- the two streams
    ifac_key = rand(64)
    keys = rand(n_links, 64)
    ks_many = device.keyset(keys)
    ks_one = device.keyset(keys[:1].clone())
    link_ids = rand(n_links, 16)
    tab = rt.LinkTable(n_links, device=0)
    st = tab.insert(link_ids, torch.arange(n_links, dtype=torch.int32, device=dev))
    check(bool((st == 0).all()) and len(tab) == n_links)
    which = torch.randperm(n, device=dev, generator=g) % n_links
    pt, iv, ifac = rand(n, plain), rand(n, 16), rand(n, isz)
    ctx = torch.zeros(n, dtype=torch.uint8, device=dev)
    flags = torch.full((n,), 3 << 2, dtype=torch.uint8, device=dev)          # LINK destination, DATA
    dh = link_ids[which].contiguous()
    max_pairs = 2 * n + 1

    def stream_of(ks, key_idx):
        framed, foff = pipeline.outbound(ks, pt, iv, dh, ctx, ifac, ifac_key, flags=flags, key_idx=key_idx)
        torch.cuda.synchronize()
        return framed[:int(foff[-1])].clone()

    stream_many = stream_of(ks_many, which.to(torch.int32))
    stream_one = stream_of(ks_one, None)
    res = pipeline.inbound(ks_many, stream_many, ifac_key, isz, max_pairs, links=tab)
    check(int(res["n_frames"]) == n and bool((res["status"][:n] == 0).all()) and
          bool((res["route"][:n] == 3).all()) and torch.equal(res["link"][:n].long(), which))
    sample = torch.arange(0, n, max(1, n // 4096), device=dev)
    at = res["pt_off"][sample].unsqueeze(1) + torch.arange(plain, device=dev).unsqueeze(0)
    check(torch.equal(res["pt"][at], pt[sample]))
    fields, f_off = res["fields"].clone(), torch.arange(max_pairs, dtype=torch.int64, device=dev) * 512
    del res
    res = pipeline.inbound(ks_one, stream_one, ifac_key, isz, max_pairs)
    check(int(res["n_frames"]) == n and bool((res["status"][:n] == 0).all()))
    del res

    def timed(fn):
        with device.LaunchClock(dev) as lc:
            ms = stretches(fn)
        return ms, lc.summary().get("decrypt", {}).get("clock_ghz")

    one_ms, one_clk = timed(lambda: pipeline.inbound(ks_one, stream_one, ifac_key, isz, max_pairs))
    many_ms, many_clk = timed(lambda: pipeline.inbound(ks_many, stream_many, ifac_key, isz, max_pairs, links=tab))
    result["inbound"] = {"n": n, "stream_bytes": stream_many.numel(),
                         "one_key": {"ms": one_ms, "median_ms": med(one_ms), "clock_ghz": one_clk},
                         "links": {"ms": many_ms, "median_ms": med(many_ms), "clock_ghz": many_clk},
                         "ratio": med(many_ms) / med(one_ms)}

    # ---- the span kernels alone
    tok_off = torch.empty(max_pairs, dtype=torch.int64, device=dev)
    tok_len, key_idx, link = (torch.empty(max_pairs, dtype=torch.int32, device=dev) for _ in range(3))
    route = torch.empty(max_pairs, dtype=torch.uint8, device=dev)
    a = stretches(lambda: device.token_spans(fields, f_off, tok_off, tok_len))
    b = stretches(lambda: device.link_spans(tab.handle, fields, f_off, n_links, tok_off, tok_len, key_idx, link, route))
    result["spans"] = {"n": max_pairs, "token_spans_ms": a, "link_spans_ms": b, "added_ms": med(b) - med(a)}
    del fields

    # ---- the table alone
    ids, miss = rand(n, 16), rand(n, 16)
    values = torch.arange(n, dtype=torch.int32, device=dev)
    big = [None]

    def fresh_insert():
        big[0] = rt.LinkTable(n, device=0)
        big[0].insert(ids, values)

    ins = stretches(fresh_insert)
    status = big[0].insert(ids, values)
    check(bool((status == 1).all()) and len(big[0]) == n)         # all present: the timed insert entered every id
    out = torch.empty(n, dtype=torch.int32, device=dev)
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    hit = stretches(lambda: device.linktable_lookup(big[0].handle, ids, out, found))
    check(torch.equal(out, values) and bool(found.all()))
    mis = stretches(lambda: device.linktable_lookup(big[0].handle, miss, out, found))
    check(not bool(found.any()))
    result["table"] = {"n": n, "capacity": big[0].capacity, "insert_fresh_table_ms": ins, "lookup_hits_ms": hit,
                       "lookup_misses_ms": mis}

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not result["ok"]:
        raise SystemExit("an output check failed")


if __name__ == "__main__":
    main()
