"""The send side of a read (rt_reply_gather, rt_hdlc_frame_counted,
pipeline.reply), timed on device-resident buffers with a host clock around
work that ends in a device synchronise (the caller's path of today has host
synchronisations inside it, so device events alone would not be fair to it).

    python tools/reply_rate.py [--steps 5] [--warmup 2] [--runs 3] [--log2 20] [--links-log2 16]
                               [--out profiles/reply_rate.json]

Shape: n = 2^log2 frames.  For (a)-(c) the three stages' outputs are made by
hand: max_pairs x 128 rows of random bytes with 118-, 115- and 83-byte replies
on a fraction ``density`` of the frames (1/64, 1/2, 1), spread evenly and dealt
to the three sources in turn.  For (d) the stream is that of
tools/proof_rate.py: link DATA packets with 16-byte access codes over
2^links-log2 links.  Prints one JSON line (also written to --out):

* "gather": device.reply_gather alone, per density;
* "reply": pipeline.reply end to end, with 16-byte access codes and without,
  per density;
* "caller": the path a caller has without it, in the same process and run: per
  source nonzero (a host synchronisation each) -> index_select -> merged in
  frame order -> ifac_sign / ifac_mask / hdlc_frame; and "reply_over_caller",
  the ratio of the medians;
* "inbound": a read with reply=True against the same read without, with no
  reply in it (no link proves) and with every frame proved; "added_ms" beside
  the spread of the same-run baseline.

Outputs are checked: the caller's stream and pipeline.reply's are the same
bytes, the counts are the replies made, the read's reply stream has one frame
per proof.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (118, 115, 83)          # LRPROOF, LINK PROOF, implicit PROOF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--links-log2", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reply_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1069)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    n, n_links, plain, isz = 1 << args.log2, 1 << args.links_log2, 383, 16
    result = {"tool": "tools/reply_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "runs": args.runs, "n": n, "links": n_links, "ifac_size": isz, "ok": True}

    def check(cond):
        result["ok"] = result["ok"] and bool(cond)

    med = lambda v: sorted(v)[len(v) // 2]           # noqa: E731

    def timed(fn):
        """--runs medians of --steps calls of fn, each from a synchronised device to a synchronised device."""
        out = []
        for _ in range(args.runs):
            ms = []
            for k in range(args.warmup + args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out.append(med(ms))
        return {"ms": out, "median_ms": med(out), "spread_ms": max(out) - min(out)}

    ifac_key = rand(64)
    seed, pub = pipeline.ifac_identity(ifac_key)
    names = pipeline.REPLY_SOURCES
    result["gather"], result["reply"], result["caller"], result["reply_over_caller"] = {}, {}, {}, {}

    def caller_path(res, size):
        """What a caller does today with the three sparse outputs."""
        idx, src = [], []
        for s, (rows, ln) in enumerate(names):
            k = torch.nonzero(res[ln]).view(-1)                      # a host synchronisation: the count
            idx.append(k)
            src.append(torch.full_like(k, s))
        frame, source = torch.cat(idx), torch.cat(src)
        order = torch.argsort(frame * 4 + source)                     # frame-major, then source
        frame, source = frame[order], source[order]
        m = frame.numel()
        packets = torch.zeros((m, 128), dtype=torch.uint8, device=dev)
        lens = torch.zeros(m, dtype=torch.int32, device=dev)
        for s, (rows, ln) in enumerate(names):
            mine = source == s
            packets[mine] = res[rows].index_select(0, frame[mine])
            lens[mine] = res[ln].index_select(0, frame[mine])
        flat = packets.view(-1)
        off = torch.arange(m, dtype=torch.int64, device=dev) * 128
        if size:
            ml = 128 + size
            ifac = torch.empty((m, size), dtype=torch.uint8, device=dev)
            device.ifac_sign(seed, pub, flat, off, lens, ifac)
            masked = torch.empty(max(m * ml, 1), dtype=torch.uint8, device=dev)
            m_off = torch.arange(m, dtype=torch.int64, device=dev) * ml
            device.ifac_mask(flat, off, lens, ifac, ifac_key, masked, m_off)
            m_len = lens + size
        else:
            ml, masked, m_off, m_len = 128, flat, off, lens
        framed = torch.empty(max(m * (2 * ml + 2), 1), dtype=torch.uint8, device=dev)
        frame_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
        device.hdlc_frame(masked, m_off, m_len, framed, frame_off)
        return framed, frame_off, m

    for name, every in (("one_in_64", 64), ("one_in_2", 2), ("all", 1)):
        res = {}
        at = torch.arange(every // 2, n, every, device=dev)
        for s, (rows, ln) in enumerate(names):
            res[rows] = rand(n, 128)
            lens = torch.zeros(n, dtype=torch.int32, device=dev)
            lens[at[s::3]] = LENGTHS[s]
            res[ln] = lens
        m = at.numel()
        out = torch.empty((n, 128), dtype=torch.uint8, device=dev)
        r_len = torch.empty(n, dtype=torch.int32, device=dev)
        r_frame = torch.empty(n, dtype=torch.int32, device=dev)
        r_src = torch.empty(n, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        sources = [(res[rows], res[ln]) for rows, ln in names]
        ws = torch.empty(int(rt._native.load().rt_reply_gather_workspace_bytes(n, 3)), dtype=torch.uint8, device=dev)
        result["gather"][name] = dict(timed(lambda: device.reply_gather(sources, out, r_len, r_frame, r_src, counts,
                                                                        workspace=ws)), replies=m)
        check(counts.tolist() == [m, m] and torch.equal(r_frame[:m].to(torch.int64), at))
        result["reply"][name], result["caller"][name], result["reply_over_caller"][name] = {}, {}, {}
        for label, size in (("ifac_16", isz), ("no_ifac", 0)):
            mine = pipeline.reply(res, ifac_key=ifac_key, ifac_size=size)
            theirs, their_off, their_m = caller_path(res, size)
            total = int(mine["frame_off"][-1])
            check(their_m == m and total == int(their_off[-1]) and torch.equal(mine["stream"][:total], theirs[:total]))
            del mine, theirs, their_off
            a = timed(lambda: pipeline.reply(res, ifac_key=ifac_key, ifac_size=size))
            b = timed(lambda: caller_path(res, size))
            result["reply"][name][label] = dict(a, replies=m, stream_bytes=total)
            result["caller"][name][label] = b
            result["reply_over_caller"][name][label] = a["median_ms"] / b["median_ms"]
        del res, sources, out

    # ---- (d) a read with and without reply: the stream of tools/proof_rate.py
    pl = 19 + rt.token_len(plain)
    keys = rand(n_links, 64)
    ks = device.keyset(keys)
    link_ids = rand(n_links, 16)
    tab = rt.LinkTable(n_links, device=0)
    check(bool((tab.insert(link_ids, torch.arange(n_links, dtype=torch.int32, device=dev)) == 0).all()))
    which = torch.randperm(n, device=dev, generator=g) % n_links
    flat = torch.empty(n * pl, dtype=torch.uint8, device=dev)
    device.encrypt_uniform(ks, rand(n, plain), plain, rand(n, 16), flat.view(n, pl)[:, 19:], key_idx=which.to(torch.int32))
    off = torch.arange(n, dtype=torch.int64, device=dev) * pl
    device.pack_headers(torch.full((n,), 3 << 2, dtype=torch.uint8, device=dev),      # LINK destination, DATA
                        torch.zeros(n, dtype=torch.uint8, device=dev), link_ids[which].contiguous(),
                        torch.zeros(n, dtype=torch.uint8, device=dev), flat, off)
    p_len = torch.full((n,), pl, dtype=torch.int32, device=dev)
    ml = pl + isz
    masked = torch.empty(n * ml, dtype=torch.uint8, device=dev)
    mo = torch.arange(n, dtype=torch.int64, device=dev) * ml
    device.ifac_mask(flat, off, p_len, rand(n, isz), ifac_key, masked, mo)
    framed = torch.empty(n * (2 * ml + 2), dtype=torch.uint8, device=dev)
    frame_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    device.hdlc_frame(masked, mo, p_len + isz, framed, frame_off)
    stream = framed[:int(frame_off[-1])].clone()
    del flat, masked, framed
    seeds, peer_pub = rand(n_links, 32), rand(n_links, 32)
    flags = lambda v: torch.full((n_links,), v, dtype=torch.uint8, device=dev)     # noqa: E731
    signers = {"no_reply": rt.LinkSigners(seeds, peer_pub, flags(0), device=0),
               "all_proved": rt.LinkSigners(seeds, peer_pub, flags(rt.proof.PROVE_ALL), device=0)}
    max_pairs = 2 * n + 1
    result["inbound"] = {}
    for name, sg in signers.items():
        read = lambda **kw: pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, links=tab, signers=sg, **kw)  # noqa: E731
        res = read(reply={"max_replies": n})
        want = n if name == "all_proved" else 0
        check(int(res["n_frames"]) == n and res["reply"]["reply_counts"].tolist() == [want, want])
        check(int(res["reply"]["frame_off"][-1]) >= want * (115 + isz + 2))
        del res
        # alternating, so that both see the same machine
        base, with_reply = [], []
        for _ in range(args.runs):
            base.append(timed(lambda: read())["ms"])
            with_reply.append(timed(lambda: read(reply={"max_replies": n}))["ms"])
        base, with_reply = [x for r in base for x in r], [x for r in with_reply for x in r]
        result["inbound"][name] = {"baseline_ms": base, "reply_ms": with_reply, "baseline_median_ms": med(base),
                                   "reply_median_ms": med(with_reply), "added_ms": med(with_reply) - med(base),
                                   "baseline_spread_ms": max(base) - min(base), "replies": want}

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not result["ok"]:
        raise SystemExit("an output check failed")


if __name__ == "__main__":
    main()
