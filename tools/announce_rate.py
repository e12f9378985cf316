"""Announce validation on the inbound path (rt_announce_validate), timed with
device events on device-resident buffers.

    python tools/announce_rate.py [--steps 5] [--warmup 1] [--runs 3] [--log2 20] [--links-log2 16]
                                  [--out profiles/announce_rate.json]

Shape: n = 2^log2 frames with 16-byte access codes: link DATA packets with
383-byte plaintexts (451-byte packets) over 2^links-log2 links, the stream of
tools/link_dispatch_rate.py, in which announces are swapped in at three
densities: none, one frame in 64 spread evenly, and every frame.  An announce
is HEADER_1 without a ratchet and with 67 bytes of app data, a 167-byte signed
message in a 234-byte packet, signed on the device (device.ed25519_sign) by one
of 256 identities whose hashes the host works out, so every one is VALID.
Prints one JSON line (also written to --out):

* "inbound": pipeline.inbound(links=table) with announces off and on, per
  density, --runs sustained stretches each, a path's stretches back to back
  (DESIGN.md §4.10);
* "validate": device.announce_validate alone over the unpacked records of each
  stream, and device.ed25519_verify over as many contiguous 167-byte messages
  as the stream has announces, for comparison;
* "compaction_holds": the call alone at one announce in 64 takes less than a
  quarter of what it takes when every frame is one.  One lane per record
  running the verification would sit near 1; the compacted call near 1/64 plus
  the select pass.

Outputs are checked: every announce VALID, every other frame NOT_ANNOUNCE, the
link packets decrypted, the comparison's signatures accepted.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

APP = 67
ANNOUNCE_LEN = 19 + 148 + APP               # 234: header, keys, hashes, signature, app data
SIGNED_LEN = 16 + 84 + APP                  # 167
IDENTITIES = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--links-log2", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "announce_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1748)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    n, n_links, plain, isz = 1 << args.log2, 1 << args.links_log2, 383, 16
    pl = 19 + rt.token_len(plain)
    result = {"tool": "tools/announce_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "runs": args.runs, "n": n, "links": n_links, "plaintext_bytes": plain,
              "packet_bytes": pl, "announce_bytes": ANNOUNCE_LEN, "signed_bytes": SIGNED_LEN, "ifac_size": isz,
              "ok": True}

    def check(cond):
        result["ok"] = result["ok"] and bool(cond)

    med = lambda v: sorted(v)[len(v) // 2]           # noqa: E731

    def timed(fn):
        """--runs medians of --steps event-timed calls of fn."""
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
        return out

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

    # ---- n announces of 256 identities, signed on the device
    seeds = rand(IDENTITIES, 32)
    ed_pub = torch.empty((IDENTITIES, 32), dtype=torch.uint8, device=dev)
    device.ed25519_public(seeds, ed_pub)
    pub = torch.cat([rand(IDENTITIES, 32), ed_pub], dim=1)
    names = rand(IDENTITIES, 10)
    dests = []
    for p, name in zip(pub.cpu().numpy(), names.cpu().numpy()):
        identity = hashlib.sha256(p.tobytes()).digest()[:16]
        dests.append(list(hashlib.sha256(name.tobytes() + identity).digest()[:16]))
    dests = torch.tensor(dests, dtype=torch.uint8, device=dev)
    who = torch.arange(n, device=dev) % IDENTITIES
    random_hash, app = rand(n, 10), rand(n, APP)
    signed = torch.cat([dests[who], pub[who], names[who], random_hash, app], dim=1).contiguous()
    check(signed.shape == (n, SIGNED_LEN))
    m_off = torch.arange(n, dtype=torch.int64, device=dev) * SIGNED_LEN
    m_len = torch.full((n,), SIGNED_LEN, dtype=torch.int32, device=dev)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    device.ed25519_sign(seeds[who].contiguous(), signed.view(-1), m_off, m_len, sig,
                        public_keys=ed_pub[who].contiguous())
    head = torch.zeros((n, 19), dtype=torch.uint8, device=dev)
    head[:, 0] = 0x01                                                              # HEADER_1, SINGLE, ANNOUNCE
    head[:, 2:18] = dests[who]
    announces = torch.cat([head, pub[who], names[who], random_hash, sig, app], dim=1).contiguous()
    check(announces.shape == (n, ANNOUNCE_LEN))
    torch.cuda.synchronize()
    del head, random_hash, app

    max_pairs = 2 * n + 1
    ifac = rand(n, isz)

    def make_stream(every):
        """The framed stream with an announce in every `every`-th frame (0: none) and its announce mask."""
        is_ann = torch.zeros(n, dtype=torch.bool, device=dev)
        if every:
            is_ann[every // 2::every] = True
        flat = links_flat.clone()
        if every:
            flat.view(n, pl)[is_ann, :ANNOUNCE_LEN] = announces[is_ann]
        p_len = torch.where(is_ann, ANNOUNCE_LEN, pl).to(torch.int32)
        ml = pl + isz
        masked = torch.empty(n * ml, dtype=torch.uint8, device=dev)
        mo = torch.arange(n, dtype=torch.int64, device=dev) * ml
        device.ifac_mask(flat, off, p_len, ifac, ifac_key, masked, mo)
        framed = torch.empty(n * (2 * ml + 2), dtype=torch.uint8, device=dev)
        frame_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        device.hdlc_frame(masked, mo, p_len + isz, framed, frame_off)
        torch.cuda.synchronize()
        return framed[:int(frame_off[-1])].clone(), is_ann

    def read(stream, on):
        return pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, links=tab, announces=on)

    ok8 = torch.empty(n, dtype=torch.uint8, device=dev)
    result["inbound"], result["validate"] = {}, {}
    alone = {}
    for name, every in (("none", 0), ("one_in_64", 64), ("all", 1)):
        stream, is_ann = make_stream(every)
        m = int(is_ann.sum())
        res = read(stream, True)
        st = res["announce_status"]
        check(int(res["n_frames"]) == n and bool((st[:n][is_ann] == 0).all()) and
              bool((st[:n][~is_ann] == 1).all()) and bool((st[n:] == 1).all()))
        check(bool((res["status"][:n][~is_ann] == 0).all()))
        del res
        off_ms = timed(lambda: read(stream, False))
        on_ms = timed(lambda: read(stream, True))
        result["inbound"][name] = {"announces": m, "stream_bytes": stream.numel(),
                                   "off": {"ms": off_ms, "median_ms": med(off_ms)},
                                   "on": {"ms": on_ms, "median_ms": med(on_ms)},
                                   "added_ms": med(on_ms) - med(off_ms)}
        # the call alone, over packets laid out as the slots of the unframed stream
        flat = links_flat.clone()
        if every:
            flat.view(n, pl)[is_ann, :ANNOUNCE_LEN] = announces[is_ann]
        p_len = torch.where(is_ann, ANNOUNCE_LEN, pl).to(torch.int32)
        rec = torch.empty((n, 96), dtype=torch.uint8, device=dev)
        device.packet_unpack(flat, off, p_len, rec)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        ident = torch.empty((n, 16), dtype=torch.uint8, device=dev)
        call_ms = timed(lambda: device.announce_validate(flat, off, rec, status, ident))
        check(bool((status[is_ann] == 0).all()) and bool((status[~is_ann] == 1).all()))
        alone[name] = med(call_ms)
        entry = {"n": n, "announces": m, "ms": call_ms, "median_ms": med(call_ms)}
        if m:
            keys_m = ed_pub[who[is_ann]].contiguous()
            sig_m, msg_m = sig[is_ann].contiguous(), signed[is_ann].contiguous().view(-1)
            ver_ms = timed(lambda: device.ed25519_verify(keys_m, sig_m, msg_m, m_off[:m].contiguous(),
                                                         m_len[:m].contiguous(), ok8[:m]))
            check(bool((ok8[:m] == 1).all()))
            entry.update(ed25519_verify_ms=ver_ms, ed25519_verify_median_ms=med(ver_ms),
                         announces_per_s=m / (med(call_ms) * 1e-3))
            del keys_m, sig_m, msg_m
        result["validate"][name] = entry
        del stream, flat, rec
    result["compaction_ratio"] = alone["one_in_64"] / alone["all"]
    result["compaction_holds"] = bool(alone["one_in_64"] < 0.25 * alone["all"])

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not result["ok"]:
        raise SystemExit("an output check failed")


if __name__ == "__main__":
    main()
