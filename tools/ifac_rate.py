"""The interface access code on the device (rt_ifac_sign / rt_ifac_check, the
table of [2^i]B), timed with device events on device-resident buffers against
k_ed25519_sign on the same packets, and the interface path with and without it.

    python tools/ifac_rate.py [--steps 10] [--warmup 2] [--log2 20] [--runs 3] [--out profiles/ifac_rate.json]

Prints one JSON line (also written to --out):

* "sign_86", "sign_418": n = 2^log2 packets of 86 bytes (19 + the 67-byte token
  of a short payload) and of 418 bytes, one key for the batch.  Per kernel
  ("ifac_sign": k_ifac_sign, "ed25519_sign": k_ed25519_sign with the public key
  given) --runs sustained stretches, each the median ms of --steps launches
  after --warmup; a kernel's stretches run back to back, the two kernels are
  never alternated launch by launch.  "speedup" is the ratio
  of the medians of the stretches, and "faster_beyond_spread" says whether the
  slowest ifac_sign stretch beats the fastest ed25519_sign stretch;
* "outbound": pipeline.outbound over n 83-byte packets (15 bytes of plaintext,
  the nearest a token gets to the 86 bytes above) with the codes supplied
  and with the codes made on the device; "inbound": pipeline.inbound of that
  stream with and without check_ifac.

Outputs are checked: the codes are the tails of k_ed25519_sign's signatures,
sampled ones equal a big-integer Ed25519, both outbound streams are equal, and
the checked inbound read accepts every packet and rejects damaged codes.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ed25519_rate import L, base_mul, median_ms      # noqa: E402


def code_ref(seed, msg, size):
    h = hashlib.sha512(seed).digest()
    a = (int.from_bytes(h[:32], "little") & ((1 << 254) - 8)) | (1 << 254)
    pk = base_mul(a % L)
    r = int.from_bytes(hashlib.sha512(h[32:] + msg).digest(), "little") % L
    rb = base_mul(r)
    k = int.from_bytes(hashlib.sha512(rb + pk + msg).digest(), "little")
    return (rb + ((r + k * a) % L).to_bytes(32, "little"))[-size:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ifac-size", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ifac_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1470)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    n, isz = 1 << args.log2, args.ifac_size
    result = {"tool": "tools/ifac_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "runs": args.runs, "n": n, "ifac_size": isz, "ok": True}

    def check(cond):
        result["ok"] = result["ok"] and bool(cond)

    ifac_key = rand(64)
    seed, pub = pipeline.ifac_identity(ifac_key)
    seed_h = bytes(seed.tolist())

    def stretches(fn):
        return [median_ms(fn, args.steps, args.warmup) for _ in range(args.runs)]

    for plen in (86, 418):
        pkt = rand(n * plen)
        off = torch.arange(n, dtype=torch.int64, device=dev) * plen
        ln = torch.full((n,), plen, dtype=torch.int32, device=dev)
        codes = torch.zeros((n, isz), dtype=torch.uint8, device=dev)
        sigs = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
        a = stretches(lambda: device.ifac_sign(seed, pub, pkt, off, ln, codes))
        b = stretches(lambda: device.ed25519_sign(seed.view(1, 32), pkt, off, ln, sigs, public_keys=pub))
        med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731
        result["sign_%d" % plen] = {
            "n": n, "packet_bytes": plen,
            "ifac_sign": {"ms": a, "median_ms": med(a), "spread_ms": max(a) - min(a)},
            "ed25519_sign": {"ms": b, "median_ms": med(b), "spread_ms": max(b) - min(b)},
            "speedup": med(b) / med(a), "faster_beyond_spread": max(a) < min(b)}
        check(torch.equal(codes, sigs[:, 64 - isz:]))
        p_h, c_h = pkt.cpu().numpy(), codes.cpu().numpy()
        for i in {0, n // 2, n - 1}:
            check(code_ref(seed_h, p_h[i * plen:(i + 1) * plen].tobytes(), isz) == c_h[i].tobytes())
        st = torch.zeros(n, dtype=torch.int32, device=dev)
        ln2 = ln.clone()
        bad = codes.clone()
        bad[::3, isz - 1] ^= 1
        device.ifac_check(seed, pub, pkt, off, ln2, bad, st)
        want = torch.zeros(n, dtype=torch.int32, device=dev)
        want[::3] = 2
        check(torch.equal(st, want) and torch.equal(ln2 == 0, want == 2))
        del pkt, sigs

    # the interface path, 83-byte packets (15 bytes of plaintext: one AES block)
    plain = 15
    ks = rt.KeySet(bytes(rand(64).tolist()), device=0)
    pt, iv, dh, ctx = rand(n, plain), rand(n, 16), rand(n, 16), rand(n)
    framed, foff = pipeline.outbound(ks, pt, iv, dh, ctx, ifac_key=ifac_key, ifac_size=isz)
    # the codes of those packets, to supply them: unmask what was sent
    torch.cuda.synchronize()
    stream = framed[:int(foff[-1])].clone()
    max_pairs = 2 * n + 1
    res = pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, check_ifac=True)
    check(int(res["n_frames"]) == n and bool((res["ifac_status"][:n] == 0).all()) and
          bool((res["status"][:n] == 0).all()))
    codes = res["ifac"][:n].clone()
    del res
    framed2, foff2 = pipeline.outbound(ks, pt, iv, dh, ctx, codes, ifac_key)
    check(torch.equal(foff, foff2) and torch.equal(framed[:int(foff[-1])], framed2[:int(foff[-1])]))
    del framed, framed2
    out_given = stretches(lambda: pipeline.outbound(ks, pt, iv, dh, ctx, codes, ifac_key))
    out_made = stretches(lambda: pipeline.outbound(ks, pt, iv, dh, ctx, ifac_key=ifac_key, ifac_size=isz))
    in_plain = stretches(lambda: pipeline.inbound(ks, stream, ifac_key, isz, max_pairs))
    in_check = stretches(lambda: pipeline.inbound(ks, stream, ifac_key, isz, max_pairs, check_ifac=True))
    med = lambda v: sorted(v)[len(v) // 2]           # noqa: E731
    result["outbound"] = {"n": n, "packet_bytes": 19 + rt.token_len(plain), "codes_supplied_ms": out_given,
                          "codes_on_device_ms": out_made, "added_ms": med(out_made) - med(out_given)}
    result["inbound"] = {"n": n, "stream_bytes": stream.numel(), "unchecked_ms": in_plain, "check_ifac_ms": in_check,
                         "added_ms": med(in_check) - med(in_plain)}

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not result["ok"]:
        raise SystemExit("an output check failed")


if __name__ == "__main__":
    main()
