"""Batched Ed25519 (rt_ed25519_verify / _sign / _public), timed with device
events on device-resident buffers, with k_x25519 from the same run as the
yardstick.

    python tools/ed25519_rate.py [--steps 10] [--warmup 2] [--log2 20] [--out profiles/ed25519_rate.json]

Prints one JSON line (also written to --out):

* "verify", "sign" (public keys given), "sign_deriving_key", "public": the
  median ms of --steps launches after --warmup over n = 2^log2 items of
  32-byte messages (a proof's packet hash), and items per second;
* "verify_announce": the same for 167-byte messages (about the signed data of
  an announce: destination hash 16, public key 64, name hash 10, random hash
  10, a 32-byte ratchet and some app data, Identity.py:545);
* "verify_one", "sign_one": one item alone on the device (one lane's whole
  computation), and "verify_one_host_call_ms": the host call with its copies;
* "x25519": k_x25519 over the same n in the same run, and each rate as a
  multiple of one exchange's time;
* "clock": the sustained shader clock of token decrypt launches of this run
  (reticulum_amd.device.LaunchClock), for the record.

Outputs are checked: the signatures verify on the device, sampled signatures
and public keys equal a big-integer Ed25519, and damaged signatures fail.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P


def base_mul(n):
    """[n]B in projective coordinates with Python integers, encoded (the check
    of the timed outputs)."""
    by = 4 * pow(5, P - 2, P) % P
    xx = (by * by - 1) * pow(D * by * by + 1, P - 2, P) % P
    bx = pow(xx, (P + 3) // 8, P)
    if (bx * bx - xx) % P:
        bx = bx * pow(2, (P - 1) // 4, P) % P
    if bx & 1:
        bx = P - bx

    def add(p, q):
        (x1, y1, z1), (x2, y2, z2) = p, q
        a = z1 * z2 % P
        b, c, d = a * a % P, x1 * x2 % P, y1 * y2 % P
        e = D * c * d % P
        f, g = (b - e) % P, (b + e) % P
        return (a * f * ((x1 + y1) * (x2 + y2) - c - d) % P, a * g * (d + c) % P, f * g % P)
    q, b = (0, 1, 1), (bx, by, 1)
    for bit in bin(n)[2:] if n else "":
        q = add(q, q)
        if bit == "1":
            q = add(q, b)
    zi = pow(q[2], P - 2, P)
    x, y = q[0] * zi % P, q[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def sign_ref(seed, msg):
    h = hashlib.sha512(seed).digest()
    a = (int.from_bytes(h[:32], "little") & ((1 << 254) - 8)) | (1 << 254)
    pk = base_mul(a % L)
    r = int.from_bytes(hashlib.sha512(h[32:] + msg).digest(), "little") % L
    rb = base_mul(r)
    k = int.from_bytes(hashlib.sha512(rb + pk + msg).digest(), "little")
    return pk, rb + ((r + k * a) % L).to_bytes(32, "little")


def median_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[steps // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ed25519_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(25519)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    n = 1 << args.log2
    result = {"tool": "tools/ed25519_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "n": n, "ok": True}

    def rate(name, ms, items):
        result[name] = {"n": items, "ms": ms, "items_s": items / (ms * 1e-3)}

    def spans(mlen, items):
        off = torch.arange(items, dtype=torch.int64, device=dev) * mlen
        return rand(items * mlen), off, torch.full((items,), mlen, dtype=torch.int32, device=dev)

    seeds = rand(n, 32)
    pubs = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    rate("public", median_ms(lambda: device.ed25519_public(seeds, pubs), args.steps, args.warmup), n)
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    for name, mlen in (("", 32), ("_announce", 167)):
        msgs, off, ln = spans(mlen, n)
        sigs = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
        ms_sign = median_ms(lambda: device.ed25519_sign(seeds, msgs, off, ln, sigs, public_keys=pubs), args.steps,
                            args.warmup)
        if not name:
            rate("sign", ms_sign, n)
            sigs2 = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
            rate("sign_deriving_key", median_ms(lambda: device.ed25519_sign(seeds, msgs, off, ln, sigs2), args.steps,
                                                args.warmup), n)
            result["ok"] = result["ok"] and bool(torch.equal(sigs, sigs2))
        rate("verify" + name, median_ms(lambda: device.ed25519_verify(pubs, sigs, msgs, off, ln, ok), args.steps,
                                        args.warmup), n)
        result["verify" + name]["message_bytes"] = mlen
        result["ok"] = result["ok"] and bool(ok.all())
        s_h, p_h, g_h, m_h = seeds.cpu().numpy(), pubs.cpu().numpy(), sigs.cpu().numpy(), msgs.cpu().numpy()
        for i in {0, n // 2, n - 1}:
            pk, sig = sign_ref(s_h[i].tobytes(), m_h[i * mlen:(i + 1) * mlen].tobytes())
            result["ok"] = result["ok"] and pk == p_h[i].tobytes() and sig == g_h[i].tobytes()
        bad = sigs.clone()
        bad[::3, 7] ^= 1
        device.ed25519_verify(pubs, bad, msgs, off, ln, ok)
        want = torch.ones(n, dtype=torch.uint8, device=dev)
        want[::3] = 0
        result["ok"] = result["ok"] and bool(torch.equal(ok, want))

    # one item alone
    msgs, off, ln = spans(32, 1)
    sig1 = torch.zeros((1, 64), dtype=torch.uint8, device=dev)
    rate("sign_one", median_ms(lambda: device.ed25519_sign(seeds[:1], msgs, off, ln, sig1, public_keys=pubs[:1]),
                               10 * args.steps, args.warmup), 1)
    rate("verify_one", median_ms(lambda: device.ed25519_verify(pubs[:1], sig1, msgs, off, ln, ok[:1]),
                                 10 * args.steps, args.warmup), 1)
    result["ok"] = result["ok"] and bool(ok[0] == 1)
    pk, sg, m = pubs[0].cpu().numpy().tobytes(), sig1[0].cpu().numpy().tobytes(), msgs.cpu().numpy().tobytes()
    rt.ed25519.verify(pk, sg, m)
    t0 = time.perf_counter()
    for _ in range(20):
        rt.ed25519.verify(pk, sg, m)
    result["verify_one_host_call_ms"] = (time.perf_counter() - t0) / 20 * 1e3

    # the yardstick, same run
    sc, pt, out = rand(n, 32), rand(n, 32), torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    ms_x = median_ms(lambda: device.x25519(sc, pt, out), args.steps, args.warmup)
    result["x25519"] = {"n": n, "ms": ms_x, "exchanges_s": n / (ms_x * 1e-3)}
    for name in ("verify", "verify_announce", "sign", "sign_deriving_key", "public"):
        result[name]["x25519_exchanges"] = result[name]["ms"] / ms_x

    # the clock this run holds, read from token decrypt launches (the launch clock's kernels)
    nt, plen = 1 << 16, 383
    tl = rt.token_len(plen)
    eph, one_pub, salt = rand(nt, 32), pubs[:1].clone(), rand(1, 16)
    device.x25519(rand(1, 32), None, one_pub)
    kidx = torch.arange(nt, dtype=torch.int32, device=dev)
    ks = device.derive_keyset_x25519(eph, one_pub, salt.expand(nt, 16))
    tok = torch.zeros((nt, tl), dtype=torch.uint8, device=dev)
    device.encrypt_uniform(ks, rand(nt, plen), plen, rand(nt, 16), tok, key_idx=kidx)
    back = torch.zeros((nt, tl - 48), dtype=torch.uint8, device=dev)
    ol, st = torch.zeros(nt, dtype=torch.int32, device=dev), torch.zeros(nt, dtype=torch.int32, device=dev)
    with device.LaunchClock(dev) as clock:
        median_ms(lambda: device.decrypt_uniform(ks, tok, tl, back, ol, st, key_idx=kidx), args.steps, args.warmup)
    result["clock"] = clock.summary()

    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not result["ok"]:
        raise SystemExit("an output check failed")


if __name__ == "__main__":
    main()
