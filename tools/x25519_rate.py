"""Batched X25519 (rt_x25519) and the Identity.decrypt device step, timed with
device events on device-resident buffers.

    python tools/x25519_rate.py [--steps 10] [--warmup 2] [--out profiles/x25519_rate.json]

Prints one JSON line (also written to --out):

* "exchange": for n = 1 and 2^16 .. 2^20 random scalar/point pairs, the median
  ms of --steps launches after --warmup, and exchanges per second.  n = 1 is
  the one-exchange latency on the device (one lane's whole ladder); its host
  call (rt_x25519_host through reticulum_amd.exchange, copies and sync
  included) is timed with a host clock.
* "identity_decrypt": n tokens of 383-byte plaintexts (Packet.ENCRYPTED_MDU)
  to one identity, ephemeral public key at the head of each token: the whole
  device step (exchange against the identity's key with the points read in
  place, HKDF and key setup, token decrypt with key_idx[i] = i) against the
  token decrypt alone with the key set already built, and the exchange's
  share of the whole step.
* "clock": the sustained shader clock of the decrypt launches of this run
  (reticulum_amd.device.LaunchClock), for the record.

Outputs are checked: the n = 1 and sampled exchanges against a big-integer
ladder, the decrypted plaintexts against the originals.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 2 ** 255 - 19


def ladder(scalar, point):
    """RFC 7748 §5 with Python integers (the check of the timed outputs)."""
    k = int.from_bytes(scalar, "little") & ~7 & ((1 << 255) - 1) | (1 << 254)
    x1 = (int.from_bytes(point, "little") & ((1 << 255) - 1)) % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (k >> t) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b, c, d = (x2 + z2) % P, (x2 - z2) % P, (x3 + z3) % P, (x3 - z3) % P
        aa, bb, da, cb = a * a % P, b * b % P, d * a % P, c * b % P
        e = (aa - bb) % P
        x3, z3 = (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P
        x2, z2 = aa * bb % P, e * (aa + 121665 * e) % P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


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
    ap.add_argument("--max-log2", type=int, default=20)
    ap.add_argument("--identity-n", type=int, default=1 << 16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "x25519_rate.json"))
    args = ap.parse_args()
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(25519)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)

    result = {"tool": "tools/x25519_rate.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "exchange": [], "ok": True}
    for n in [1] + [1 << k for k in range(16, args.max_log2 + 1)]:
        sc, pt, out = rand(n, 32), rand(n, 32), torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        ms = median_ms(lambda: device.x25519(sc, pt, out), args.steps if n > 1 else 10 * args.steps, args.warmup)
        s, p, o = sc.cpu().numpy(), pt.cpu().numpy(), out.cpu().numpy()
        for i in {0, n // 2, n - 1}:
            result["ok"] = result["ok"] and o[i].tobytes() == ladder(s[i].tobytes(), p[i].tobytes())
        result["exchange"].append({"n": n, "ms": ms, "exchanges_s": n / (ms * 1e-3)})
    k, u = os.urandom(32), os.urandom(32)
    rt.exchange(k, u)
    t0 = time.perf_counter()
    for _ in range(20):
        rt.exchange(k, u)
    result["one_exchange_host_call_ms"] = (time.perf_counter() - t0) / 20 * 1e3
    result["one_exchange_device_ms"] = result["exchange"][0]["ms"]

    # Identity.decrypt, device step: n tokens to one identity
    n, L = args.identity_n, 383
    tl = rt.token_len(L)
    prv, salt = rand(1, 32), rand(1, 16)
    pub = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    device.x25519(prv, None, pub)
    eph, msg, iv = rand(n, 32), rand(n, L), rand(n, 16)
    wire = torch.zeros((n, 32 + tl), dtype=torch.uint8, device=dev)       # ephemeral_pub || token
    device.x25519(eph, None, wire[:, :32])
    kidx = torch.arange(n, dtype=torch.int32, device=dev)
    device.encrypt_uniform(device.derive_keyset_x25519(eph, pub, salt.expand(n, 16)), msg, L, iv, wire[:, 32:],
                           key_idx=kidx)
    off = torch.arange(n, dtype=torch.int64, device=dev) * (32 + tl)
    back = torch.zeros((n, tl - 48), dtype=torch.uint8, device=dev)
    ol, st = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    shared = torch.zeros((n, 32), dtype=torch.uint8, device=dev)

    def keys():
        return device.derive_keyset_x25519(prv, wire.view(-1), salt.expand(n, 16), point_off=off)

    def whole():
        device.decrypt_uniform(keys(), wire[:, 32:], tl, back, ol, st, key_idx=kidx)

    ks = keys()
    with device.LaunchClock(dev) as clock:
        t_dec = median_ms(lambda: device.decrypt_uniform(ks, wire[:, 32:], tl, back, ol, st, key_idx=kidx),
                          args.steps, args.warmup)
    t_whole = median_ms(whole, args.steps, args.warmup)
    t_keys = median_ms(keys, args.steps, args.warmup)
    t_x = median_ms(lambda: device.x25519(prv, wire.view(-1), shared, point_off=off), args.steps, args.warmup)
    result["ok"] = result["ok"] and bool((st == 0).all()) and bool(torch.equal(back[:, :L], msg))
    result["identity_decrypt"] = {"n": n, "plaintext_bytes": L, "whole_ms": t_whole, "token_decrypt_alone_ms": t_dec,
                                  "exchange_and_key_setup_ms": t_keys, "exchange_ms": t_x,
                                  "exchange_share_of_whole": t_x / t_whole, "packets_s": n / (t_whole * 1e-3)}
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
