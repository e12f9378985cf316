"""Resource integrity hash + proof (rt_resource_hashes), device-resident timing.

    python tools/bench_resource_hash.py [--steps 20] [--warmup 3] [--out profiles/resource_hash.jsonl]

Rows (one JSON line each, also appended to --out):

* "shape": the shipped library on 262 144 x 16 384 B (the c4 shape), 1 024 x
  1 048 575 B (Resource.MAX_EFFICIENT_SIZE), 64 x 16 384 B and 1 x 1 048 575 B:
  ms per launch (median of --steps launches, torch.cuda.Event), segments/s,
  bytes/s, and the ratio to the segment-token decrypt (16 KiB tokens,
  device.decrypt_uniform) of the same number of bytes in this process.  The
  1 x 1 048 575 B row also carries hashlib's time for the same two digests on
  the host.
* "split": k_resource_hashes (one lane per segment) against
  k_resource_hashes_split (one workgroup per segment) in this one process,
  from two variant builds of the library that differ only in the launcher's
  threshold (-DRNSTOK_RESOURCE_SPLIT_BELOW=0u: never split; =0xFFFFFFFFu:
  always), with the outputs compared byte for byte.  The variants are built
  into tools/_bin/ on first use.
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "tools", "_bin")
FLAGS = "-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-result -Wno-unused-value"
VARIANTS = {"lane": "0u", "split": "0xFFFFFFFFu"}


def variant_path(name):
    return os.path.join(BIN, f"librnstok_reshash_{name}.so")


def build_variants():
    os.makedirs(BIN, exist_ok=True)
    for name, below in VARIANTS.items():
        if not os.path.exists(variant_path(name)):
            subprocess.check_call(["make", "-s", "-j6", "-C", os.path.join(ROOT, "reticulum_amd", "csrc"),
                                   "OUT=" + variant_path(name),
                                   f"FLAGS={FLAGS} -DRNSTOK_RESOURCE_SPLIT_BELOW={below}"])


class Variant:
    """rt_resource_hashes of one variant library, on its own context."""

    def __init__(self, name):
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        self.lib = ctypes.CDLL(variant_path(name))
        self.lib.rt_create.restype = vp
        self.lib.rt_create.argtypes = [ctypes.c_int]
        self.lib.rt_last_error.restype = ctypes.c_char_p
        self.lib.rt_resource_hash_split_below.restype = u32
        self.lib.rt_resource_hashes.restype = ctypes.c_int
        self.lib.rt_resource_hashes.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp]
        assert self.lib.rt_resource_hash_split_below() == int(VARIANTS[name].rstrip("u"), 0)
        self.ctx = self.lib.rt_create(0)
        if not self.ctx:
            raise SystemExit(f"{name}: rt_create failed: {self.lib.rt_last_error()}")

    def run(self, data, off, ln, rh, h, p):
        import torch
        rc = self.lib.rt_resource_hashes(self.ctx, data.data_ptr(), off.data_ptr(), ln.data_ptr(), rh.data_ptr(),
                                         rh.shape[1], None, h.data_ptr(), p.data_ptr(), None, off.numel(),
                                         torch.cuda.current_stream().cuda_stream)
        if rc:
            raise SystemExit(f"rt_resource_hashes failed: {self.lib.rt_last_error()}")


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


def random_bytes(nbytes, dev, g):
    """nbytes of device-resident random uint8, filled 256 MiB at a time."""
    import torch
    t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for i in range(0, nbytes, 1 << 28):
        t[i:i + (1 << 28)].random_(0, 256, generator=g)
    return t


def segments(n, seg, dev, g):
    import torch
    stride = (seg + 15) // 16 * 16
    data = random_bytes(n * stride, dev, g)
    off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    ln = torch.full((n,), seg, dtype=torch.int32, device=dev)
    rh = torch.randint(0, 256, (n, 4), dtype=torch.uint8, device=dev, generator=g)
    h = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    p = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    return data, off, ln, rh, h, p


def decrypt_ms(nbytes, dev, g, steps, warmup):
    """Segment-token decrypt (16 KiB tokens) of about nbytes of plaintext."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    L = 16384
    n = max(1, round(nbytes / L))
    tl = rt.token_len(L)
    ks = rt.KeySet(bytes(range(64)))
    pt = random_bytes(n * L, dev, g).view(n, L)
    iv = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
    tok = torch.empty((n, tl), dtype=torch.uint8, device=dev)
    back = torch.empty((n, tl - 48), dtype=torch.uint8, device=dev)
    ol = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    device.encrypt_uniform(ks, pt, L, iv, tok)
    ms = median_ms(lambda: device.decrypt_uniform(ks, tok, tl, back, ol, st), steps, warmup)
    assert bool((st == 0).all()) and torch.equal(back[:, :L], pt)
    return ms, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resource_hash.jsonl"))
    ap.add_argument("--skip-large", action="store_true", help="leave out the two multi-GiB shapes")
    args = ap.parse_args()
    build_variants()
    import torch
    from reticulum_amd import _native, device
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(436)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    below = int(_native.load().rt_resource_hash_split_below())
    shapes = [(64, 16384), (1, 1048575)] + ([] if args.skip_large else [(262144, 16384), (1024, 1048575)])
    for n, seg in shapes:
        data, off, ln, rh, h, p = segments(n, seg, dev, g)
        ms = median_ms(lambda: device.resource_hashes(data, off, ln, rh, h, p), args.steps, args.warmup)
        # spot check against hashlib (segment 0 and the last one)
        ok = True
        for i in {0, n - 1}:
            s = data[int(off[i]):int(off[i]) + seg].cpu().numpy().tobytes()
            e = hashlib.sha256(s + rh[i].cpu().numpy().tobytes()).digest()
            ok = ok and h[i].cpu().numpy().tobytes() == e and \
                p[i].cpu().numpy().tobytes() == hashlib.sha256(s + e).digest()
        row = {"row": "shape", "segments": n, "segment_bytes": seg, "split_below": below,
               "kernel": "split" if n < below else "lane", "ok": ok, "ms": ms, "segments_s": n / (ms * 1e-3),
               "bytes_s": n * seg / (ms * 1e-3)}
        if n == 1:
            s = data[:seg].cpu().numpy().tobytes()
            r4 = rh[0].cpu().numpy().tobytes()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e = hashlib.sha256(s + r4).digest()
                hashlib.sha256(s + e).digest()
            row["hashlib_host_ms"] = (time.perf_counter() - t0) / args.steps * 1e3
        del data
        dms, ntok = decrypt_ms(n * seg, dev, g, args.steps, args.warmup)
        row.update({"decrypt_16k_tokens": ntok, "decrypt_ms": dms, "hash_over_decrypt": ms / dms})
        emit(row)

    lane, split = Variant("lane"), Variant("split")
    for n, seg in [(1, 1048575), (64, 16384), (1, 16384), (128, 16384), (256, 16384), (512, 16384), (1024, 16384),
                   (1280, 16384), (1536, 16384), (2048, 16384), (4096, 16384), (256, 1048575), (1024, 1048575), (1024, 464)]:
        data, off, ln, rh, h, p = segments(n, seg, dev, g)
        h2, p2 = torch.zeros_like(h), torch.zeros_like(p)
        lms = median_ms(lambda: lane.run(data, off, ln, rh, h, p), args.steps, args.warmup)
        sms = median_ms(lambda: split.run(data, off, ln, rh, h2, p2), args.steps, args.warmup)
        emit({"row": "split", "segments": n, "segment_bytes": seg, "lane_ms": lms, "split_ms": sms,
              "split_over_lane": sms / lms, "identical": bool(torch.equal(h, h2) and torch.equal(p, p2)),
              "nonzero": bool(h.any() and p.any())})

    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
