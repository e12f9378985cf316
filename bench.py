"""Benchmark: device-resident AES-256-CBC + HMAC-SHA256 token throughput.

BASELINE.json metric: "device-resident packets/s + GiB/s AES-256-CBC+HMAC-SHA256
at 1/2/4/8 MI355X".  Workload (BASELINE.json configs[1]):
2^20 packets x 500 B plaintext per GPU, one link key; one STEP = encrypt+MAC
of the batch (Token.encrypt, Token.py:87-97) followed by verify+decrypt of the
tokens it produced (Token.decrypt, Token.py:100-114).  Inputs are generated on
the device before timing (synthetic, uniform random bytes).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c3|c4|c5] [--full] [--dump-outputs DIR]
  torchrun --nproc-per-node N bench.py --gpus N ...   (one process per GPU)

A plain run does what the headline needs and no more: set up the batch, check
one round trip of it, warm up, time K steps, print the line.  --full adds every
other measurement of the line (the other HBM layout, aligned slots, the
in-run clock's stamped pass, the host-origin and composed-interface paths, the
8-GPU rank shares, c3, per-call threads, the CPU baselines and, at N > 1, the
host-origin aggregate and the sharded c4 pass); without it those fields are
null.  --dump-outputs DIR writes what the last timed step computed as
DIR/<name>.npy (dump_outputs below); the inputs are seeded, so two builds run
with the same arguments can be compared output for output.

Multi-GPU: packets are independent, so each rank owns its own 2^20-packet
shard (weak scaling) and no collective touches the data path; RCCL is used
only for the barrier and the max-over-ranks reduction of the timings.
Rank 0 prints one JSON line.

--config c4 / c5 run BASELINE.json's sharded configs instead: rank 0 holds
the whole batch (c4: 262 144 x 16 KiB Resource chunks, one key; c5: 8 M
packets of 64 B-4 KiB, 65 536 keys, half encrypted and half decrypted), and
shard.sharded_call moves each rank its share over RCCL (xGMI), runs the
kernels, and gathers the outputs back; scatter, compute and gather are timed
separately.  With N > 1 the default c2 run with --full also
makes one sharded c4 pass and reports it under "sharded_c4".
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# --- roofline model ---------------------------
# Canonical VALU lane-ops per packet (SURVEY §8(d) constants):
#   AES block 352, SHA-256 compression 1464, tag compare 8 (decrypt only).
AES_BLOCK_OPS, SHA_CMP_OPS, TAG_CMP_OPS = 352, 1464, 8
LDS_LOOKUPS_PER_BLOCK = 224        # 16 per round x 14 rounds (AES-256)


def blocks(L):
    return L // 16 + 1


def sha_compressions(L):
    # ipad/opad midstates are per key; inner hash over iv||ct after the ipad
    # block, plus one outer compression.
    return math.ceil((64 + 16 + 16 * blocks(L) + 9) / 64) - 1 + 1


def ops_enc(L):
    return AES_BLOCK_OPS * blocks(L) + SHA_CMP_OPS * sha_compressions(L)


def ops_dec(L):
    return ops_enc(L) + TAG_CMP_OPS


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3, help="minimum untimed warmup steps")
    ap.add_argument("--warmup-seconds", type=float, default=0.3,
                    help="keep warming up until this much back-to-back work has run (clock ramp)")
    ap.add_argument("--packets", type=int, default=1 << 20, help="packets per GPU")
    ap.add_argument("--length", type=int, default=500, help="plaintext bytes per packet")
    ap.add_argument("--keys", type=int, default=1, help="1 = single link key (c2); 65536 = c3")
    ap.add_argument("--pt-stride", type=int, default=0, help="bytes between plaintext rows in HBM (0: packed)")
    ap.add_argument("--tok-stride", type=int, default=0, help="bytes between token rows in HBM (0: packed)")
    ap.add_argument("--tok-offset", type=int, default=0,
                    help="byte offset of the first token row in its buffer (with --tok-stride: row alignment)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="CPU baseline budget (0 disables)")
    ap.add_argument("--cpu-workers", type=int, default=0, help="0 = every CPU this process may run on")
    ap.add_argument("--config", choices=["c2", "c3", "c4", "c5"], default="c2",
                    help="c2 (default) / c3: weak-scaling token steps; c4 / c5: sharded batch held by rank 0")
    ap.add_argument("--sharded-reps", type=int, default=3, help="timed passes of a sharded config")
    ap.add_argument("--sharded-chunks", type=int, default=4,
                    help="N > 1: chunks per rank of the pipelined sharded pass (0 disables it)")
    ap.add_argument("--sharded-timeout", type=float, default=150.0,
                    help="N > 1: seconds allowed for the sharded c4 pass after the headline")
    ap.add_argument("--layout", choices=["rows", "interleaved"], default="rows",
                    help="HBM layout the headline is timed on: packed rows (default: the reference's byte strings, "
                         "the layout socket bytes arrive in) or the unit-interleaved device layout "
                         "(rt_encrypt_interleaved, coalesced, for batches produced on the device in that layout); "
                         "the other layout is timed right after it")
    ap.add_argument("--one-layout", action="store_true", help="time only --layout")
    ap.add_argument("--no-aligned", dest="aligned", action="store_false",
                    help="skip the aligned-slot rows measurement (aligned_rows in the line)")
    ap.add_argument("--e2e", action="store_true", default=True, help="also time the PCIe-inclusive path")
    ap.add_argument("--no-e2e", dest="e2e", action="store_false")
    ap.add_argument("--no-node", dest="node", action="store_false",
                    help="skip the composed interface path (reticulum_amd.pipeline) at N = 1")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beside the headline (other layout, aligned slots, stamped clock "
                         "pass, host-origin and interface paths, rank shares, c3, per-call threads, CPU baselines; "
                         "N > 1: host-origin aggregate and sharded c4); the options above that skip one apply to it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (c2 / c3 steps) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def warmup(step, stream, min_steps, min_seconds):
    """At least `min_steps` untimed steps, continued until `min_seconds` of
    back-to-back work have run: after an idle spell the GPU's clocks ramp up
    over ~25 steps (~50 ms) of this load, c2 steps falling from 2.0-2.45 ms to
    a steady 1.75 ms (tools/steps_probe.py, profiles/r02ao_steps_probe.txt).
    At most 8 steps are queued ahead of the GPU, which never idles in between."""
    import torch
    t0, n, prev = time.perf_counter(), 0, None
    while n < min_steps or time.perf_counter() - t0 < min_seconds:
        for _ in range(4):
            step()
        n += 4
        ev = torch.cuda.Event()
        ev.record(stream)
        if prev is not None:
            prev.synchronize()
        prev = ev
    torch.cuda.synchronize()
    return n, time.perf_counter() - t0


DUMP_SEED = 20250
DUMP_MAX_PACKETS = 1 << 20      # per-packet vectors: whole up to this many packets, else a seeded sample
DUMP_ROW_BYTES = 24_000_000     # float32 bytes given to the sampled token + plaintext rows


def _seeded_rows(n, k, seed):
    """``k`` of ``n`` row numbers, sorted, the first and the last row among
    them; the same for every run with the same ``n`` and ``k``."""
    import numpy as np
    if k >= n:
        return np.arange(n, dtype=np.int64)
    idx = np.random.Generator(np.random.PCG64(seed)).choice(n, size=k, replace=False)
    idx[:2] = (0, n - 1)
    return np.unique(idx).astype(np.int64)


def capture_outputs(tok, back, out_len, status, L):
    """What a caller of the timed step receives, taken on the device right
    after the last timed step (queued GPU work only; dump_outputs writes it):
    * out_len, status: the decrypt's per-packet length and status;
    * token_row_sums, plaintext_row_sums: the byte sum of every packet's token
      and of its decrypted plaintext (float64, exact);
    * tokens, plaintexts: whole rows of a seeded sample of packets, one byte
      per element, with their packet numbers in sample_rows.
    Past DUMP_MAX_PACKETS packets the per-packet vectors cover a seeded sample
    too (packet_rows).  Sizes are bounded by the constants above: under 64 MB
    in all for any batch."""
    import torch
    n, tl = tok.shape
    dev = tok.device
    out = {}
    pk = _seeded_rows(n, DUMP_MAX_PACKETS, DUMP_SEED)
    pk_d = None
    if len(pk) < n:
        pk_d = torch.from_numpy(pk).to(dev)
        out["packet_rows"] = pk_d.to(torch.float64)
    pick = (lambda v: v) if pk_d is None else (lambda v: v.index_select(0, pk_d))
    out["out_len"] = pick(out_len).to(torch.float32)
    out["status"] = pick(status).to(torch.float32)
    out["token_row_sums"] = pick(tok.sum(dim=1, dtype=torch.int64)).to(torch.float64)
    out["plaintext_row_sums"] = pick(back[:, :L].sum(dim=1, dtype=torch.int64)).to(torch.float64)
    rows = _seeded_rows(n, max(2, DUMP_ROW_BYTES // (4 * (tl + L))), DUMP_SEED + 1)
    rows_d = torch.from_numpy(rows).to(dev)
    out["sample_rows"] = rows_d.to(torch.float64)
    out["tokens"] = tok.index_select(0, rows_d).to(torch.float32)
    out["plaintexts"] = back[:, :L].index_select(0, rows_d).to(torch.float32)
    return out


def dump_outputs(directory, captured):
    """Write capture_outputs' arrays as ``directory``/<name>.npy (float32 /
    float64); returns their shapes and the bytes written for the line."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    shapes, total = {}, 0
    for name, t in captured.items():
        a = t.cpu().numpy()
        assert a.dtype in (np.float32, np.float64)
        np.save(os.path.join(directory, name + ".npy"), a)
        shapes[name] = {"shape": list(a.shape), "dtype": str(a.dtype)}
        total += a.nbytes
    return {"arrays": shapes, "bytes": total,
            "note": "outputs of the last timed step of the headline layout (bench.capture_outputs): per-packet "
                    "out_len, status and byte sums of every token and plaintext, whole token and plaintext rows "
                    "of a seeded sample of packets (sample_rows)"}


def cpu_baseline(seconds, workers, L):
    """The pure-Python restatement (oracle/cpuref.py, reference work shape)
    on the host cores, enc+dec round trips of 500 B packets."""
    if seconds <= 0:
        return None
    import multiprocessing as mp
    from oracle import cpuref  # noqa: F401  (checked importable before forking)
    if workers <= 0:
        workers = host_cpus()
    ctx = mp.get_context("spawn")
    with ctx.Pool(workers) as pool:
        t0 = time.perf_counter()
        res = pool.map(_cpu_worker, [(seconds, L, i) for i in range(workers)])
        wall = time.perf_counter() - t0
    pkts = sum(r[0] for r in res)
    busy = max(r[1] for r in res)
    rate = pkts / busy
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {
        "value": rate, "unit": "round trips/s (packets encrypted then decrypted)", "gib_s": rate * L / 2**30,
        "cores": workers, "cpu_count": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)), "kind": "port",
        "sample": f"{pkts} round trips (encrypt+decrypt) of {L} B packets, one key, oracle/cpuref.py "
                  f"(pure Python, per-call key schedule like AES.py:83,100) on {workers} processes for "
                  f"~{seconds:.0f} s each; wall {wall:.1f} s; cpu '{model}'; cpuref/reference speed "
                  f"ratio measured in the build container: enc 1.64, dec 1.95 (tools/calibrate_cpuref.py)",
    }


def cpu_openssl(seconds, threads, L):
    """BASELINE.md §5 item 5, the optional "strong CPU" row: the same token on
    OpenSSL libcrypto (AES-NI / SHA-NI, key schedule and HMAC pads once per
    key) over the host cores (tools/cpu_openssl.c, pinned to the golden
    vectors by tests/test_cpu_openssl.py).  Not the reference path."""
    lib_path = os.path.join(ROOT, "tools", "libcpu_openssl.so")
    if seconds <= 0 or not os.path.exists(lib_path):
        return None
    import ctypes
    lib = ctypes.CDLL(lib_path)
    lib.cpu_openssl_run.restype = ctypes.c_double
    lib.cpu_openssl_run.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    if threads <= 0:
        threads = host_cpus()
    done = ctypes.c_uint64()
    t0 = time.perf_counter()
    rate = lib.cpu_openssl_run(threads, seconds, L, ctypes.byref(done))
    wall = time.perf_counter() - t0
    if rate <= 0:
        return {"error": "OpenSSL round trip failed"}
    return {"value": rate, "unit": "round trips/s (packets encrypted then decrypted)", "gib_s": rate * L / 2**30,
            "cores": threads, "kind": "openssl (not the reference path)",
            "sample": f"{done.value} round trips of {L} B packets, one key per thread, OpenSSL libcrypto "
                      f"EVP aes-256-cbc + SHA-256 HMAC with hoisted pads, {threads} threads for ~{seconds:.0f} s; "
                      f"wall {wall:.1f} s"}


def host_cpus():
    """The CPUs this process can actually use: its affinity mask, capped by
    the cgroup CPU quota when one is set (cgroup v2 cpu.max, v1
    cfs_quota/period).  A GPU box shows every core of the machine in
    os.cpu_count() and the affinity mask while its container is given a
    share; 256 workers on a 16-CPU share ran 38 % slower than 16 (r02d)."""
    n = len(os.sched_getaffinity(0))
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
            if q != "max":
                quota = int(q) / int(p)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                p = int(f.read())
            if q > 0:
                quota = q / p
        except (OSError, ValueError):
            pass
    if quota:
        n = min(n, max(1, int(quota)))
    return max(1, n)


def _cpu_worker(arg):
    seconds, L, seed = arg
    import random
    from oracle import cpuref
    rnd = random.Random(seed)
    key = bytes(rnd.getrandbits(8) for _ in range(64))
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        pt = bytes(rnd.getrandbits(8) for _ in range(L))
        iv = bytes(rnd.getrandbits(8) for _ in range(16))
        tok = cpuref.encrypt(key, iv, pt)
        st, back = cpuref.decrypt(key, tok)
        assert st == 0 and back == pt
        n += 1
    return n, time.perf_counter() - t0


def main():
    args = parse()
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    # RNSTOK_BENCH_REHEARSE=1: every rank on GPU local % count over gloo, to
    # rehearse the N > 1 control flow on a one-GPU box (not a measurement)
    rehearse = os.environ.get("RNSTOK_BENCH_REHEARSE") == "1"
    if rehearse:
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    if world > 1:
        import datetime
        # a bounded timeout: a stuck collective ends the run instead of hanging it
        if rehearse:
            dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=300))
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local),
                                    timeout=datetime.timedelta(seconds=300))

    import reticulum_amd as rt
    from reticulum_amd import _native, device

    if args.config in ("c4", "c5"):
        if args.dump_outputs:
            raise SystemExit("bench: --dump-outputs covers the token steps (c2 / c3), not the sharded configs")
        res = sharded_bench(args.config, args, world, rank, local, reps=args.sharded_reps)
        if rank == 0:
            print(json.dumps(res))
        if world > 1:
            dist.destroy_process_group()
        return
    if args.config == "c3" and args.keys == 1:
        args.keys = 65536

    n, L = args.packets, args.length
    tl = rt.token_len(L)
    dev = torch.device("cuda", local)
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    ps, ts = max(args.pt_stride, L), max(args.tok_stride, tl)
    pt = torch.randint(0, 256, (n, ps), dtype=torch.uint8, device=dev, generator=g)[:, :L]
    iv = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
    to = args.tok_offset
    tok = torch.empty(n * ts + to, dtype=torch.uint8, device=dev)[to:].as_strided((n, tl), (ts, 1))
    back = torch.empty((n, max(ps, tl - 48)), dtype=torch.uint8, device=dev)[:, :tl - 48]
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    kg = torch.Generator().manual_seed(7)
    keys = torch.randint(0, 256, (args.keys, 64), dtype=torch.uint8, generator=kg).numpy()
    ks = rt.KeySet(keys, device=local)
    key_setup = key_setup_times(keys, local, dev) if args.keys > 1 else None
    key_idx = None
    if args.keys > 1:
        key_idx = torch.randint(0, args.keys, (n,), dtype=torch.int32, device=dev, generator=g)
    stream = torch.cuda.current_stream()

    # Both HBM layouts of the same packets: packed rows (pt row i = packet i,
    # the reference's byte strings) and the unit-interleaved device layout
    # (rt_encrypt_interleaved: 16-B unit u of packet p at 16*(u*n + p), every
    # wave load/store one contiguous KiB: north_star's "coalesced HBM loads
    # across the packet batch").  Tokens and plaintexts are identical in both
    # (checked below); --layout picks the one the headline value is timed on,
    # the other is timed right after it in the same run (--full only).
    layouts = [args.layout]
    if args.full and not args.one_layout:
        layouts += [x for x in ("interleaved", "rows") if x != args.layout]
    pt_u = tok_u = back_u = None
    if "interleaved" in layouts:
        pt_u = device.interleave(pt, L)
        tok_u = torch.empty((tl // 16, n, 16), dtype=torch.uint8, device=dev)
        back_u = torch.empty(((tl - 48) // 16, n, 16), dtype=torch.uint8, device=dev)

    def make_step(layout):
        ilv = layout == "interleaved"

        def step(ev=None):
            if ev is not None:
                ev[0].record(stream)
            if ilv:
                device.encrypt_interleaved(ks, pt_u, L, iv, tok_u, key_idx=key_idx, stream=stream)
            else:
                device.encrypt_uniform(ks, pt, L, iv, tok, key_idx=key_idx, stream=stream)
            if ev is not None:
                ev[1].record(stream)
            if ilv:
                device.decrypt_interleaved(ks, tok_u, tl, back_u, out_len, status, key_idx=key_idx, stream=stream)
            else:
                device.decrypt_uniform(ks, tok, tl, back, out_len, status, key_idx=key_idx, stream=stream)
            if ev is not None:
                ev[2].record(stream)
        return step

    steps = {lay: make_step(lay) for lay in layouts}
    # correctness gate on the benchmarked data (size-independent properties),
    # before the warmup so that nothing idles the GPU between warmup and timing
    for lay in layouts:
        steps[lay]()
        torch.cuda.synchronize()
        got = device.deinterleave(back_u, tl - 48) if lay == "interleaved" else back
        ok = bool((status == 0).all()) and bool((out_len == L).all()) and torch.equal(got[:, :L], pt)
        if not ok:
            raise SystemExit(f"bench: round trip failed on the benchmark batch ({lay} layout)")
    if len(layouts) == 2 and not torch.equal(device.deinterleave(tok_u, tl), tok):
        raise SystemExit("bench: the two layouts' tokens differ")

    # The same packed rows placed in 128-B-aligned slots (token ciphertext and
    # plaintext rows starting on a cache line): a caller-side layout choice
    # (DESIGN.md §4.9).  Same kernels, same bytes; timed after the headline.
    aligned_step = None
    if (args.full and args.aligned and not args.one_layout and args.layout == "rows"
            and ps == L and ts == tl and args.tok_offset == 0):
        pt_a = device.aligned_rows(n, L, 0, dev)          # plaintext rows on lines
        pt_a.copy_(pt)
        tok_a = device.aligned_rows(n, tl, 16, dev)       # each token's ciphertext on a line
        back_a = device.aligned_rows(n, tl - 48, 0, dev)
        ps_a, ts_a, to_a = pt_a.stride(0), tok_a.stride(0), 128 - 16

        def aligned_step(ev=None):
            if ev is not None:
                ev[0].record(stream)
            device.encrypt_uniform(ks, pt_a, L, iv, tok_a, key_idx=key_idx, stream=stream)
            if ev is not None:
                ev[1].record(stream)
            device.decrypt_uniform(ks, tok_a, tl, back_a, out_len, status, key_idx=key_idx, stream=stream)
            if ev is not None:
                ev[2].record(stream)
        aligned_step()
        torch.cuda.synchronize()
        if not (bool((status == 0).all()) and bool((out_len == L).all()) and torch.equal(back_a[:, :L], pt)
                and torch.equal(tok_a, tok)):
            raise SystemExit("bench: round trip failed on the aligned-slot batch")

    def timed(step, after=None):
        """The timed steps run unstamped (stamping adds a
        workgroup barrier and four atomics per workgroup to every launch);
        with --full the in-run clock comes from a stamped pass of the same
        steps right after them, whose elapsed time is reported beside the
        headline's.  ``after`` runs between the two (it may only queue GPU
        work: the outputs of the last timed step are still in place)."""
        evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
        clock = device.LaunchClock(dev) if args.full else None      # the stamped pass (rt_clock_stamps)
        if world > 1:
            dist.barrier()
        warm = warmup(step, stream, args.warmup, args.warmup_seconds)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            step(evs[k])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if after is not None:
            after()
        if clock is not None:
            with clock:
                t2 = time.perf_counter()
                for k in range(args.steps):
                    step()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
        if world > 1:
            dist.barrier()
        el = t1 - t0
        e_ms = sorted(e[0].elapsed_time(e[1]) for e in evs)
        d_ms = sorted(e[1].elapsed_time(e[2]) for e in evs)
        e_avg, d_avg = sum(e_ms) / len(e_ms), sum(d_ms) / len(d_ms)
        if world > 1:
            t = torch.tensor([el, e_avg, d_avg], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el, e_avg, d_avg = t.tolist()
        if clock is None:
            return el, e_avg, d_avg, e_ms, d_ms, warm, {"note": "no stamped pass in this run (bench.py --full)"}
        clk = clock.summary()
        clk["stamped_pass_ms_per_step"] = (t3 - t2) / args.steps * 1e3
        clk["unstamped_ms_per_step"] = (t1 - t0) / args.steps * 1e3
        clk["note"] = ("from a stamped pass of the same steps right after the timed (unstamped) ones; "
                       "stamped_pass_ms_per_step vs unstamped_ms_per_step is the stamps' cost on this box")
        return el, e_avg, d_avg, e_ms, d_ms, warm, clk

    captured = {}
    capture = None
    if args.dump_outputs and rank == 0:
        def capture():
            if layouts[0] == "interleaved":
                rows = device.deinterleave(tok_u, tl), device.deinterleave(back_u, tl - 48)
            else:
                rows = tok, back
            captured.update(capture_outputs(rows[0], rows[1], out_len, status, L))
    elapsed, enc_avg, dec_avg, enc_ms, dec_ms, (warm_steps, warm_s), clk = timed(steps[layouts[0]], capture)
    other = None
    if len(layouts) == 2:
        el2, e2, d2, _, _, _, clk2 = timed(steps[layouts[1]])
        other = {"layout": layouts[1], "value": n * world * args.steps / el2, "ms_per_step": el2 / args.steps * 1e3,
                 "encrypt_ms": e2, "decrypt_ms": d2, "in_run_clock": clk2,
                 "note": "the same packets in the other HBM layout, timed right after the headline in this run "
                         "(same warmup rule); tokens identical to the headline layout's (checked)"}
    aligned = None
    if aligned_step is not None:
        el3, e3, d3, _, _, _, clk3 = timed(aligned_step)
        aligned = {"value": n * world * args.steps / el3, "ms_per_step": el3 / args.steps * 1e3,
                   "encrypt_ms": e3, "decrypt_ms": d3, "in_run_clock": clk3,
                   "row_strides": {"plaintext": ps_a, "token": ts_a, "token_line_offset": to_a},
                   "note": "the headline's packed rows copied into 128-B-aligned slots (each token's ciphertext "
                           "and each plaintext row starts on a cache line); same kernels and bytes, tokens "
                           "identical (checked); a caller-side layout choice, not the headline (DESIGN.md §4.9)"}

    # PCIe-inclusive (host buffers, pinned) rate for DESIGN.md: every rank at
    # once on its own shard, over its own PCIe link (the node's host-origin rate)
    # (N > 1: below, after the headline line exists, under a deadline)
    e2e = e2e_rate(ks, pt, iv, L, tl, n, stream) if args.full and args.e2e and world == 1 else None
    node = shard8 = c5share = c3leg = percall = None
    if args.full and args.node and world == 1 and args.config == "c2":
        try:
            node = node_rate(dev)
        except Exception as exc:          # never fatal for the headline
            node = {"error": f"{type(exc).__name__}: {exc}"}
        try:
            shard8 = shard_rate(dev, _native.load().rt_num_cus(_native.context(local)))
        except Exception as exc:
            shard8 = {"error": f"{type(exc).__name__}: {exc}"}
        try:
            node["host"] = node_host_rate(dev)
        except Exception as exc:
            node["host"] = {"error": f"{type(exc).__name__}: {exc}"}
        try:
            c5share = c5_share_rate(dev, _native.load().rt_num_cus(_native.context(local)))
            # the same packets, each in its own 128-B-aligned slot
            al = c5_share_rate(dev, _native.load().rt_num_cus(_native.context(local)), align=True)
            c5share["aligned_slots"] = {k: al[k] for k in ("ok", "layout", "encrypt", "decrypt")}
        except Exception as exc:
            c5share = {"error": f"{type(exc).__name__}: {exc}"}
        try:
            c3leg = c3_rate(dev, _native.load().rt_num_cus(_native.context(local)))
        except Exception as exc:
            c3leg = {"error": f"{type(exc).__name__}: {exc}"}
        try:
            percall = per_call_rate()
        except Exception as exc:
            percall = {"error": f"{type(exc).__name__}: {exc}"}

    lib = _native.load()
    n_cu = lib.rt_num_cus(_native.context(local))
    peak_valu = n_cu * 128 * 2.4e9            # int32 lane-ops/s: 4 SIMD x 32 lanes per CU per clock
    peak_lds = n_cu * 32 * 2.4e9              # ds_read_b32 lane-lookups/s (2 cycles per wave64 instr per CU)
    ops_e, ops_d = ops_enc(L) * n, ops_dec(L) * n
    dom = "decrypt" if dec_avg > enc_avg else "encrypt"
    dom_ms = max(enc_avg, dec_avg)
    dom_ops = ops_d if dom == "decrypt" else ops_e
    traffic = traffic_from_profiles(dom, n, L, args.keys, args.layout)
    achieved = dom_ops / (dom_ms * 1e-3)
    bytes_enc = n * (L + 16 + tl + 0)         # read pt + iv, write token
    bytes_dec = n * (tl + (tl - 48) + 8)      # read token, write pt + len + status
    hbm_bytes = bytes_dec if dom == "decrypt" else bytes_enc
    in_run = in_run_clock(clk, dom, achieved, n_cu, {"encrypt": enc_avg, "decrypt": dec_avg})

    # the CPU baselines run on rank 0 at N = 1 here; at N > 1 after the sharded
    # pass, while the other ranks wait idle (below)
    cpu = cpu_baseline(args.cpu_seconds, args.cpu_workers, L) if args.full and world == 1 else None
    cpu_ssl = cpu_openssl(min(args.cpu_seconds, 5.0), args.cpu_workers, L) if args.full and world == 1 else None
    pkts_total = n * world * args.steps
    value = pkts_total / elapsed
    if key_setup is not None:
        # the per-key setup timed apart from the steps, and
        # amortised: once per run (the timed steps + one setup) and, worst
        # case, a fresh key table for every batch (one setup per step)
        st_s = key_setup["device_ms"] * 1e-3
        key_setup["amortised_per_run_value"] = pkts_total / (elapsed + st_s)
        key_setup["amortised_per_step_value"] = n * world / (elapsed / args.steps + st_s)
    line = {
        "metric": BASELINE_METRIC,
        "value": value,
        "unit": "packets/s (round trips: each packet encrypted+MACed, then verified+decrypted)",
        "gib_s": value * L / 2**30,
        "n_gpus": world,
        "steps": args.steps,
        "full": args.full,
        "warmup": args.warmup,
        "warmup_run": {"steps": warm_steps, "seconds": warm_s,
                       "note": "untimed steps actually run before the timed region: at least --warmup, continued "
                               "until --warmup-seconds of back-to-back work (GPU clock ramp-up, bench.warmup)"},
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "key_setup": key_setup,
        "dtype": "u8/u32 (integer)",
        "data": "synthetic uniform random plaintext and IVs generated on device (torch.randint), random keys",
        "config": {"workload": ("c2: 2^20 x 500 B packets per GPU, single link key" if args.keys == 1 else
                                f"c3: 2^20 x 500 B packets per GPU, {args.keys} per-packet keys")
                   if (n == 1 << 20 and L == 500) else f"{n} x {L} B packets per GPU, {args.keys} key(s)",
                   "packets_per_gpu": n, "plaintext_bytes": L, "token_bytes": tl, "keys": args.keys,
                   "row_strides": {"plaintext": ps, "token": ts, "token_offset": args.tok_offset}, "layout": args.layout,
                   "layout_note": ("unit-interleaved: 16-B unit u of packet p at 16*(u*n + p) (rt_encrypt_interleaved; "
                                   "coalesced HBM loads across the batch); the packed-row layout's numbers are under "
                                   "other_layout" if args.layout == "interleaved" else
                                   "packed rows (packet i at i*stride); the interleaved layout's numbers are under "
                                   "other_layout"),
                   "step": "encrypt+MAC then verify+decrypt of the same batch", "parallelism": f"shard{world}"},
        "kernels": {
            "encrypt": {"ms": enc_avg, "ms_median": enc_ms[len(enc_ms) // 2], "packets_s": n / (enc_avg * 1e-3),
                        "gib_s": n * L / (enc_avg * 1e-3) / 2**30,
                        "valu_frac": ops_e / (enc_avg * 1e-3) / peak_valu,
                        "lds_frac": n * blocks(L) * LDS_LOOKUPS_PER_BLOCK / (enc_avg * 1e-3) / peak_lds},
            "decrypt": {"ms": dec_avg, "ms_median": dec_ms[len(dec_ms) // 2], "packets_s": n / (dec_avg * 1e-3),
                        "gib_s": n * L / (dec_avg * 1e-3) / 2**30,
                        "valu_frac": ops_d / (dec_avg * 1e-3) / peak_valu,
                        "lds_frac": n * blocks(L) * LDS_LOOKUPS_PER_BLOCK / (dec_avg * 1e-3) / peak_lds},
        },
        "roofline": {"bound": "valu", "kernel": dom, "achieved": achieved / 1e12, "peak": peak_valu / 1e12,
                     "unit": "TOP/s", "frac": achieved / peak_valu,
                     "traffic": (traffic or {}).get("bytes_calibrated") or (traffic or {}).get("bytes_with_x2_fetch_correction"),
                     "traffic_guide_x2": (traffic or {}).get("bytes_with_x2_fetch_correction"),
                     "traffic_detail": traffic,
                     "ops_per_packet": ops_dec(L) if dom == "decrypt" else ops_enc(L),
                     "algorithmic_bytes_per_launch": hbm_bytes,
                     "algorithmic_hbm_gb_s": hbm_bytes / (dom_ms * 1e-3) / 1e9,
                     **ceiling_fracs(dom, L, args.keys, achieved / peak_valu),
                     "in_run_clock": in_run,
                     "cycles_per_launch": (in_run.get(dom) or {}).get("cycles_per_launch"),
                     "clock_ghz": (in_run.get(dom) or {}).get("clock_ghz"),
                     "frac_at_measured_clock": in_run.get("frac_at_measured_clock"),
                     "sustained_clock_ghz_committed_pmc": sustained_clock_ghz(dom, n, L, args.keys, args.layout),
                     "lds_frac": n * blocks(L) * LDS_LOOKUPS_PER_BLOCK / (dom_ms * 1e-3) / peak_lds,
                     "issue_model": issue_model(dom, n, L, args.keys, n_cu, dom_ms,
                                                (in_run.get(dom) or {}).get("clock_ghz")
                                                or sustained_clock_ghz(dom, n, L, args.keys, args.layout),
                                                (_newest_pmc(dom, n, L, args.keys, args.layout)[1] or {}).get(dom)),
                     "note": "achieved = canonical int32 VALU lane-ops per launch (SURVEY §8(d): 352/AES block, "
                             "1464/SHA-256 compression, +8 tag compare) / HIP-event kernel time; peak = CUs x 128 "
                             "lanes x 2.4 GHz (MI355X_MICROARCH.md), i.e. two wave64 VALU instructions per SIMD per "
                             "4-cycle issue slot, which gfx950 reaches only by dual issue of full-rate VGPR-only ops "
                             "from two waves (tools/issue_model_probe.hip, profiles/r03b_issue_model_probe.txt); "
                             "clock_ghz / cycles_per_launch / frac_at_measured_clock are measured in THIS run: every "
                             "workgroup of the timed launches stamps its span in shader cycles and 100 MHz ticks "
                             "(rt_clock_stamps; in_run_clock has both kernels); sustained_clock_ghz_committed_pmc is "
                             "the builder's PMC run (GRBM_GUI_ACTIVE / 8 XCDs / kernel-trace average); traffic = HBM bytes per launch from "
                             "the committed PMC with FETCH_SIZE scaled by a pure-read calibration of the kernel's own "
                             "read pattern where one exists (traffic_detail.fetch_calibration; the guide's x2 streaming "
                             "correction, traffic_guide_x2, overstates packed rows' sector-sized requests); ceiling_frac = the "
                             "guide-peak fraction this instruction stream reaches at most (its ISA slot floor: every "
                             "dual-issuable op paired, every LDS lookup a slot), ceiling_frac_valu_only the same with "
                             "every lookup hidden behind other waves' VALU issue; frac_over_ceiling = frac / "
                             "ceiling_frac (DESIGN.md §4.5, §4.10); the PMC summary is the newest committed "
                             "profiles/*_pmc.json of this workload (traffic_detail.source). issue_model = the kernel's issue slots "
                             "from its ISA (floor: every dual-issuable op paired; ceiling: none), its issued slots from "
                             "the PMC (SQ_INSTS_VALU - SQ_ACTIVE_INST_VALU2 + SQ_INSTS_LDS), and measured_core = the "
                             "kernel's own compute core timed from registers (tools/floor_probe.hip); DESIGN.md §4.5"},
        "cpu_baseline": cpu,
        "cpu_openssl": cpu_ssl,
        "other_layout": other,
        "aligned_rows": aligned,
        "e2e_pcie": e2e,
        "node_pipeline": node,
        "c4_rank_share_8gpu": shard8,
        "c5_rank_share_8gpu": c5share,
        "c3_per_key": c3leg,
        "per_call_threads": percall,
        "sharded_c4": None,
    }
    if captured:
        line["dumped_outputs"] = dump_outputs(args.dump_outputs, captured)

    # c4 sharded over the same ranks (scatter / kernels / gather over RCCL):
    # the xGMI legs of SURVEY §8(e), measured beside the weak-scaling headline.
    # Never fatal for the headline: an exception is reported in the line, and
    # a pass that does not finish within --sharded-timeout (a stuck
    # point-to-point transfer) makes rank 0 print the line with the error and
    # every rank exit, before the process group's own 300 s timeout would
    # abort the job without a line.
    if world > 1 and args.full and args.e2e:
        # every rank's host-origin path at once; a stuck barrier or reduction
        # here must not cost the headline line either
        guard = _LineGuard(line if rank == 0 else None, 120.0, field="e2e_pcie", what="host-origin pass")
        try:
            line["e2e_pcie"] = e2e_rate(ks, pt, iv, L, tl, n, stream, sync_all=dist.barrier,
                                        reduce_max=lambda v: _reduce_max(v, dev), world=world)
        except Exception as e:  # reported, never fatal for the headline line
            line["e2e_pcie"] = {"error": f"{type(e).__name__}: {e}"}
        guard.finish()
    if world > 1 and args.full and os.environ.get("RNSTOK_BENCH_SHARDED", "1") != "0":
        guard = _LineGuard(line if rank == 0 else None, args.sharded_timeout)
        try:
            line["sharded_c4"] = sharded_bench("c4", args, world, rank, local, reps=2)
        except Exception as e:  # reported, never fatal for the headline line
            line["sharded_c4"] = {"error": f"{type(e).__name__}: {e}"}
        dist.barrier()
        guard.finish()
    elif world > 1:
        dist.barrier()
    if world > 1 and args.full:
        # north_star: the reference path timed on the same box's host cores in
        # the same run, at every N.  Rank 0 runs it after the GPU work; the
        # other ranks block on the rendezvous store (a socket read, no spinning
        # host thread competing for the cores being timed).
        _cpu_phase(line, args, L, rank)
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


def _reduce_max(values, dev):
    """Elementwise max of a list of floats over all ranks."""
    import torch
    import torch.distributed as dist
    on = dev if dist.get_backend() == "nccl" else "cpu"
    t = torch.tensor(values, dtype=torch.float64, device=on)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return t.tolist()


def _cpu_phase(line, args, L, rank):
    """N > 1: cpu_baseline and cpu_openssl on rank 0; the other ranks wait on
    the process group's store until rank 0 is done (dist.barrier instead when
    the store is not reachable)."""
    import torch.distributed as dist
    store = None
    try:
        store = dist.distributed_c10d._get_default_store()
    except Exception:   # noqa: BLE001 (private API; fall back to a barrier)
        store = None
    key = "rnstok_bench_cpu_done"
    if rank == 0:
        try:
            line["cpu_baseline"] = cpu_baseline(args.cpu_seconds, args.cpu_workers, L)
            line["cpu_openssl"] = cpu_openssl(min(args.cpu_seconds, 5.0), args.cpu_workers, L)
        except Exception as e:  # reported, never fatal for the headline line
            line["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
        if line.get("cpu_baseline") and "error" not in line["cpu_baseline"]:
            line["cpu_baseline"]["note"] = ("timed on rank 0 after the GPU phases of this N > 1 run, the other "
                                            "ranks idle (blocked on the rendezvous store)")
        if store is not None:
            store.set(key, "1")
    if store is not None:
        if rank != 0:
            import datetime
            store.wait([key], datetime.timedelta(seconds=max(120.0, 4 * args.cpu_seconds + 60)))
    else:
        dist.barrier()


class _LineGuard:
    """Deadline for an optional phase of an N > 1 run (the sharded pass, the
    host-origin pass).  On expiry rank 0 prints the headline line (``field``
    carrying the error) and every rank leaves with status 0; finish() cancels
    it."""

    def __init__(self, line, seconds, field="sharded_c4", what="sharded pass"):
        import threading
        self.line, self.lock, self.done = line, threading.Lock(), False
        self.field, self.what = field, what
        self.timer = threading.Timer(seconds, self._expire, args=(seconds,))
        self.timer.daemon = True
        self.timer.start()

    def _expire(self, seconds):
        with self.lock:
            if self.done:
                return
            self.done = True
            if self.line is not None:
                prev = self.line.get(self.field)
                self.line[self.field] = {"error": f"{self.what} unfinished after {seconds} s", "partial": prev}
                print(json.dumps(self.line), flush=True)
            sys.stderr.flush()
            os._exit(0)

    def finish(self):
        with self.lock:
            self.done = True
        self.timer.cancel()


def key_setup_times(keys, local, dev, reps=5):
    """Per-key setup of a c3 run, timed apart from the token steps (SURVEY
    §8(d) c3): the AES-256 key schedules and HMAC ipad/opad midstates of every
    key, built on the GPU.  `host_ms`: from the host key table
    (rt_keyset_create: copy in + expansion); `device_ms`: from a key table
    already in HBM (device.keyset, rt_keyset_create_device, e.g. after
    shard.broadcast_keys).  Wall time of the call + stream sync, best of `reps`
    after one untimed call each (the first pays the allocator)."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    keys_d = torch.from_numpy(keys).to(dev)

    def best(make):
        make()
        torch.cuda.synchronize()
        b = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            k = make()
            torch.cuda.synchronize()
            b = min(b, time.perf_counter() - t0)
            del k
        return b * 1e3

    host_ms = best(lambda: rt.KeySet(keys, device=local))
    dev_ms = best(lambda: device.keyset(keys_d))
    return {"keys": int(keys.shape[0]), "host_ms": host_ms, "device_ms": dev_ms,
            "keys_per_s_device": keys.shape[0] / (dev_ms * 1e-3),
            "note": "AES-256 encryption + equivalent-inverse decryption schedules and HMAC-SHA256 ipad/opad midstates "
                    "of every key (544 B records), built on the GPU; "
                    "host_ms from the host table (rt_keyset_create), device_ms from a table already in HBM "
                    "(rt_keyset_create_device); best of 5 after one untimed call; amortised_* values use device_ms"}


def sharded_bench(cfg, args, world, rank, local, reps=3):
    """BASELINE.json configs c4 / c5: one batch held by rank 0, sharded over
    the ranks with shard.sharded_call (RCCL grouped point-to-point sends over
    xGMI), per-rank kernels, gather back to rank 0.  Times are max over ranks
    of each phase, averaged over `reps` passes after one warm-up pass; the
    gathered outputs are checked on rank 0 (round trip)."""
    import torch
    import torch.distributed as dist
    import reticulum_amd as rt
    from reticulum_amd import device, shard

    dev = torch.device("cuda", local)
    dist_on = dist.is_available() and dist.is_initialized()
    g = torch.Generator(device=dev).manual_seed(4242)
    kg = torch.Generator().manual_seed(4243)
    # batch size: shard_n when given (tests: the exact per-rank share of an
    # 8-GPU run), else --packets when changed from its c2 default, else the
    # BASELINE size of the config
    shard_n = getattr(args, "shard_n", None)
    if cfg == "c4":
        n = shard_n or (args.packets if args.packets != 1 << 20 else 262_144)
        L = 16384
        n_keys = 1
        lens = torch.full((n,), L, dtype=torch.int32)
    else:
        n = shard_n or (args.packets if args.packets != 1 << 20 else 8 << 20)
        n_keys = 65536
        lens = torch.randint(64, 4097, (n,), dtype=torch.int32, generator=kg)
    keys = torch.randint(0, 256, (n_keys, 64), dtype=torch.uint8, generator=kg).numpy()
    keys_ms = None
    if dist_on and world > 1:
        # rank 0 holds the key table; every rank receives it over RCCL and
        # expands its own copy on its GPU
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        ks = shard.broadcast_keyset(torch.from_numpy(keys).to(dev) if rank == 0 else None, src=0, device=dev)
        torch.cuda.synchronize()
        dist.barrier()
        keys_ms = (time.perf_counter() - t0) * 1e3
    else:
        ks = rt.KeySet(keys if n_keys > 1 else keys[0].tobytes(), device=local)
    uniform = cfg == "c4"

    def offsets(lengths):
        o = torch.zeros(lengths.numel(), dtype=torch.int64, device=lengths.device)
        if lengths.numel() > 1:
            o[1:] = torch.cumsum(lengths[:-1].to(torch.int64), 0)
        return o

    def tok_lengths(lengths):
        return (16 + 16 * (lengths // 16 + 1) + 32).to(torch.int32)

    def enc_work(b, o, l, rows):
        iv, kidx = rows if n_keys > 1 else (rows[0], None)
        tl = tok_lengths(l)
        toff = offsets(tl)
        tok = torch.empty(int(tl.to(torch.int64).sum()), dtype=torch.uint8, device=dev)
        if l.numel():
            if uniform:
                m = l.numel()
                device.encrypt_uniform(ks, b.view(m, L), L, iv, tok.view(m, -1), key_idx=kidx)
            else:
                device.encrypt(ks, b, o, l, iv, tok, toff, key_idx=kidx, sort=True)
        return tok, toff, tl, []

    def dec_work(b, o, l, rows):
        kidx = rows[0] if n_keys > 1 else None
        cap = (l - 48).clamp(min=0)
        poff = offsets(cap)
        pt = torch.empty(max(int(cap.to(torch.int64).sum()), 1), dtype=torch.uint8, device=dev)
        ol = torch.empty(l.numel(), dtype=torch.int32, device=dev)
        st = torch.empty(l.numel(), dtype=torch.int32, device=dev)
        if l.numel():
            if uniform:
                m = l.numel()
                T = int(l[0])
                device.decrypt_uniform(ks, b.view(m, T), T, pt[:m * (T - 48)].view(m, T - 48), ol, st, key_idx=kidx)
            else:
                device.decrypt(ks, b, o, l, pt, poff, ol, st, key_idx=kidx, sort=True)
        return pt, poff, cap.to(torch.int32), [ol, st]

    def run(work, buf, off, ln, rows, specs):
        if not dist_on:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = work(buf, off, ln, rows)
            torch.cuda.synchronize()
            return out, {"scatter_s": 0.0, "compute_s": time.perf_counter() - t0, "gather_s": 0.0}
        return shard.sharded_call(work, buf, off, ln, rows=rows, row_specs=specs, balance=not uniform,
                                  device=dev, sync=torch.cuda.synchronize)

    def run_piped(work, buf, off, ln, rows, specs, cap, out_specs):
        return shard.sharded_call_pipelined(work, buf, off, ln, rows=rows, row_specs=specs, out_cap=cap,
                                            out_row_specs=out_specs, chunks=args.sharded_chunks,
                                            balance=not uniform, device=dev, sync=torch.cuda.synchronize)

    def max_times(t):
        v = torch.tensor([t["scatter_s"], t["compute_s"], t["gather_s"]], dtype=torch.float64, device=dev)
        if dist_on:
            dist.all_reduce(v, op=dist.ReduceOp.MAX)
        return v.tolist()

    # rank 0's batch (inputs resident in its HBM before timing)
    if rank == 0:
        lens_d = lens.to(dev)
        off_d = offsets(lens_d)
        pt_buf = torch.randint(0, 256, (int(lens.to(torch.int64).sum()),), dtype=torch.uint8, device=dev,
                               generator=g)
        iv_d = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
        kidx_d = torch.randint(0, n_keys, (n,), dtype=torch.int32, device=dev, generator=g) if n_keys > 1 else None
    # c4: every segment encrypted, then its token decrypted;
    # c5: half the packets encrypted, the other half (valid tokens made before
    # timing) decrypted
    h = n // 2
    phases = [("encrypt", enc_work, slice(0, n) if cfg == "c4" else slice(0, h)),
              ("decrypt", dec_work, slice(0, n) if cfg == "c4" else slice(h, n))]
    report = {"metric": BASELINE_METRIC, "config": {}, "n_gpus": world, "reps": reps, "phases": {}}
    total = {"scatter_s": 0.0, "compute_s": 0.0, "gather_s": 0.0}
    ok = True
    for name, work, sel in phases:
        npk = sel.stop - sel.start
        if rank == 0:
            ln = lens_d[sel]
            kx = kidx_d[sel] if n_keys > 1 else None
            if name == "encrypt":
                b0 = int(off_d[sel][0]) if npk else 0
                buf = pt_buf[b0:b0 + int(ln.to(torch.int64).sum())]
                off = off_d[sel] - b0
                rows = [iv_d[sel]] + ([kx] if n_keys > 1 else [])
            else:   # the decrypt phase's tokens, made on rank 0 before timing
                tl = tok_lengths(ln)
                off = offsets(tl)
                buf = torch.empty(int(tl.to(torch.int64).sum()), dtype=torch.uint8, device=dev)
                device.encrypt(ks, pt_buf, off_d[sel], ln, iv_d[sel], buf, off, key_idx=kx, sort=not uniform)
                ln, src_off, src_len = tl, off_d[sel], lens_d[sel]
                rows = [kx] if n_keys > 1 else []
            torch.cuda.synchronize()
        else:
            buf = off = ln = None
            rows = []
        specs = ([(torch.uint8, 16)] + ([(torch.int32, 0)] if n_keys > 1 else [])) if name == "encrypt" \
            else ([(torch.int32, 0)] if n_keys > 1 else [])
        sums = [0.0, 0.0, 0.0]
        out = None
        for r in range(reps + 1):
            out, t = run(work, buf, off, ln, rows, specs)
            m = max_times(t)
            if r:
                sums = [a + b for a, b in zip(sums, m)]
        sc, co, ga = (x / reps for x in sums)
        # the same pass with the legs overlapped (shard.sharded_call_pipelined):
        # its output must equal the serial pass's
        piped_s = piped_ok = None
        if dist_on and world > 1 and getattr(args, "sharded_chunks", 0) > 0:
            cap = tok_lengths if name == "encrypt" else (lambda x: (x - 48).clamp(min=0))
            out_specs = [] if name == "encrypt" else [(torch.int32, 0), (torch.int32, 0)]
            best = float("inf")
            for r in range(reps + 1):
                pout, pt_ = run_piped(work, buf, off, ln, rows, specs, cap, out_specs)
                m = max_times({"scatter_s": 0.0, "compute_s": pt_["total_s"], "gather_s": 0.0})[1]
                if r:
                    best = min(best, m)
            piped_s = best
            if rank == 0:
                gb_, go_, gl_, gr_ = out
                pb_, po_, pl_, pr_ = pout
                used = int(gl_.to(torch.int64).sum())
                piped_ok = torch.equal(pb_[:used], gb_[:used]) and torch.equal(pl_, gl_.to(torch.int32)) and \
                    all(torch.equal(a, b) for a, b in zip(pr_, gr_))
                ok = ok and piped_ok
        total["scatter_s"] += sc
        total["compute_s"] += co
        total["gather_s"] += ga
        if rank == 0:
            gb, go, gl, grows = out
            if name == "encrypt":        # round trip of the gathered tokens on rank 0
                cap = gl - 48
                poff = offsets(cap)
                back = torch.empty(int(cap.to(torch.int64).sum()), dtype=torch.uint8, device=dev)
                ol = torch.empty(npk, dtype=torch.int32, device=dev)
                st = torch.empty(npk, dtype=torch.int32, device=dev)
                device.decrypt(ks, gb, go, gl, back, poff, ol, st, key_idx=rows[1] if n_keys > 1 else None,
                               sort=not uniform)
                torch.cuda.synchronize()
                ok = ok and bool((st == 0).all()) and torch.equal(ol, ln.to(torch.int32))
                if uniform:
                    ok = ok and torch.equal(back.view(npk, -1)[:, :L], buf.view(npk, L))
                else:
                    idx = torch.arange(0, npk, 997, device=dev)
                    for i in idx.tolist()[:64]:
                        ok = ok and torch.equal(back[int(poff[i]):int(poff[i]) + int(ln[i])],
                                                buf[int(off[i]):int(off[i]) + int(ln[i])])
            else:                        # gathered plaintexts == the originals
                ol, st = grows
                ok = ok and bool((st == 0).all()) and torch.equal(ol, src_len)
                for i in range(0, npk, 997):
                    a = int(src_off[i])
                    ok = ok and torch.equal(gb[int(go[i]):int(go[i]) + int(src_len[i])],
                                            pt_buf[a:a + int(src_len[i])])
        byts = int(lens[sel].to(torch.int64).sum())
        report["phases"][name] = {"packets": npk, "plaintext_bytes": byts,
                                  "scatter_ms": sc * 1e3, "compute_ms": co * 1e3, "gather_ms": ga * 1e3,
                                  "device_resident_packets_s": npk / co,
                                  "device_resident_gib_s": byts / co / 2**30,
                                  "end_to_end_packets_s": npk / (sc + co + ga),
                                  "pipelined_ms": piped_s * 1e3 if piped_s else None,
                                  "pipelined_chunks": args.sharded_chunks if piped_s else None,
                                  "pipelined_end_to_end_packets_s": npk / piped_s if piped_s else None,
                                  "pipelined_equals_serial": piped_ok,
                                  "xgmi_scatter_gb_s": None, "xgmi_gather_gb_s": None}
        total["pipelined_s"] = total.get("pipelined_s", 0.0) + (piped_s or 0.0)
    pkts = n
    byts_all = int(lens.to(torch.int64).sum())
    # canonical ops of the compute phases over the real lengths (SURVEY
    # §8(d)), priced against every rank's VALU peak; the time is the
    # host-timed compute phase (max over ranks: bucketing, allocation and
    # launches included), so this frac is a lower bound of the kernels'
    L64 = lens.to(torch.int64)
    B = L64 // 16 + 1
    ops = AES_BLOCK_OPS * B + SHA_CMP_OPS * ((64 + 16 + 16 * B + 9 + 63) // 64)
    if cfg == "c4":
        ops_all = 2 * int(ops.sum()) + TAG_CMP_OPS * n
    else:
        ops_all = int(ops.sum()) + TAG_CMP_OPS * (n - h)
    from reticulum_amd import _native
    n_cu = _native.load().rt_num_cus(_native.context(local))
    peak = world * n_cu * 128 * 2.4e9
    report["roofline"] = {"bound": "valu", "kernel": "compute phases (every rank's bucketing passes and kernels)",
                          "achieved": ops_all / total["compute_s"] / 1e12, "peak": peak / 1e12, "unit": "TOP/s",
                          "frac": ops_all / total["compute_s"] / peak, "traffic": None,
                          "note": "canonical int32 VALU lane-ops (352/AES block, 1464/SHA-256 compression, +8 per "
                                  "tag compare) summed over the real lengths / host-timed compute phases (max over "
                                  "ranks) / (ranks x CUs x 128 x 2.4 GHz): a lower bound of the kernels' fraction; "
                                  "per-kernel HBM traffic of these shapes: profiles/r04m_c5, profiles/r04j_pmc.json"}
    report.update({
        "value": pkts / total["compute_s"],
        "unit": ("round trips/s (device-resident, all ranks, compute phases: every segment encrypted, then its "
                 "token decrypted)" if cfg == "c4" else "packets/s (device-resident, all ranks, compute phases)"),
        "gib_s": byts_all / total["compute_s"] / 2**30,
        "end_to_end_packets_s": pkts / (total["scatter_s"] + total["compute_s"] + total["gather_s"]),
        "scatter_ms": total["scatter_s"] * 1e3, "compute_ms": total["compute_s"] * 1e3,
        "gather_ms": total["gather_s"] * 1e3, "key_broadcast_setup_ms": keys_ms, "scaling": "strong", "ok": ok,
        "pipelined_ms": total.get("pipelined_s", 0.0) * 1e3 or None,
        "pipelined_end_to_end_packets_s": pkts / total["pipelined_s"] if total.get("pipelined_s") else None,
        "pipelined_note": (f"shard.sharded_call_pipelined, {getattr(args, 'sharded_chunks', 0)} chunks per rank: the inputs of chunk "
                           f"k and the outputs of chunk k-2 move in one grouped RCCL batch while chunk k-1 computes; "
                           f"best of {reps} passes, max over ranks; output checked equal to the serial pass's"),
        "data": "synthetic random plaintext, IVs and keys generated on rank 0's device",
    })
    report["config"] = {
        "workload": ("c4: 262 144 x 16 KiB Resource chunks, one key, held by rank 0, sharded by count; "
                     "encrypt, then decrypt of the tokens"
                     if cfg == "c4" else "c5: 8 M packets of 64 B-4 KiB, 65 536 keys, 50/50 encrypt/decrypt, "
                                          "held by rank 0, sharded by AES+SHA work"),
        "packets": n, "parallelism": f"shard{world} (RCCL point-to-point scatter/gather)" if dist_on else "1 GPU"}
    if dist_on and world > 1:
        moved = byts_all * (world - 1) / world
        report["xgmi_note"] = (f"rank 0 sends {(world - 1)}/{world} of the inputs and receives {(world - 1)}/{world} "
                               f"of the outputs: ~{moved / 1e9:.2f} GB each way")
        for name in report["phases"]:
            ph = report["phases"][name]
            ph["xgmi_scatter_gb_s"] = ph["plaintext_bytes"] * (world - 1) / world / (ph["scatter_ms"] * 1e-3) / 1e9
            ph["xgmi_gather_gb_s"] = ph["plaintext_bytes"] * (world - 1) / world / (ph["gather_ms"] * 1e-3) / 1e9
    return report


BASELINE_METRIC = "device-resident packets/s + GiB/s AES-256-CBC+HMAC-SHA256 at 1/2/4/8 MI355X"


# Issue-slot model of the c2 kernels.  gfx950 gives
# each SIMD one VALU issue per 4 cycles; two full-rate VGPR-only ops of two
# waves may share it (dual issue, counted by SQ_ACTIVE_INST_VALU2), while every
# 4-cycle form (v_perm, v_alignbit, v_add3), a pair of SGPR-reading ops and
# each LDS instruction takes a slot alone (tools/issue_model_probe.hip,
# profiles/r03a/r03b_issue_model_probe.txt).  Slots per wave of 64 packets of
# 500 B from the ISA (tools/asm_mix.py --slots on the round-3 kernels):
#   encrypt: quad 0 (AES only) + 7 loop quads (AES + SHA) + 3 compressions
#   decrypt: 8 loop quads + 2 compressions
# "floor": every dual-issuable op paired; "ceiling": none paired.
SLOTS_PER_WAVE_PACKET_500B = {
    "encrypt": {"floor": 1929 + 7 * 3030 + 3 * 1102, "ceiling": 2290 + 7 * 3666 + 3 * 1385},
    "decrypt": {"floor": 8 * 3039 + 2 * 1095, "ceiling": 8 * 3724 + 2 * 1375},
}
# LDS lookups (ds_read_b32) per wave-packet inside those slot counts: 896 per
# AES quad (16 per block-round, 14 rounds, 4 blocks)
LOOKUP_SLOTS_PER_WAVE_PACKET_500B = {"encrypt": 8 * 896, "decrypt": 8 * 896}


def ceiling_fracs(kernel, L, keys, frac):
    """The guide-peak fraction the running instruction stream can reach at
    most (c2 shape: 500 B, one key), from its ISA slot floor: the peak is two
    wave64 VALU instructions per SIMD slot, so canonical lane-ops / (slots x
    128).  ceiling_frac charges every LDS lookup a slot (the issue-slot model
    of DESIGN.md §4.5); ceiling_frac_valu_only lets other waves' VALU work
    hide every lookup (tools/coissue_probe.hip).  None off the c2 shape."""
    if L != 500 or keys != 1 or kernel not in SLOTS_PER_WAVE_PACKET_500B:
        return {"ceiling_frac": None, "ceiling_frac_valu_only": None, "frac_over_ceiling": None}
    ops = 64 * (ops_dec(L) if kernel == "decrypt" else ops_enc(L))
    floor = SLOTS_PER_WAVE_PACKET_500B[kernel]["floor"]
    c = ops / (floor * 128)
    cv = ops / ((floor - LOOKUP_SLOTS_PER_WAVE_PACKET_500B[kernel]) * 128)
    return {"ceiling_frac": c, "ceiling_frac_valu_only": cv, "frac_over_ceiling": frac / c,
            "frac_over_ceiling_valu_only": frac / cv}


# The same per-wave-packet composition measured instead of counted: the
# kernels' own enc_quad / dec_quad / sha256_compress in register-only loops
# at c2's launch shape (tools/floor_probe.hip, profiles/r02af_floor_probe.txt;
# SIMD-cycles per wave-iteration: enc quad 12 583, quad 0 8 381, dec quad at
# 768 threads 13 437, compression 5 306).
CORE_CYCLES_PER_WAVE_PACKET_500B = {
    "encrypt": 8381 + 7 * 12583 + 3 * 5306,
    "decrypt": 8 * 13437 + 2 * 5306,
}


def in_run_clock(summary, dom, achieved, n_cu, event_ms):
    """The timed launches' own clock (device.LaunchClock over the timed
    steps): per kernel the sustained shader clock, the cycles per launch and
    the mean workgroup span beside the HIP-event time; for the dominant kernel
    the roofline fraction against the peak at that clock (CUs x 128 lanes x
    the measured clock instead of 2.4 GHz), which separates the code from the
    box's clock."""
    out = {k: (dict(v, event_ms=event_ms.get(k)) if isinstance(v, dict) else v) for k, v in summary.items()}
    d = out.get(dom)
    if d:
        out["frac_at_measured_clock"] = achieved / (n_cu * 128 * d["clock_ghz"] * 1e9)
        out["span_over_event"] = d["wg_span_ms"] / d["event_ms"] if d.get("event_ms") else None
    return out


def issue_model(kernel, n, L, keys, n_cu, ms, clock_ghz, pmc=None):
    """Issue-slot bounds of the dominant kernel (c2 shape only), and with the
    committed PMC summary of the same kernel (``pmc``: its counters) the slots
    it actually issued: SQ_INSTS_VALU - SQ_ACTIVE_INST_VALU2 + SQ_INSTS_LDS."""
    if L != 500 or keys != 1 or not clock_ghz:
        return None
    n_simd = n_cu * 4
    waves_per_simd = n / 64 / n_simd
    sl = SLOTS_PER_WAVE_PACKET_500B[kernel]
    floor = 4 * sl["floor"] * waves_per_simd
    ceiling = 4 * sl["ceiling"] * waves_per_simd
    core = CORE_CYCLES_PER_WAVE_PACKET_500B[kernel] * waves_per_simd
    ms_at = lambda cyc: cyc / (clock_ghz * 1e9) * 1e3   # noqa: E731
    out = {"model": "issue slots: one per SIMD per 4 cycles; two dual-issuable VALU ops of two waves may share one",
           "clock_ghz": clock_ghz,
           "floor_cycles_per_simd": floor, "floor_ms": ms_at(floor), "frac_of_floor": ms_at(floor) / ms,
           "floor_ms_at_2p4ghz": floor / 2.4e9 * 1e3,
           "ceiling_cycles_per_simd": ceiling, "ceiling_ms": ms_at(ceiling),
           "measured_core": {"cycles_per_simd": core, "ms": ms_at(core), "frac": ms_at(core) / ms,
                             "source": "tools/floor_probe.hip (the kernel's own quad/compression code from "
                                       "registers only, no memory or packet loop), profiles/r02af_floor_probe.txt"}}
    if pmc:
        try:
            slots = (pmc["SQ_INSTS_VALU"] - pmc["SQ_ACTIVE_INST_VALU2"] + pmc["SQ_INSTS_LDS"]) / n_simd
            cyc = pmc["GRBM_GUI_ACTIVE"] / 8
            out["pmc"] = {"issued_slots_per_simd": slots, "slot_cycles": 4 * slots, "kernel_cycles_per_xcd": cyc,
                          "slot_cycles_over_kernel_cycles": 4 * slots / cyc,
                          "dual_issued_frac_of_valu": 2 * pmc["SQ_ACTIVE_INST_VALU2"] / pmc["SQ_INSTS_VALU"]}
            # two limits (tools/coissue_probe.hip): the SIMDs'
            # VALU slots, and the CU-wide LDS pipe at 128 B/clk (2 cycles per
            # wave64 ds_read_b32), which other waves' VALU work can overlap
            valu_cyc = 4 * (pmc["SQ_INSTS_VALU"] - pmc["SQ_ACTIVE_INST_VALU2"]) / n_simd
            lds_cyc = 2.0 * pmc["SQ_INSTS_LDS"] / n_cu
            out["two_limits"] = {"valu_slot_cycles_per_simd": valu_cyc, "lds_pipe_cycles_per_cu": lds_cyc,
                                 "kernel_cycles": cyc, "valu_share": valu_cyc / cyc, "lds_pipe_share": lds_cyc / cyc,
                                 "lds_time_hidden_behind_valu": max(0.0, valu_cyc + lds_cyc - cyc) / min(valu_cyc, lds_cyc)}
        except (KeyError, TypeError, ZeroDivisionError):
            pass
    return out


def _newest_pmc(kernel, n, L, keys, layout="rows"):
    import glob
    import re

    def order(path):   # r02y < r02aa < r02ak: round, then tag length, then tag
        m = re.match(r"r(\d+)([a-z]+)_(?:ilv)?pmc\.json$", os.path.basename(path))
        return (int(m.group(1)), len(m.group(2)), m.group(2)) if m else (-1, 0, "")

    suffix = "_pmc.json" if layout == "rows" else "_ilvpmc.json"     # interleaved-layout runs: rNNx_ilvpmc.json
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*" + suffix)), key=order, reverse=True):
        try:
            with open(path) as f:
                d = json.load(f)
        except (OSError, ValueError):
            continue
        meta = d.get("_workload", {})
        if meta.get("packets") == n and meta.get("length") == L and meta.get("keys") == keys and kernel in d:
            return path, d
    return None, None


def sustained_clock_ghz(kernel, n, L, keys, layout="rows"):
    """Shader clock under this load: GRBM_GUI_ACTIVE per launch (summed over
    the 8 XCDs) / 8 over the kernel's average duration in the kernel trace of
    the same profiling run (profiles/<round>_kernel_stats.csv)."""
    import csv
    path, d = _newest_pmc(kernel, n, L, keys, layout)
    if not path:
        return None
    stats = path.replace("_ilvpmc.json", "_ilv_kernel_stats.csv").replace("_pmc.json", "_kernel_stats.csv")
    tags = ("k_encrypt<14, ", "k_encrypt_split<14, ") if kernel == "encrypt" else ("k_decrypt<14, ",)
    try:
        with open(stats) as f:
            rows = [r for r in csv.DictReader(f) if any(t in r["Name"] for t in tags)]
        ns = float(rows[0]["AverageNs"])
        return d[kernel]["GRBM_GUI_ACTIVE"] / 8 / ns
    except (OSError, KeyError, IndexError, ValueError):
        return None


# FETCH_SIZE scale per kernel read pattern, from a pure-read kernel over known
# bytes in the same pattern (MI355X_MICROARCH.md §HBM: "calibrate on a known
# byte count in your own access pattern"; tools/fetch_calib.sh,
# profiles/r06_fetch_calib.txt): packed c2 token rows read as k_decrypt reads
# them report 548.1 MB for 587.2 MB (a mix of 64-B and 128-B requests, each
# tallied at 64 B), so their bytes are FETCH_SIZE x 1.071; the guide's x2 holds
# for whole-line streams (the interleaved layout, tokens with their ciphertext
# on lines: 0.684 x).
FETCH_CALIBRATION = {
    ("decrypt", "rows"): (587.2 / 548.1, "FETCH_SIZE x 1.071: packed 560-B token rows read in 8-unit groups, "
                                         "548.1 MB counted for 587.2 MB known (profiles/r06_fetch_calib.txt)"),
}


def traffic_from_profiles(kernel, n, L, keys, layout="rows"):
    """HBM bytes per launch of `kernel` from the newest committed PMC summary
    whose workload matches (profiles/<round>_pmc.json, tools/pmc_summary.py)."""
    path, d = _newest_pmc(kernel, n, L, keys, layout)
    if path:
        raw = d[kernel].get("hbm_bytes_per_launch_uncorrected")
        if raw:
            m = d[kernel]
            k = FETCH_CALIBRATION.get((kernel, layout))
            cal = (k[0] * m["FETCH_SIZE"] + m["WRITE_SIZE"]) * 1024 if k and "FETCH_SIZE" in m and "WRITE_SIZE" in m else None
            return {"bytes": raw, "bytes_with_x2_fetch_correction": d[kernel].get("hbm_bytes_per_launch"),
                    "bytes_calibrated": cal, "fetch_calibration": k[1] if k else None,
                    "source": os.path.relpath(path, ROOT),
                    "calibration": "roofline.traffic = bytes_calibrated where the kernel's read pattern is "
                                   "calibrated (FETCH_SIZE x the pattern's known/counted ratio + WRITE_SIZE), else "
                                   "FETCH_SIZE x 2 + WRITE_SIZE (the guide's correction for coalesced 16-B streams, "
                                   "whose 128-B requests are tallied at 64 B: our control reads 0.50x its known "
                                   "bytes); bytes = FETCH_SIZE + WRITE_SIZE as counted. Pure reads of known bytes "
                                   "(tools/fetch_calib.sh, profiles/r06_fetch_calib.txt): packed 560-B token rows "
                                   "0.933x, the same tokens with each ciphertext on a line 0.684x, 500-B plaintext "
                                   "rows in 64-B steps 1.408x"}
    return None


def node_rate(dev, steps=10, g=None, n=1 << 20, L=383, isz=16):
    """The interface path composed on the device (reticulum_amd.pipeline,
    DESIGN.md §4.8): n DATA packets of L B plaintext (383 B: a 432-B token,
    451-B packet, 467 B with a 16-B IFAC) out through token encrypt -> header
    pack -> IFAC mask -> HDLC framing into one stream, and that stream back in
    through deframing -> IFAC unmask -> unpack -> token decrypt.  Median of
    ``steps`` HIP-event timings per direction after the clock warmup; a
    sample of 4096 plaintexts, every status and every IFAC checked."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import pipeline
    g = g if g is not None else torch.Generator(device=dev).manual_seed(6)
    pt = torch.randint(0, 256, (n, L), dtype=torch.uint8, device=dev, generator=g)
    iv = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
    dh = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
    ctx = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=g)
    ifac = torch.randint(0, 256, (n, isz), dtype=torch.uint8, device=dev, generator=g)
    ikey = torch.randint(0, 256, (64,), dtype=torch.uint8, device=dev, generator=g)
    ks = rt.KeySet(bytes(range(64)), device=dev.index if dev.index is not None else 0)
    state = {}

    def outb():
        state["framed"], state["foff"] = pipeline.outbound(ks, pt, iv, dh, ctx, ifac, ikey)

    outb()
    torch.cuda.synchronize()
    total = int(state["foff"][-1])
    stream_buf = state["framed"][:total].clone()

    def inb():
        state["res"] = pipeline.inbound(ks, stream_buf, ikey, isz, 2 * n)

    inb()
    torch.cuda.synchronize()
    r = state["res"]
    rows = torch.randint(0, n, (4096,), device=dev, generator=g)
    idx = r["pt_off"][rows].unsqueeze(1) + torch.arange(L, device=dev)
    ok = (int(r["n_frames"]) == n and bool((r["status"][:n] == 0).all()) and bool((r["pt_len"][:n] == L).all())
          and torch.equal(r["pt"][idx], pt[rows]) and torch.equal(r["ifac"][:n], ifac))
    res = {"packets": n, "plaintext_bytes": L, "ifac_size": isz, "stream_bytes": total, "ok": ok}
    stream = torch.cuda.current_stream(dev)
    for name, f in (("outbound", outb), ("inbound", inb)):
        warmup(f, stream, 2, 0.3)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev:
            a.record(stream)
            f()
            b.record(stream)
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)[steps // 2]
        res[name] = {"ms": ms, "packets_s": n / (ms * 1e-3), "stream_gb_s": total / (ms * 1e-3) / 1e9}
    res["note"] = ("reticulum_amd.pipeline: outbound = token encrypt, Packet.pack header, IFAC mask, HDLC framing "
                   "(one stream); inbound = HDLC deframing, IFAC unmask, Packet.unpack + hash, token decrypt; "
                   "device-resident, one link key, synthetic payloads; DESIGN.md \u00a74.8")
    return res


def node_host_rate(dev, n=1 << 20, L=383, isz=16, slices=32, n_streams=3, reps=3):
    """The composed interface path host-origin (north_star: "This path starts
    and ends in host memory (Interface socket buffers)"; TCPInterface.py:
    387-401 -> Link.py:1175-1182 inbound, Link.py:1161 -> TCPInterface.py:323
    outbound), pinned host buffers at both ends, `slices` slices round-robin
    on `n_streams` streams so one slice's H2D, another's kernels and a third's
    D2H overlap:
    * outbound: plaintexts, IVs, destination hashes, contexts and IFACs H2D ->
      pipeline.outbound -> the slice's HDLC stream D2H as GPU stores, its
      length read on the device (device.copy_to_host_upto: the host does not
      know a framed slice's length before it runs);
    * inbound: the framed stream H2D in slices cut at frame boundaries (each
      slice one read of the interface) -> pipeline.inbound -> the plaintext
      buffer and the per-packet offsets, lengths and statuses D2H as GPU
      stores.
    Best of ``reps`` passes; a sample of plaintexts and every status checked on
    the host copies, and the host stream equal to the device-resident one."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device, pipeline
    g = torch.Generator(device=dev).manual_seed(6)
    pt = torch.randint(0, 256, (n, L), dtype=torch.uint8, device=dev, generator=g)
    iv = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
    dh = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
    ctx = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=g)
    ifac = torch.randint(0, 256, (n, isz), dtype=torch.uint8, device=dev, generator=g)
    ikey = torch.randint(0, 256, (64,), dtype=torch.uint8, device=dev, generator=g)
    ks = rt.KeySet(bytes(range(64)), device=dev.index if dev.index is not None else 0)
    framed, foff = pipeline.outbound(ks, pt, iv, dh, ctx, ifac, ikey)
    torch.cuda.synchronize()
    fo = foff.cpu()
    total = int(fo[-1])
    ins_h = [x.cpu().pin_memory() for x in (pt, iv, dh, ctx, ifac)]
    ins_d = [torch.empty_like(x) for x in (pt, iv, dh, ctx, ifac)]
    ml = 19 + rt.token_len(L) + isz
    step = -(-n // slices)
    cuts = [(a, min(a + step, n)) for a in range(0, n, step)]
    cap = [(b - a) * (2 * ml + 2) for a, b in cuts]
    cap_off = [sum(cap[:k]) for k in range(len(cap))]
    out_h = torch.empty(sum(cap), dtype=torch.uint8).pin_memory()
    olen_h = torch.zeros(len(cuts), dtype=torch.int64).pin_memory()
    side = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
    stream_h = framed[:total].cpu().pin_memory()
    stream_d = torch.empty(total, dtype=torch.uint8, device=dev)
    pt_h = torch.empty(total, dtype=torch.uint8).pin_memory()
    meta_h = torch.empty(3 * n, dtype=torch.int64).pin_memory()     # per slice: (pt_off, pt_len, status) rows
    hold = []

    def outbound_pass():
        hold.clear()
        for k, (a, b) in enumerate(cuts):
            s = side[k % n_streams]
            with torch.cuda.stream(s):
                for hx, dx in zip(ins_h, ins_d):
                    dx[a:b].copy_(hx[a:b], non_blocking=True)
                fr, fo_ = pipeline.outbound(ks, *(dx[a:b] for dx in ins_d), ikey, stream=s)
                device.copy_to_host_upto(out_h[cap_off[k]:cap_off[k] + cap[k]], fr, fo_[-1:], stream=s)
                device.copy_to_host(olen_h[k:k + 1], fo_[-1:], stream=s)
                hold.append((fr, fo_))      # keep the slices' buffers alive until the pass is synchronised

    def inbound_pass():
        hold.clear()
        for k, (a, b) in enumerate(cuts):
            s = side[k % n_streams]
            lo, hi = int(fo[a]), int(fo[b])
            with torch.cuda.stream(s):
                stream_d[lo:hi].copy_(stream_h[lo:hi], non_blocking=True)
                # stream offsets, not slots: the plaintext buffer crosses PCIe
                # whole, and slots would add 256 B per packet to it
                r = pipeline.inbound(ks, stream_d[lo:hi], ikey, isz, 2 * (b - a), stream=s, aligned=False)
                device.copy_to_host(pt_h[lo:hi], r["pt"], stream=s)
                m = torch.stack([r["pt_off"][:b - a], r["pt_len"][:b - a].to(torch.int64),
                                 r["status"][:b - a].to(torch.int64)])
                device.copy_to_host(_meta_slot(meta_h, a, b), m, stream=s)
                hold.append((r, m))

    res = {"packets": n, "plaintext_bytes": L, "ifac_size": isz, "stream_bytes": total, "slices": len(cuts),
           "streams": n_streams}
    for name, f in (("outbound", outbound_pass), ("inbound", inbound_pass)):
        best = float("inf")
        for _ in range(reps + 1):         # the first pass warms the allocator and the clocks
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        res[name] = {"ms": best * 1e3, "packets_s": n / best,
                     "pcie_gb_s": ((n * (L + 16 + 16 + 1 + isz) + total) if name == "outbound" else 2 * total)
                     / best / 1e9}
    # checks on the host copies: every slice's stream equals the device-resident one, statuses, plaintexts
    ok = True
    for k, (a, b) in enumerate(cuts):
        lo, hi = int(fo[a]), int(fo[b])
        ok = ok and int(olen_h[k]) == hi - lo and torch.equal(out_h[cap_off[k]:cap_off[k] + hi - lo], stream_h[lo:hi])
    meta = torch.cat([_meta_slot(meta_h, a, b) for a, b in cuts], dim=1)
    ok = ok and bool((meta[2] == 0).all()) and bool((meta[1] == L).all())
    pt_c = pt.cpu()
    for k, (a, b) in enumerate(cuts):
        lo = int(fo[a])
        for i in (a, (a + b) // 2, b - 1):
            o = lo + int(_meta_slot(meta_h, a, b)[0, i - a])
            ok = ok and torch.equal(pt_h[o:o + L], pt_c[i])
    res["ok"] = ok
    res["note"] = ("host-origin composed interface path: pinned host buffers at both ends, H2D on the copy engine, "
                   "D2H as GPU stores into the pinned buffers, slices round-robin on streams; outbound pcie_gb_s "
                   "counts inputs + framed stream, inbound the stream both ways (plaintext buffer = stream size)")
    return res


def _meta_slot(meta_h, a, b):
    """Host rows (pt_off, pt_len, status) of packets [a, b) in node_host_rate's
    pinned metadata buffer (one contiguous (3, b - a) block per slice)."""
    return meta_h.view(-1)[3 * a:3 * b].view(3, b - a)


def shard_rate(dev, n_cu, steps=10, L=16384, per_cu=128):
    """The per-rank shape of c4 at 8 GPUs (32 768 x 16 KiB, 128
    tokens per CU), device-resident on this GPU: the lane-cooperative long-token
    kernels it routes to (k_encrypt_long4, k_decrypt_long2).
    Median of ``steps`` HIP-event timings per direction after the clock
    warmup, every token round-tripped, and the fraction of the integer-VALU
    peak (the same canonical op count as the headline)."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import _native, device
    n = per_cu * n_cu
    tl = rt.token_len(L)
    g = torch.Generator(device=dev).manual_seed(4)
    pt = torch.randint(0, 256, (n, L), dtype=torch.uint8, device=dev, generator=g)
    iv = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
    tok = torch.empty((n, tl), dtype=torch.uint8, device=dev)
    back = torch.empty((n, tl - 48), dtype=torch.uint8, device=dev)
    ol = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    ks = rt.KeySet(bytes(range(64)), device=dev.index if dev.index is not None else 0)
    stream = torch.cuda.current_stream(dev)
    enc = lambda: device.encrypt_uniform(ks, pt, L, iv, tok, stream=stream)
    dec = lambda: device.decrypt_uniform(ks, tok, tl, back, ol, st, stream=stream)
    enc()
    dec()
    torch.cuda.synchronize()
    ok = bool((st == 0).all()) and torch.equal(back[:, :L], pt)
    lib = _native.load()
    ctx = _native.context(dev.index if dev.index is not None else 0)
    res = {"tokens": n, "token_plaintext_bytes": L, "tokens_per_cu": per_cu, "ok": ok,
           "kernels": {"encrypt": int(lib.rt_plan_uniform(ctx, n, L, 0, 0)),
                       "decrypt": int(lib.rt_plan_uniform(ctx, n, tl, 0, 1))}}
    peak = n_cu * 128 * 2.4e9
    for name, f, ops in (("encrypt", enc, ops_enc(L)), ("decrypt", dec, ops_dec(L))):
        warmup(f, stream, 2, 0.3)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        with device.LaunchClock(dev) as lc:
            for a, b in ev:
                a.record(stream)
                f()
                b.record(stream)
            torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)[steps // 2]
        clk = lc.summary().get(name, {})
        res[name] = {"ms": ms, "tokens_s": n / (ms * 1e-3), "frac_of_valu_peak": ops * n / (ms * 1e-3) / peak,
                     "clock_ghz": clk.get("clock_ghz"), "cycles_per_launch": clk.get("cycles_per_launch")}
    res["note"] = ("one rank's share of c4 at 8 GPUs; CBC encryption is a serial chain per token, so this shape "
                   "is bound by the chain's round latency, not by issue (DESIGN.md \u00a74.2); kernels = "
                   "RT_KERNEL_* from rt_plan_uniform; clock_ghz / cycles_per_launch stamped by the kernels in "
                   "this run (rt_clock_stamps)")
    return res


def per_call_rate(threads=16, calls=1000, L=383, seconds_cap=20.0):
    """The reference's call pattern (RNS/Link.py:1161-1182: one synchronous
    Token call per packet, from many interface and application threads):
    ``threads`` threads, each with its own link key, alternately encrypting a
    ``L``-byte packet and decrypting the token through ``Token`` (one GPU
    round trip per call; the host entry points' eight staging lanes let eight
    run at once), and the same from one thread.  Calls/s over all threads."""
    import threading
    import reticulum_amd as rt
    res = {"plaintext_bytes": L}
    for name, n_th in (("threads", threads), ("one_thread", 1)):
        toks = [rt.Token(os.urandom(64)) for _ in range(n_th)]
        pts = [os.urandom(L) for _ in range(n_th)]
        for t, p in zip(toks, pts):                      # key sets built, kernels warm
            assert t.decrypt(t.encrypt(p)) == p
        bad, done = [], [0] * n_th
        barrier = threading.Barrier(n_th + 1)
        deadline = time.perf_counter() + seconds_cap

        def work(i):
            t, p = toks[i], pts[i]
            barrier.wait()
            for _ in range(calls // 2):
                if t.decrypt(t.encrypt(p)) != p:
                    bad.append(i)
                done[i] += 2
                if time.perf_counter() > deadline:
                    break
        th = [threading.Thread(target=work, args=(i,)) for i in range(n_th)]
        for x in th:
            x.start()
        barrier.wait()
        t0 = time.perf_counter()
        for x in th:
            x.join()
        el = time.perf_counter() - t0
        res[name] = {"threads": n_th, "calls_s": sum(done) / el, "seconds": el, "ok": not bad}
    res["note"] = ("one synchronous Token call per packet, as Link.encrypt/decrypt make them; host buffers, copies "
                   "included; calls_s counts encrypts and decrypts (DESIGN.md \u00a74.2, INTEGRATION.md \u00a71)")
    return res


def c5_share_rate(dev, n_cu, n=1 << 20, steps=10, n_keys=65536, align=False):
    """The per-rank shape of c5 at 8 GPUs (8 M packets of
    64-4096 B, 65 536 keys, 50/50 encrypt/decrypt; one rank's share is 2^20
    packets), device-resident on this GPU through the product's packed entry
    points with length bucketing (rt_encrypt_ex / rt_decrypt_ex,
    RT_F_SORT_BY_LENGTH: the bucketing passes are inside the timed region).
    The first half of the packets is encrypted, the second half's tokens
    (made before timing) are decrypted.  Median of ``steps`` HIP-event timings
    per direction after the clock warmup; canonical ops summed over the real
    lengths (352 per AES block, 1464 per SHA-256 compression,
    +8 per tag compare); every decrypt status and length checked, and a
    sample of plaintexts and tokens against each other (round trip).
    ``align``: every packet in its own 128-B-aligned slot (plaintexts on a
    line, each token's ciphertext on a line) instead of end to end."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    g = torch.Generator(device=dev).manual_seed(5)
    kg = torch.Generator().manual_seed(55)
    lens = torch.randint(64, 4097, (n,), dtype=torch.int32, generator=kg)
    keys = torch.randint(0, 256, (n_keys, 64), dtype=torch.uint8, generator=kg).numpy()
    ks = rt.KeySet(keys, device=dev.index if dev.index is not None else 0)
    kidx = torch.randint(0, n_keys, (n,), dtype=torch.int32, device=dev, generator=g)
    h = n // 2
    le, ld = lens[:h].to(dev), lens[h:].to(dev)

    # align: True (every buffer) or a set of "enc_in", "enc_out", "dec_in", "dec_out"
    sides = {"enc_in", "enc_out", "dec_in", "dec_out"} if align is True else set(align or ())

    def offs(x, phase=0, side=None):
        al = side in sides
        w = x.to(torch.int64)
        if al:
            w = (w + 127) // 128 * 128
        o = torch.zeros(x.numel(), dtype=torch.int64, device=dev)
        o[1:] = torch.cumsum(w[:-1], 0)
        return o + ((-phase) % 128 if al else 0)

    def span(o, x):
        return int(o[-1]) + int(x[-1]) + 1

    tlen = lambda x: (16 + 16 * (x // 16 + 1) + 32).to(torch.int32)     # noqa: E731
    # encrypt half: plaintexts -> tokens
    oe, ive = offs(le, 0, "enc_in"), torch.randint(0, 256, (h, 16), dtype=torch.uint8, device=dev, generator=g)
    pe = torch.randint(0, 256, (span(oe, le),), dtype=torch.uint8, device=dev, generator=g)
    te_len = tlen(le)
    te_off = offs(te_len, 16, "enc_out")
    te = torch.empty(span(te_off, te_len), dtype=torch.uint8, device=dev)
    # decrypt half: tokens made before timing
    od, ivd = offs(ld), torch.randint(0, 256, (n - h, 16), dtype=torch.uint8, device=dev, generator=g)
    pd = torch.randint(0, 256, (span(od, ld),), dtype=torch.uint8, device=dev, generator=g)
    td_len = tlen(ld)
    td_off = offs(td_len, 16, "dec_in")
    td = torch.empty(span(td_off, td_len), dtype=torch.uint8, device=dev)
    device.encrypt(ks, pd, od, ld, ivd, td, td_off, key_idx=kidx[h:], sort=True)
    boff = offs(td_len - 48, 0, "dec_out")
    back = torch.empty(span(boff, td_len - 48), dtype=torch.uint8, device=dev)
    ol = torch.empty(n - h, dtype=torch.int32, device=dev)
    st = torch.empty(n - h, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    enc = lambda: device.encrypt(ks, pe, oe, le, ive, te, te_off, key_idx=kidx[:h], sort=True, stream=stream)  # noqa
    dec = lambda: device.decrypt(ks, td, td_off, td_len, back, boff, ol, st, key_idx=kidx[h:], sort=True,  # noqa
                                 stream=stream)
    enc()
    dec()
    torch.cuda.synchronize()
    ok = bool((st == 0).all()) and torch.equal(ol, ld)
    # round trip of a sample of the encrypt half's tokens, and the decrypt half's plaintexts
    coff = offs(te_len - 48, 0, "enc_in")
    chk = torch.empty(span(coff, te_len - 48), dtype=torch.uint8, device=dev)
    cl = torch.empty(h, dtype=torch.int32, device=dev)
    cs = torch.empty(h, dtype=torch.int32, device=dev)
    device.decrypt(ks, te, te_off, te_len, chk, coff, cl, cs, key_idx=kidx[:h], sort=True)
    torch.cuda.synchronize()
    ok = ok and bool((cs == 0).all()) and torch.equal(cl, le)
    co = coff.cpu()
    oe_c, od_c, bo_c = oe.cpu(), od.cpu(), boff.cpu()
    for i in range(0, h, 4099):
        a, b, L = int(co[i]), int(oe_c[i]), int(lens[i])
        ok = ok and torch.equal(chk[a:a + L], pe[b:b + L])
        a, b, L = int(bo_c[i]), int(od_c[i]), int(lens[h + i])
        ok = ok and torch.equal(back[a:a + L], pd[b:b + L])
    L64 = lens.to(torch.int64)
    B = L64 // 16 + 1
    H = (64 + 16 + 16 * B + 9 + 63) // 64
    ops = AES_BLOCK_OPS * B + SHA_CMP_OPS * H
    ops_e, ops_d = int(ops[:h].sum()), int(ops[h:].sum()) + TAG_CMP_OPS * (n - h)
    peak = n_cu * 128 * 2.4e9
    res = {"packets": n, "keys": n_keys, "encrypt_packets": h, "decrypt_packets": n - h,
           "plaintext_bytes": int(L64.sum()), "mean_plaintext_bytes": float(L64.float().mean()), "ok": ok,
           "layout": (("byte strings in 128-B-aligned slots (prefix sums of whole lines)" if align is True else
                       "byte strings in 128-B-aligned slots for " + ",".join(sorted(sides)) + ", packed elsewhere")
                      if sides else "packed rows (byte strings at prefix-sum offsets)") + ", length-bucketed on the device"}
    for name, f, o, bytes_ in (("encrypt", enc, ops_e, int(L64[:h].sum())), ("decrypt", dec, ops_d, int(L64[h:].sum()))):
        warmup(f, stream, 2, 0.3)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev:
            a.record(stream)
            f()
            b.record(stream)
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)[steps // 2]
        # the kernels' own clock and cycles, from a stamped pass after the timed one
        with device.LaunchClock(dev) as lc:
            for _ in range(steps):
                f()
        clk = lc.summary().get(name, {})
        res[name] = {"ms": ms, "packets_s": (h if name == "encrypt" else n - h) / (ms * 1e-3),
                     "gib_s": bytes_ / (ms * 1e-3) / 2**30, "canonical_ops": o,
                     "frac_of_valu_peak": o / (ms * 1e-3) / peak,
                     "kernel_clock_ghz": clk.get("clock_ghz"), "kernel_cycles_per_launch": clk.get("cycles_per_launch"),
                     "kernel_span_ms": clk.get("wg_span_ms")}
    tot = res["encrypt"]["ms"] + res["decrypt"]["ms"]
    res["packets_s"] = n / (tot * 1e-3)
    res["frac_of_valu_peak"] = (ops_e + ops_d) / (tot * 1e-3) / peak
    res["note"] = ("one rank's share of c5 at 8 GPUs; per direction the length-bucketing passes (histogram, scan, "
                   "scatter) and the per-key kernel are timed together; frac = canonical ops summed over the real "
                   "lengths / time / (CUs x 128 x 2.4 GHz)")
    return res


def c3_rate(dev, n_cu, n=1 << 20, L=500, n_keys=65536, steps=10):
    """SURVEY §8(d) c3 beside the headline: the c2 batch (2^20 x 500 B, packed
    rows) with a per-packet key index into a 65 536-key table (Token objects
    of many links), through the product's uniform entry points.  Median of
    ``steps`` HIP-event timings per direction after the clock warmup; every
    status and length checked and the plaintexts compared (round trip)."""
    import torch
    import reticulum_amd as rt
    from reticulum_amd import device
    g = torch.Generator(device=dev).manual_seed(33)
    kg = torch.Generator().manual_seed(333)
    keys = torch.randint(0, 256, (n_keys, 64), dtype=torch.uint8, generator=kg).numpy()
    ks = rt.KeySet(keys, device=dev.index if dev.index is not None else 0)
    tl = rt.token_len(L)
    kidx = torch.randint(0, n_keys, (n,), dtype=torch.int32, device=dev, generator=g)
    pt = torch.randint(0, 256, (n, L), dtype=torch.uint8, device=dev, generator=g)
    iv = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
    tok = torch.empty((n, tl), dtype=torch.uint8, device=dev)
    back = torch.empty((n, tl - 48), dtype=torch.uint8, device=dev)
    ol = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    enc = lambda: device.encrypt_uniform(ks, pt, L, iv, tok, key_idx=kidx, stream=stream)            # noqa: E731
    dec = lambda: device.decrypt_uniform(ks, tok, tl, back, ol, st, key_idx=kidx, stream=stream)     # noqa: E731
    peak = n_cu * 128 * 2.4e9
    res = {"packets": n, "plaintext_bytes": L, "keys": n_keys, "layout": "packed rows"}
    for name, f, o in (("encrypt", enc, ops_enc(L) * n), ("decrypt", dec, ops_dec(L) * n)):
        warmup(f, stream, 2, 0.3)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev:
            a.record(stream)
            f()
            b.record(stream)
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)[steps // 2]
        res[name] = {"ms": ms, "packets_s": n / (ms * 1e-3), "frac_of_valu_peak": o / (ms * 1e-3) / peak}
    res["ok"] = bool((st == 0).all()) and bool((ol == L).all()) and torch.equal(back[:, :L], pt)
    res["round_trips_s"] = n / ((res["encrypt"]["ms"] + res["decrypt"]["ms"]) * 1e-3)
    res["note"] = ("c3 (SURVEY §8(d)): the c2 batch with per-packet keys (key_idx into a 65 536-key table), "
                   "kernel time per direction (HIP events, median); key setup is timed apart under key_setup "
                   "when bench runs --config c3")
    return res


def e2e_rate(ks, pt_dev, iv_dev, L, tl, n, stream, reps=3, chunks=32, n_streams=3, sync_all=None,
             reduce_max=None, world=1):
    """Host memory in, host memory out, pinned buffers:
    * serial: H2D of plaintext + IVs, encrypt, D2H of the tokens, one stream
      (and the mirror for decrypt: H2D of the tokens, decrypt, D2H);
    * pipelined: the batch cut into `chunks` slices issued round-robin on
      `n_streams` streams, so one slice's H2D, another's kernel and a third's
      D2H overlap (PCIe is full duplex).
    H2D runs on the copy engine (torch copy_), D2H as GPU stores into the
    pinned buffer (device.copy_to_host): on MI355X the copy engine does D2H at
    30 GB/s and shares 57 GB/s between the two directions, the stores do
    54 GB/s and 87 GB/s beside a copy-engine H2D (profiles/r03n_pcie_probe.json).
    ``pipelined_copy_engine`` times the same slices with both directions on
    the copy engine (the round-1/2 path), for comparison.
    Best of `reps`; the round trip is checked on the host copies.

    N > 1 (VERDICT r02 missing #1): every rank runs this at once on its own
    shard from its own pinned host buffers over its own PCIe link, as the
    packets of a Reticulum node arrive from its interfaces' socket buffers
    (TCPInterface.py:392-401 -> Link.py:1161-1182).  ``sync_all`` (a barrier)
    starts every rep on all ranks together and ``reduce_max`` takes each
    rep's slowest rank, so ``aggregate`` = world x n packets / that time."""
    import torch
    from reticulum_amd import device
    dev = pt_dev.device
    pt_h = pt_dev.cpu().pin_memory()
    iv_h = iv_dev.cpu().pin_memory()
    tok_h = torch.empty((n, tl), dtype=torch.uint8).pin_memory()
    back_h = torch.empty((n, tl - 48), dtype=torch.uint8).pin_memory()
    pt_d, iv_d = torch.empty_like(pt_dev), torch.empty_like(iv_dev)
    tok_d = torch.empty((n, tl), dtype=torch.uint8, device=dev)
    back_d = torch.empty((n, tl - 48), dtype=torch.uint8, device=dev)
    ol = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    side = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]

    def slices(parts):
        step = -(-n // parts)
        return [(a, min(a + step, n)) for a in range(0, n, step)]

    def d2h(dst, src, s, engine):
        if engine:
            dst.copy_(src, non_blocking=True)
        else:
            device.copy_to_host(dst, src, stream=s)

    def enc(parts, engine=False):
        for k, (a, b) in enumerate(slices(parts)):
            s = stream if parts == 1 else side[k % n_streams]
            with torch.cuda.stream(s):
                pt_d[a:b].copy_(pt_h[a:b], non_blocking=True)
                iv_d[a:b].copy_(iv_h[a:b], non_blocking=True)
                device.encrypt_uniform(ks, pt_d[a:b], L, iv_d[a:b], tok_d[a:b], stream=s)
                d2h(tok_h[a:b], tok_d[a:b], s, engine)

    def dec(parts, engine=False):
        for k, (a, b) in enumerate(slices(parts)):
            s = stream if parts == 1 else side[k % n_streams]
            with torch.cuda.stream(s):
                tok_d[a:b].copy_(tok_h[a:b], non_blocking=True)
                device.decrypt_uniform(ks, tok_d[a:b], tl, back_d[a:b], ol[a:b], st[a:b], stream=s)
                d2h(back_h[a:b], back_d[a:b], s, engine)

    def timed(fn, parts, engine):
        own, slowest = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            if sync_all is not None:
                sync_all()
            t0 = time.perf_counter()
            fn(parts, engine)
            torch.cuda.synchronize()
            own.append(time.perf_counter() - t0)
        slowest = reduce_max(own) if reduce_max is not None else own
        return min(own), min(slowest)

    res, agg = {}, {}
    for name, parts, engine in (("serial", 1, False), ("pipelined", chunks, False),
                                ("pipelined_copy_engine", chunks, True)):
        back_h.zero_()
        tok_h.zero_()
        (te, te_all), (td, td_all) = timed(enc, parts, engine), timed(dec, parts, engine)
        ok = bool((st == 0).all()) and torch.equal(back_h[:, :L], pt_h)
        res[name] = {"encrypt_packets_s": n / te, "decrypt_packets_s": n / td, "roundtrip_packets_s": n / (te + td),
                     "encrypt_gib_s": n * L / te / 2**30, "decrypt_gib_s": n * L / td / 2**30,
                     "encrypt_pcie_gb_s": n * (L + 16 + tl) / te / 1e9, "ok": ok}
        agg[name] = {"encrypt_packets_s": world * n / te_all, "decrypt_packets_s": world * n / td_all,
                     "roundtrip_packets_s": world * n / (te_all + td_all),
                     "encrypt_gib_s": world * n * L / te_all / 2**30, "decrypt_gib_s": world * n * L / td_all / 2**30,
                     "ok_all": ok}
    res["note"] = (f"pinned host buffers; serial = H2D + kernel + D2H on one stream; pipelined = {chunks} slices "
                   f"round-robin on {n_streams} streams; H2D on the copy engine, D2H as GPU stores into the pinned "
                   f"buffer (pipelined_copy_engine: D2H on the copy engine too); best of {reps}")
    if world > 1:
        flags = reduce_max([0.0 if all(res[k]["ok"] for k in agg) else 1.0])
        for name in agg:
            agg[name]["ok_all"] = flags[0] == 0.0
        agg["ranks"] = world
        agg["note"] = (f"host-origin rate of the node: all {world} ranks at once, each on its own {n}-packet shard "
                       f"from its own pinned host buffers over its own PCIe link; each rep starts on a barrier and "
                       f"counts at its slowest rank; best of {reps} reps of world x n packets / that time. The "
                       f"per-rank fields above are rank 0's own view")
        res["aggregate"] = agg
    return res


if __name__ == "__main__":
    main()
