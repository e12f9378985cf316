// dproof_host.h — the host's planning for settling the proofs of packets sent
// to SINGLE destinations (dproof_kernels.hip): how the stage's work lists are
// laid out for a call of n records against a receipt table of `cap` slots and
// `max_receipts` ids, the grids, and the arithmetic of the scan budget (which
// stray proofs get their frame of pairs, which are deferred).  Plain C++ with
// no HIP in it, for the kernels and the host alike, so that tests/dproof_host/
// can build it alone under the sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define DP_FN inline __attribute__((always_inline))
#endif

namespace rnstok {

constexpr uint32_t DP_THREADS = 256;
constexpr uint32_t DP_NONE = 0xFFFFFFFFu;
constexpr uint32_t DP_HASH = 32, DP_SIGNATURE = 64;
constexpr uint32_t DP_IMPLICIT = DP_SIGNATURE;             // PacketReceipt.IMPL_LENGTH
constexpr uint32_t DP_EXPLICIT = DP_HASH + DP_SIGNATURE;   // PacketReceipt.EXPL_LENGTH
constexpr uint32_t DP_MAX_RECORDS = (1u << 30) - 2u;       // a slot word's index field, as LINK_MAX_BATCH
constexpr uint32_t DP_MAX_TRIALS = (1u << 30) - 2u;
// the head of the work lists, in words: the pass-one candidates, the live keyed
// receipts (L) and the strays, each counted on the device
constexpr uint32_t DP_W_CAND = 0, DP_W_LIVE = 1, DP_W_STRAYS = 2, DP_W_HEAD = 16;

DP_FN uint32_t dproof_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + DP_THREADS - 1) / DP_THREADS); }
DP_FN uint64_t dp_round4(uint64_t words) { return (words + 3) & ~3ull; }

// Where the lists of a call lie, as word offsets from the start of the work
// memory (every one a multiple of four words: 16-byte aligned), and the whole
// size in bytes.
struct DproofLayout {
    uint64_t part, start;          // blocks + 1 each: strays per workgroup of records, then where their ranks start
    uint64_t cand;                 // n: the records pass one verifies
    uint64_t slot;                 // n: the slot of the receipt a record is judged against, DP_NONE for none
    uint64_t rid;                  // n: the receipt id a stray's scan validated, DP_NONE for none
    uint64_t stray;                // n: 1 for a stray
    uint64_t slist;                // n: the strays by rank
    uint64_t live;                 // cap: the ids of the live keyed receipts
    uint64_t slot_of;              // max_receipts: a live keyed receipt's slot by id
    uint64_t bytes;
};

DP_FN DproofLayout dproof_layout(uint32_t n, uint32_t cap, uint32_t max_receipts) {
    DproofLayout l;
    const uint64_t N = n, nb = dproof_blocks(n);
    uint64_t at = DP_W_HEAD;
    const auto take = [&at](uint64_t words) {
        const uint64_t o = at;
        at += dp_round4(words);
        return o;
    };
    l.part = take(nb + 1);
    l.start = take(nb + 1);
    l.cand = take(N);
    l.slot = take(N);
    l.rid = take(N);
    l.stray = take(N);
    l.slist = take(N);
    l.live = take(cap);
    l.slot_of = take(max_receipts);
    l.bytes = 4 * at;
    return l;
}

// The bytes a call of n records needs; a call of fewer fits (the layout grows with n).
DP_FN uint64_t dproof_workspace_bytes(uint32_t n, uint32_t cap, uint32_t max_receipts) {
    return dproof_layout(n, cap, max_receipts).bytes;
}

// The scan budget.  A stray proof is tried against every live keyed receipt: a
// frame of L pairs.  The strays are ranked in record order, and the stray of
// rank r gets its frame when the frames up to and including its own fit
// scan_trials; only whole frames go in, so every stray behind the first that
// does not fit is deferred too.  With L = 0 there is nothing to try: no stray
// fits, and none is deferred either (dproof_deferred).
DP_FN bool dproof_fits(uint32_t rank, uint32_t L, uint32_t scan_trials) {
    return L != 0 && ((uint64_t)rank + 1) * L <= scan_trials;
}
DP_FN bool dproof_deferred(uint32_t rank, uint32_t L, uint32_t scan_trials) {
    return L != 0 && !dproof_fits(rank, L, scan_trials);
}
// How many of `strays` get a frame, and the pairs pass two runs (at most scan_trials).
DP_FN uint32_t dproof_frames(uint32_t strays, uint32_t L, uint32_t scan_trials) {
    if (L == 0) return 0;
    const uint32_t room = scan_trials / L;
    return strays < room ? strays : room;
}
DP_FN uint64_t dproof_pairs(uint32_t strays, uint32_t L, uint32_t scan_trials) {
    return (uint64_t)dproof_frames(strays, L, scan_trials) * L;
}

// The grid of pass two, from the bound alone.
DP_FN uint32_t dproof_scan_blocks(uint32_t scan_trials) { return dproof_blocks(scan_trials); }

}  // namespace rnstok
