// destination_host.h — the host's planning for destination delivery
// (destination_kernels.hip): how the stage's workspace is laid out for a call
// of n frames with a retry budget of R pairs, the grids, and the arithmetic of
// the retry budget (which second-pass frames get their pairs, which are
// deferred).  Plain C++ with no HIP in it, for the kernels and the host alike,
// so that tests/destination_host/ can build it alone under the sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/rnstok.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DD_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define DD_FN inline __attribute__((always_inline))
#endif

namespace rnstok {

constexpr uint32_t DD_THREADS = 256;
constexpr uint32_t DD_NONE = 0xFFFFFFFFu;
constexpr uint32_t DD_EPHEMERAL = 32;          // Identity.KEYSIZE//8//2: the ephemeral X25519 key before the token
constexpr uint32_t DD_PROOF_HEADER = 19;       // flags, hops, packet hash[:16], context
constexpr uint32_t DD_PROOF_IMPLICIT = 83;     // header ‖ signature (64)
constexpr uint32_t DD_PROOF_EXPLICIT = 115;    // header ‖ packet hash (32) ‖ signature (64)
constexpr uint32_t DD_MAX_FRAMES = (1u << 30) - 2u;
// the head of the workspace, in words
constexpr uint32_t DD_W_SELECTED = 0, DD_W_PAIRS2 = 1, DD_W_PROOFS = 2, DD_W_HEAD = 16;

DD_FN uint32_t deliver_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + DD_THREADS - 1) / DD_THREADS); }
DD_FN uint64_t dd_round4(uint64_t words) { return (words + 3) & ~3ull; }

// Where the arrays of a call lie, as word offsets from the start of the
// workspace (every one a multiple of four words: 16-byte aligned), and the
// whole size in bytes.  n frames, R = retry_trials; the pairs of the first pass
// are 0..n-1 and those of the second n..n+R-1.
struct DeliverLayout {
    uint64_t part, part2;          // blocks + 1 each: per-workgroup counts, then where they start
    uint64_t drow;                 // n: the destination's row
    uint64_t ncand;                // n: candidates of a selected frame
    uint64_t rank;                 // n + 2: pair_off of the first pass (a last token takes the unused pairs)
    uint64_t start;                // n + 2: pair_off of the second pass
    uint64_t rem;                  // n: candidates left after the first pass, 0 for a decided frame
    uint64_t first1, first2;       // n + 1 each: rt_verify_trials' answers
    uint64_t tlen1, tlen2;         // n + 1 each: token lengths of the two passes (0: not tried)
    uint64_t toff;                 // n + 1 uint64: where each token starts
    uint64_t dkey, dlen, dst, dpl; // n each: the decrypt's key, length, status and plaintext length
    uint64_t plist;                // n: the frames to prove
    uint64_t pfrm, pcand, krow;    // n + R each: a pair's frame, candidate and key record
    uint64_t salt;                 // (n + R) x 16 bytes
    uint64_t shared;               // (n + R) x 32 bytes
    uint64_t bytes;
};

DD_FN DeliverLayout deliver_layout(uint32_t n, uint32_t retry) {
    DeliverLayout l;
    const uint64_t N = n, P = (uint64_t)n + retry, nb = deliver_blocks(n);
    uint64_t at = DD_W_HEAD;
    const auto take = [&at](uint64_t words) {
        const uint64_t o = at;
        at += dd_round4(words);
        return o;
    };
    l.part = take(nb + 1);
    l.part2 = take(nb + 1);
    l.drow = take(N);
    l.ncand = take(N);
    l.rank = take(N + 2);
    l.start = take(N + 2);
    l.rem = take(N);
    l.first1 = take(N + 1);
    l.first2 = take(N + 1);
    l.tlen1 = take(N + 1);
    l.tlen2 = take(N + 1);
    l.toff = take(2 * (N + 1));
    l.dkey = take(N);
    l.dlen = take(N);
    l.dst = take(N);
    l.dpl = take(N);
    l.plist = take(N);
    l.pfrm = take(P);
    l.pcand = take(P);
    l.krow = take(P);
    l.salt = take(4 * P);
    l.shared = take(8 * P);
    l.bytes = 4 * at;
    return l;
}

// The bytes an object built for max_frames and retry_trials holds: every call
// of n <= max_frames frames fits (the layout grows with n).
DD_FN uint64_t deliver_workspace_bytes(uint32_t max_frames, uint32_t retry) {
    return deliver_layout(max_frames, retry).bytes;
}

// Sums that stop at the top of a word: a budget is compared with them, never
// an address made of them.
DD_FN uint32_t dd_sat_add(uint32_t a, uint32_t b) {
    const uint64_t s = (uint64_t)a + b;
    return s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
}

// What a frame that is still undecided after the first pass asks of the
// budget: its remaining candidates, cut at retry + 1 (more than the budget is
// more than the budget).
DD_FN uint32_t deliver_ask(uint32_t remaining, uint32_t retry) {
    return remaining > retry ? dd_sat_add(retry, 1u) : remaining;
}

// Whether a frame whose pairs would start at `start` (the asks of the
// undecided frames before it in stream order, summed) gets its `ask` pairs:
// only whole frames go in.  A frame that does not fit leaves start + ask above
// the budget for every frame behind it, so those are deferred too.
DD_FN bool deliver_fits(uint32_t start, uint32_t ask, uint32_t retry) {
    return ask != 0 && (uint64_t)start + ask <= retry;
}

// pair_off of the second pass: inside the budget's rows whatever the sums.
DD_FN uint32_t deliver_pair_off(uint32_t start, uint32_t retry) { return start < retry ? start : retry; }

// The key record of pair p of the second pass, behind the max_frames records
// of the first.
DD_FN uint32_t deliver_retry_row(uint32_t max_frames, uint32_t p) { return max_frames + p; }

// The PROOF packet around its signature (Packet.py:170-228 for a
// ProofDestination, Identity.py:942-953): where the signature starts.
DD_FN uint32_t deliver_proof_bytes(bool implicit_proof) { return implicit_proof ? DD_PROOF_IMPLICIT : DD_PROOF_EXPLICIT; }

}  // namespace rnstok
