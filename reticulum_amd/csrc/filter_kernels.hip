// filter_kernels.hip — the packet hash list and Transport's packet filter.
//
// Transport.inbound drops a packet it has seen before: packet_filter
// (Transport.py:1377-1427) looks the packet's hash up in packet_hashlist and
// packet_hashlist_prev, and a packet that passes is remembered in the first
// (Transport.py:1525-1545); the job loop moves the first set to the second
// when it has grown past half of hashlist_maxsize (Transport.py:656-658).  Here
// the two sets are two generations of an open-addressing table in device
// memory and the rules are a few compares, one lane per unpacked packet.
//
// Each generation is one of table_device.h's tables (layout, probe, claim and
// remove are there): the key is the 32-byte packet hash, and
// slot s of a generation owns hashes[s].  HashListState.sel says which
// generation is the current one; every kernel reads it, and the cull flips it
// on the device, so no call ever brings a count back to the host.
//
// Its own rules.  A batch is filtered as if its packets came one after another
// in index order.  Equal hashes imply equal type bits, destination hash and
// context, so all copies of a hash take the same branch of the rules (but for
// the transport id rule, which is decided before the list is touched).
// k_filter_claim decides everything that does not depend on the other packets
// of the batch; a packet that is to be remembered and is not yet in the
// current generation meets the other copies of its hash in one slot (claim(),
// the batch's keys being the hashes in its records).  k_filter_settle: the
// packet whose index a slot still carries is the first of its hash; it passes,
// and enters the hash while the generation has room.  k_filter_finish: the
// other copies are duplicates where the hash was entered (a SINGLE announce,
// or a packet the list is not consulted for, passes all the same).
//
// A generation holds at most `max` entries.  A packet that would be remembered
// in a full generation passes and adds one to the overflow count.  When the
// new hashes of one batch outnumber the room left, the number entered is the
// room, and which of them are entered is not specified.
#include "table_device.h"

namespace rnstok {

namespace {

constexpr uint32_t REC_BYTES = 96, REC_HASH = 52;      // rt_packet_fields, its packet_hash
// status[i] between the kernels: PROVISIONAL | DUP_IF_ENTERED? | slot
constexpr uint32_t DUP_IF_ENTERED = 1u << 30;
constexpr uint32_t SLOT_BITS = DUP_IF_ENTERED - 1u;
constexpr uint32_t PKT_ANNOUNCE = 1u, PKT_PROOF = 3u, DEST_SINGLE = 0u, DEST_GROUP = 1u, DEST_PLAIN = 2u;
constexpr uint32_t HEADER_2 = 1u, CTX_KEEPALIVE = 0xFAu, CTX_LRPROOF = 0xFFu;

// KEEPALIVE, RESOURCE_REQ, RESOURCE_PRF, RESOURCE, CACHE_REQUEST, CHANNEL
// (Transport.py:1388-1393): contexts 0x01, 0x03, 0x05, 0x08, 0x0E and 0xFA.
__device__ __forceinline__ bool context_passes(uint32_t c) {
    return c < 16u ? (0x412Au >> c) & 1u : c == CTX_KEEPALIVE;
}

template <bool FILTER>
__device__ __forceinline__ const uint8_t *hash_of(const uint8_t *base, uint32_t i) {
    return FILTER ? base + (uint64_t)REC_BYTES * i + REC_HASH : base + 32ull * i;
}
__device__ __forceinline__ void add_one(uint32_t *p) {
    __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// First kernel.  FILTER: the rules over a.fields; status[i] leaves final, or
// PROVISIONAL | slot for a packet that waits for k_filter_settle.  Without
// FILTER (rt_hashlist_add): every item of `base` (32 B each) is to be entered.
template <bool FILTER>
__global__ __launch_bounds__(TABLE_THREADS) void k_filter_claim(FilterArgs a, const uint8_t *base) {
    const uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x;
    if (i >= a.n) return;
    if (!FILTER && a.mask && !a.mask[i]) {       // a masked add: the item is left out
        a.status[i] = RT_FILTER_PASS;
        return;
    }
    bool consult = false, remember = true, dup_passes = false;
    int32_t dup_status = RT_FILTER_DUPLICATE;
    if (FILTER) {
        const uint32_t *r = (const uint32_t *)(a.fields + (uint64_t)REC_BYTES * i);
        const uint32_t w0 = r[0], w1 = r[1], ctx = r[2] & 0xFFu;
        if ((w0 & 0xFFu) != 1u) {
            a.status[i] = RT_FILTER_NO_PACKET;
            return;
        }
        const uint32_t hops = ((w0 >> 16) & 0xFFu) + 1u, header = w0 >> 24;        // Transport.py:1496
        const uint32_t dtype = (w1 >> 16) & 0xFFu, ptype = w1 >> 24;
        int32_t drop = RT_FILTER_PASS;
        if (header == HEADER_2 && ptype != PKT_ANNOUNCE &&
            !same(u32x4{r[5], r[6], r[7], r[8]}, ld16(a.identity))) {
            drop = RT_FILTER_OTHER_TRANSPORT;
        } else if (context_passes(ctx)) {
        } else if (dtype == DEST_PLAIN || dtype == DEST_GROUP) {
            if (ptype == PKT_ANNOUNCE) drop = RT_FILTER_BAD_ANNOUNCE;
            else if (hops > 1u) drop = RT_FILTER_HOPS;
        } else {
            consult = true;
        }
        if (drop != RT_FILTER_PASS) {
            a.status[i] = drop;
            a.fields[(uint64_t)REC_BYTES * i] = 0;
            return;
        }
        // Transport.py:1537, 1542
        remember = !(ptype == PKT_PROOF && ctx == CTX_LRPROOF);
        if (remember && a.transit.slots)
            remember = find(view_of(a.transit), u32x4{r[9], r[10], r[11], r[12]}) == a.transit.cap;
        dup_passes = ptype == PKT_ANNOUNCE && dtype == DEST_SINGLE;
        dup_status = ptype == PKT_ANNOUNCE ? RT_FILTER_BAD_ANNOUNCE : RT_FILTER_DUPLICATE;
        base = a.fields;
    }
    if (!consult && !remember) {
        a.status[i] = RT_FILTER_PASS;
        return;
    }
    const auto batch_hash = [base](uint32_t j) { return ld32(hash_of<FILTER>(base, j)); };
    const H32 h = batch_hash(i);
    const uint32_t cur = a.l.st->sel;
    // what a copy found present gets
    const int32_t seen = consult && !dup_passes ? dup_status : RT_FILTER_PASS;
    if (seen != RT_FILTER_PASS && find(view_of(a.l, cur ^ 1u), h) != a.l.cap) {
        // the previous generation has it: dropped, and not moved to the current one
        a.status[i] = seen;
        a.fields[(uint64_t)REC_BYTES * i] = 0;
        return;
    }
    // the count does not move while this kernel runs (k_filter_settle adds to it)
    const bool may_claim = remember && a.l.st->count[cur] < a.l.max;
    const uint32_t prov = PROVISIONAL | (seen != RT_FILTER_PASS ? DUP_IF_ENTERED : 0u);
    const Claim c = claim(view_of(a.l, cur), h, i, may_claim, batch_hash);
    // present: nothing to enter.  Absent and no slot taken: it passes; if it
    // was to be remembered, the generation is full (or its chain has no free slot)
    const int32_t out = c.kind == CLAIM_PRESENT ? seen
                        : c.kind == CLAIM_MET   ? (int32_t)(prov | c.slot)
                                                : RT_FILTER_PASS;
    if (c.kind == CLAIM_NONE && remember) add_one(&a.l.st->overflow);
    a.status[i] = out;
    if (FILTER && out > 0) a.fields[(uint64_t)REC_BYTES * i] = 0;
}

// Second kernel: the lowest batch index that met in a slot is the first of
// its hash.  It passes, and enters the hash while the generation has room.
template <bool FILTER>
__global__ __launch_bounds__(TABLE_THREADS) void k_filter_settle(FilterArgs a, const uint8_t *base) {
    const uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x;
    if (FILTER) base = a.fields;
    const uint32_t cur = a.l.st->sel;
    const TabView g = view_of(a.l, cur);
    bool won = false;
    uint32_t s = 0;
    uint64_t w = 0;
    if (i < a.n && ((uint32_t)a.status[i] & PROVISIONAL)) {
        s = (uint32_t)a.status[i] & SLOT_BITS;
        w = slot_load(g.slots + s);
        won = w_state(w) == ST_PENDING && w_idx(w) == i;
    }
    // room is handed out a wave at a time: one add to the count, and one back
    // for the lanes that came too late
    const uint32_t at = wave_reserve(&a.l.st->count[cur], won);
    const bool late = won && at >= a.l.max;
    count_live(&a.l.st->count[cur], late, 0xFFFFFFFFu);
    count_live(&a.l.st->overflow, late, 1u);
    if (!won) return;
    if (!late) {
        st32(g.keys + 32ull * s, ld32(hash_of<FILTER>(base, i)));
        slot_store(g.slots + s, word(w_tag(w), ST_FULL, IDX_MASK));
    } else {
        tombstone(g.slots + s);                  // other chains of this batch may run through the slot
    }
    a.status[i] = RT_FILTER_PASS;
}

// Third kernel: the copies behind the first of their hash.
template <bool FILTER>
__global__ __launch_bounds__(TABLE_THREADS) void k_filter_finish(FilterArgs a) {
    const uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t v = (uint32_t)a.status[i];
    if (!(v & PROVISIONAL)) return;
    int32_t out = RT_FILTER_PASS;
    if (w_state(view_of(a.l).slots[v & SLOT_BITS]) != ST_FULL) {
        add_one(&a.l.st->overflow);              // the first copy found no room, nor does this one
    } else if (FILTER && (v & DUP_IF_ENTERED)) {
        const uint32_t ptype = a.fields[(uint64_t)REC_BYTES * i + 7];
        out = ptype == PKT_ANNOUNCE ? RT_FILTER_BAD_ANNOUNCE : RT_FILTER_DUPLICATE;
        a.fields[(uint64_t)REC_BYTES * i] = 0;
    }
    a.status[i] = out;
}

__global__ __launch_bounds__(TABLE_THREADS) void k_hash_contains(HashList l, const uint8_t *hashes, uint8_t *found_out,
                                                                 uint32_t n) {
    const uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x;
    if (i >= n) return;
    const H32 h = ld32(hashes + 32ull * i);
    const uint32_t cur = l.st->sel;
    found_out[i] = find(view_of(l, cur), h) != l.cap ? 1u : find(view_of(l, cur ^ 1u), h) != l.cap ? 2u : 0u;
}

// The cull (Transport.py:656-658), decided where the count is: the current
// generation becomes the previous one when it holds more than max / 2 entries,
// and the other one, emptied by k_hash_clear, the current.
__global__ void k_hash_cull(HashList l) {
    HashListState *st = l.st;
    const uint32_t cur = st->sel;
    const bool rotate = st->count[cur] > l.max / 2u;
    if (rotate) {
        st->sel = cur ^ 1u;
        st->count[cur ^ 1u] = 0;
    }
    st->rotate = rotate ? 1u : 0u;
}
__global__ __launch_bounds__(TABLE_THREADS) void k_hash_clear(HashList l) {
    const uint32_t s = blockIdx.x * TABLE_THREADS + threadIdx.x;
    if (s >= l.cap || !l.st->rotate) return;
    view_of(l).slots[s] = W_EMPTY;
}

__global__ void k_hash_counts(HashList l, uint32_t *out) {
    const uint32_t cur = l.st->sel;
    out[0] = l.st->count[cur];
    out[1] = l.st->count[cur ^ 1u];
    out[2] = l.st->overflow;
}

template <bool FILTER>
hipError_t launch_enter(const FilterArgs &a, const uint8_t *base, hipStream_t s) {
    const dim3 grid = table_grid(a.n), block(TABLE_THREADS);
    hipLaunchKernelGGL(k_filter_claim<FILTER>, grid, block, 0, s, a, base);
    hipLaunchKernelGGL(k_filter_settle<FILTER>, grid, block, 0, s, a, base);
    hipLaunchKernelGGL(k_filter_finish<FILTER>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_packet_filter(const FilterArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    return launch_enter<true>(a, nullptr, s);
}

hipError_t launch_hashlist_add(const HashList &l, const uint8_t *hashes, int32_t *scratch, uint32_t n, hipStream_t s,
                               const uint8_t *mask) {
    if (n == 0) return hipSuccess;
    return launch_enter<false>(FilterArgs{l, LinkTab{}, nullptr, nullptr, scratch, n, mask}, hashes, s);
}

// Remove, as the link table's, from the current generation.
hipError_t launch_hashlist_remove(const HashList &l, const uint8_t *hashes, int32_t *status, uint32_t n,
                                  hipStream_t s) {
    return launch_table_remove<H32>(l, hashes, status, n, s);
}

hipError_t launch_hashlist_contains(const HashList &l, const uint8_t *hashes, uint8_t *found_out, uint32_t n,
                                    hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hash_contains, table_grid(n), dim3(TABLE_THREADS), 0, s, l, hashes, found_out, n);
    return hipGetLastError();
}

hipError_t launch_hashlist_cull(const HashList &l, hipStream_t s) {
    hipLaunchKernelGGL(k_hash_cull, dim3(1), dim3(1), 0, s, l);
    hipLaunchKernelGGL(k_hash_clear, table_grid(l.cap), dim3(TABLE_THREADS), 0, s, l);
    return hipGetLastError();
}

hipError_t launch_hashlist_counts(const HashList &l, uint32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_hash_counts, dim3(1), dim3(1), 0, s, l, out);
    return hipGetLastError();
}

}  // namespace rnstok
