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
// Layout.  The slot word is the link table's
// (table_device.h).  A packet hash is a SHA-256, so its own bytes pick the
// slot: bytes 0..3 (little endian) the home slot, bytes 4..7 the tag, and all
// 32 bytes are compared before a hit counts.  Slot s of a generation owns
// hashes[s] (32 B).  HashListState.sel says which generation is the current
// one; every kernel reads it, and the cull flips it on the device, so no call
// ever brings a count back to the host.
//
// Determinism.  A batch is filtered as if its packets came one after another
// in index order.  Equal hashes imply equal type bits, destination hash and
// context, so all copies of a hash take the same branch of the rules (but for
// the transport id rule, which is decided before the list is touched).
// k_filter_claim decides everything that does not depend on the other packets
// of the batch; a packet that is to be remembered and is not yet in the
// current generation claims the first free slot of its chain with a PENDING
// word that carries its batch index, or lowers the index of the PENDING slot
// its own hash already has (compared through the batch's records) with a
// 64-bit atomic minimum.  k_filter_settle: the packet whose index a slot still
// carries is the first of its hash; it passes, and enters the hash while the
// generation has room.  k_filter_finish: the other copies are duplicates where
// the hash was entered (a SINGLE announce, or a packet the list is not
// consulted for, passes all the same).  Which free slot a hash lands in may
// differ from run to run; statuses and later lookups do not.
//
// A generation holds at most `max` entries.  A packet that would be remembered
// in a full generation passes and adds one to the overflow count.  When the
// new hashes of one batch outnumber the room left, the number entered is the
// room, and which of them are entered is not specified.
#include "table_device.h"
#include "../../include/rnstok.h"

namespace rnstok {

namespace {

constexpr uint32_t REC_BYTES = 96, REC_HASH = 52;      // rt_packet_fields, its packet_hash
// status[i] between the kernels: PROVISIONAL | DUP_IF_ENTERED? | slot
constexpr uint32_t DUP_IF_ENTERED = 1u << 30;
constexpr uint32_t SLOT_BITS = DUP_IF_ENTERED - 1u;
constexpr uint32_t PKT_ANNOUNCE = 1u, PKT_PROOF = 3u, DEST_SINGLE = 0u, DEST_GROUP = 1u, DEST_PLAIN = 2u;
constexpr uint32_t HEADER_2 = 1u, CTX_KEEPALIVE = 0xFAu, CTX_LRPROOF = 0xFFu;

struct H32 {
    u32x4 lo, hi;
};
__device__ __forceinline__ H32 ld32(const uint8_t *p) { return H32{ld16(p), ld16(p + 16)}; }
__device__ __forceinline__ void st32(uint8_t *p, const H32 &h) {
    st16(p, h.lo);
    st16(p + 16, h.hi);
}
__device__ __forceinline__ bool same32(const H32 &a, const H32 &b) { return same(a.lo, b.lo) && same(a.hi, b.hi); }

struct Gen {
    uint64_t *slots;
    uint8_t *hashes;
};
__device__ __forceinline__ Gen gen_of(const HashList &l, uint32_t g) {
    return g ? Gen{l.slots[1], l.hashes[1]} : Gen{l.slots[0], l.hashes[0]};
}

// Whether a settled entry with this hash is in the generation.  Plain loads:
// for a generation no kernel beside this one writes.
__device__ __forceinline__ uint32_t find(const Gen &g, uint32_t cap, const H32 &h) {
    const uint32_t mask = cap - 1u;
    for (uint32_t p = 0; p < cap; ++p) {
        const uint32_t s = (h.lo.x + p) & mask;
        const uint64_t w = g.slots[s];
        if (w == W_EMPTY) return cap;
        if (w_state(w) == ST_FULL && w_tag(w) == h.lo.y && same32(ld32(g.hashes + 32ull * s), h)) return s;
    }
    return cap;
}

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
        if (remember && a.transit.slots) remember = find(a.transit, u32x4{r[9], r[10], r[11], r[12]}) == a.transit.cap;
        dup_passes = ptype == PKT_ANNOUNCE && dtype == DEST_SINGLE;
        dup_status = ptype == PKT_ANNOUNCE ? RT_FILTER_BAD_ANNOUNCE : RT_FILTER_DUPLICATE;
        base = a.fields;
    }
    if (!consult && !remember) {
        a.status[i] = RT_FILTER_PASS;
        return;
    }
    const H32 h = ld32(hash_of<FILTER>(base, i));
    const uint32_t cur = a.l.st->sel, cap = a.l.cap, mask = cap - 1u;
    const Gen g = gen_of(a.l, cur);
    // what a copy found present gets
    const int32_t seen = consult && !dup_passes ? dup_status : RT_FILTER_PASS;
    if (seen != RT_FILTER_PASS && find(gen_of(a.l, cur ^ 1u), cap, h) != cap) {
        // the previous generation has it: dropped, and not moved to the current one
        a.status[i] = seen;
        a.fields[(uint64_t)REC_BYTES * i] = 0;
        return;
    }
    // the count does not move while this kernel runs (k_filter_settle adds to it)
    const bool claim = remember && a.l.st->count[cur] < a.l.max;
    const uint32_t prov = PROVISIONAL | (seen != RT_FILTER_PASS ? DUP_IF_ENTERED : 0u);
    const uint64_t mine = word(h.lo.y, ST_PENDING, i);
    int32_t out = RT_FILTER_PASS;
    bool done = false;
    // Every failed compare-and-swap means another item took a slot for good,
    // so the generation has no free slot after at most cap of them.
    for (uint32_t attempt = 0; attempt <= cap && !done; ++attempt) {
        uint32_t free_s = cap;
        uint64_t free_w = 0;
        for (uint32_t p = 0; p < cap; ++p) {
            const uint32_t s = (h.lo.x + p) & mask;
            const uint64_t w = slot_load(g.slots + s);
            const uint32_t st = w_state(w);
            if (w == W_EMPTY || st == ST_TOMB) {
                if (free_s == cap) {
                    free_s = s;
                    free_w = w;
                }
                if (w == W_EMPTY) break;
                continue;
            }
            if (w_tag(w) != h.lo.y) continue;
            if (st == ST_FULL) {
                if (same32(ld32(g.hashes + 32ull * s), h)) {               // present: nothing to enter
                    out = seen;
                    done = true;
                    break;
                }
            } else if (claim && same32(ld32(hash_of<FILTER>(base, w_idx(w))), h)) {     // PENDING: a copy in this batch
                slot_min(g.slots + s, mine);
                out = (int32_t)(prov | s);
                done = true;
                break;
            }
        }
        if (done || !claim || free_s == cap) break;
        if (slot_cas(g.slots + free_s, free_w, mine)) {
            out = (int32_t)(prov | free_s);
            done = true;
        }
    }
    // absent and no slot taken: it passes; if it was to be remembered, the
    // generation is full (or its chain has no free slot)
    if (!done && remember) add_one(&a.l.st->overflow);
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
    const Gen g = gen_of(a.l, cur);
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
    const uint64_t m = __ballot(won);
    if (!m) return;
    const uint32_t lane = (uint32_t)__lane_id(), first = (uint32_t)__builtin_ctzll(m), k = (uint32_t)__popcll(m);
    uint32_t before = 0;
    if (lane == first)
        before = __hip_atomic_fetch_add(&a.l.st->count[cur], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    before = __shfl(before, (int)first);
    const uint32_t room = before < a.l.max ? a.l.max - before : 0u;
    if (lane == first && k > room) {
        __hip_atomic_fetch_sub(&a.l.st->count[cur], k - room, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&a.l.st->overflow, k - room, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!won) return;
    if ((uint32_t)__popcll(m & ((1ull << lane) - 1ull)) < room) {
        st32(g.hashes + 32ull * s, ld32(hash_of<FILTER>(base, i)));
        slot_store(g.slots + s, word(w_tag(w), ST_FULL, IDX_MASK));
    } else {
        slot_store(g.slots + s, W_TOMB);         // other chains of this batch may run through the slot
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
    const Gen g = gen_of(a.l, a.l.st->sel);
    int32_t out = RT_FILTER_PASS;
    if (w_state(g.slots[v & SLOT_BITS]) != ST_FULL) {
        add_one(&a.l.st->overflow);              // the first copy found no room, nor does this one
    } else if (FILTER && (v & DUP_IF_ENTERED)) {
        const uint32_t ptype = a.fields[(uint64_t)REC_BYTES * i + 7];
        out = ptype == PKT_ANNOUNCE ? RT_FILTER_BAD_ANNOUNCE : RT_FILTER_DUPLICATE;
        a.fields[(uint64_t)REC_BYTES * i] = 0;
    }
    a.status[i] = out;
}

// Remove, as the link table's: the items that find their hash in the current
// generation meet in its slot's index, and the lowest index reports it.
__global__ __launch_bounds__(TABLE_THREADS) void k_hash_unclaim(HashList l, const uint8_t *hashes, int32_t *status,
                                                                uint32_t n) {
    const uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x;
    if (i >= n) return;
    const H32 h = ld32(hashes + 32ull * i);
    const Gen g = gen_of(l, l.st->sel);
    const uint32_t mask = l.cap - 1u;
    int32_t st = RT_LINK_MISSING;
    for (uint32_t p = 0; p < l.cap; ++p) {
        const uint32_t s = (h.lo.x + p) & mask;
        const uint64_t w = slot_load(g.slots + s);
        if (w == W_EMPTY) break;
        if (w_state(w) == ST_FULL && w_tag(w) == h.lo.y && same32(ld32(g.hashes + 32ull * s), h)) {
            slot_min(g.slots + s, word(h.lo.y, ST_FULL, i));
            st = (int32_t)(PROVISIONAL | s);
            break;
        }
    }
    status[i] = st;
}
__global__ __launch_bounds__(TABLE_THREADS) void k_hash_unsettle(HashList l, int32_t *status, uint32_t n) {
    const uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x;
    const uint32_t cur = l.st->sel;
    const Gen g = gen_of(l, cur);
    bool won = false;
    if (i < n && ((uint32_t)status[i] & PROVISIONAL)) {
        const uint32_t s = (uint32_t)status[i] & ~PROVISIONAL;
        const uint64_t w = slot_load(g.slots + s);
        won = w_state(w) == ST_FULL && w_idx(w) == i;
        if (won) slot_store(g.slots + s, W_TOMB);
        status[i] = won ? RT_LINK_OK : RT_LINK_MISSING;
    }
    count_live(&l.st->count[cur], won, 0xFFFFFFFFu);         // minus one each
}

__global__ __launch_bounds__(TABLE_THREADS) void k_hash_contains(HashList l, const uint8_t *hashes, uint8_t *found_out,
                                                                 uint32_t n) {
    const uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x;
    if (i >= n) return;
    const H32 h = ld32(hashes + 32ull * i);
    const uint32_t cur = l.st->sel;
    found_out[i] = find(gen_of(l, cur), l.cap, h) != l.cap ? 1u : find(gen_of(l, cur ^ 1u), l.cap, h) != l.cap ? 2u : 0u;
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
    gen_of(l, l.st->sel).slots[s] = W_EMPTY;
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

hipError_t launch_hashlist_add(const HashList &l, const uint8_t *hashes, int32_t *scratch, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return launch_enter<false>(FilterArgs{l, LinkTab{}, nullptr, nullptr, scratch, n}, hashes, s);
}

hipError_t launch_hashlist_remove(const HashList &l, const uint8_t *hashes, int32_t *status, uint32_t n,
                                  hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hash_unclaim, table_grid(n), dim3(TABLE_THREADS), 0, s, l, hashes, status, n);
    hipLaunchKernelGGL(k_hash_unsettle, table_grid(n), dim3(TABLE_THREADS), 0, s, l, status, n);
    return hipGetLastError();
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
