// table_device.h — the open-addressing tables in device memory: the link
// table (link_kernels.hip; also the packet filter's transit table and the
// receipt table of proof_kernels.hip) and the two generations of the packet
// hash list (filter_kernels.hip).  One slot word, one probe, one way to claim
// and to remove; a table is a key type and its own rules.  DESIGN.md §4.3c.
//
// Layout.  A key is a (truncated) SHA-256, so its own bytes are the hash:
// bytes 0..3 (little endian) pick the home slot, bytes 4..7 are the tag, and
// the whole key is compared before a match counts.  Slot s is one 64-bit word
// plus the entry it owns: keys[s], and what the table keeps beside it.
//
//   word = tag << 32 | state << 30 | index
//   state EMPTY (word 0)   never used: a probe stops here
//         TOMB             removed: a probe walks on, an insert may take it
//         FULL             entry present; index is all ones when settled
//         PENDING          claimed by an insert in flight; index = batch index
//
// A miss costs one 8-byte load per slot probed (an empty word, or a tag that
// differs); the key is fetched only behind a matching tag.
//
// Determinism.  Items of a batch run concurrently, but what they decide does
// not depend on their order.  Entering is two kernels.  First, claim(): an
// item whose key is already present (FULL) learns so; otherwise it claims the
// first free slot of its chain by compare-and-swap with a PENDING word that
// carries its batch index, and an item that meets a PENDING slot of its own
// key (compared through the batch's keys) lowers that word's index to its own
// with a 64-bit atomic minimum instead of claiming: all items of one key meet
// in one slot (a slot an item passed over was held by another key for good)
// and the lowest index stays.  Second, the caller's settle kernel: the item
// whose index the slot still carries owns it.  Remove works alike on the index
// field of the FULL word (unclaim(), unsettle()).  Which free slot a key lands
// in may differ from run to run; what is found does not.
//
// Slot words are read and written with agent-scope atomics inside the kernels
// that change them (the XCDs' L2s are not coherent for plain accesses within a
// kernel); the kernels that only look up use plain loads.
#pragma once
#include "token_device.h"
#include "token_launch.h"
#include "../../include/rnstok.h"

namespace rnstok {

constexpr uint32_t TABLE_THREADS = 256;
constexpr uint32_t ST_TOMB = 1u << 30, ST_FULL = 2u << 30, ST_PENDING = 3u << 30, ST_MASK = 3u << 30;
constexpr uint32_t IDX_MASK = ST_TOMB - 1u;
constexpr uint64_t W_EMPTY = 0, W_TOMB = ST_TOMB;
// status[i] between the two kernels of a call: this flag plus the item's slot
constexpr uint32_t PROVISIONAL = 0x80000000u;

__device__ __forceinline__ uint64_t word(uint32_t tag, uint32_t state, uint32_t idx) {
    return (uint64_t)tag << 32 | state | idx;
}
__device__ __forceinline__ uint32_t w_state(uint64_t w) { return (uint32_t)w & ST_MASK; }
__device__ __forceinline__ uint32_t w_idx(uint64_t w) { return (uint32_t)w & IDX_MASK; }
__device__ __forceinline__ uint32_t w_tag(uint64_t w) { return (uint32_t)(w >> 32); }
__device__ __forceinline__ uint64_t slot_load(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void slot_store(uint64_t *p, uint64_t w) {
    __hip_atomic_store(p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool slot_cas(uint64_t *p, uint64_t expect, uint64_t want) {
    return __hip_atomic_compare_exchange_strong(p, &expect, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void slot_min(uint64_t *p, uint64_t w) {
    __hip_atomic_fetch_min(p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The two keys: 16 bytes (a link id, a receipt's hash[:16]) and 32 (a packet hash).
struct H32 {
    u32x4 lo, hi;
};
__device__ __forceinline__ bool same(u32x4 a, u32x4 b) {
    return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0u;
}
__device__ __forceinline__ H32 ld32(const uint8_t *p) { return H32{ld16(p), ld16(p + 16)}; }
__device__ __forceinline__ void st32(uint8_t *p, const H32 &h) {
    st16(p, h.lo);
    st16(p + 16, h.hi);
}
__device__ __forceinline__ bool same32(const H32 &a, const H32 &b) { return same(a.lo, b.lo) && same(a.hi, b.hi); }

template <class K>
struct Key;
template <>
struct Key<u32x4> {
    static constexpr uint64_t BYTES = 16;
    static __device__ __forceinline__ u32x4 load(const uint8_t *p) { return ld16(p); }
    static __device__ __forceinline__ void store(uint8_t *p, u32x4 k) { st16(p, k); }
    static __device__ __forceinline__ bool equal(u32x4 a, u32x4 b) { return same(a, b); }
    static __device__ __forceinline__ uint32_t home(u32x4 k) { return k.x; }
    static __device__ __forceinline__ uint32_t tag(u32x4 k) { return k.y; }
};
template <>
struct Key<H32> {
    static constexpr uint64_t BYTES = 32;
    static __device__ __forceinline__ H32 load(const uint8_t *p) { return ld32(p); }
    static __device__ __forceinline__ void store(uint8_t *p, const H32 &k) { st32(p, k); }
    static __device__ __forceinline__ bool equal(const H32 &a, const H32 &b) { return same32(a, b); }
    static __device__ __forceinline__ uint32_t home(const H32 &k) { return k.lo.x; }
    static __device__ __forceinline__ uint32_t tag(const H32 &k) { return k.lo.y; }
};

// What the probes walk: cap slot words and the keys beside them.  live_of() is
// the word that counts the entries present.
struct TabView {
    uint64_t *slots;
    uint8_t *keys;
    uint32_t cap;
};
__device__ __forceinline__ TabView view_of(const LinkTab &t) { return TabView{t.slots, t.ids, t.cap}; }
__device__ __forceinline__ TabView view_of(const HashList &l, uint32_t g) {
    return g ? TabView{l.slots[1], l.hashes[1], l.cap} : TabView{l.slots[0], l.hashes[0], l.cap};
}
// a hash list's calls change its current generation
__device__ __forceinline__ TabView view_of(const HashList &l) { return view_of(l, l.st->sel); }
__device__ __forceinline__ uint32_t *live_of(const LinkTab &t) { return t.live; }
__device__ __forceinline__ uint32_t *live_of(const HashList &l) { return &l.st->count[l.st->sel]; }

// The lanes of the wave that say `mine` take `each` of *counter apiece with one
// add per wave; returns where a lane's share starts (for each == 1, its
// position: the value before the add plus its rank among those lanes).
__device__ __forceinline__ uint32_t wave_reserve(uint32_t *counter, bool mine, uint32_t each = 1u) {
    const uint64_t m = __ballot(mine);
    if (!m) return 0;
    const uint32_t lane = (uint32_t)__lane_id(), first = (uint32_t)__builtin_ctzll(m);
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    const uint32_t all = each * (uint32_t)__popcll(m);
    uint32_t base = 0;
    if (lane == first) base = __hip_atomic_fetch_add(counter, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (uint32_t)__builtin_amdgcn_readlane((int)base, (int)first) + each * rank;
}
// One add to a count per wave: `mine` lanes contribute `delta` each.
__device__ __forceinline__ void count_live(uint32_t *live, bool mine, uint32_t delta) {
    (void)wave_reserve(live, mine, delta);
}

// The slot of a settled entry with this key, or cap.  At most cap probes.
// Plain loads: for kernels that run with no writer of the table beside them;
// ATOMIC for those that change slot words.
template <bool ATOMIC = false, class K>
__device__ __forceinline__ uint32_t find(TabView v, const K &k) {
    const uint32_t mask = v.cap - 1u, home = Key<K>::home(k), tag = Key<K>::tag(k);
    for (uint32_t p = 0; p < v.cap; ++p) {
        const uint32_t s = (home + p) & mask;
        const uint64_t w = ATOMIC ? slot_load(v.slots + s) : v.slots[s];
        if (w == W_EMPTY) return v.cap;
        if (w_state(w) == ST_FULL && w_tag(w) == tag && Key<K>::equal(Key<K>::load(v.keys + Key<K>::BYTES * s), k))
            return s;
    }
    return v.cap;
}

// Entering, first kernel.  The key of batch item i is present already
// (PRESENT, at `slot`), or the item has met the others of its key in `slot`
// (MET: claimed, or found PENDING; the word's index is min(i, theirs) now), or
// nothing was taken (NONE: no free slot in the chain, or !may_claim).
// batch_key(j) loads the key of batch item j.
enum ClaimKind : uint32_t { CLAIM_NONE, CLAIM_PRESENT, CLAIM_MET };
struct Claim {
    ClaimKind kind;
    uint32_t slot;
};
template <class K, class BatchKey>
__device__ __forceinline__ Claim claim(TabView v, const K &k, uint32_t i, bool may_claim, BatchKey batch_key) {
    const uint32_t mask = v.cap - 1u, home = Key<K>::home(k), tag = Key<K>::tag(k);
    const uint64_t mine = word(tag, ST_PENDING, i);
    // Every failed compare-and-swap means another item took a slot for good,
    // so the table has no free slot after at most cap of them.
    for (uint32_t attempt = 0; attempt <= v.cap; ++attempt) {
        uint32_t free_s = v.cap;
        uint64_t free_w = 0;
        for (uint32_t p = 0; p < v.cap; ++p) {
            const uint32_t s = (home + p) & mask;
            const uint64_t w = slot_load(v.slots + s);
            const uint32_t st = w_state(w);
            if (w == W_EMPTY || st == ST_TOMB) {
                if (free_s == v.cap) {
                    free_s = s;
                    free_w = w;
                }
                if (w == W_EMPTY) break;
                continue;
            }
            if (w_tag(w) != tag) continue;
            if (st == ST_FULL) {
                if (Key<K>::equal(Key<K>::load(v.keys + Key<K>::BYTES * s), k)) return Claim{CLAIM_PRESENT, s};
            } else if (may_claim && Key<K>::equal(batch_key(w_idx(w)), k)) {      // PENDING: an item of this batch
                slot_min(v.slots + s, mine);
                return Claim{CLAIM_MET, s};
            }
        }
        if (!may_claim || free_s == v.cap) break;
        if (slot_cas(v.slots + free_s, free_w, mine)) return Claim{CLAIM_MET, free_s};
    }
    return Claim{CLAIM_NONE, v.cap};
}

// Remove, first step: the items that hold a FULL entry meet in its word's
// index field.  unclaim() finds the entry first (its slot, or cap).
__device__ __forceinline__ void full_lower(uint64_t *slot, uint32_t tag, uint32_t i) {
    slot_min(slot, word(tag, ST_FULL, i));
}
template <class K>
__device__ __forceinline__ uint32_t unclaim(TabView v, const K &k, uint32_t i) {
    const uint32_t s = find<true>(v, k);
    if (s != v.cap) full_lower(v.slots + s, Key<K>::tag(k), i);
    return s;
}
// Remove, second step: the lowest index leaves the mark of a removal.
__device__ __forceinline__ void tombstone(uint64_t *slot) { slot_store(slot, W_TOMB); }
__device__ __forceinline__ bool unsettle(uint64_t *slot, uint32_t i) {
    const uint64_t w = slot_load(slot);
    const bool won = w_state(w) == ST_FULL && w_idx(w) == i;
    if (won) tombstone(slot);
    return won;
}

inline dim3 table_grid(uint32_t n) { return dim3((n + TABLE_THREADS - 1) / TABLE_THREADS); }

// Remove of n keys (K each) from a table Tab (one view_of(Tab) gives): two
// kernels; status[i] leaves as RT_LINK_OK for the lowest index of a key that
// was present, RT_LINK_MISSING for every other item.
template <class Tab, class K>
__global__ __launch_bounds__(TABLE_THREADS) void k_table_unclaim(Tab t, const uint8_t *keys, int32_t *status,
                                                                 uint32_t n) {
    const uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x;
    if (i >= n) return;
    const TabView v = view_of(t);
    const uint32_t s = unclaim(v, Key<K>::load(keys + Key<K>::BYTES * i), i);
    status[i] = s != v.cap ? (int32_t)(PROVISIONAL | s) : RT_LINK_MISSING;
}
template <class Tab>
__global__ __launch_bounds__(TABLE_THREADS) void k_table_unsettle(Tab t, int32_t *status, uint32_t n) {
    const uint32_t i = blockIdx.x * TABLE_THREADS + threadIdx.x;
    bool won = false;
    if (i < n && ((uint32_t)status[i] & PROVISIONAL)) {
        won = unsettle(view_of(t).slots + ((uint32_t)status[i] & ~PROVISIONAL), i);
        status[i] = won ? RT_LINK_OK : RT_LINK_MISSING;
    }
    count_live(live_of(t), won, 0xFFFFFFFFu);        // minus one each
}
template <class K, class Tab>
hipError_t launch_table_remove(const Tab &t, const uint8_t *keys, int32_t *status, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL((k_table_unclaim<Tab, K>), table_grid(n), dim3(TABLE_THREADS), 0, s, t, keys, status, n);
    hipLaunchKernelGGL(k_table_unsettle<Tab>, table_grid(n), dim3(TABLE_THREADS), 0, s, t, status, n);
    return hipGetLastError();
}

}  // namespace rnstok
