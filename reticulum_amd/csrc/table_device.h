// table_device.h — the slot word of the open-addressing tables in device
// memory (the link table, link_kernels.hip; the packet hash list,
// filter_kernels.hip) and what both do with it.  DESIGN.md §4.3c.
//
//   word = tag << 32 | state << 30 | index
//   state EMPTY (word 0)   never used: a probe stops here
//         TOMB             removed: a probe walks on, an insert may take it
//         FULL             entry present; index is all ones when settled
//         PENDING          claimed by an insert in flight; index = batch index
//
// Slot words are read and written with agent-scope atomics inside the kernels
// that change them (the XCDs' L2s are not coherent for plain accesses within a
// kernel); the kernels that only look up use plain loads.
#pragma once
#include "token_device.h"
#include "token_launch.h"

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
__device__ __forceinline__ bool same(u32x4 a, u32x4 b) {
    return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0u;
}
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
// One add to the live count per wave: `mine` lanes contribute `delta` each.
__device__ __forceinline__ void count_live(uint32_t *live, bool mine, uint32_t delta) {
    const uint64_t m = __ballot(mine);
    if (m && (uint32_t)__lane_id() == (uint32_t)__builtin_ctzll(m))
        __hip_atomic_fetch_add(live, delta * (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot of a settled entry with this id, or cap.  At most cap probes.
// Plain loads: for kernels that run with no writer of the table beside them.
__device__ __forceinline__ uint32_t find(const LinkTab &t, u32x4 id) {
    const uint32_t mask = t.cap - 1u;
    for (uint32_t p = 0; p < t.cap; ++p) {
        const uint32_t s = (id.x + p) & mask;
        const uint64_t w = t.slots[s];
        if (w == W_EMPTY) return t.cap;
        if (w_state(w) == ST_FULL && w_tag(w) == id.y && same(ld16(t.ids + 16ull * s), id)) return s;
    }
    return t.cap;
}

inline dim3 table_grid(uint32_t n) { return dim3((n + TABLE_THREADS - 1) / TABLE_THREADS); }

}  // namespace rnstok
