// link_kernels.hip — the link table and the dispatch of inbound link packets.
//
// Transport.inbound finds the link of a DATA packet by walking active_links
// for the first link whose link_id equals the packet's destination hash
// (Transport.py:2161-2176), and Link.receive decides by packet type and
// context whether the packet is decrypted (Link.py:941-1148).  Here the walk
// is one probe of an open-addressing hash table in device memory and the
// decision a few compares, one lane per packet, fused with the token span
// (k_token_spans) so that the decrypt gets its span and its key index from one
// pass over the unpacked fields.
//
// Table layout.  A link id is a truncated SHA-256, so its
// own bytes are the hash: bytes 0..3 (little endian) pick the home slot, bytes
// 4..7 are the tag, and all 16 bytes are compared before a match counts.  Slot
// s is one 64-bit word plus the entry it owns, ids[s] (16 B) and values[s]:
//
//   word = tag << 32 | state << 30 | index
//   state EMPTY (word 0)   never used: a probe stops here
//         TOMB             removed: a probe walks on, an insert may take it
//         FULL             entry present; index is all ones when settled
//         PENDING          claimed by an insert in flight; index = batch index
//
// A miss costs one 8-byte load per slot probed (an empty word, or a tag that
// differs); the 16-byte id is fetched only behind a matching tag.
//
// Determinism.  Items of a batch run concurrently, but what they decide does
// not depend on their order.  Insert is two kernels.  k_link_claim: an item
// whose id is already present (FULL) is a duplicate; otherwise it claims the
// first free slot of its chain by compare-and-swap with a PENDING word that
// carries its batch index, and an item that meets a PENDING slot of its own id
// (compared through the batch's ids) lowers that word's index to its own with
// a 64-bit atomic minimum instead of claiming: all items of one id meet in one
// slot and the lowest index stays.  k_link_settle: the item whose index the
// slot still carries writes the entry and makes the slot FULL, the others are
// duplicates.  Remove works alike on the index field of the FULL word.  Which
// free slot an id lands in may differ from run to run; what is found does not.
//
// Slot words are read and written with agent-scope atomics inside the kernels
// that change them (the XCDs' L2s are not coherent for plain accesses within a
// kernel); the kernels that only look up use plain loads.  The word and its
// helpers are in table_device.h, shared with the packet hash list.
#include "table_device.h"
#include "../../include/rnstok.h"

namespace rnstok {

namespace {

constexpr uint32_t LINK_THREADS = TABLE_THREADS;

__global__ __launch_bounds__(LINK_THREADS) void k_link_lookup(LinkTab t, const uint8_t *ids, uint32_t *values_out,
                                                              uint8_t *found_out, uint32_t n) {
    const uint32_t i = blockIdx.x * LINK_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = find(t, ld16(ids + 16ull * i));
    const bool hit = s != t.cap;
    values_out[i] = hit ? t.values[s] : 0xFFFFFFFFu;
    found_out[i] = hit ? 1u : 0u;
}

// Insert, first kernel.  status[i] leaves as RT_LINK_DUPLICATE (present before
// the batch), RT_LINK_FULL, or PROVISIONAL | slot.
__global__ __launch_bounds__(LINK_THREADS) void k_link_claim(LinkTab t, const uint8_t *ids, int32_t *status,
                                                             uint32_t n) {
    const uint32_t i = blockIdx.x * LINK_THREADS + threadIdx.x;
    if (i >= n) return;
    const u32x4 id = ld16(ids + 16ull * i);
    const uint32_t mask = t.cap - 1u;
    const uint64_t mine = word(id.y, ST_PENDING, i);
    // Every failed compare-and-swap means another item took a slot for good,
    // so the table is full after at most cap of them.
    for (uint32_t attempt = 0; attempt <= t.cap; ++attempt) {
        uint32_t free_s = t.cap;
        uint64_t free_w = 0;
        for (uint32_t p = 0; p < t.cap; ++p) {
            const uint32_t s = (id.x + p) & mask;
            const uint64_t w = slot_load(t.slots + s);
            const uint32_t st = w_state(w);
            if (w == W_EMPTY || st == ST_TOMB) {
                if (free_s == t.cap) {
                    free_s = s;
                    free_w = w;
                }
                if (w == W_EMPTY) break;
                continue;
            }
            if (w_tag(w) != id.y) continue;
            if (st == ST_FULL) {
                if (same(ld16(t.ids + 16ull * s), id)) {
                    status[i] = RT_LINK_DUPLICATE;
                    return;
                }
            } else if (same(ld16(ids + 16ull * w_idx(w)), id)) {     // PENDING: an item of this batch
                slot_min(t.slots + s, mine);
                status[i] = (int32_t)(PROVISIONAL | s);
                return;
            }
        }
        if (free_s == t.cap) break;
        if (slot_cas(t.slots + free_s, free_w, mine)) {
            status[i] = (int32_t)(PROVISIONAL | free_s);
            return;
        }
    }
    status[i] = RT_LINK_FULL;
}

// Insert, second kernel: the lowest batch index that met in a slot owns it.
__global__ __launch_bounds__(LINK_THREADS) void k_link_settle(LinkTab t, const uint8_t *ids, const uint32_t *values,
                                                              int32_t *status, uint32_t n) {
    const uint32_t i = blockIdx.x * LINK_THREADS + threadIdx.x;
    bool won = false;
    if (i < n && ((uint32_t)status[i] & PROVISIONAL)) {
        const uint32_t s = (uint32_t)status[i] & ~PROVISIONAL;
        const uint64_t w = slot_load(t.slots + s);
        won = w_state(w) == ST_PENDING && w_idx(w) == i;
        if (won) {
            st16(t.ids + 16ull * s, ld16(ids + 16ull * i));
            t.values[s] = values[i];
            slot_store(t.slots + s, word(w_tag(w), ST_FULL, IDX_MASK));
        }
        status[i] = won ? RT_LINK_OK : RT_LINK_DUPLICATE;
    }
    count_live(t.live, won, 1u);
}

// Remove, first kernel: the items that find their id meet in its slot's index.
__global__ __launch_bounds__(LINK_THREADS) void k_link_unclaim(LinkTab t, const uint8_t *ids, int32_t *status,
                                                               uint32_t n) {
    const uint32_t i = blockIdx.x * LINK_THREADS + threadIdx.x;
    if (i >= n) return;
    const u32x4 id = ld16(ids + 16ull * i);
    const uint32_t mask = t.cap - 1u;
    int32_t st = RT_LINK_MISSING;
    for (uint32_t p = 0; p < t.cap; ++p) {
        const uint32_t s = (id.x + p) & mask;
        const uint64_t w = slot_load(t.slots + s);
        if (w == W_EMPTY) break;
        if (w_state(w) == ST_FULL && w_tag(w) == id.y && same(ld16(t.ids + 16ull * s), id)) {
            slot_min(t.slots + s, word(id.y, ST_FULL, i));
            st = (int32_t)(PROVISIONAL | s);
            break;
        }
    }
    status[i] = st;
}

// Remove, second kernel: the lowest index leaves the mark of a removal.
__global__ __launch_bounds__(LINK_THREADS) void k_link_unsettle(LinkTab t, int32_t *status, uint32_t n) {
    const uint32_t i = blockIdx.x * LINK_THREADS + threadIdx.x;
    bool won = false;
    if (i < n && ((uint32_t)status[i] & PROVISIONAL)) {
        const uint32_t s = (uint32_t)status[i] & ~PROVISIONAL;
        const uint64_t w = slot_load(t.slots + s);
        won = w_state(w) == ST_FULL && w_idx(w) == i;
        if (won) slot_store(t.slots + s, W_TOMB);
        status[i] = won ? RT_LINK_OK : RT_LINK_MISSING;
    }
    count_live(t.live, won, 0xFFFFFFFFu);        // minus one each
}

// Rebuild in place, three steps on the stream: the live entries go to a
// temporary in any order (their ids are distinct), the slot words are zeroed
// (hipMemsetAsync), and the entries are put back from an empty table.
__global__ __launch_bounds__(LINK_THREADS) void k_link_gather(LinkTab t, uint8_t *tmp_ids, uint32_t *tmp_values,
                                                              uint32_t *count) {
    const uint32_t s = blockIdx.x * LINK_THREADS + threadIdx.x;
    const bool full = s < t.cap && w_state(t.slots[s]) == ST_FULL;
    const uint64_t m = __ballot(full);
    if (!m) return;
    const uint32_t lane = (uint32_t)__lane_id(), first = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == first)
        base = __hip_atomic_fetch_add(count, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, (int)first);
    if (full) {
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        st16(tmp_ids + 16ull * at, ld16(t.ids + 16ull * s));
        tmp_values[at] = t.values[s];
    }
}
__global__ __launch_bounds__(LINK_THREADS) void k_link_refill(LinkTab t, const uint8_t *tmp_ids,
                                                              const uint32_t *tmp_values, const uint32_t *count,
                                                              uint64_t *report, uint32_t ticket) {
    const uint32_t i = blockIdx.x * LINK_THREADS + threadIdx.x;
    const uint32_t live = *count;
    if (i == 0) {
        *t.live = live;
        if (report) *report = (uint64_t)ticket << 32 | live;      // to the host, in mapped memory
    }
    if (i >= live) return;
    const u32x4 id = ld16(tmp_ids + 16ull * i);
    const uint32_t mask = t.cap - 1u;
    const uint64_t mine = word(id.y, ST_FULL, IDX_MASK);
    for (uint32_t p = 0; p < t.cap; ++p) {           // live <= cap entries: an empty slot is always met
        const uint32_t s = (id.x + p) & mask;
        if (slot_load(t.slots + s) == W_EMPTY && slot_cas(t.slots + s, W_EMPTY, mine)) {
            st16(t.ids + 16ull * s, id);
            t.values[s] = tmp_values[i];
            return;
        }
    }
}

// Link.receive's decision for a DATA packet: the contexts whose branch calls
// decrypt (Link.py:943-1145; LRRTT through rtt_packet :519, LINKCLOSE through
// teardown_packet :676).  NONE, RESOURCE_ADV, RESOURCE_REQ, RESOURCE_HMU,
// RESOURCE_ICL, RESOURCE_RCL, REQUEST, RESPONSE, CHANNEL are the bits of the
// mask; LINKIDENTIFY 0xFB, LINKCLOSE 0xFC, LRRTT 0xFE.
__device__ __forceinline__ bool context_decrypts(uint32_t c) {
    return c < 16u ? (0x46DDu >> c) & 1u : (c == 0xFBu || c == 0xFCu || c == 0xFEu);
}

constexpr uint32_t DEST_LINK = 3u, PKT_DATA = 0u, PKT_PROOF = 3u;

__global__ __launch_bounds__(LINK_THREADS) void k_link_spans(LinkSpanArgs a) {
    const uint32_t i = blockIdx.x * LINK_THREADS + threadIdx.x;
    if (i >= a.n) return;
    // ok, destination_type, packet_type, context: bytes 0, 6, 7, 8 of the record;
    // data_offset / data_len words 3 / 4; the destination hash words 9..12
    const uint32_t *r = (const uint32_t *)(a.fields + 96ull * i);
    const uint32_t w0 = r[0], w1 = r[1];
    const uint32_t dtype = (w1 >> 16) & 0xFFu, ptype = w1 >> 24;
    uint32_t route = RT_ROUTE_NOT_LINK, off = 0, len = 0, key = 0;
    int32_t link = -1;
    if ((w0 & 0xFFu) == 1u && dtype == DEST_LINK && (ptype == PKT_DATA || ptype == PKT_PROOF)) {
        const uint32_t s = find(a.t, u32x4{r[9], r[10], r[11], r[12]});
        route = RT_ROUTE_NO_LINK;
        if (s != a.t.cap) {
            const uint32_t v = a.t.values[s];
            link = (int32_t)v;
            route = RT_ROUTE_LINK_PLAIN;
            if (ptype == PKT_DATA && context_decrypts(r[2] & 0xFFu) && v < a.n_keys) {
                route = RT_ROUTE_LINK_DECRYPT;
                off = r[3];
                len = r[4];
                key = v;
            }
        }
    }
    a.tok_off[i] = a.pkt_off[i] + off;
    a.tok_len[i] = len;
    a.key_idx[i] = key;
    a.link[i] = link;
    a.route[i] = (uint8_t)route;
}

inline dim3 grid_for(uint32_t n) { return table_grid(n); }

}  // namespace

hipError_t launch_link_lookup(const LinkTab &t, const uint8_t *ids, uint32_t *values_out, uint8_t *found_out,
                              uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_link_lookup, grid_for(n), dim3(LINK_THREADS), 0, s, t, ids, values_out, found_out, n);
    return hipGetLastError();
}

hipError_t launch_link_insert(const LinkTab &t, const uint8_t *ids, const uint32_t *values, int32_t *status,
                              uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_link_claim, grid_for(n), dim3(LINK_THREADS), 0, s, t, ids, status, n);
    hipLaunchKernelGGL(k_link_settle, grid_for(n), dim3(LINK_THREADS), 0, s, t, ids, values, status, n);
    return hipGetLastError();
}

hipError_t launch_link_remove(const LinkTab &t, const uint8_t *ids, int32_t *status, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_link_unclaim, grid_for(n), dim3(LINK_THREADS), 0, s, t, ids, status, n);
    hipLaunchKernelGGL(k_link_unsettle, grid_for(n), dim3(LINK_THREADS), 0, s, t, status, n);
    return hipGetLastError();
}

uint64_t link_rebuild_workspace_bytes(uint32_t cap) { return 20ull * cap + 16; }

hipError_t launch_link_rebuild(const LinkTab &t, void *workspace, uint64_t *report, uint32_t ticket, hipStream_t s) {
    uint8_t *tmp_ids = (uint8_t *)workspace;
    uint32_t *tmp_values = (uint32_t *)(tmp_ids + 16ull * t.cap);
    uint32_t *count = tmp_values + t.cap;
    hipError_t e = hipMemsetAsync(count, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_link_gather, grid_for(t.cap), dim3(LINK_THREADS), 0, s, t, tmp_ids, tmp_values, count);
    if ((e = hipMemsetAsync(t.slots, 0, 8ull * t.cap, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_link_refill, grid_for(t.cap), dim3(LINK_THREADS), 0, s, t, tmp_ids, tmp_values, count, report,
                       ticket);
    return hipGetLastError();
}

hipError_t launch_link_spans(const LinkSpanArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_link_spans, grid_for(a.n), dim3(LINK_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace rnstok
