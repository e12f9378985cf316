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
// The table is one of table_device.h's (layout, probe, claim and remove, and
// why a batch's outcome does not depend on its lanes' order):
// the key is the 16-byte link id, and slot s owns ids[s] and values[s].  Its
// own rules.  Insert: an id present before the batch is RT_LINK_DUPLICATE, a
// chain without a free slot RT_LINK_FULL (k_link_claim); of the items of one id
// the lowest index writes the entry, the others are duplicates (k_link_settle).
// Remove is the shared kernel pair.  The rebuild gathers the live entries,
// zeroes the slot words and puts the entries back.
#include "table_device.h"

namespace rnstok {

namespace {

constexpr uint32_t LINK_THREADS = TABLE_THREADS;

__global__ __launch_bounds__(LINK_THREADS) void k_link_lookup(LinkTab t, const uint8_t *ids, uint32_t *values_out,
                                                              uint8_t *found_out, uint32_t n) {
    const uint32_t i = blockIdx.x * LINK_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = find(view_of(t), ld16(ids + 16ull * i));
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
    const auto batch_id = [ids](uint32_t j) { return ld16(ids + 16ull * j); };
    const Claim c = claim(view_of(t), batch_id(i), i, true, batch_id);
    status[i] = c.kind == CLAIM_PRESENT ? RT_LINK_DUPLICATE
                : c.kind == CLAIM_MET   ? (int32_t)(PROVISIONAL | c.slot)
                                        : RT_LINK_FULL;
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

// Rebuild in place, three steps on the stream: the live entries go to a
// temporary in any order (their ids are distinct), the slot words are zeroed
// (hipMemsetAsync), and the entries are put back from an empty table.
__global__ __launch_bounds__(LINK_THREADS) void k_link_gather(LinkTab t, uint8_t *tmp_ids, uint32_t *tmp_values,
                                                              uint32_t *count) {
    const uint32_t s = blockIdx.x * LINK_THREADS + threadIdx.x;
    const bool full = s < t.cap && w_state(t.slots[s]) == ST_FULL;
    const uint32_t at = wave_reserve(count, full);
    if (full) {
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
        const uint32_t s = find(view_of(a.t), u32x4{r[9], r[10], r[11], r[12]});
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
    return launch_table_remove<u32x4>(t, ids, status, n, s);
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
