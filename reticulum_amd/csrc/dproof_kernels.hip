// dproof_kernels.hip — settling the proofs that come back for packets this node
// sent to SINGLE destinations, over the records rt_packet_unpack wrote
// (Transport.py:2326-2363 with packet.link unset; PacketReceipt.validate_proof,
// Packet.py:480-524).  DESIGN.md §4.3j.
//
// A receipt is held as in proof_kernels.hip, a link table over hash[:16] whose
// value is the receipt's id beside the full hashes by id, and in addition the
// Ed25519 key of the identity the packet went to (keys, 32 bytes by id) and a
// byte that says whether there is one (keyed; a receipt on a link has none and
// no proof of this kind delivers it).  An explicit proof, hash ‖ signature, is
// tried against the receipt with that hash; an implicit one, the signature
// alone, against every outstanding receipt.  An honest implicit proof is
// addressed to hash[:16] of the packet it proves (ProofDestination,
// Packet.py:376-381), so the receipt at that address is tried first and the
// whole table only where that fails: a stray.
//   k_dproof_select   one lane per record: the rules that need no signature,
//       the lookup (data[:16], or the destination hash), the 32-byte compare of
//       an explicit proof; compacts the candidates of pass one.
//   k_dproof_verify   one lane per candidate: the receipt's stored hash under
//       its key.  A lane that verifies lowers the index field of the receipt's
//       slot word to its record index (full_lower); an explicit proof that
//       fails is BAD_SIGNATURE, an implicit one a stray.
//   k_dproof_list     one lane per table slot lists the live keyed receipts
//       (their count L stays on the device); one lane per record counts the
//       strays of its workgroup.
//   k_dproof_offsets  one workgroup: where each workgroup's strays start.
//   k_dproof_rank     ranks the strays in record order; rank r gets a frame of
//       L pairs when (r + 1) L <= scan_trials, the others are DEFERRED.
//   k_dproof_scan     one lane per pair (stray p / L, receipt p mod L), the grid
//       sized for scan_trials; lowers slot words as pass one does.
//   k_dproof_close    one lane per record, reads slot words only: the lowest
//       index that verified a receipt is DELIVERED, the others find it gone.
//   k_dproof_remove   the winners leave the mark of a removal.
// Only the two verify kernels and the remove kernel write slot words.  The
// lists' order depends on the scheduling; results are scattered by record
// index, so nothing the caller sees depends on it.
#include "table_device.h"
#include "ed25519_device.h"
#include "dproof_host.h"

namespace rnstok {

namespace {

constexpr uint32_t DP_PKT_PROOF = 3u, DP_DEST_LINK = 3u;
constexpr uint32_t DP_CTX_RESOURCE_PRF = 0x05u, DP_CTX_LRPROOF = 0xFFu;

__device__ __forceinline__ uint32_t dp_le32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

struct Lists {
    uint32_t *part, *start, *cand, *slot, *rid, *stray, *slist, *live, *slot_of;
};
__device__ __forceinline__ Lists lists_of(const DproofArgs &a) {
    const DproofLayout l = dproof_layout(a.n, a.t.cap, a.max_receipts);
    return Lists{a.work + l.part, a.work + l.start, a.work + l.cand,  a.work + l.slot,   a.work + l.rid,
                 a.work + l.stray, a.work + l.slist, a.work + l.live, a.work + l.slot_of};
}

// The keyed receipt at this 16-byte address: its slot (v.cap for none) and id.
__device__ __forceinline__ uint32_t receipt_at(const DproofArgs &a, const uint8_t *h, uint32_t &id) {
    const uint32_t s = find(view_of(a.t), u32x4{dp_le32(h), dp_le32(h + 4), dp_le32(h + 8), dp_le32(h + 12)});
    if (s == a.t.cap) return s;
    id = a.t.values[s];
    return id < a.max_receipts ? s : a.t.cap;
}

__global__ void __launch_bounds__(DP_THREADS) k_dproof_select(const DproofArgs a) {
    const uint32_t i = blockIdx.x * DP_THREADS + threadIdx.x;
    const Lists w = lists_of(a);
    bool cand = false;
    if (i < a.n) {
        const rt_packet_fields &f = ((const rt_packet_fields *)a.fields)[i];
        int32_t st = RT_DPROOF_NOT_PROOF, rec = -1;
        uint32_t slot = DP_NONE, stray = 0;
        if (f.ok == 1 && f.packet_type == DP_PKT_PROOF && f.context != DP_CTX_LRPROOF &&
            f.context != DP_CTX_RESOURCE_PRF) {
            if (f.destination_type == DP_DEST_LINK && a.link && (uint32_t)a.link[i] < a.n_links)
                st = RT_DPROOF_ON_LINK;
            else if (f.data_len != DP_EXPLICIT && f.data_len != DP_IMPLICIT)
                st = RT_DPROOF_BAD_LENGTH;
            else {
                st = RT_DPROOF_NO_RECEIPT;
                uint32_t id = 0;
                if (f.data_len == DP_EXPLICIT) {
                    const uint8_t *h = a.pkt + a.pkt_off[i] + f.data_offset;
                    const uint32_t s = receipt_at(a, h, id);
                    if (s != a.t.cap) {
                        const uint8_t *want = a.hashes + (uint64_t)DP_HASH * id;
                        uint32_t diff = 0;
                        for (uint32_t k = 16; k < DP_HASH; ++k) diff |= (uint32_t)(h[k] ^ want[k]);
                        if (!diff && a.keyed[id]) {
                            slot = s;
                            cand = true;
                        }
                    }
                } else {
                    const uint32_t s = receipt_at(a, f.destination_hash, id);
                    if (s != a.t.cap && a.keyed[id]) {
                        slot = s;
                        cand = true;
                    } else {
                        stray = 1;
                    }
                }
                if (cand) {
                    // the verdict should the signature hold and no lower index take the receipt
                    st = RT_DPROOF_DELIVERED;
                    rec = (int32_t)id;
                }
            }
        }
        a.status[i] = st;
        a.receipt[i] = rec;
        w.slot[i] = slot;
        w.rid[i] = DP_NONE;
        w.stray[i] = stray;
    }
    const uint32_t at = wave_reserve(a.work + DP_W_CAND, cand);
    if (cand) w.cand[at] = i;
}

// What both passes do with a (record, receipt) pair: the proof's signature over
// the receipt's stored hash under the receipt's key.  On success the slot's
// index field is lowered to the record index.
__device__ __forceinline__ bool verify_pair(const DproofArgs &a, uint32_t i, uint32_t id, uint32_t slot) {
    const rt_packet_fields &f = ((const rt_packet_fields *)a.fields)[i];
    const uint8_t *sig = a.pkt + a.pkt_off[i] + f.data_offset + (f.data_len == DP_EXPLICIT ? DP_HASH : 0u);
    const uint8_t *hash = a.hashes + (uint64_t)DP_HASH * id;
    uint32_t pk[8], r[8], s[8];
    load_words(pk, a.keys + (uint64_t)32 * id);
    load_words(r, sig);
    load_words(s, sig + 32);
    if (!ed25519_verify_words(pk, r, s, hash, DP_HASH)) return false;
    full_lower(a.t.slots + slot, dp_le32(hash + 4), i);
    return true;
}

// One wave per SIMD with the overflow in AGPRs, as k_settle_verify has
__global__ void __launch_bounds__(DP_THREADS) k_dproof_verify(const DproofArgs a) {
    const uint32_t count = a.work[DP_W_CAND];                   // at most n: one add per candidate
    const uint32_t first = blockIdx.x * DP_THREADS;
    if (first >= count) return;
    const uint32_t j = first + threadIdx.x;
    if (j >= count) return;
    const Lists w = lists_of(a);
    const uint32_t i = w.cand[j];
    if (verify_pair(a, i, (uint32_t)a.receipt[i], w.slot[i])) return;
    const rt_packet_fields &f = ((const rt_packet_fields *)a.fields)[i];
    a.receipt[i] = -1;
    if (f.data_len == DP_EXPLICIT) {
        a.status[i] = RT_DPROOF_BAD_SIGNATURE;                  // the slot stays: close looks for a winner below
    } else {
        a.status[i] = RT_DPROOF_NO_RECEIPT;
        w.slot[i] = DP_NONE;
        w.stray[i] = 1;
    }
}

// The grid covers the records and the table's slots, whichever are more.
__global__ void __launch_bounds__(DP_THREADS) k_dproof_list(const DproofArgs a) {
    const uint32_t g = blockIdx.x * DP_THREADS + threadIdx.x;
    const Lists w = lists_of(a);
    const uint32_t strays = (uint32_t)__syncthreads_count(g < a.n && w.stray[g] != 0);
    if (threadIdx.x == 0 && blockIdx.x < dproof_blocks(a.n)) w.part[blockIdx.x] = strays;
    bool live = false;
    uint32_t id = 0;
    if (g < a.t.cap) {
        const uint64_t word = a.t.slots[g];
        if (w_state(word) == ST_FULL) {
            id = a.t.values[g];
            live = id < a.max_receipts && a.keyed[id] != 0;
        }
    }
    const uint32_t at = wave_reserve(a.work + DP_W_LIVE, live);  // at most cap: one add per slot
    if (live) {
        w.live[at] = id;
        w.slot_of[id] = g;
    }
}

// One workgroup: start[b] = the strays of the workgroups before b, and their total.
__global__ void __launch_bounds__(DP_THREADS) k_dproof_offsets(const DproofArgs a) {
    __shared__ uint32_t sh[DP_THREADS];
    const Lists w = lists_of(a);
    const uint32_t nb = dproof_blocks(a.n), t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += DP_THREADS) {
        const uint32_t b = base + t, mine = b < nb ? w.part[b] : 0u;
        sh[t] = mine;
        __syncthreads();
        for (uint32_t d = 1; d < DP_THREADS; d <<= 1) {
            const uint32_t add = t >= d ? sh[t - d] : 0u;
            __syncthreads();
            sh[t] += add;
            __syncthreads();
        }
        if (b < nb) w.start[b] = carry + sh[t] - mine;
        carry += sh[DP_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) a.work[DP_W_STRAYS] = carry;
}

__global__ void __launch_bounds__(DP_THREADS) k_dproof_rank(const DproofArgs a) {
    __shared__ uint32_t waves[DP_THREADS / 64];
    const uint32_t i = blockIdx.x * DP_THREADS + threadIdx.x;
    const Lists w = lists_of(a);
    const bool stray = i < a.n && w.stray[i] != 0;
    const uint64_t m = __ballot(stray);
    const uint32_t lane = (uint32_t)__lane_id(), wave = threadIdx.x / 64;
    if (lane == 0) waves[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!stray) return;
    uint32_t rank = w.start[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t k = 0; k < wave; ++k) rank += waves[k];
    const uint32_t L = a.work[DP_W_LIVE];
    if (dproof_fits(rank, L, a.scan_trials))
        w.slist[rank] = i;
    else if (dproof_deferred(rank, L, a.scan_trials))
        a.status[i] = RT_DPROOF_DEFERRED;
}

__global__ void __launch_bounds__(DP_THREADS) k_dproof_scan(const DproofArgs a) {
    const uint32_t L = a.work[DP_W_LIVE];
    const uint64_t pairs = dproof_pairs(a.work[DP_W_STRAYS], L, a.scan_trials);       // at most scan_trials
    const uint64_t first = (uint64_t)blockIdx.x * DP_THREADS;
    if (first >= pairs) return;
    const uint64_t p = first + threadIdx.x;
    if (p >= pairs) return;
    const Lists w = lists_of(a);
    const uint32_t i = w.slist[(uint32_t)(p / L)], id = w.live[(uint32_t)(p % L)];
    if (verify_pair(a, i, id, w.slot_of[id]))
        __hip_atomic_fetch_min(w.rid + i, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot words are only read here: every record judged against a receipt
// sees the same winner, the all-ones index where no signature held.
__global__ void __launch_bounds__(DP_THREADS) k_dproof_close(const DproofArgs a) {
    const uint32_t i = blockIdx.x * DP_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const Lists w = lists_of(a);
    const int32_t st = a.status[i];
    if (st == RT_DPROOF_DELIVERED || st == RT_DPROOF_BAD_SIGNATURE) {
        // a proof that verified and is not the first to: the receipt is gone; so
        // it is for a bad signature that comes after the proof that was delivered
        const uint32_t winner = w_idx(slot_load(a.t.slots + w.slot[i]));
        if (st == RT_DPROOF_DELIVERED ? winner != i : winner < i) {
            a.status[i] = RT_DPROOF_NO_RECEIPT;
            a.receipt[i] = -1;
            w.slot[i] = DP_NONE;
        }
    } else if (st == RT_DPROOF_NO_RECEIPT && w.stray[i] != 0 && w.rid[i] != DP_NONE) {
        // a stray whose scan validated a receipt: delivered when no lower index took it
        const uint32_t id = w.rid[i], slot = w.slot_of[id];
        if (w_idx(slot_load(a.t.slots + slot)) == i) {
            a.status[i] = RT_DPROOF_DELIVERED;
            a.receipt[i] = (int32_t)id;
            w.slot[i] = slot;
        }
    }
}

__global__ void __launch_bounds__(DP_THREADS) k_dproof_remove(const DproofArgs a) {
    const uint32_t i = blockIdx.x * DP_THREADS + threadIdx.x;
    const Lists w = lists_of(a);
    const bool won = i < a.n && a.status[i] == RT_DPROOF_DELIVERED;
    if (won) tombstone(a.t.slots + w.slot[i]);
    count_live(a.t.live, won, 0xFFFFFFFFu);                     // minus one each
}

// rt_receipt_store_keyed: hash, key and keyed of every receipt the insert entered
__global__ void __launch_bounds__(DP_THREADS) k_receipt_store_keyed(uint8_t *store, uint8_t *key_store, uint8_t *keyed,
                                                                    uint32_t max_receipts, const uint8_t *hashes,
                                                                    const uint8_t *keys, const uint32_t *ids,
                                                                    const int32_t *status, uint32_t n) {
    const uint32_t i = blockIdx.x * DP_THREADS + threadIdx.x;
    if (i >= n || status[i] != RT_LINK_OK || ids[i] >= max_receipts) return;
    const uint64_t to = 32ull * ids[i], from = 32ull * i;
    st16(store + to, ld16(hashes + from));
    st16(store + to + 16, ld16(hashes + from + 16));
    if (keys) {
        st16(key_store + to, ld16(keys + from));
        st16(key_store + to + 16, ld16(keys + from + 16));
    }
    keyed[ids[i]] = keys ? 1 : 0;
}

dim3 dp_grid(uint32_t n) { return dim3(dproof_blocks(n)); }

}  // namespace

hipError_t launch_dproof_settle(const DproofArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    // the three counts start at 0 in every call
    hipError_t e = hipMemsetAsync(a.work, 0, 4 * DP_W_HEAD, s);
    if (e != hipSuccess) return e;
    const dim3 block(DP_THREADS), records = dp_grid(a.n);
    hipLaunchKernelGGL(k_dproof_select, records, block, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_dproof_verify, records, block, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_dproof_list, dp_grid(a.n > a.t.cap ? a.n : a.t.cap), block, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_dproof_offsets, dim3(1), block, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_dproof_rank, records, block, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.scan_trials) {
        hipLaunchKernelGGL(k_dproof_scan, dim3(dproof_scan_blocks(a.scan_trials)), block, 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_dproof_close, records, block, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_dproof_remove, records, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_receipt_store_keyed(uint8_t *store, uint8_t *key_store, uint8_t *keyed, uint32_t max_receipts,
                                      const uint8_t *hashes, const uint8_t *keys, const uint32_t *ids,
                                      const int32_t *status, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_receipt_store_keyed, dp_grid(n), dim3(DP_THREADS), 0, s, store, key_store, keyed,
                       max_receipts, hashes, keys, ids, status, n);
    return hipGetLastError();
}

}  // namespace rnstok
