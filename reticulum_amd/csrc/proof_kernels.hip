// proof_kernels.hip — packet proofs on a link, both directions, over the
// records rt_packet_unpack wrote: the last step of Transport.inbound that costs
// one Ed25519 operation per packet.
//
// Proving (Link.receive, Link.py:943-955 and :1140-1145; Packet.prove;
// Link.prove_packet, Link.py:378-389).  A link whose destination proves all
// packets answers every DATA packet with context NONE that it could decrypt,
// and a link with a channel every CHANNEL packet (before the decrypt, so
// whatever the token's outcome), with  packet hash ‖ sign(packet hash)  sent
// unencrypted as a LINK PROOF packet (Packet.py:199-200):
//   flags 0x0F (HEADER_1, BROADCAST, LINK, PROOF) ‖ hops 0 ‖ link id (16) ‖
//   context 0x00 ‖ packet hash (32) ‖ signature (64)             115 bytes
//   k_prove_select  one lane per record: decides, writes proof_len (115 / 0)
//       and appends the candidates to a list, one ballot and one atomic add
//       per wave.
//   k_prove_sign    one lane per candidate, the grid sized for n; a block past
//       the count returns at once.  The message is the 32-byte hash in the
//       record, so both SHA-512 inputs are one block; R = [r]B comes from the
//       table of [2^i]B and A from the signers' rows (ifac_sign_words, the
//       signature of rt_ed25519_sign bit for bit, constant time in the seed).
//
// Settling (Transport.py:2326-2363; PacketReceipt.validate_link_proof,
// Packet.py:434-459).  A PROOF that is neither a link request proof nor a
// resource proof is matched by data[:32] against the outstanding receipts and
// verified under the key of the link it came on; on success the receipt is
// delivered and removed.  The receipts are a link table over hash[:16] whose
// value is the receipt's id, beside an array of the full hashes by id:
//   k_settle_select  one lane per record: the rules that need no signature,
//       the table lookup (plain loads, as find), the full 32-byte compare; the
//       candidates are compacted as above, each with its slot.
//   k_settle_verify  one lane per candidate: verifies hash and signature where
//       they lie in the packet (a 32-byte message).  A lane whose signature
//       holds lowers the index field of the receipt's slot word to its record
//       index (a 64-bit atomic minimum, table_device.h's full_lower): the lowest
//       index that verified stays, whatever copies with bad signatures lie
//       below it.
//   k_settle_close   one lane per candidate: the record whose index the slot
//       carries is delivered; the others that verified, and the bad signatures
//       behind it, find the receipt gone (NO_RECEIPT), as they would had the
//       packets come one after another.  Reads the slot words only, so every
//       candidate of a receipt sees the same winner.
//   k_settle_remove  the delivered records leave the mark of a removal.
// Only the verify and the remove kernel write slot words, with
// table_device.h's removal steps (full_lower, tombstone).
// The lists' order depends on the scheduling; results are scattered by record
// index, so nothing the caller sees depends on it.
#include "table_device.h"
#include "prove_device.h"

namespace rnstok {

namespace {

constexpr uint32_t PROOF_THREADS = 256;
constexpr uint32_t PKT_DATA = 0u, PKT_PROOF = 3u, DEST_LINK = 3u;
constexpr uint32_t CTX_NONE = 0x00u, CTX_RESOURCE_PRF = 0x05u, CTX_CHANNEL = 0x0Eu, CTX_LRPROOF = 0xFFu;
constexpr uint32_t HASH = 32, SIGNATURE = 64, PROOF_HEADER = 19;
constexpr uint32_t PROOF_BYTES = PROOF_HEADER + HASH + SIGNATURE;      // 115
constexpr uint32_t FLAG_PROVE_ALL = 1u, FLAG_HAS_CHANNEL = 2u;
// the workspace: the candidate count in word 0, the indices from word 16 (a
// line of its own for the counter); settling keeps the candidates' slots behind
constexpr uint32_t LIST_AT = 16;

// Appends the wave's candidates to the list: one ballot and one atomic add per
// wave (wave_reserve, table_device.h).
__device__ __forceinline__ void append(uint32_t *work, bool cand, uint32_t i) {
    const uint32_t at = wave_reserve(work, cand);
    if (cand) work[LIST_AT + at] = i;
}

__global__ void __launch_bounds__(PROOF_THREADS) k_prove_select(const ProveArgs a) {
    const uint32_t i = blockIdx.x * PROOF_THREADS + threadIdx.x;
    bool cand = false;
    if (i < a.n) {
        const rt_packet_fields &f = ((const rt_packet_fields *)a.fields)[i];
        const uint32_t l = (uint32_t)a.link[i];                 // -1: no link
        if (f.ok == 1 && f.packet_type == PKT_DATA && l < a.n_links) {
            const uint32_t fl = a.flags[l];
            if (f.context == CTX_CHANNEL)
                cand = (fl & FLAG_HAS_CHANNEL) != 0;
            else if (f.context == CTX_NONE)
                cand = (fl & FLAG_PROVE_ALL) != 0 && a.route[i] == RT_ROUTE_LINK_DECRYPT && a.status[i] == RT_ST_OK;
        }
        a.proof_len[i] = cand ? PROOF_BYTES : 0u;
    }
    append(a.work, cand, i);
}

// Two waves per SIMD without scratch, as k_ifac_sign has
__global__ void __launch_bounds__(PROOF_THREADS, 2) k_prove_sign(const ProveArgs a) {
    const uint32_t count = a.work[0];                           // at most n: one add per candidate
    const uint32_t first = blockIdx.x * PROOF_THREADS;
    if (first >= count) return;
    const uint32_t j = first + threadIdx.x;
    if (j >= count) return;
    const uint32_t i = a.work[LIST_AT + j];
    const rt_packet_fields &f = ((const rt_packet_fields *)a.fields)[i];
    const uint64_t key = (uint64_t)(uint32_t)a.link[i] * a.key_stride;
    uint32_t sig[16];
    ifac_sign_words(sig, a.seeds + key, a.publics + key, f.packet_hash, HASH);
    uint8_t *row = a.proofs + (uint64_t)i * a.proof_stride;
    prove_write<HASH>(row, 0x0F, f.destination_hash, f.packet_hash, sig);
}

__device__ __forceinline__ uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__global__ void __launch_bounds__(PROOF_THREADS) k_settle_select(const SettleArgs a) {
    const uint32_t i = blockIdx.x * PROOF_THREADS + threadIdx.x;
    bool cand = false;
    if (i < a.n) {
        const rt_packet_fields &f = ((const rt_packet_fields *)a.fields)[i];
        int32_t st = RT_PROOF_NOT_PROOF, id = -1;
        if (f.ok == 1 && f.packet_type == PKT_PROOF && f.context != CTX_LRPROOF && f.context != CTX_RESOURCE_PRF) {
            if (f.destination_type != DEST_LINK)
                st = RT_PROOF_NOT_LINK;
            else if ((uint32_t)a.link[i] >= a.n_links)           // -1: not in the link table
                st = RT_PROOF_NO_LINK;
            else if (f.data_len < HASH + SIGNATURE)
                st = RT_PROOF_SHORT;
            else {
                st = RT_PROOF_NO_RECEIPT;
                const uint8_t *h = a.pkt + a.pkt_off[i] + f.data_offset;
                const uint32_t s = find(view_of(a.t), u32x4{le32(h), le32(h + 4), le32(h + 8), le32(h + 12)});
                if (s != a.t.cap) {
                    const uint32_t v = a.t.values[s];
                    if (v < a.max_receipts) {
                        const uint8_t *want = a.hashes + (uint64_t)HASH * v;
                        uint32_t diff = 0;
                        for (uint32_t k = 16; k < HASH; ++k) diff |= (uint32_t)(h[k] ^ want[k]);
                        if (!diff) {
                            // the verdict should the signature hold and no lower index take the receipt
                            st = RT_PROOF_DELIVERED;
                            id = (int32_t)v;
                            a.work[LIST_AT + a.n + i] = s;
                            cand = true;
                        }
                    }
                }
            }
        }
        a.status[i] = st;
        a.receipt[i] = id;
    }
    append(a.work, cand, i);
}

// One wave per SIMD with the overflow in AGPRs, as k_ed25519_verify has
__global__ void __launch_bounds__(PROOF_THREADS) k_settle_verify(const SettleArgs a) {
    const uint32_t count = a.work[0];
    const uint32_t first = blockIdx.x * PROOF_THREADS;
    if (first >= count) return;
    const uint32_t j = first + threadIdx.x;
    if (j >= count) return;
    const uint32_t i = a.work[LIST_AT + j];
    const rt_packet_fields &f = ((const rt_packet_fields *)a.fields)[i];
    const uint8_t *data = a.pkt + a.pkt_off[i] + f.data_offset;
    uint32_t pk[8], r[8], s[8];
    load_words(pk, a.peer_publics + (uint64_t)HASH * (uint32_t)a.link[i]);
    load_words(r, data + HASH);
    load_words(s, data + HASH + 32);
    if (ed25519_verify_words(pk, r, s, data, HASH)) {
        const uint32_t slot = a.work[LIST_AT + a.n + i];
        full_lower(a.t.slots + slot, le32(data + 4), i);
    } else {
        a.status[i] = RT_PROOF_BAD_SIGNATURE;
        a.receipt[i] = -1;
    }
}

// The slot words are only read here: every candidate of a receipt sees the
// same winner, the all-ones index where no signature held.
__global__ void __launch_bounds__(PROOF_THREADS) k_settle_close(const SettleArgs a) {
    const uint32_t count = a.work[0];
    const uint32_t j = blockIdx.x * PROOF_THREADS + threadIdx.x;
    if (j >= count) return;
    const uint32_t i = a.work[LIST_AT + j];
    const uint32_t winner = w_idx(slot_load(a.t.slots + a.work[LIST_AT + a.n + i]));
    // a proof that verified and is not the first to: the receipt is gone; so it
    // is for a bad signature that comes after the proof that was delivered
    if (a.status[i] == RT_PROOF_DELIVERED ? winner != i : winner < i) {
        a.status[i] = RT_PROOF_NO_RECEIPT;
        a.receipt[i] = -1;
    }
}

__global__ void __launch_bounds__(PROOF_THREADS) k_settle_remove(const SettleArgs a) {
    const uint32_t count = a.work[0];
    const uint32_t first = blockIdx.x * PROOF_THREADS;
    if (first >= count) return;                                 // the whole block: the waves below stay whole
    const uint32_t j = first + threadIdx.x;
    bool won = false;
    if (j < count) {
        const uint32_t i = a.work[LIST_AT + j];
        won = a.status[i] == RT_PROOF_DELIVERED;
        if (won) tombstone(a.t.slots + a.work[LIST_AT + a.n + i]);
    }
    count_live(a.t.live, won, 0xFFFFFFFFu);                     // minus one each
}

// rt_receipt_store: the full hash of every receipt the insert entered
__global__ void __launch_bounds__(PROOF_THREADS) k_receipt_store(uint8_t *store, uint32_t max_receipts,
                                                                 const uint8_t *hashes, const uint32_t *ids,
                                                                 const int32_t *status, uint32_t n) {
    const uint32_t i = blockIdx.x * PROOF_THREADS + threadIdx.x;
    if (i >= n || status[i] != RT_LINK_OK || ids[i] >= max_receipts) return;
    st16(store + 32ull * ids[i], ld16(hashes + 32ull * i));
    st16(store + 32ull * ids[i] + 16, ld16(hashes + 32ull * i + 16));
}

dim3 proof_grid(uint32_t n) { return dim3((unsigned)(((uint64_t)n + PROOF_THREADS - 1) / PROOF_THREADS)); }

}  // namespace

uint64_t prove_workspace_bytes(uint32_t n) { return 4ull * (LIST_AT + (uint64_t)n); }
uint64_t settle_workspace_bytes(uint32_t n) { return 4ull * (LIST_AT + 2ull * n); }

hipError_t launch_link_prove(const ProveArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    // the count starts at 0 in every call
    hipError_t e = hipMemsetAsync(a.work, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_prove_select, proof_grid(a.n), dim3(PROOF_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_prove_sign, proof_grid(a.n), dim3(PROOF_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_proof_settle(const SettleArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.work, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_settle_select, proof_grid(a.n), dim3(PROOF_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_settle_verify, proof_grid(a.n), dim3(PROOF_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_settle_close, proof_grid(a.n), dim3(PROOF_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_settle_remove, proof_grid(a.n), dim3(PROOF_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_receipt_store(uint8_t *store, uint32_t max_receipts, const uint8_t *hashes, const uint32_t *ids,
                                const int32_t *status, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_receipt_store, proof_grid(n), dim3(PROOF_THREADS), 0, s, store, max_receipts, hashes, ids,
                       status, n);
    return hipGetLastError();
}

}  // namespace rnstok
