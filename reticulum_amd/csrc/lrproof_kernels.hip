// lrproof_kernels.hip — link request proofs on the device: the initiator side
// of link establishment for the node's own pending links (Transport.py:2270-2318,
// Link.py:391-451, 326-333, 348-361).
//
// For every LRPROOF among the records rt_packet_unpack wrote the stage decides
// as the reference does what becomes of the pending link it names, as if the
// packets came one after another in index order, and for the links that come
// up it does all of Link.validate_proof that is arithmetic: the signature, the
// exchange, the handshake key (as a record of the key set), the entry in the
// link table and the link's rows of the signers.
//
// A proof that changes its link at all leaves it CLOSED, in HANDSHAKE or ACTIVE
// (a rebalance is always followed by the activation: the signature it checked
// is the one validate_proof checks), and no later proof finds it PENDING.  So
// every record is classified against the rows as the call found them, the
// records that decide a link meet in its word of the pending table, and the
// lowest index stays (table_device.h's full_lower, as the receipts are settled).
//
//   k_lrproof_select  one lane per record: packet type, context (the branch
//       never reads the destination type), the pending table, the row's state,
//       and lrproof_plan's length,
//       mode and hop rules (lrproof_host.h).  The records that need a signature
//       are compacted, each with its signed message laid out: link id ‖
//       data[64:96] ‖ the destination's key ‖ 0 or 3 signalling bytes encoded
//       anew.
//   k_lrproof_verify  one lane per candidate: the Ed25519 verify core of
//       k_ed25519_verify over those 80 or 83 bytes.
//   k_lrproof_decide  one lane per record: a record that decides its link lowers
//       the index field of the row's slot word to its own index.
//   k_lrproof_claim   one lane per record: the record whose index the word
//       carries is the winner; the records behind it read NOT_PENDING, those
//       before it keep HOPS or BAD_SIZE.  A winner whose signature holds claims
//       its link id in the link table (table_device.h's claim) where the row's
//       slot is in range.  Also which packet hashes the hash list learns.
//   k_lrproof_settle  one lane per record: the winners write the row's state,
//       hops, rebalanced and MTU, the link table's entry, join the list of
//       activated links, and put the row's slot word back.
//   k_lrproof_exchange  one lane per activated link: X25519(row's private,
//       data[64:96]), bit 255 not masked (k_linkreq_exchange's ladder without
//       its base-point lane), the salt and row of the key setup, and the new
//       link's rows of the signers.
//   (key setup)       launch_hkdf_key_setup_rows, as the link requests use it.
// The signature is settled before any ladder runs: a forged proof costs one
// verification and no exchange, and what it leaves behind (the row in
// HANDSHAKE, nothing in the link table) is what the reference leaves.
//
// The grids of the verify kernel, the exchange and the key setup are sized for
// the most the call can hold; a workgroup past the count returns at once, so a
// read without a proof costs the five launches over the records (select,
// verify's early return, decide, claim, settle), four of which pass over them.
#include "ed25519_device.h"
#include "lrproof_host.h"
#include "table_device.h"

namespace rnstok {

namespace {

constexpr uint32_t LP_THREADS = 256;
constexpr uint32_t PKT_PROOF = 3u, CTX_LRPROOF = 0xFFu;
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
// what select (and verify) found out about a record
constexpr uint32_t C_LIVE = 1u,        // its row was PENDING
    C_HOP = 2u,                        // the hop count matches
    C_VERIFY = 4u,                     // its signature is checked
    C_SIG = 8u,                        // and holds
    C_MODE = 16u,                      // hop match, wrong mode: the link closes
    C_KEEP = 32u;                      // the row was CLOSED or in HANDSHAKE and the hop count matches: remembered
// the workspace, in words: [0] candidates, [1] activated links, from word 16
// on the arrays of LrProofWork
constexpr uint32_t W_CAND = 0, W_WON = 1, W_HEAD = 16;
constexpr uint32_t MSG_ROW = 96, MSG_LEN_AT = 95;

struct LrProofWork {
    uint32_t *head;
    uint32_t *cand;       // n: the candidates' record indices, in any order
    uint32_t *prow;       // n: the record's pending row
    uint32_t *pslot;      // n: the slot of the pending table it was found in
    uint32_t *cls;        // n: C_*
    uint32_t *cslot;      // n: the slot of the link table a winner claimed
    uint32_t *won;        // cap: the activated records, in any order
    uint32_t *krow;       // cap: the key set row of activated link w
    uint8_t *salt;        // cap x 16: its link id
    uint8_t *shared;      // cap x 32: its shared secret
    uint8_t *msg;         // n x 96: candidate j's signed bytes, their number in byte 95
};
__host__ __device__ inline uint32_t lp_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + LP_THREADS - 1) / LP_THREADS); }
__host__ __device__ inline uint32_t lp_cap(uint32_t n, uint32_t n_rows) { return n < n_rows ? n : n_rows; }
__host__ __device__ inline uint64_t lp_words(uint64_t n, uint64_t cap) { return (W_HEAD + 5 * n + 2 * cap + 3) & ~3ull; }
__host__ __device__ inline LrProofWork work_of(const LrProofArgs &a) {
    LrProofWork w;
    const uint64_t n = a.n, cap = lp_cap(a.n, a.n_rows);
    w.head = a.work;
    w.cand = a.work + W_HEAD;
    w.prow = w.cand + n;
    w.pslot = w.prow + n;
    w.cls = w.pslot + n;
    w.cslot = w.cls + n;
    w.won = w.cslot + n;
    w.krow = w.won + cap;
    w.salt = (uint8_t *)(a.work + lp_words(n, cap));            // 16-byte aligned from here
    w.shared = w.salt + 16 * cap;
    w.msg = w.shared + 32 * cap;
    return w;
}

__device__ __forceinline__ const rt_packet_fields &record(const LrProofArgs &a, uint32_t i) {
    return ((const rt_packet_fields *)a.fields)[i];
}
__device__ __forceinline__ u32x4 words16(const uint8_t *p) {
    const uint32_t *w = (const uint32_t *)p;            // a record's hashes sit on words
    return u32x4{w[0], w[1], w[2], w[3]};
}
// the hop count as Transport.inbound counts it (Transport.py:1496)
__device__ __forceinline__ int32_t hops_of(const rt_packet_fields &f) { return (int32_t)f.hops + 1; }
__device__ __forceinline__ uint32_t state_of(uint32_t c) {
    return (c & C_MODE) ? RT_PENDING_CLOSED : (c & C_SIG) ? RT_PENDING_ACTIVE : RT_PENDING_HANDSHAKE;
}

__global__ void __launch_bounds__(LP_THREADS) k_lrproof_select(const LrProofArgs a, const LrProofWork w) {
    const uint32_t i = blockIdx.x * LP_THREADS + threadIdx.x;
    bool cand = false;
    uint32_t row = NO_ROW, n_sig = 0, confirmed = 0;
    if (i < a.n) {
        const rt_packet_fields &f = record(a, i);
        int32_t st = RT_LRPROOF_NOT_LRPROOF;
        uint32_t c = 0, mtu = 0, ps = 0;
        if (f.ok == 1 && f.packet_type == PKT_PROOF && f.context == CTX_LRPROOF) {
            const uint32_t s = find(view_of(a.pending), words16(f.destination_hash));
            if (s == a.pending.cap || (row = a.pending.values[s]) >= a.n_rows) {
                st = RT_LRPROOF_NO_LINK;
                row = NO_ROW;
            } else {
                ps = s;
                const uint32_t state = a.row_state[row];
                const bool hop = hops_of(f) == a.row_hops[row];
                if (state != RT_PENDING_PENDING) {
                    st = RT_LRPROOF_NOT_PENDING;
                    if (state != RT_PENDING_ACTIVE && hop) c = C_KEEP;
                } else {
                    const uint8_t *data = a.pkt + a.pkt_off[i] + f.data_offset;
                    const uint32_t b0 = f.data_len > LP_DATA ? data[LP_DATA] : 0u;
                    const uint32_t b1 = f.data_len == LP_DATA_MTU ? data[LP_DATA + 1] : 0u;
                    const uint32_t b2 = f.data_len == LP_DATA_MTU ? data[LP_DATA + 2] : 0u;
                    const LrProofPlan p = lrproof_plan(f.data_len, b0, b1, b2, hop, a.row_rebalanced[row] != 0);
                    st = p.status;
                    mtu = p.mtu;
                    cand = p.verify != 0;
                    n_sig = p.n_sig;
                    confirmed = p.confirmed;
                    c = C_LIVE | (hop ? C_HOP : 0u) | (cand ? C_VERIFY : 0u) |
                        (st == RT_LRPROOF_BAD_MODE ? C_MODE : 0u);
                }
            }
        }
        a.status[i] = st;
        a.established[i] = -1;
        a.mtu[i] = (int32_t)mtu;
        w.prow[i] = row;
        w.pslot[i] = ps;
        w.cls[i] = c;
        w.cslot[i] = NO_ROW;
    }
    const uint32_t at = wave_reserve(w.head + W_CAND, cand);
    if (cand) {
        const rt_packet_fields &f = record(a, i);
        const uint8_t *data = a.pkt + a.pkt_off[i] + f.data_offset;
        const uint8_t *pk = a.row_dest_publics + 32ull * row;
        uint8_t *msg = w.msg + (uint64_t)MSG_ROW * at;
        w.cand[at] = i;
        for (uint32_t k = 0; k < 16; ++k) msg[k] = f.destination_hash[k];
        for (uint32_t k = 0; k < 32; ++k) msg[16 + k] = data[LP_PEER_PUB + k];
        for (uint32_t k = 0; k < 32; ++k) msg[48 + k] = pk[k];
        uint8_t sg[3];
        lrproof_signalling(sg, confirmed);
        for (uint32_t k = 0; k < 3; ++k) msg[LP_SIGNED + k] = sg[k];
        msg[MSG_LEN_AT] = (uint8_t)(LP_SIGNED + n_sig);
    }
}

// One wave per SIMD with the overflow in AGPRs, as k_ed25519_verify has
__global__ void __launch_bounds__(LP_THREADS) k_lrproof_verify(const LrProofArgs a, const LrProofWork w) {
    const uint32_t count = w.head[W_CAND];                      // at most n: one add per candidate
    const uint32_t first = blockIdx.x * LP_THREADS;
    if (first >= count) return;
    const uint32_t j = first + threadIdx.x;
    if (j >= count) return;
    const uint32_t i = w.cand[j];
    const rt_packet_fields &f = record(a, i);
    const uint8_t *data = a.pkt + a.pkt_off[i] + f.data_offset;
    const uint8_t *msg = w.msg + (uint64_t)MSG_ROW * j;
    uint32_t pk[8], r[8], s[8];
    load_words(pk, a.row_dest_publics + 32ull * w.prow[i]);
    load_words(r, data);
    load_words(s, data + 32);
    if (ed25519_verify_words(pk, r, s, msg, msg[MSG_LEN_AT])) w.cls[i] |= C_SIG;
}

__global__ void __launch_bounds__(LP_THREADS) k_lrproof_decide(const LrProofArgs a, const LrProofWork w) {
    const uint32_t i = blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t c = w.cls[i];
    if (!(c & C_LIVE)) return;
    // lrproof_decisive: a hop match decides unless the length is wrong; a mismatch where the rebalance fires
    const bool decisive = (c & C_HOP) ? a.status[i] != RT_LRPROOF_BAD_SIZE : (c & C_VERIFY) && (c & C_SIG);
    if (decisive) full_lower(a.pending.slots + w.pslot[i], words16(record(a, i).destination_hash).y, i);
}

__global__ void __launch_bounds__(LP_THREADS) k_lrproof_claim(const LrProofArgs a, const LrProofWork w) {
    const uint32_t i = blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t c = w.cls[i];
    const rt_packet_fields &f = record(a, i);
    bool remember = (c & C_KEEP) != 0;
    if (c & C_LIVE) {
        int32_t st = a.status[i];
        const uint32_t winner = w_idx(slot_load(a.pending.slots + w.pslot[i]));     // all ones: nobody decided
        if (winner < i) {
            // the link was decided before this packet came: validate_proof is still reached on a link that is
            // among the pending ones (not ACTIVE) when the hop count matches what the winner left
            st = RT_LRPROOF_NOT_PENDING;
            remember = state_of(w.cls[winner]) != RT_PENDING_ACTIVE && hops_of(f) == hops_of(record(a, winner));
        } else if (winner == i) {
            const uint32_t state = state_of(c);
            remember = true;
            if (state == RT_PENDING_CLOSED) {
                st = RT_LRPROOF_BAD_MODE;
            } else if (state == RT_PENDING_HANDSHAKE) {
                st = RT_LRPROOF_BAD_SIGNATURE;
            } else {
                st = RT_LRPROOF_NO_SLOT;
                remember = false;
                const uint32_t slot = (uint32_t)a.row_slots[w.prow[i]];
                if (slot < a.n_keys && slot < a.n_links) {
                    const uint8_t *fields = a.fields;
                    const auto batch_id = [fields](uint32_t j) {
                        return words16(((const rt_packet_fields *)fields)[j].destination_hash);
                    };
                    const Claim cl = claim(view_of(a.links), batch_id(i), i, true, batch_id);
                    if (cl.kind == CLAIM_MET) {
                        st = RT_LRPROOF_ACTIVATED;
                        remember = true;
                        w.cslot[i] = cl.slot;
                    }
                }
            }
        } else {
            remember = (c & C_HOP) != 0;                // BAD_SIZE with a hop match; HOPS never
        }
        a.status[i] = st;
        if (st != RT_LRPROOF_ACTIVATED) a.mtu[i] = 0;
    }
    if (a.remember) {
        a.remember[i] = remember;
        if (remember) {
            st16(a.hashes + 32ull * i, words16(f.packet_hash));
            st16(a.hashes + 32ull * i + 16, words16(f.packet_hash + 16));
        }
    }
}

__global__ void __launch_bounds__(LP_THREADS) k_lrproof_settle(const LrProofArgs a, const LrProofWork w) {
    const uint32_t i = blockIdx.x * LP_THREADS + threadIdx.x;
    bool won = false;
    if (i < a.n && (w.cls[i] & C_LIVE)) {
        uint64_t *pword = a.pending.slots + w.pslot[i];
        const uint64_t pw = slot_load(pword);
        if (w_idx(pw) == i) {                           // the winner; only it writes the word in this kernel
            const uint32_t row = w.prow[i];
            int32_t st = a.status[i];
            if (st == RT_LRPROOF_ACTIVATED) {
                const uint32_t s = w.cslot[i];
                const uint64_t sw = slot_load(a.links.slots + s);
                if (w_state(sw) == ST_PENDING && w_idx(sw) == i) {
                    const rt_packet_fields &f = record(a, i);
                    const uint32_t slot = (uint32_t)a.row_slots[row];
                    st16(a.links.ids + 16ull * s, words16(f.destination_hash));
                    a.links.values[s] = slot;
                    slot_store(a.links.slots + s, word(w_tag(sw), ST_FULL, IDX_MASK));
                    a.established[i] = (int32_t)slot;
                    a.row_state[row] = RT_PENDING_ACTIVE;
                    a.row_mtu[row] = a.mtu[i];
                    if (!(w.cls[i] & C_HOP)) {
                        a.row_rebalanced[row] = 1;
                        a.row_hops[row] = hops_of(f);
                    }
                    won = true;
                } else {
                    a.status[i] = RT_LRPROOF_NO_SLOT;   // another call's entry of this id: the row stays as it is
                    a.mtu[i] = 0;
                    if (a.remember) a.remember[i] = 0;  // and, as every NO_SLOT, its hash is not remembered
                }
            } else if (st == RT_LRPROOF_BAD_MODE) {
                a.row_state[row] = RT_PENDING_CLOSED;
            } else if (st == RT_LRPROOF_BAD_SIGNATURE) {
                a.row_state[row] = RT_PENDING_HANDSHAKE;
            }
            slot_store(pword, word(w_tag(pw), ST_FULL, IDX_MASK));
        }
    }
    count_live(a.links.live, won, 1u);
    const uint32_t at = wave_reserve(w.head + W_WON, won);
    if (won) w.won[at] = i;
}

// Three waves per SIMD without scratch, as k_linkreq_exchange and k_x25519
__global__ void __launch_bounds__(LP_THREADS) k_lrproof_exchange(const LrProofArgs a, const LrProofWork w) {
    const uint32_t count = w.head[W_WON];                       // at most cap: one add per activated link
    const uint32_t first = blockIdx.x * LP_THREADS;
    if (first >= count) return;
    const uint32_t j = first + threadIdx.x;
    if (j >= count) return;
    const uint32_t i = w.won[j], row = w.prow[i];
    const rt_packet_fields &f = record(a, i);
    const uint8_t *data = a.pkt + a.pkt_off[i] + f.data_offset;
    uint32_t e[8], u[8], out[8];
    load_words(e, a.row_privates + 32ull * row);
    load_words(u, data + LP_PEER_PUB);
    // X25519PrivateKey.exchange takes the peer's 256-bit value mod p as it is
    // (k_linkreq_exchange): bit 255 counts 2^255 = 19 (mod p).  Twice, for a
    // value that passes 2^255 again; peer_pub is public.
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t c = 19u * (u[7] >> 31);
        u[7] &= 0x7fffffffu;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            c += u[k];
            u[k] = (uint32_t)c;
            c >>= 32;
        }
    }
    x25519_words(out, e, u);
    store_words(w.shared + 32ull * j, out);
    st16(w.salt + 16ull * j, words16(f.destination_hash));
    const uint32_t slot = (uint32_t)a.established[i];
    w.krow[j] = slot;
    // the new link's rows of the signers; the row index is public, the bytes are copied whatever they are
    if (a.sg_peer) {
        for (uint32_t k = 0; k < 32; ++k) a.sg_peer[32ull * slot + k] = a.row_dest_publics[32ull * row + k];
        a.sg_flags[slot] = a.row_flags[row] & (RT_LINK_PROVE_ALL | RT_LINK_HAS_CHANNEL);
        if (a.sg_stride) {
            for (uint32_t k = 0; k < 32; ++k) {
                a.sg_seeds[slot * a.sg_stride + k] = a.row_sig_seeds[32ull * row + k];
                a.sg_publics[slot * a.sg_stride + k] = a.row_sig_publics[32ull * row + k];
            }
        }
    }
}

}  // namespace

uint64_t lrproof_workspace_bytes(uint32_t n, uint32_t n_rows) {
    const uint64_t cap = lp_cap(n, n_rows);
    return 4ull * lp_words(n, cap) + (16 + 32) * cap + (uint64_t)MSG_ROW * n;
}

hipError_t launch_link_establish(const LrProofArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const LrProofWork w = work_of(a);
    const uint32_t cap = lp_cap(a.n, a.n_rows);
    // both counts start at 0 in every call
    hipError_t e = hipMemsetAsync(a.work, 0, 4ull * W_HEAD, s);
    if (e != hipSuccess) return e;
    const dim3 grid(lp_blocks(a.n)), block(LP_THREADS);
    hipLaunchKernelGGL(k_lrproof_select, grid, block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_lrproof_verify, grid, block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_lrproof_decide, grid, block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_lrproof_claim, grid, block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_lrproof_settle, grid, block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (cap == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lrproof_exchange, dim3(lp_blocks(cap)), block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    HkdfArgs h{};
    h.ikm = w.shared; h.ikm_stride = 32; h.ikm_len = 32;
    h.salt = w.salt; h.salt_stride = 16; h.salt_len = 16;
    h.length = 64; h.n = cap;
    return launch_hkdf_key_setup_rows(h, a.sbox, a.rec, w.krow, w.head + W_WON, s);
}

}  // namespace rnstok
