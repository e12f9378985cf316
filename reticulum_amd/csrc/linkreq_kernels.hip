// linkreq_kernels.hip — link requests on the device: the responder side of
// link establishment for requests to the node's own SINGLE destinations
// (Transport.py:2127-2158, Destination.py:414-435, Link.py:186-227, 336-376).
//
// For every LINKREQUEST among the records rt_packet_unpack wrote the stage
// decides as the reference does whether a link is born, and for those that are
// it does all of Link.validate_request that is arithmetic: the link id, the
// ephemeral public key, the exchange, the handshake key (as a record of the key
// set), the signature and the LRPROOF packet (Packet.py:170-185), the entry in
// the link table and the link's rows of the signers.
//
//   k_linkreq_select  one lane per record: the rules that need no key (packet
//       type, transport id, destination table, accept flag, the MTU step, data
//       size, mode), the link id with the shared SHA-256 message core, and the
//       number of valid requests of each workgroup.
//   k_linkreq_scan    one workgroup: where each workgroup's requests start in
//       stream order.
//   k_linkreq_claim   one lane per record: request r in stream order takes
//       slots[r] and row r of the ephemeral keys; those with a slot claim their
//       id in the link table (table_device.h's claim: an id present before is a
//       duplicate, the items of one id meet in one slot word).
//   k_linkreq_settle  one lane per record: the lowest index that met in a slot
//       word owns it, writes the entry and joins the list of accepted requests;
//       the others are duplicates.
//   k_linkreq_exchange  two lanes per accepted request, one ladder each: the
//       public key X25519(prv, 9) and the shared secret X25519(prv, peer_pub).
//       The first also lays out the 83 signed bytes; the second the salt and
//       the row of the key setup, and the new link's rows of the signers.
//   (key setup)       launch_hkdf_key_setup_rows (k_hkdf_key_setup's ROWS
//       instance, hkdf_kernels.hip): record slot of the key set from hkdf(64,
//       shared, salt = link id), the derived key in registers and scratch only.
//   k_linkreq_prove   one lane per accepted request: the signature with the
//       fixed-base table (ifac_sign_words, constant time in the seed) and the
//       118-byte packet.
// The exchange and the signature are kernels of their own: each keeps the
// register budget of the kernel it shares its code with (k_x25519, k_ifac_sign;
// DESIGN.md §4.3g), and a fused kernel would hold both working sets.
//
// The grids of the last three are sized for the most requests the call can
// accept; a workgroup past the count returns at once, so a read without a
// request costs the four passes over the records.
#include "ed25519_device.h"
#include "linkreq_host.h"
#include "table_device.h"

namespace rnstok {

namespace {

constexpr uint32_t LR_THREADS = 256;
constexpr uint32_t PKT_LINKREQUEST = 2u, DEST_SINGLE = 0u, HEADER_2 = 1u;
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
// the workspace, in words: [0] valid requests, [1] accepted requests, from
// word 16 on the arrays of LinkReqWork
constexpr uint32_t W_VALID = 0, W_ACCEPTED = 1, W_HEAD = 16;

struct LinkReqWork {
    uint32_t *head;
    uint32_t *part;       // workgroups + 1: valid requests per workgroup, then where they start
    uint32_t *rank;       // n: a valid request's position in stream order
    uint32_t *cslot;      // n: the slot word it met in
    uint32_t *drow;       // n: its destination's row
    uint32_t *won;        // cap: the accepted requests' record indices, in any order
    uint32_t *krow;       // cap: the key set row of accepted request w
    uint8_t *salt;        // cap x 16: its link id
    uint8_t *shared;      // cap x 32: its shared secret
    uint8_t *msg;         // cap x 96: link id ‖ pub ‖ destination's key ‖ signalling (83 bytes)
};
__host__ __device__ inline uint32_t lr_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + LR_THREADS - 1) / LR_THREADS); }
__host__ __device__ inline uint32_t lr_cap(const LinkReqArgs &a) { return a.n < a.m ? a.n : a.m; }
__host__ __device__ inline LinkReqWork work_of(const LinkReqArgs &a) {
    LinkReqWork w;
    const uint64_t n = a.n, cap = lr_cap(a), nb = lr_blocks(a.n);
    w.head = a.work;
    w.part = a.work + W_HEAD;
    w.rank = w.part + ((nb + 1 + 3) & ~3ull);
    w.cslot = w.rank + n;
    w.drow = w.cslot + n;
    w.won = w.drow + n;
    w.krow = w.won + cap;
    uint32_t *bytes = w.krow + cap + ((4 - ((3 * n + 2 * cap) & 3)) & 3);     // 16-byte aligned from here
    w.salt = (uint8_t *)bytes;
    w.shared = w.salt + 16 * cap;
    w.msg = w.shared + 32 * cap;
    return w;
}

__device__ __forceinline__ const rt_packet_fields &record(const LinkReqArgs &a, uint32_t i) {
    return ((const rt_packet_fields *)a.fields)[i];
}
__device__ __forceinline__ u32x4 words16(const uint8_t *p) {
    const uint32_t *w = (const uint32_t *)p;            // a record's hashes sit on words
    return u32x4{w[0], w[1], w[2], w[3]};
}

__global__ void __launch_bounds__(LR_THREADS) k_linkreq_select(const LinkReqArgs a, const LinkReqWork w) {
    const uint32_t i = blockIdx.x * LR_THREADS + threadIdx.x;
    bool valid = false;
    if (i < a.n) {
        const rt_packet_fields &f = record(a, i);
        int32_t st = RT_LINKREQ_NOT_REQUEST;
        uint32_t mtu = 0, row = NO_ROW;
        u32x4 id = {0u, 0u, 0u, 0u};
        if (f.ok == 1 && f.packet_type == PKT_LINKREQUEST) {
            const uint8_t *pkt = a.pkt + a.pkt_off[i];
            const uint8_t *data = pkt + f.data_offset;
            uint32_t s = a.dests.cap;
            if (f.header_type == HEADER_2 && !same(words16(f.transport_id), ld16(a.transport_id)))
                st = RT_LINKREQ_OTHER_TRANSPORT;
            else if (f.destination_type != DEST_SINGLE ||
                     (s = find(view_of(a.dests), words16(f.destination_hash))) == a.dests.cap ||
                     (row = a.dests.values[s]) >= a.n_dests)
                st = RT_LINKREQ_NO_DESTINATION;
            else if (!(a.dest_flags[row] & RT_DEST_ACCEPTS))
                st = RT_LINKREQ_NOT_ACCEPTING;
            else {
                const uint32_t b0 = f.data_len == LR_DATA_MTU ? data[64] : 0u;
                const uint32_t b1 = f.data_len == LR_DATA_MTU ? data[65] : 0u;
                const uint32_t b2 = f.data_len == LR_DATA_MTU ? data[66] : 0u;
                const LinkReqPlan p = linkreq_plan(f.data_len, b0, b1, b2, a.has_nh_mtu != 0, a.nh_mtu);
                st = p.status;
                if (st == RT_LINKREQ_ACCEPTED) {
                    valid = true;
                    mtu = p.mtu;
                    // the hashable part (Packet.py:342-353) without the signalling bytes still in the data
                    const uint32_t skip = f.header_type == HEADER_2 ? 18u : 2u;
                    const uint32_t m = 1u + (f.data_offset - skip) + f.data_len - p.unhashed;
                    uint32_t h[8];
                    sha256_init(h);
                    sha_tail(h, m, 8ull * m, PrefixedAt{(uint32_t)f.flags & 0x0Fu, pkt + skip, 0u});
                    id = u32x4{bswap(h[0]), bswap(h[1]), bswap(h[2]), bswap(h[3])};
                }
            }
        }
        a.status[i] = st;
        a.accepted[i] = -1;
        a.mtu[i] = (int32_t)mtu;
        a.proof_len[i] = 0u;
        st16(a.link_id + 16ull * i, id);
        w.drow[i] = row;
    }
    const int c = __syncthreads_count(valid);
    if (threadIdx.x == 0) w.part[blockIdx.x] = (uint32_t)c;
}

// One workgroup: exclusive sums of the workgroups' counts in place, the total
// behind them and in the head.
__global__ void __launch_bounds__(LR_THREADS) k_linkreq_scan(const LinkReqWork w, uint32_t nb) {
    __shared__ uint32_t sh[LR_THREADS];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += LR_THREADS) {
        const uint32_t i = base + t;
        const uint32_t v = i < nb ? w.part[i] : 0u;
        sh[t] = v;
        __syncthreads();
        for (uint32_t d = 1; d < LR_THREADS; d <<= 1) {
            const uint32_t add = t >= d ? sh[t - d] : 0u;
            __syncthreads();
            sh[t] += add;
            __syncthreads();
        }
        if (i < nb) w.part[i] = carry + sh[t] - v;
        carry += sh[LR_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) {
        w.part[nb] = carry;
        w.head[W_VALID] = carry;
    }
}

__global__ void __launch_bounds__(LR_THREADS) k_linkreq_claim(const LinkReqArgs a, const LinkReqWork w) {
    __shared__ uint32_t wave_n[LR_THREADS / 64];
    const uint32_t i = blockIdx.x * LR_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const bool valid = i < a.n && a.status[i] == RT_LINKREQ_ACCEPTED;
    const uint64_t bal = __ballot(valid);
    if (lane == 0) wave_n[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (!valid) return;
    uint32_t r = w.part[blockIdx.x] + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (uint32_t j = 0; j < wv; ++j) r += wave_n[j];
    w.rank[i] = r;
    int32_t st = RT_LINKREQ_NO_SLOT;
    if (r < a.m) {
        const uint32_t slot = (uint32_t)a.slots[r];
        if (slot < a.n_keys && slot < a.n_links) {
            const uint8_t *ids = a.link_id;
            const auto batch_id = [ids](uint32_t j) { return ld16(ids + 16ull * j); };
            const Claim c = claim(view_of(a.links), batch_id(i), i, true, batch_id);
            if (c.kind == CLAIM_PRESENT)
                st = RT_LINKREQ_DUPLICATE;
            else if (c.kind == CLAIM_MET) {
                st = RT_LINKREQ_ACCEPTED;          // should the slot word still carry i when the claims are done
                w.cslot[i] = c.slot;
            }
        }
    }
    a.status[i] = st;
}

__global__ void __launch_bounds__(LR_THREADS) k_linkreq_settle(const LinkReqArgs a, const LinkReqWork w) {
    const uint32_t i = blockIdx.x * LR_THREADS + threadIdx.x;
    bool won = false;
    uint32_t slot = 0;
    if (i < a.n && a.status[i] == RT_LINKREQ_ACCEPTED) {
        const uint32_t s = w.cslot[i];
        const uint64_t sw = slot_load(a.links.slots + s);
        won = w_state(sw) == ST_PENDING && w_idx(sw) == i;
        if (won) {
            slot = (uint32_t)a.slots[w.rank[i]];
            st16(a.links.ids + 16ull * s, ld16(a.link_id + 16ull * i));
            a.links.values[s] = slot;
            slot_store(a.links.slots + s, word(w_tag(sw), ST_FULL, IDX_MASK));
            a.accepted[i] = (int32_t)slot;
        } else {
            a.status[i] = RT_LINKREQ_DUPLICATE;
        }
    }
    count_live(a.links.live, won, 1u);
    const uint32_t at = wave_reserve(w.head + W_ACCEPTED, won);
    if (won) w.won[at] = i;
}

// Three waves per SIMD without scratch, as k_x25519
__global__ void __launch_bounds__(LR_THREADS) k_linkreq_exchange(const LinkReqArgs a, const LinkReqWork w) {
    const uint32_t count = w.head[W_ACCEPTED];                  // at most cap: one add per accepted request
    const uint32_t first = blockIdx.x * (LR_THREADS / 2);
    if (first >= count) return;
    const uint32_t j = first + (threadIdx.x >> 1), which = threadIdx.x & 1u;
    if (j >= count) return;
    const uint32_t i = w.won[j], r = w.rank[i];
    const rt_packet_fields &f = record(a, i);
    const uint8_t *data = a.pkt + a.pkt_off[i] + f.data_offset;
    uint32_t e[8], u[8], out[8];
    load_words(e, a.ephemeral + 32ull * r);
    load_words(u, data);                                        // peer_pub
    // X25519PrivateKey.exchange (X25519.py:139-145) takes the peer's 256-bit
    // value mod p as it is, where x25519_words drops bit 255 as curve25519()
    // does: the bit counts 2^255 = 19 (mod p).  Twice, for a value that passes
    // 2^255 again; peer_pub is public, so nothing here needs to be uniform.
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
    if (!which) {                                               // the base point: the link's public key
        u[0] = 9u;
#pragma unroll
        for (int k = 1; k < 8; ++k) u[k] = 0u;
    }
    x25519_words(out, e, u);
    if (which) {
        store_words(w.shared + 32ull * j, out);
        st16(w.salt + 16ull * j, ld16(a.link_id + 16ull * i));
        const uint32_t slot = (uint32_t)a.accepted[i];
        w.krow[j] = slot;
        // the new link's rows of the signers
        if (a.sg_peer) {
            const uint32_t d = w.drow[i];
            for (uint32_t k = 0; k < 32; ++k) a.sg_peer[32ull * slot + k] = data[32 + k];
            a.sg_flags[slot] = a.dest_flags[d] & (RT_LINK_PROVE_ALL | RT_LINK_HAS_CHANNEL);
            if (a.sg_stride) {
                for (uint32_t k = 0; k < 32; ++k) {
                    a.sg_seeds[slot * a.sg_stride + k] = a.dest_seeds[32ull * d + k];
                    a.sg_publics[slot * a.sg_stride + k] = a.dest_publics[32ull * d + k];
                }
            }
        }
    } else {
        uint8_t *msg = w.msg + 96ull * j;
        const uint8_t *id = a.link_id + 16ull * i, *pk = a.dest_publics + 32ull * w.drow[i];
        for (uint32_t k = 0; k < 16; ++k) msg[k] = id[k];
        store_words(msg + 16, out);
        for (uint32_t k = 0; k < 32; ++k) msg[48 + k] = pk[k];
        uint8_t sg[3];
        linkreq_signalling(sg, (uint32_t)a.mtu[i]);
        for (uint32_t k = 0; k < 3; ++k) msg[80 + k] = sg[k];
    }
}

// Two waves per SIMD without scratch, as k_ifac_sign and k_prove_sign
__global__ void __launch_bounds__(LR_THREADS, 2) k_linkreq_prove(const LinkReqArgs a, const LinkReqWork w) {
    const uint32_t count = w.head[W_ACCEPTED];
    const uint32_t first = blockIdx.x * LR_THREADS;
    if (first >= count) return;
    const uint32_t j = first + threadIdx.x;
    if (j >= count) return;
    const uint8_t *msg = w.msg + 96ull * j;
    uint32_t sig[16];
    {
        const uint32_t d = w.drow[w.won[j]];
        ifac_sign_words(sig, a.dest_seeds + 32ull * d, a.dest_publics + 32ull * d, msg, LR_SIGNED);
    }
    // (the record index is read again here, not held across the signature)
    const uint32_t i = w.won[j];
    uint8_t *row = a.proofs + (uint64_t)i * a.proof_stride;
    linkreq_proof_head(row, msg);
    // byte k of the signature with a constant k (a computed word index would put sig in scratch)
#pragma unroll
    for (uint32_t k = 0; k < 64; ++k) row[LR_PROOF_HEADER + k] = (uint8_t)(sig[k >> 2] >> (8 * (k & 3)));
    linkreq_proof_tail(row, msg);
    a.proof_len[i] = LR_PROOF_BYTES;
}

// rt_keyset_set_rows_x25519: the rows the mask selects, NO_ROW for the others
__global__ void __launch_bounds__(LR_THREADS) k_rows_select(const uint32_t *rows, const uint8_t *mask, uint32_t n_keys,
                                                            uint32_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * LR_THREADS + threadIdx.x;
    if (i >= n) return;
    out[i] = (!mask || mask[i]) && rows[i] < n_keys ? rows[i] : NO_ROW;
}

}  // namespace

uint64_t linkreq_workspace_bytes(uint32_t n, uint32_t m) {
    const uint64_t cap = n < m ? n : m, nb = lr_blocks(n);
    return 4ull * (W_HEAD + ((nb + 1 + 3) & ~3ull) + 3ull * n + 2 * cap + 4) + (16 + 32 + 96) * cap;
}

hipError_t launch_link_accept(const LinkReqArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const LinkReqWork w = work_of(a);
    const uint32_t nb = lr_blocks(a.n), cap = lr_cap(a);
    // both counts start at 0 in every call
    hipError_t e = hipMemsetAsync(a.work, 0, 4ull * W_HEAD, s);
    if (e != hipSuccess) return e;
    const dim3 grid(nb), block(LR_THREADS);
    hipLaunchKernelGGL(k_linkreq_select, grid, block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_linkreq_scan, dim3(1), block, 0, s, w, nb);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_linkreq_claim, grid, block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_linkreq_settle, grid, block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (cap == 0) return hipSuccess;
    hipLaunchKernelGGL(k_linkreq_exchange, dim3(lr_blocks(2 * cap)), block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    HkdfArgs h{};
    h.ikm = w.shared; h.ikm_stride = 32; h.ikm_len = 32;
    h.salt = w.salt; h.salt_stride = 16; h.salt_len = 16;
    h.length = 64; h.n = cap;
    if ((e = launch_hkdf_key_setup_rows(h, a.sbox, a.rec, w.krow, w.head + W_ACCEPTED, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_linkreq_prove, dim3(lr_blocks(cap)), block, 0, s, a, w);
    return hipGetLastError();
}

hipError_t launch_rows_select(const uint32_t *rows, const uint8_t *mask, uint32_t n_keys, uint32_t *out, uint32_t n,
                              hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_select, dim3(lr_blocks(n)), dim3(LR_THREADS), 0, s, rows, mask, n_keys, out, n);
    return hipGetLastError();
}

}  // namespace rnstok
