// destination_kernels.hip — destination delivery on the device: the DATA
// packets of a read that are addressed to the node's own SINGLE destinations
// (Transport.py:2188-2202, Destination.py:414-429 and :622-654,
// Identity.py:848-898 and :942-953, Packet.py:327-381).
//
// For every record rt_packet_unpack wrote the stage decides as the reference
// does whether the packet reaches a destination, tries the destination's
// ratchets in list order and then the identity's own key (left out where the
// destination enforces ratchets), decrypts under the first candidate whose
// token key opens the token, and writes the PROOF packet of a PROVE_ALL
// destination.  A candidate's key is Token(hkdf(64, X25519(candidate,
// data[:32]), salt = identity hash)) in a record of the scratch key set; the
// first candidate "opens" by rt_verify_trials' rule (the first key whose tag
// verifies over a well-formed token; a bad padding under that key means the
// packet is not opened, as every later candidate that verifies is the same key).
//
//   k_deliver_select   one lane per record: the rules that need no key (DATA,
//       destination type, the destination table, the data's length), the
//       token's span, the number of candidates, and each workgroup's count of
//       selected frames.
//   k_deliver_scan     one workgroup: where each workgroup's share starts, in
//       stream order (sums that stop at the top of a word; used for both passes).
//   k_deliver_rank     one lane per record: selected frame r in stream order
//       gets pair r, key record r and candidate 0.
//   k_deliver_exchange one lane per pair: X25519(candidate, ephemeral key) with
//       the exchange Identity.decrypt performs (X25519PrivateKey.exchange takes
//       the peer's 256-bit value mod p as it is), the salt and the key row of
//       launch_hkdf_key_setup_rows, which follows; launch_verify_trials then
//       tries every pair.  Pass one: one pair per selected frame.
//   k_deliver_ask      one lane per record: what a frame the first pass left
//       undecided asks of the retry budget, and each workgroup's sum.
//   k_deliver_plan     one lane per record: whole frames go into the budget's
//       rows in stream order as (frame, candidate) pairs; a frame that does not
//       fit is DEFERRED, and so is every undecided frame behind it
//       (destination_host.h).  Pass two runs exchange, key setup and trials
//       over these pairs.
//   k_deliver_pick     one lane per record: the winning candidate and its key
//       record for launch_decrypt, which follows over all n records (a record
//       without a winner has token length 0 there and costs a lane nothing).
//   k_deliver_finish   one lane per record: status, pt_len, deliver_status and
//       ratchet of the opened frames, proof_len, the list of frames to prove.
//   k_deliver_prove    one lane per frame to prove: prove_device.h's core, the
//       one k_prove_sign runs.
// No loop on the host depends on a device count: the grids of exchange, key
// setup, trials and prove are sized for the most pairs the call can have, and a
// workgroup past the count returns at once.
#include "destination_host.h"
#include "prove_device.h"
#include "table_device.h"

namespace rnstok {

namespace {

constexpr uint32_t PKT_DATA = 0u, DEST_SINGLE = 0u, DEST_LINK = 3u;
constexpr int32_t ST_TOO_SHORT = 1, ST_BAD_HMAC = 2;           // RT_ST_* (include/rnstok.h)
constexpr uint8_t PROOF_FLAGS = 0x03;                          // HEADER_1, broadcast, SINGLE, PROOF

__device__ __forceinline__ const rt_packet_fields &record(const DeliverArgs &a, uint32_t i) {
    return ((const rt_packet_fields *)a.fields)[i];
}
__device__ __forceinline__ u32x4 words16(const uint8_t *p) {
    const uint32_t *w = (const uint32_t *)p;            // a record's hashes sit on words
    return u32x4{w[0], w[1], w[2], w[3]};
}
// The ratchets of row d: [first, first + count) of a.ratchets, none where the
// offsets do not lie inside it.
__device__ __forceinline__ uint32_t ratchets_of(const DeliverArgs &a, uint32_t d, uint32_t *first) {
    const uint32_t r0 = a.ratchet_off[d], r1 = a.ratchet_off[d + 1];
    *first = r0;
    return r0 <= r1 && r1 <= a.n_ratchets ? r1 - r0 : 0u;
}

// Inclusive sums of v over the workgroup (sums that stop at the top of a word).
__device__ __forceinline__ uint32_t block_sums(uint32_t v, uint32_t *sh) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < DD_THREADS; d <<= 1) {
        const uint32_t add = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] = dd_sat_add(sh[t], add);
        __syncthreads();
    }
    return sh[t];
}

__global__ void __launch_bounds__(DD_THREADS) k_deliver_select(const DeliverArgs a, const DeliverLayout l) {
    uint32_t *w = a.work;
    const uint32_t i = blockIdx.x * DD_THREADS + threadIdx.x;
    bool sel = false;
    if (i < a.n) {
        const rt_packet_fields &f = record(a, i);
        int32_t st = RT_DELIVER_NOT_DATA;
        uint32_t row = DD_NONE, nc = 0, tlen = 0;
        uint64_t toff = 0;
        if (f.ok == 1 && f.packet_type == PKT_DATA && f.destination_type != DEST_LINK) {
            const uint32_t s = find(view_of(a.dests), words16(f.destination_hash));
            if (s == a.dests.cap || (row = a.dests.values[s]) >= a.n_dests) {
                st = RT_DELIVER_NO_DESTINATION;
                row = DD_NONE;
            } else if (f.destination_type != DEST_SINGLE) {
                st = RT_DELIVER_TYPE_MISMATCH;                  // Transport.py:2194
            } else if (f.data_len <= DD_EPHEMERAL) {
                st = RT_DELIVER_SHORT;                          // Identity.py:858
            } else {
                uint32_t first;
                nc = ratchets_of(a, row, &first) + ((a.flags[row] & RT_DEST_ENFORCE_RATCHETS) ? 0u : 1u);
                tlen = f.data_len - DD_EPHEMERAL;
                toff = a.pkt_off[i] + f.data_offset + DD_EPHEMERAL;
                st = RT_DELIVER_NOT_OPENED;                     // until a candidate opens it
                // a token that is not well-formed never opens (Token.py:114): no candidate is tried
                sel = nc != 0u && tlen >= 64u && ((tlen - 48u) & 15u) == 0u;
                if (!sel) {
                    // decided here: what Token.decrypt says under a key that is not the token's
                    a.pt_off[i] = toff + a.pt_shift;
                    a.status[i] = tlen <= 32u ? ST_TOO_SHORT : ST_BAD_HMAC;
                    a.pt_len[i] = 0u;
                    tlen = 0u;
                }
            }
        }
        a.deliver_status[i] = st;
        a.destination[i] = (int32_t)row;                        // DD_NONE reads -1
        a.ratchet[i] = -1;
        a.proof_len[i] = 0u;
        w[l.drow + i] = row;
        w[l.ncand + i] = nc;
        w[l.tlen1 + i] = tlen;
        w[l.tlen2 + i] = 0u;
        w[l.dlen + i] = 0u;
        w[l.dkey + i] = 0u;
        ((uint64_t *)(w + l.toff))[i] = toff;
        if (i == 0) {                                           // the last token of the trials: it takes the unused pairs
            w[l.tlen1 + a.n] = 0u;
            w[l.tlen2 + a.n] = 0u;
            ((uint64_t *)(w + l.toff))[a.n] = 0ull;
        }
    }
    const int c = __syncthreads_count(sel);
    if (threadIdx.x == 0) w[l.part + blockIdx.x] = (uint32_t)c;
}

// One workgroup: exclusive sums of the workgroups' values in place, the total
// behind them and in *total_out.
__global__ void __launch_bounds__(DD_THREADS) k_deliver_scan(uint32_t *part, uint32_t nb, uint32_t *total_out) {
    __shared__ uint32_t sh[DD_THREADS];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += DD_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? part[i] : 0u;
        block_sums(v, sh);
        // (exclusive: the inclusive sum of the lane before)
        const uint32_t before = threadIdx.x ? sh[threadIdx.x - 1] : 0u;
        if (i < nb) part[i] = dd_sat_add(carry, before);
        carry = dd_sat_add(carry, sh[DD_THREADS - 1]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[nb] = carry;
        if (total_out) *total_out = carry;
    }
}

__global__ void __launch_bounds__(DD_THREADS) k_deliver_rank(const DeliverArgs a, const DeliverLayout l) {
    __shared__ uint32_t wave_n[DD_THREADS / 64];
    uint32_t *w = a.work;
    const uint32_t i = blockIdx.x * DD_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const bool sel = i < a.n && w[l.tlen1 + i] != 0u;
    const uint64_t bal = __ballot(sel);
    if (lane == 0) wave_n[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (i >= a.n) return;
    uint32_t r = w[l.part + blockIdx.x] + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (uint32_t j = 0; j < wv; ++j) r += wave_n[j];
    w[l.rank + i] = r;                                          // pair_off: the selected frames before i
    if (sel) {
        w[l.pfrm + r] = i;
        w[l.pcand + r] = 0u;
    }
    if (i == 0) {
        w[l.rank + a.n] = w[DD_W_SELECTED];
        w[l.rank + a.n + 1] = a.n;
    }
}

// Three waves per SIMD without scratch, as k_x25519 and k_linkreq_exchange.
// Pairs base .. base + *count - 1; pair p of the launch takes key record row0 + p.
__global__ void __launch_bounds__(DD_THREADS) k_deliver_exchange(const DeliverArgs a, const DeliverLayout l,
                                                                 uint32_t base, uint32_t count_word, uint32_t row0) {
    uint32_t *w = a.work;
    const uint32_t count = w[count_word];
    const uint32_t first = blockIdx.x * DD_THREADS;
    if (first >= count) return;
    const uint32_t p = first + threadIdx.x;
    if (p >= count) return;
    const uint32_t q = base + p;
    const uint32_t i = w[l.pfrm + q], c = w[l.pcand + q], d = w[l.drow + i];
    const rt_packet_fields &f = record(a, i);
    const uint8_t *data = a.pkt + a.pkt_off[i] + f.data_offset;
    uint32_t r0;
    const uint32_t nr = ratchets_of(a, d, &r0);
    uint32_t e[8], u[8], out[8];
    load_words(e, c < nr ? a.ratchets + 32ull * (r0 + c) : a.privates + 32ull * d);
    load_words(u, data);                                        // the ephemeral public key
    // X25519PrivateKey.exchange (X25519.py:139-145) takes the peer's 256-bit
    // value mod p as it is, where x25519_words drops bit 255 as curve25519()
    // does: the bit counts 2^255 = 19 (mod p).  Twice, for a value that passes
    // 2^255 again; the key is public, so nothing here needs to be uniform.
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t cy = 19u * (u[7] >> 31);
        u[7] &= 0x7fffffffu;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            cy += u[k];
            u[k] = (uint32_t)cy;
            cy >>= 32;
        }
    }
    x25519_words(out, e, u);
    store_words((uint8_t *)(w + l.shared) + 32ull * q, out);
    st16((uint8_t *)(w + l.salt) + 16ull * q, ld16(a.id_hashes + 16ull * d));
    w[l.krow + q] = row0 + p;
}

__global__ void __launch_bounds__(DD_THREADS) k_deliver_ask(const DeliverArgs a, const DeliverLayout l) {
    __shared__ uint32_t sh[DD_THREADS];
    uint32_t *w = a.work;
    const uint32_t i = blockIdx.x * DD_THREADS + threadIdx.x;
    uint32_t ask = 0;
    if (i < a.n) {
        if (w[l.tlen1 + i] != 0u && w[l.first1 + i] == DD_NONE) ask = deliver_ask(w[l.ncand + i] - 1u, a.retry);
        w[l.rem + i] = ask;
    }
    block_sums(ask, sh);
    if (threadIdx.x == 0) w[l.part2 + blockIdx.x] = sh[DD_THREADS - 1];
}

__global__ void __launch_bounds__(DD_THREADS) k_deliver_plan(const DeliverArgs a, const DeliverLayout l) {
    __shared__ uint32_t sh[DD_THREADS];
    uint32_t *w = a.work;
    const uint32_t i = blockIdx.x * DD_THREADS + threadIdx.x;
    const uint32_t ask = i < a.n ? w[l.rem + i] : 0u;
    block_sums(ask, sh);
    if (i >= a.n) return;
    const uint32_t start = dd_sat_add(w[l.part2 + blockIdx.x], threadIdx.x ? sh[threadIdx.x - 1] : 0u);
    w[l.start + i] = deliver_pair_off(start, a.retry);
    if (deliver_fits(start, ask, a.retry)) {
        w[l.tlen2 + i] = w[l.tlen1 + i];
        for (uint32_t k = 0; k < ask; ++k) {
            w[l.pfrm + a.n + start + k] = i;
            w[l.pcand + a.n + start + k] = 1u + k;
        }
        // the frames that fit are the first undecided ones: the end of the last is the number of pairs
        atomicMax(w + DD_W_PAIRS2, start + ask);
    } else if (ask) {
        a.deliver_status[i] = RT_DELIVER_DEFERRED;
        w[l.tlen1 + i] = 0u;                                    // nothing more is written for it
    }
    if (i == 0) {
        w[l.start + a.n] = deliver_pair_off(w[l.part2 + deliver_blocks(a.n)], a.retry);
        w[l.start + a.n + 1] = a.retry;
    }
}

__global__ void __launch_bounds__(DD_THREADS) k_deliver_pick(const DeliverArgs a, const DeliverLayout l) {
    uint32_t *w = a.work;
    const uint32_t i = blockIdx.x * DD_THREADS + threadIdx.x;
    if (i >= a.n || w[l.tlen1 + i] == 0u) return;               // not selected, or deferred
    a.pt_off[i] = ((const uint64_t *)(w + l.toff))[i] + a.pt_shift;
    a.status[i] = ST_BAD_HMAC;                                  // unless a candidate opens it
    a.pt_len[i] = 0u;
    uint32_t c = DD_NONE, key = 0;
    if (w[l.first1 + i] != DD_NONE) {
        c = 0u;
        key = w[l.rank + i];
    } else if (w[l.tlen2 + i] != 0u && w[l.first2 + i] != DD_NONE) {
        c = 1u + w[l.first2 + i];
        key = deliver_retry_row(a.max_frames, w[l.start + i] + w[l.first2 + i]);
    }
    if (c == DD_NONE) return;
    uint32_t r0;
    const uint32_t nr = ratchets_of(a, w[l.drow + i], &r0);
    a.ratchet[i] = c < nr ? (int32_t)c : -1;
    w[l.dkey + i] = key;
    w[l.dlen + i] = w[l.tlen1 + i];
}

__global__ void __launch_bounds__(DD_THREADS) k_deliver_finish(const DeliverArgs a, const DeliverLayout l) {
    uint32_t *w = a.work;
    const uint32_t i = blockIdx.x * DD_THREADS + threadIdx.x;
    bool prove = false;
    if (i < a.n && w[l.dlen + i] != 0u) {
        const int32_t st = (int32_t)w[l.dst + i];
        a.status[i] = st;
        a.pt_len[i] = w[l.dpl + i];
        if (st == 0) {
            a.deliver_status[i] = RT_DELIVER_DELIVERED;
            prove = (a.flags[w[l.drow + i]] & RT_LINK_PROVE_ALL) != 0;
            if (prove) a.proof_len[i] = deliver_proof_bytes(a.implicit_proof != 0);
        } else {
            a.ratchet[i] = -1;                                  // bad padding under the key that verified: not opened
        }
    }
    const uint32_t at = wave_reserve(w + DD_W_PROOFS, prove);
    if (prove) w[l.plist + at] = i;
}

// Two waves per SIMD without scratch, as k_prove_sign and k_ifac_sign
__global__ void __launch_bounds__(DD_THREADS, 2) k_deliver_prove(const DeliverArgs a, const DeliverLayout l) {
    const uint32_t *w = a.work;
    const uint32_t count = w[DD_W_PROOFS];
    const uint32_t first = blockIdx.x * DD_THREADS;
    if (first >= count) return;
    const uint32_t j = first + threadIdx.x;
    if (j >= count) return;
    const uint32_t i = w[l.plist + j];
    const rt_packet_fields &f = record(a, i);
    const uint64_t key = 32ull * w[l.drow + i];
    uint32_t sig[16];
    ifac_sign_words(sig, a.seeds + key, a.publics + key, f.packet_hash, PROVE_HASH);
    uint8_t *row = a.proofs + (uint64_t)i * a.proof_stride;
    // addressed to the first 16 bytes of the packet hash (Packet.py:376-381)
    if (a.implicit_proof)
        prove_write<0>(row, PROOF_FLAGS, f.packet_hash, f.packet_hash, sig);
    else
        prove_write<PROVE_HASH>(row, PROOF_FLAGS, f.packet_hash, f.packet_hash, sig);
}

hipError_t keys_and_trials(const DeliverArgs &a, const DeliverLayout &l, uint32_t base, uint32_t pairs,
                           uint32_t count_word, uint32_t row0, uint64_t tlen, uint64_t pair_off, uint64_t first,
                           hipStream_t s) {
    uint32_t *w = a.work;
    hipError_t e;
    if (pairs) {
        hipLaunchKernelGGL(k_deliver_exchange, dim3(deliver_blocks(pairs)), dim3(DD_THREADS), 0, s, a, l, base,
                           count_word, row0);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        HkdfArgs h{};
        h.ikm = (const uint8_t *)(w + l.shared) + 32ull * base; h.ikm_stride = 32; h.ikm_len = 32;
        h.salt = (const uint8_t *)(w + l.salt) + 16ull * base; h.salt_stride = 16; h.salt_len = 16;
        h.length = 64; h.n = pairs;
        if ((e = launch_hkdf_key_setup_rows(h, a.sbox, a.rec, w + l.krow + base, w + count_word, s)) != hipSuccess)
            return e;
    }
    TrialArgs t{};
    t.rec = a.rec; t.tok = a.pkt; t.tok_off = (const uint64_t *)(w + l.toff); t.tok_len = w + tlen;
    t.pair_off = w + pair_off; t.pair_key = w + l.krow + base; t.first = w + first;
    t.n_tok = a.n + 1; t.n_pairs = pairs;
    return launch_verify_trials(t, s);
}

}  // namespace

hipError_t launch_destination_deliver(const DeliverArgs &a, int n_cu, SpareQueue *spare, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const DeliverLayout l = deliver_layout(a.n, a.retry);
    uint32_t *w = a.work;
    const uint32_t nb = deliver_blocks(a.n);
    const dim3 grid(nb), block(DD_THREADS);
    // the counts start at 0 in every call
    hipError_t e = hipMemsetAsync(w, 0, 4ull * DD_W_HEAD, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_deliver_select, grid, block, 0, s, a, l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_deliver_scan, dim3(1), block, 0, s, w + l.part, nb, w + DD_W_SELECTED);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_deliver_rank, grid, block, 0, s, a, l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // pass one: candidate 0 of every selected frame, key records 0 .. m-1
    if ((e = keys_and_trials(a, l, 0u, a.n, DD_W_SELECTED, 0u, l.tlen1, l.rank, l.first1, s)) != hipSuccess) return e;
    // pass two: the remaining candidates of the frames still undecided, as far as the budget goes
    hipLaunchKernelGGL(k_deliver_ask, grid, block, 0, s, a, l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_deliver_scan, dim3(1), block, 0, s, w + l.part2, nb, (uint32_t *)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_deliver_plan, grid, block, 0, s, a, l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = keys_and_trials(a, l, a.n, a.retry, DD_W_PAIRS2, a.max_frames, l.tlen2, l.start, l.first2, s)) !=
        hipSuccess)
        return e;
    hipLaunchKernelGGL(k_deliver_pick, grid, block, 0, s, a, l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    DecArgs d{};
    d.rec = a.rec; d.sbox = a.sbox; d.tok = a.pkt; d.tok_off = (const uint64_t *)(w + l.toff); d.tok_len = w + l.dlen;
    d.key_idx = w + l.dkey; d.pt = a.pt; d.pt_off = a.pt_off; d.out_len = w + l.dpl; d.status = (int32_t *)(w + l.dst);
    d.n = a.n; d.clk = a.clk;
    if ((e = launch_decrypt(d, 14, n_cu, spare, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_deliver_finish, grid, block, 0, s, a, l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_deliver_prove, grid, block, 0, s, a, l);
    return hipGetLastError();
}

}  // namespace rnstok
