// resource_kernels.hip — Resource hashmap (RNS/Resource.py:426-468, 505-506).
//
// A Resource is sent as one large token (Link.encrypt of random_hash(4) ||
// data, Resource.py:399-422) cut into SDU-sized parts (464 B for the default
// MTU, Resource.SDU = Packet.MDU).  Each part is advertised by its map hash
//     map_hash_j = SHA-256(part_j || random_hash)[:4]        (get_map_hash, :505-506)
// and the sender re-rolls random_hash whenever a map hash repeats one of the
// previous COLLISION_GUARD_SIZE (= 2*WINDOW_MAX + HASHMAP_MAX_LEN = 224) map
// hashes (:446-462).  The receiver recomputes the same hash for every part it
// gets (receive_part, :865-866).
//
// k_map_hashes: one lane per part.  The part's full 64-byte blocks are read
// with 16-byte loads (any alignment) and compressed; the last partial block,
// the random hash and the SHA padding are assembled from byte loads.  A part
// of 464 B is 8 compressions.  Parts of many resources can share a launch:
// part j belongs to resource part_res[j] and uses that resource's salt.
// k_map_collisions: for every part, compare its map hash with the previous
// `guard` parts of the same resource (parts of a resource are contiguous and
// in order) and record the first colliding index per resource (atomic min),
// which is where the reference's loop breaks out to re-roll.
#include "token_device.h"
#include "token_launch.h"

namespace rnstok {

namespace {

__global__ __launch_bounds__(256) void k_map_hashes(MapArgs m) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m.n_parts) return;
    const uint8_t *P = m.data + (m.part_off ? m.part_off[j] : (uint64_t)j * m.sdu);
    const uint32_t len = m.part_len ? m.part_len[j] : (uint32_t)min((uint64_t)m.sdu, m.size - (uint64_t)j * m.sdu);
    const uint32_t r = m.part_res ? m.part_res[j] : 0u;
    const uint8_t *S = m.salts + (uint64_t)r * m.salt_len;
    uint32_t h[8];
    sha256_init(h);
    const uint32_t full = len >> 6;
    for (uint32_t b = 0; b < full; ++b) {
        const uint8_t *B = P + 64ull * b;
        uint32_t w[16];
        sha_units(w, ld16(B), ld16(B + 16), ld16(B + 32), ld16(B + 48));
        sha256_compress(h, w);
    }
    // tail: rem bytes of the part || salt || 0x80 || zeros || bit length (1 or 2 blocks)
    const uint32_t rem = len - 64u * full;
    const uint8_t *T = P + 64ull * full;
    const uint64_t bits = ((uint64_t)len + m.salt_len) * 8u;
    sha_tail(h, rem + m.salt_len, bits, Bytes2At{T, rem, S});
    // digest[:4] = big-endian first state word (MAPHASH_LEN = 4)
    const uint32_t d = bswap(h[0]);
    __builtin_memcpy(m.out + 4ull * j, &d, 4);
}

__global__ __launch_bounds__(256) void k_map_collisions(MapArgs m) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m.n_parts) return;
    const uint32_t r = m.part_res ? m.part_res[j] : 0u;
    uint32_t mine, other;
    __builtin_memcpy(&mine, m.out + 4ull * j, 4);
    const uint32_t lo = j > m.guard ? j - m.guard : 0u;
    for (uint32_t k = lo; k < j; ++k) {
        if (m.part_res && m.part_res[k] != r) continue;
        __builtin_memcpy(&other, m.out + 4ull * k, 4);
        if (other == mine) {
            atomicMin(m.first_collision + r, j);
            break;
        }
    }
}

}  // namespace

// The same comparison with the workgroup's window of map hashes (its 256
// parts and the `guard` parts before them) staged in LDS once, instead of
// every lane reading its `guard` predecessors from memory (0.12 ms of
// global reads per 2^20 parts at guard 224).
constexpr uint32_t COLL_TILE = 256, COLL_LDS_GUARD_MAX = 4096;
__global__ __launch_bounds__(COLL_TILE) void k_map_collisions_lds(MapArgs m) {
    extern __shared__ uint32_t win[];                 // [span] hashes, then [span] resource ids
    const uint32_t j0 = blockIdx.x * COLL_TILE, lo = j0 > m.guard ? j0 - m.guard : 0u;
    const uint32_t hi = j0 + COLL_TILE < m.n_parts ? j0 + COLL_TILE : m.n_parts, span = hi - lo;
    uint32_t *res = win + m.guard + COLL_TILE;
    for (uint32_t k = threadIdx.x; k < span; k += COLL_TILE) {
        uint32_t v;
        __builtin_memcpy(&v, m.out + 4ull * (lo + k), 4);
        win[k] = v;
        res[k] = m.part_res ? m.part_res[lo + k] : 0u;
    }
    __syncthreads();
    const uint32_t j = j0 + threadIdx.x;
    if (j >= m.n_parts) return;
    const uint32_t mine = win[j - lo], r = res[j - lo];
    const uint32_t from = j > m.guard ? j - m.guard : 0u;
    if (res[0] == res[span - 1]) {               // the window is one resource (parts are contiguous)
        for (uint32_t k = from; k < j; ++k) {
            if (win[k - lo] == mine) {
                atomicMin(m.first_collision + r, j);
                break;
            }
        }
        return;
    }
    for (uint32_t k = from; k < j; ++k) {
        if (res[k - lo] == r && win[k - lo] == mine) {
            atomicMin(m.first_collision + r, j);
            break;
        }
    }
}

// ------------------------------------------- integrity hash and proof --
//
// Resource.py:436-439 (sender), :698-699 and :759-760 (receiver):
//     hash  = SHA-256(data || random_hash)
//     proof = SHA-256(data || hash)
// Both messages start with `data`, so the full 64-byte blocks of the segment
// are compressed once and the midstate is finished twice, each time over
// (the rem < 64 trailing bytes || a suffix of at most 32 B || padding): one
// or two blocks.  The suffix is held as big-endian words in registers (the
// random hash loaded once, the digest straight from the state words) and
// shifted behind the trailing bytes, so the proof never waits on memory.

namespace {

// The segment's trailing rem (< 64) bytes as big-endian words, zero filled.
// Byte loads: a segment may start and end at any address.
__device__ __forceinline__ void load_tail(uint32_t tw[16], const uint8_t *T, uint32_t rem) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        uint32_t w = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((uint32_t)(4 * k + j) < rem) w |= (uint32_t)T[4 * k + j] << (24 - 8 * j);
        tw[k] = w;
    }
}

// h = SHA-256 state after (tail bytes || sfx[0..slen) || pad), from midstate
// `mid`; total = message length in bytes.  sfx: big-endian words, zero
// beyond slen (<= 32).
__device__ __forceinline__ void finish_suffix(uint32_t h[8], const uint32_t mid[8], const uint32_t tw[16],
                                              uint32_t rem, const uint32_t sfx[8], uint32_t slen, uint64_t total) {
    // suffix || 0x80, as 9 words, then moved right by rem bytes: first by
    // rem & 3 bytes (funnel shifts), then by rem >> 2 words (four select stages)
    uint32_t s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k)
        s[k] = (k < 8 ? sfx[k] : 0u) | ((slen >> 2) == (uint32_t)k ? 0x80000000u >> (8u * (slen & 3u)) : 0u);
    const uint32_t sh = 8u * (rem & 3u), wo = rem >> 2;
    uint32_t x[32];
#pragma unroll
    for (int k = 0; k < 32; ++k)
        x[k] = k < 10 ? __builtin_amdgcn_alignbit(k > 0 ? s[k - 1] : 0u, k < 9 ? s[k] : 0u, sh) : 0u;
#pragma unroll
    for (int bit = 1; bit < 16; bit <<= 1) {
        const bool on = (wo & (uint32_t)bit) != 0u;
#pragma unroll
        for (int k = 31; k >= 0; --k) x[k] = on ? (k >= bit ? x[k - bit] : 0u) : x[k];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] |= tw[k];
    // rem + slen < 96: one or two blocks, in the form this site always had (with it k_resource_hashes is
    // instruction for instruction what it was; sha256_device.h's sha_pad_blocks gives the same count)
    const uint32_t tb = (rem + slen + 8u) / 64u + 1u;
    const uint64_t bits = total * 8u;
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = mid[k];
#pragma nounroll
    for (uint32_t b = 0; b < tb; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = b ? x[16 + k] : x[k];
        if (b + 1u == tb) sha_put_bits(w, bits);
        sha256_compress_fenced(h, w);
    }
}

// 32 bytes at p (any alignment) as big-endian words
__device__ __forceinline__ void load_digest(uint32_t d[8], const uint8_t *p) {
    const u32x4 a = ld16(p), b = ld16(p + 16);
    d[0] = bswap(a.x); d[1] = bswap(a.y); d[2] = bswap(a.z); d[3] = bswap(a.w);
    d[4] = bswap(b.x); d[5] = bswap(b.y); d[6] = bswap(b.z); d[7] = bswap(b.w);
}
__device__ __forceinline__ void store_digest(uint8_t *p, const uint32_t d[8]) {
    st16(p, u32x4{bswap(d[0]), bswap(d[1]), bswap(d[2]), bswap(d[3])});
    st16(p + 16, u32x4{bswap(d[4]), bswap(d[5]), bswap(d[6]), bswap(d[7])});
}

// Segment i from the midstate over its full blocks: both digests, the
// receiver's comparison, the outputs.  T = the first byte after the full blocks.
__device__ __forceinline__ void finish_segment(const ResHashArgs &a, uint32_t i, const uint32_t mid[8],
                                               const uint8_t *T, uint32_t len) {
    const uint32_t rem = len & 63u;
    uint32_t tw[16], sfx[8], hash[8];
    load_tail(tw, T, rem);
    const uint8_t *R = a.random_hashes + (uint64_t)i * a.rh_len;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint32_t w = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((uint32_t)(4 * k + j) < a.rh_len) w |= (uint32_t)R[4 * k + j] << (24 - 8 * j);
        sfx[k] = w;
    }
    finish_suffix(hash, mid, tw, rem, sfx, a.rh_len, (uint64_t)len + a.rh_len);
    store_digest(a.hash + 32ull * i, hash);
    uint32_t bad = 0u;
    if (a.expect_hash) {                 // receiver: the proof is over the advertised hash (:759)
        uint32_t e[8];
        load_digest(e, a.expect_hash + 32ull * i);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            bad |= e[k] ^ hash[k];
            hash[k] = e[k];
        }
    }
    if (a.status) a.status[i] = bad ? 1 : 0;
    if (!a.proof) return;
    uint32_t proof[8];
    finish_suffix(proof, mid, tw, rem, hash, 32u, (uint64_t)len + 32u);
    if (bad) {                           // a corrupt resource is never proved (:719)
#pragma unroll
        for (int k = 0; k < 8; ++k) proof[k] = 0u;
    }
    store_digest(a.proof + 32ull * i, proof);
}

// One lane per segment.
__global__ __launch_bounds__(RES_HASH_THREADS) void k_resource_hashes(ResHashArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint8_t *P = a.data + a.seg_off[i];
    const uint32_t len = a.seg_len[i], full = len >> 6;
    uint32_t h[8];
    sha256_init(h);
    u32x4 b0, b1, b2, b3;
    if (full) { b0 = ld16(P); b1 = ld16(P + 16); b2 = ld16(P + 32); b3 = ld16(P + 48); }
    for (uint32_t b = 0; b < full; ++b) {
        uint32_t w[16];
        sha_units(w, b0, b1, b2, b3);
        if (b + 1u < full) {             // the next block is requested before this one's rounds
            const uint8_t *B = P + 64ull * (b + 1u);
            b0 = ld16(B); b1 = ld16(B + 16); b2 = ld16(B + 32); b3 = ld16(B + 48);
        }
        sha256_compress(h, w);
    }
    finish_segment(a, i, h, P + 64ull * full, len);
}

}  // namespace

// Few segments: one workgroup per segment.  A segment is one serial chain, so
// the lane-per-segment kernel runs a batch of n <= 64 on one wave and keeps
// each block's message schedule on the chain's critical path.  The schedule
// of block b does not depend on the chain: wave 1 (producer) expands W[0..63]
// + K of 64 consecutive blocks at once, one block per lane with coalesced
// 64-B loads, into one half of an LDS ring; wave 0 (consumer) runs only the
// 64 rounds per block from the other half.  (k_decrypt_long2's producer /
// consumer split, token_kernels.hip.)  The producer's chunk costs one
// schedule, the consumer's 64 blocks of rounds, so the producer always waits:
// the handshake is one workgroup barrier per chunk, in uniform control flow,
// instead of spinning flags.  Ring layout: [half][quad q of 16][block l of
// 64] x 16 B, so the producer's lanes write consecutive 16-B units and the
// consumer reads four rounds' words with one broadcast ds_read_b128.
constexpr uint32_t RES_SPLIT_CHUNK = 64, RES_SPLIT_HALF = 16u * RES_SPLIT_CHUNK;    // u32x4 units per half
__global__ __launch_bounds__(128) void k_resource_hashes_split(ResHashArgs a) {
    __shared__ u32x4 ring[2 * RES_SPLIT_HALF];          // 32 KiB
    const uint32_t i = blockIdx.x;                      // grid = n
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint8_t *P = a.data + a.seg_off[i];
    const uint32_t len = a.seg_len[i], full = len >> 6;
    const uint32_t nchunks = (full + RES_SPLIT_CHUNK - 1u) / RES_SPLIT_CHUNK;
    uint32_t h[8];
    // the shared initial state, read here and not through sha256_init: with the call inlined this kernel's
    // prologue is scheduled otherwise and one segment of 1 MiB ran 0.1 % slower, outside the parent's spread
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = SHA256_IV[k];
    // step c: the producer expands chunk c while the consumer runs chunk c - 1
    for (uint32_t c = 0; c <= nchunks; ++c) {
        if (wave == 1u) {
            const uint32_t blk = c * RES_SPLIT_CHUNK + lane;
            if (c < nchunks && blk < full) {
                const uint8_t *B = P + 64ull * blk;
                uint32_t w[16];
                sha_units(w, ld16(B), ld16(B + 16), ld16(B + 32), ld16(B + 48));
                u32x4 *slot = ring + (c & 1u) * RES_SPLIT_HALF + lane;
                constexpr uint32_t Kc[64] = {
                    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
                    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
                    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
                    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
                    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
                    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
                    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
                    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    uint32_t wk[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int t = 4 * q + j;
                        uint32_t wt;
                        if (t < 16) {
                            wt = w[t];
                        } else {
                            const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
                            const uint32_t s0 = xor3(rotr(w15, 7), rotr(w15, 18), w15 >> 3);
                            const uint32_t s1 = xor3(rotr(w2, 17), rotr(w2, 19), w2 >> 10);
                            wt = w[t & 15] = (w[t & 15] + s0 + w[(t + 9) & 15]) + s1;
                        }
                        wk[j] = wt + Kc[t];
                    }
                    slot[q * RES_SPLIT_CHUNK] = u32x4{wk[0], wk[1], wk[2], wk[3]};
                }
            }
        } else if (c > 0u) {
            const uint32_t first = (c - 1u) * RES_SPLIT_CHUNK;
            const uint32_t nb = full - first < RES_SPLIT_CHUNK ? full - first : RES_SPLIT_CHUNK;
            const u32x4 *half = ring + ((c - 1u) & 1u) * RES_SPLIT_HALF;
            for (uint32_t l = 0; l < nb; ++l) {
                uint32_t v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = h[k];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const u32x4 wk4 = half[q * RES_SPLIT_CHUNK + l];
                    const uint32_t wk[4] = {wk4.x, wk4.y, wk4.z, wk4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = 4 * q + j;
                        const uint32_t A = v[(0 - r) & 7], B = v[(1 - r) & 7], C = v[(2 - r) & 7], D = v[(3 - r) & 7];
                        const uint32_t E = v[(4 - r) & 7], F = v[(5 - r) & 7], G = v[(6 - r) & 7], H = v[(7 - r) & 7];
                        const uint32_t t1 = (H + wk[j]) + xor3(rotr(E, 6), rotr(E, 11), rotr(E, 25)) + bfi(E, F, G);
                        const uint32_t t2 = xor3(rotr(A, 2), rotr(A, 13), rotr(A, 22)) + maj3(A, B, C);
                        v[(3 - r) & 7] = D + t1;
                        v[(7 - r) & 7] = t1 + t2;
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) h[k] += v[k];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0u) finish_segment(a, i, h, P + 64ull * full, len);
}

uint32_t resource_hash_split_below() { return RES_HASH_SPLIT_BELOW; }

hipError_t launch_resource_hashes(const ResHashArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    if (a.n < RES_HASH_SPLIT_BELOW)
        hipLaunchKernelGGL(k_resource_hashes_split, dim3(a.n), dim3(128), 0, s, a);
    else
        hipLaunchKernelGGL(k_resource_hashes, dim3((a.n + RES_HASH_THREADS - 1) / RES_HASH_THREADS),
                           dim3(RES_HASH_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_map_hashes(const MapArgs &m, hipStream_t s) {
    if (m.n_parts == 0) return hipSuccess;
    const uint32_t threads = 256, grid = (m.n_parts + threads - 1) / threads;
    hipLaunchKernelGGL(k_map_hashes, dim3(grid), dim3(threads), 0, s, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !m.first_collision) return e;
    e = hipMemsetAsync(m.first_collision, 0xff, 4ull * m.n_res, s);      // "no collision" = 0xffffffff
    if (e != hipSuccess) return e;
    if (m.guard == 0) return hipSuccess;
    if (m.guard <= COLL_LDS_GUARD_MAX)
        hipLaunchKernelGGL(k_map_collisions_lds, dim3((m.n_parts + COLL_TILE - 1) / COLL_TILE), dim3(COLL_TILE),
                           8u * (m.guard + COLL_TILE), s, m);
    else
        hipLaunchKernelGGL(k_map_collisions, dim3(grid), dim3(threads), 0, s, m);
    return hipGetLastError();
}

}  // namespace rnstok
