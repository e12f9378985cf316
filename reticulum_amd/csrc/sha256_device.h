// sha256_device.h — SHA-256 (FIPS 180-4), HMAC (RNS/Cryptography/HMAC.py:47-125)
// and the HKDF message blocks (RNS/Cryptography/HKDF.py:35-62), once for every
// kernel: the token MAC, HKDF, IFAC, the packet hash and the Resource hashes.
//
// Two parts.  The first is plain C++ with no HIP builtins: how a message's
// bytes become 16-word blocks, where 0x80 and the bit length go, and the fixed
// blocks of HMAC and HKDF.  tests/sha256_host/pad_check.cpp compiles it with
// g++ and sanitizers.  The second, under hipcc only, is the compression in
// VGPRs and what runs it.
//
// The rule for the end of a message lives in sha_pad_blocks / sha_pad_block:
// m message bytes are followed by 0x80, zeros up to 56 mod 64, and the 64-bit
// big-endian bit length.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SHA_FN __host__ __device__ inline __attribute__((always_inline))
#define SHA_CONST static __device__ const
#else
#define SHA_FN inline __attribute__((always_inline))
#define SHA_CONST static constexpr
#endif
#if defined(__clang__)
#define SHA_UNROLL _Pragma("unroll")
#else
#define SHA_UNROLL
#endif

namespace rnstok {

// ------------------------------------------------- message blocks (plain) --

SHA_FN uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

// The initial hash value.
SHA_CONST uint32_t SHA256_IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
SHA_FN void sha256_init(uint32_t h[8]) {
    SHA_UNROLL
    for (int k = 0; k < 8; ++k) h[k] = SHA256_IV[k];
}

// The bit length, in the last two words of a message's last block.
SHA_FN void sha_put_bits(uint32_t w[16], uint64_t bits) {
    w[14] = (uint32_t)(bits >> 32);
    w[15] = (uint32_t)bits;
}

// Blocks taken by the last m bytes of a message and its padding: the whole
// blocks of m, then one more where 0x80 and the length fit behind the rest
// (at most 55 bytes), two where they do not.
SHA_FN constexpr uint32_t sha_pad_blocks(uint32_t m) { return m / 64u + ((m & 63u) + 9u <= 64u ? 1u : 2u); }

// Block b (< sha_pad_blocks(m)) of  at(0) .. at(m-1) || 0x80 || zeros || bits
// as big-endian words; bits is the length of the whole message, what was
// hashed before at(0) included.  at(q) is called for q < m only.
template <class ByteAt>
SHA_FN void sha_pad_block(uint32_t w[16], uint32_t b, uint32_t m, uint64_t bits, ByteAt at) {
    SHA_UNROLL
    for (int k = 0; k < 16; ++k) {
        uint32_t v = 0;
        SHA_UNROLL
        for (int j = 0; j < 4; ++j) {
            const uint32_t q = 64u * b + 4u * k + j;
            v = (v << 8) | (q < m ? (uint32_t)at(q) : (q == m ? 0x80u : 0u));
        }
        w[k] = v;
    }
    if (b + 1u == sha_pad_blocks(m)) sha_put_bits(w, bits);
}

// Byte functors for sha_pad_block: bytes at p; a[0..alen) then b; and `first`
// then src (the packet hash: Packet.get_hashable_part) from byte `base` on.
struct BytesAt {
    const uint8_t *p;
    SHA_FN uint32_t operator()(uint32_t q) const { return p[q]; }
};
struct Bytes2At {
    const uint8_t *a;
    uint32_t alen;
    const uint8_t *b;
    SHA_FN uint32_t operator()(uint32_t q) const { return q < alen ? a[q] : b[q - alen]; }
};
struct PrefixedAt {
    uint32_t first;
    const uint8_t *src;
    uint32_t base;
    SHA_FN uint32_t operator()(uint32_t q) const { return base + q == 0u ? first : src[base + q - 1u]; }
};

// HMAC: the key block under a pad.  key: NW big-endian words, zeros beyond.
constexpr uint32_t HMAC_IPAD = 0x36363636u, HMAC_OPAD = 0x5c5c5c5cu;
template <int NW = 16>
SHA_FN void hmac_pad_block(uint32_t w[16], const uint32_t *key, uint32_t pad) {
    SHA_UNROLL
    for (int k = 0; k < 16; ++k) w[k] = k < NW ? key[k] ^ pad : pad;
}

// A key of len <= 64 bytes as 16 big-endian words, zero padded (HMAC.py:73-82).
SHA_FN void hmac_key_words(uint32_t key[16], const uint8_t *bytes, uint32_t len) {
    SHA_UNROLL
    for (int k = 0; k < 16; ++k) {
        uint32_t v = 0;
        SHA_UNROLL
        for (int j = 0; j < 4; ++j) {
            const uint32_t q = 4u * k + j;
            v = (v << 8) | (q < len ? bytes[q] : 0u);
        }
        key[k] = v;
    }
}

// HMAC outer hash: the one block after the opad block, inner digest || padding,
// a message of HMAC_OUTER_BITS.  (hmac_outer and hmac_finish below fill the
// same block in their own statement order: with this call in its place the
// encrypt and decrypt kernels kept their instructions and changed their
// register assignment.)
constexpr uint32_t HMAC_OUTER_BITS = (64u + 32u) * 8u;
SHA_FN void hmac_outer_block(uint32_t w[16], const uint32_t inner[8]) {
    SHA_UNROLL
    for (int k = 0; k < 8; ++k) w[k] = inner[k];
    w[8] = 0x80000000u;
    SHA_UNROLL
    for (int k = 9; k < 15; ++k) w[k] = 0u;
    w[15] = HMAC_OUTER_BITS;
}

// big-endian word at a 4-byte aligned address
SHA_FN uint32_t ld_be32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
    return bswap(v);
}

// HKDF extract, PRK = HMAC(salt, ikm): the inner hash's one block after the
// ipad block, for an aligned ikm of whole words, ikm_len <= 52.
SHA_FN void hkdf_prk_block(uint32_t w[16], const uint8_t *ikm, uint32_t ikm_len) {
    SHA_UNROLL
    for (int k = 0; k < 14; ++k)
        w[k] = 4u * k < ikm_len ? ld_be32(ikm + 4 * k) : (4u * k == ikm_len ? 0x80000000u : 0u);
    w[14] = 0u;
    w[15] = (64u + ikm_len) * 8u;
}

// HKDF expand with no context, T_blk = HMAC(PRK, T_{blk-1} || (blk+1) % 256)
// (HKDF.py:56-60): the inner hash's one block after the ipad block.  prev =
// T_{blk-1}, not read for blk 0.
SHA_FN void hkdf_expand_block(uint32_t w[16], const uint32_t *prev, uint32_t blk) {
    const uint32_t ctr = (((blk + 1u) & 255u) << 24) | 0x00800000u;
    SHA_UNROLL
    for (int k = 0; k < 16; ++k) w[k] = 0u;
    if (blk) {
        SHA_UNROLL
        for (int k = 0; k < 8; ++k) w[k] = prev[k];
        w[8] = ctr;
        w[15] = (64u + 33u) * 8u;
    } else {
        w[0] = ctr;
        w[15] = (64u + 1u) * 8u;
    }
}

#if defined(__HIPCC__)

// ------------------------------------------------- compression (device) --

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// v_bitop3_b32 (gfx950): any 3-input bitwise function in ONE full-rate VALU op
// (measured: tools/valu_peak.hip — v_bitop3 issues at the v_add/v_xor rate
// while v_perm/v_alignbit/v_bfi/v_add3/v_and_or/SDWA issue at half rate).
// Truth table index = {S0,S1,S2} bits, i.e. TT = f(0xF0, 0xCC, 0xAA).
template <uint32_t TT>
__device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
}
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return bitop3<0x96>(a, b, c); }
__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) { return bitop3<0xE8>(a, b, c); }
// (m & a) | (~m & b): SHA-256 Ch(e,f,g) and byte merges
__device__ __forceinline__ uint32_t bfi(uint32_t m, uint32_t a, uint32_t b) { return bitop3<0xCA>(m, a, b); }
// (a & m) | c
__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t m, uint32_t c) { return bitop3<0xEA>(a, m, c); }

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }

// SHA-256 compression split into rounds so its VALU chain can be interleaved
// with an AES chain (whose time is LDS latency) inside one wave.  The eight
// working variables rotate through v[] by index instead of by moves:
// at round i, a = v[(0-i)&7], b = v[(1-i)&7], ..., h = v[(7-i)&7].
struct Sha256 {
    uint32_t v[8];
    uint32_t w[16];

    __device__ __forceinline__ void start(const uint32_t h[8]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = h[k];
    }
    __device__ __forceinline__ void round(int i) {
        constexpr uint32_t K[64] = {
            0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
            0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
            0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
            0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
            0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
            0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
            0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
            0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
        uint32_t wi;
        if (i < 16) {
            wi = w[i];
        } else {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            const uint32_t s0 = xor3(rotr(w15, 7), rotr(w15, 18), w15 >> 3);
            const uint32_t s1 = xor3(rotr(w2, 17), rotr(w2, 19), w2 >> 10);
            wi = w[i & 15] = (w[i & 15] + s0 + w[(i + 9) & 15]) + s1;
        }
        const uint32_t a = v[(0 - i) & 7], b = v[(1 - i) & 7], c = v[(2 - i) & 7], d = v[(3 - i) & 7];
        const uint32_t e = v[(4 - i) & 7], f = v[(5 - i) & 7], g = v[(6 - i) & 7], h = v[(7 - i) & 7];
        const uint32_t t1 = (h + K[i] + wi) + xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25)) + bfi(e, f, g);
        const uint32_t t2 = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22)) + maj3(a, b, c);
        v[(3 - i) & 7] = d + t1;      // new e
        v[(7 - i) & 7] = t1 + t2;     // new a
    }
    __device__ __forceinline__ void finish(uint32_t h[8]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] += v[k];
    }
};

__device__ __forceinline__ void sha256_compress(uint32_t h[8], const uint32_t w[16]) {
    Sha256 S;
    S.start(h);
#pragma unroll
    for (int k = 0; k < 16; ++k) S.w[k] = w[k];
#pragma unroll
    for (int i = 0; i < 64; ++i) S.round(i);
    S.finish(h);
}

// The same with the scheduler fenced every 4 rounds: a message whose words
// are all known up front otherwise has its whole schedule (W[16..63] + K)
// hoisted ahead of the rounds, 64 live values; kernels that run many
// compressions back to back at 3 waves/SIMD (k_hkdf_key_setup) spilled them.
__device__ __forceinline__ void sha256_compress_fenced(uint32_t h[8], const uint32_t w[16]) {
    Sha256 S;
    S.start(h);
#pragma unroll
    for (int k = 0; k < 16; ++k) S.w[k] = w[k];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        S.round(i);
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    S.finish(h);
}

// The last m bytes at(0..m-1) of a message of `bits` bits, and its padding,
// into h.  Sites that keep one compression for several steps (k_ifac's mask,
// hmac_finish) call sha_pad_block themselves.
template <class ByteAt>
__device__ __forceinline__ void sha_tail(uint32_t h[8], uint32_t m, uint64_t bits, ByteAt at) {
    const uint32_t nblk = sha_pad_blocks(m);
    for (uint32_t b = 0; b < nblk; ++b) {
        uint32_t w[16];
        sha_pad_block(w, b, m, bits, at);
        sha256_compress(h, w);
    }
}

// SHA-256 message words from four 16-B units (big-endian words).
__device__ __forceinline__ void sha_units(uint32_t w[16], u32x4 a, u32x4 b, u32x4 c, u32x4 d) {
    w[0] = bswap(a.x); w[1] = bswap(a.y); w[2] = bswap(a.z); w[3] = bswap(a.w);
    w[4] = bswap(b.x); w[5] = bswap(b.y); w[6] = bswap(b.z); w[7] = bswap(b.w);
    w[8] = bswap(c.x); w[9] = bswap(c.y); w[10] = bswap(c.z); w[11] = bswap(c.w);
    w[12] = bswap(d.x); w[13] = bswap(d.y); w[14] = bswap(d.z); w[15] = bswap(d.w);
}

// Final padded SHA block holding fu (0..3) 16-B units s0..s2 of the message,
// then 0x80, zeros and the 64-bit big-endian bit length.
__device__ __forceinline__ void sha_final_units(uint32_t h[8], uint32_t fu, u32x4 s0, u32x4 s1, u32x4 s2,
                                                uint64_t bits) {
    uint32_t w[16];
    const u32x4 z = {0u, 0u, 0u, 0u};
    sha_units(w, fu > 0 ? s0 : z, fu > 1 ? s1 : z, fu > 2 ? s2 : z, z);
#pragma unroll
    for (int k = 0; k < 16; k += 4) {
        uint32_t hit = (uint32_t)(4 * fu) == (uint32_t)k ? 0x80000000u : 0u;
        w[k] |= hit;
    }
    w[14] = (uint32_t)(bits >> 32);
    w[15] |= (uint32_t)bits;
    sha256_compress(h, w);
}

// Final padded block of an HMAC inner hash: the first fu (0..3) 16-B units of
// u (big-endian words), 0x80, zeros, the 64-bit message length in bits.
__device__ __forceinline__ void sha_final_block(uint32_t fin[16], const uint32_t u[16], uint32_t fu, uint64_t bits) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
        fin[k] = (uint32_t)k < 4u * fu ? u[k] : ((uint32_t)k == 4u * fu ? 0x80000000u : 0u);
    fin[14] = (uint32_t)(bits >> 32);
    fin[15] = (uint32_t)bits;
}

// ------------------------------------------------------------------ HMAC --

// HMAC ipad / opad midstates for a key (HMAC.py:73-82).  FENCED: one
// compression at a time, no interleaving of the two chains (register
// pressure in k_hkdf_key_setup).
template <bool FENCED = false>
__device__ __forceinline__ void hmac_midstates(const uint32_t key[16], uint32_t hi[8], uint32_t ho[8]) {
    sha256_init(hi);
    sha256_init(ho);
    if (FENCED) {
        uint32_t w[16];
        hmac_pad_block(w, key, HMAC_IPAD);
        sha256_compress_fenced(hi, w);
        hmac_pad_block(w, key, HMAC_OPAD);
        sha256_compress_fenced(ho, w);
    } else {
        uint32_t wi[16], wo[16];
        hmac_pad_block(wi, key, HMAC_IPAD);
        hmac_pad_block(wo, key, HMAC_OPAD);
        sha256_compress(hi, wi);
        sha256_compress(ho, wo);
    }
}

// HMAC outer hash: tag = SHA256(opad_state, inner_digest || pad), 96-byte message.
template <bool FENCED = false>
__device__ __forceinline__ void hmac_outer(uint32_t tag[8], const uint32_t inner[8], const uint32_t opad[8]) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) { w[i] = inner[i]; tag[i] = opad[i]; }
    w[8] = 0x80000000u;
#pragma unroll
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = HMAC_OUTER_BITS;
    if (FENCED)
        sha256_compress_fenced(tag, w);
    else
        sha256_compress(tag, w);
}

// The last compressions of an HMAC through ONE inlined sha256_compress, so a
// kernel's packet loop carries a single copy of the 64 unrolled rounds:
// k = first..2 runs the full block `blk` (k = 0), the final padded block `fin`
// (k = 1) and the outer hash of the inner digest under the opad midstate
// (k = 2).  h: the inner state in, the tag out.
__device__ __forceinline__ void hmac_finish(uint32_t h[8], uint32_t first, const uint32_t blk[16],
                                            const uint32_t fin[16], const uint32_t opad[8]) {
#pragma nounroll
    for (uint32_t k = first; k < 3u; ++k) {
        uint32_t w[16];
        if (k == 2u) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                w[j] = h[j];
                h[j] = opad[j];
            }
            w[8] = 0x80000000u;
#pragma unroll
            for (int j = 9; j < 15; ++j) w[j] = 0u;
            w[15] = HMAC_OUTER_BITS;
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = k == 0u ? blk[j] : fin[j];
        }
        sha256_compress(h, w);
    }
}

#endif  // __HIPCC__

}  // namespace rnstok
