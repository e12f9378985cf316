// hkdf_kernels.hip — batched HKDF-SHA256 (RNS/Cryptography/HKDF.py:35-62).
//
// Identity.encrypt / __decrypt derive a fresh 64-byte token key per packet
// (Identity.py:837-846, salt = the identity hash, context None) and
// Link.handshake one per link; the derived keys feed Token(key).  Here one
// lane derives one key: the salt becomes the HMAC key (HMAC.py:73-82: zero
// padded to 64 bytes, hashed first when longer), PRK = HMAC(salt, ikm), then
// T_i = HMAC(PRK, T_{i-1} || context || i mod 256) with the PRK's ipad/opad
// midstates computed once.  With 32-byte ikm, 16-byte salt, no context and a
// 64-byte output that is 10 SHA-256 compressions per lane.
//
// The generic instance assembles the messages word by word from byte loads
// (global memory is read once per byte; the previous block T_{i-1} comes from
// registers), so any lengths work.  The common shape (ikm and salt whole
// 4-byte words, ikm <= 52 bytes so PRK's message is one block, no context)
// takes the FAST instance: dword loads and the padded blocks written as
// constants.  Both are VALU-bound like the token MAC.
#include "keysetup_device.h"
#include "token_device.h"
#include "token_launch.h"

namespace rnstok {

namespace {

// Byte q of  pre (4 * npre bytes, put in as words by sha_msg) || seg || tail.
// For q < skip, a byte of pre, q - skip wraps past seg_len and `tail` comes
// back: no load, and sha_msg overwrites those words with pre.
struct SegTailAt {
    const uint8_t *seg;
    uint32_t seg_len, skip, tail;
    __device__ __forceinline__ uint32_t operator()(uint32_t q) const {
        return q - skip < seg_len ? seg[q - skip] : tail;
    }
};

// SHA-256 of  pre[0..npre) words || seg || tail (if tail >= 0)  appended to
// `prior` bytes already absorbed into h (prior = 64 after an HMAC ipad/opad
// block), with the final padding.  npre is 0 or 8 (the previous HKDF block).
__device__ __forceinline__ void sha_msg(uint32_t h[8], uint32_t prior, const uint32_t pre[8], uint32_t npre,
                                     const uint8_t *seg, uint32_t seg_len, int tail) {
    // 32-bit like the byte index of the builder: seg_len is a context, salt or ikm length, far below 2^32
    const uint32_t m = 4u * npre + seg_len + (tail >= 0 ? 1u : 0u);
    const uint64_t bits = ((uint64_t)prior + m) * 8ull;
    const uint32_t nblk = sha_pad_blocks(m);
    for (uint32_t b = 0; b < nblk; ++b) {
        uint32_t w[16];
        sha_pad_block(w, b, m, bits, SegTailAt{seg, seg_len, 4u * npre, (uint32_t)tail});
        if (b == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if ((uint32_t)k < npre) w[k] = pre[k];
        }
        sha256_compress(h, w);
    }
}

// HMAC(salt, .) ipad / opad midstates for key row i.
template <bool FAST, bool FENCED = false>
__device__ __forceinline__ void salt_midstates(const HkdfArgs &a, uint64_t i, uint32_t hi[8], uint32_t ho[8]) {
    // HMAC key = salt; None / empty salt -> 32 zero bytes (HKDF.py:45-46), which
    // zero-pads to the same 64-byte block as an empty key.
    uint32_t key[16];
    const uint32_t sl = a.salt ? a.salt_len : 0u;
    const uint8_t *salt = a.salt ? a.salt + i * a.salt_stride : nullptr;
    if (FAST) {                                       // sl % 4 == 0, sl <= 64
#pragma unroll
        for (int k = 0; k < 16; ++k) key[k] = 4u * k < sl ? ld_be32(salt + 4 * k) : 0u;
    } else if (sl > 64u) {                            // HMAC.py: long keys are hashed first
        uint32_t d[8];
        sha256_init(d);
        sha_msg(d, 0u, nullptr, 0u, salt, sl, -1);
#pragma unroll
        for (int k = 0; k < 16; ++k) key[k] = k < 8 ? d[k] : 0u;
    } else {
        hmac_key_words(key, salt, sl);
    }
    hmac_midstates<FENCED>(key, hi, ho);
}

// SHARED: one salt row for every key (salt_stride 0: a batch to one identity,
// Identity.py:837-846, salt = the identity hash).  Its midstates are then
// computed once per lane and reused over the lane's keys (grid-stride loop).
template <bool FAST, bool SHARED>
__global__ __launch_bounds__(256) void k_hkdf(HkdfArgs a) {
    const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t step = SHARED ? (uint64_t)gridDim.x * blockDim.x : (uint64_t)a.n;   // else one key per lane
    if (first >= a.n) return;
    uint32_t shi[8], sho[8];
    if (SHARED) salt_midstates<FAST>(a, 0, shi, sho);
    for (uint64_t i = first; i < a.n; i += step) {
        const uint8_t *ikm = a.ikm + i * a.ikm_stride;
        uint32_t hi[8], ho[8], inner[8], prk[8];
        if (SHARED) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                hi[k] = shi[k];
                ho[k] = sho[k];
            }
        } else {
            salt_midstates<FAST>(a, i, hi, ho);
        }
        uint32_t key[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) inner[k] = hi[k];
        if (FAST) {                                       // ikm_len % 4 == 0, ikm_len <= 52: one block
            uint32_t w[16];
            hkdf_prk_block(w, ikm, a.ikm_len);
            sha256_compress(inner, w);
        } else {
            sha_msg(inner, 64u, nullptr, 0u, ikm, a.ikm_len, -1);
        }
        hmac_outer(prk, inner, ho);                      // PRK = HMAC(salt, ikm)  (HKDF.py:51)
#pragma unroll
        for (int k = 0; k < 16; ++k) key[k] = k < 8 ? prk[k] : 0u;
        hmac_midstates(key, hi, ho);
        uint32_t t[8];
        uint8_t *out = a.out + (uint64_t)i * a.out_stride;
        for (uint32_t blk = 0, done = 0; done < a.length; ++blk) {
#pragma unroll
            for (int k = 0; k < 8; ++k) inner[k] = hi[k];
            // T_blk = HMAC(PRK, T_{blk-1} || context || (blk+1) % 256)  (HKDF.py:56-60)
            if (FAST) {                                   // T_{blk-1} (32 B, none for blk 0) || counter byte
                uint32_t w[16];
                hkdf_expand_block(w, t, blk);
                sha256_compress(inner, w);
            } else {
                sha_msg(inner, 64u, t, blk ? 8u : 0u, a.context, a.context_len, (int)((blk + 1u) & 255u));
            }
            hmac_outer(t, inner, ho);
            const uint32_t take = a.length - done < 32u ? a.length - done : 32u;
            if (take == 32u) {
                st16(out + done, u32x4{bswap(t[0]), bswap(t[1]), bswap(t[2]), bswap(t[3])});
                st16(out + done + 16, u32x4{bswap(t[4]), bswap(t[5]), bswap(t[6]), bswap(t[7])});
            } else {
                for (uint32_t j = 0; j < take; ++j) {
                    uint32_t wv = t[0];
#pragma unroll
                    for (int k = 1; k < 8; ++k)
                        if ((j >> 2) == (uint32_t)k) wv = t[k];
                    out[done + j] = (uint8_t)(wv >> (24u - 8u * (j & 3u)));
                }
            }
            done += take;
        }
    }
}

// HKDF and key setup fused (the FAST shape: no context, ikm <= 52 B and salt
// <= 64 B in whole aligned words): per-packet keying as Identity.encrypt /
// __decrypt construct it (Identity.py:837-846, Token(hkdf(64, shared_key,
// salt))).  Each lane derives its key into registers — T1 (and T2 for 64-B
// keys) — and builds its record exactly as k_key_setup does from memory, so
// the derived keys never reach HBM and one launch replaces two.  The loop is
// wave-uniform (records are staged per wave); SHARED keeps the salt's
// midstates for the lane's keys.
// ROWS (the link requests' stage and rt_keyset_set_rows_x25519; 64-byte keys,
// one salt row per item): key i goes to record rows[i] of an existing table,
// and with `count` only the first min(*count, a.n) items exist: the grid is
// sized for a.n, and a workgroup past the count leaves its loop at once.
template <bool ROWS>
struct KeyRows {};
template <>
struct KeyRows<true> {
    const uint32_t *rows, *count;
};
template <bool SHARED, int NK, bool ROWS = false>
// 3 waves per SIMD: the 48 KiB staging area admits 3 workgroups per CU
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_hkdf_key_setup(HkdfArgs a, const uint8_t *sbox, uint32_t *rec_out, KeyRows<ROWS> to) {
    __shared__ uint8_t sb[256];
    __shared__ u32x4 stage[4][KS_STAGE_PIECES];
    sb[threadIdx.x] = sbox[threadIdx.x];          // blockDim.x == 256
    __syncthreads();
    if constexpr (ROWS) {
        if (to.count && *to.count < a.n) a.n = *to.count;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t shi[8], sho[8];
    if (SHARED) salt_midstates<true, true>(a, 0, shi, sho);
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t kb = (uint64_t)blockIdx.x * blockDim.x + (wave << 6); kb < a.n; kb += step) {
        const uint32_t kbase = (uint32_t)kb;
        const uint32_t i = kbase + lane < a.n ? kbase + lane : a.n - 1u;   // tail lanes: a copy of the last key
        uint32_t hi[8], ho[8], inner[8], prk[8];
        if (SHARED) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                hi[k] = shi[k];
                ho[k] = sho[k];
            }
        } else {
            salt_midstates<true, true>(a, i, hi, ho);
        }
        const uint8_t *ikm = a.ikm + (uint64_t)i * a.ikm_stride;
        {
            uint32_t w[16];
            hkdf_prk_block(w, ikm, a.ikm_len);
#pragma unroll
            for (int k = 0; k < 8; ++k) inner[k] = hi[k];
            sha256_compress_fenced(inner, w);
        }
        hmac_outer<true>(prk, inner, ho);                      // PRK = HMAC(salt, ikm)  (HKDF.py:51)
        {
            uint32_t key[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) key[k] = k < 8 ? prk[k] : 0u;
            hmac_midstates<true>(key, hi, ho);
        }
        uint32_t t1[8], t2[8];
        {                                                // T1 = HMAC(PRK, 0x01)  (HKDF.py:56-60)
            uint32_t w[16];
            hkdf_expand_block(w, nullptr, 0u);
#pragma unroll
            for (int k = 0; k < 8; ++k) inner[k] = hi[k];
            sha256_compress_fenced(inner, w);
            hmac_outer<true>(t1, inner, ho);
        }
        if (NK == 8) {                                   // T2 = HMAC(PRK, T1 || 0x02)
            uint32_t w[16];
            hkdf_expand_block(w, t1, 1u);
#pragma unroll
            for (int k = 0; k < 8; ++k) inner[k] = hi[k];
            sha256_compress_fenced(inner, w);
            hmac_outer<true>(t2, inner, ho);
        }
        // key = T1 || T2 (big-endian words): sk = key[:HALF], ek = key[HALF:]  (Token.py:61-70)
        uint32_t skw[16], ekw[NK];
#pragma unroll
        for (int k = 0; k < 16; ++k) skw[k] = k < (NK == 8 ? 8 : 4) ? t1[k] : 0u;
#pragma unroll
        for (int k = 0; k < NK; ++k) ekw[k] = bswap(NK == 8 ? t2[k] : t1[4 + k]);
        if constexpr (ROWS)
            key_record<NK, true>(sb, ekw, skw, stage[wave], lane, kbase, a.n, rec_out, to.rows);
        else
            key_record<NK>(sb, ekw, skw, stage[wave], lane, kbase, a.n, rec_out);
    }
}

}  // namespace

// The shape the FAST instances take: no context, ikm (<= 52 B: PRK's message
// is one block) and salt (<= 64 B) in whole aligned words.
static bool hkdf_fast_shape(const HkdfArgs &a) {
    const auto aligned4 = [](const uint8_t *p, uint64_t stride) { return (((uintptr_t)p | stride) & 3u) == 0; };
    return a.context_len == 0 && a.ikm_len % 4u == 0 && a.ikm_len <= 52u && aligned4(a.ikm, a.ikm_stride) &&
           (a.salt == nullptr || (a.salt_len % 4u == 0 && a.salt_len <= 64u && aligned4(a.salt, a.salt_stride)));
}

hipError_t launch_hkdf(const HkdfArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint32_t threads = 256;
    const bool fast = hkdf_fast_shape(a);
    // a shared salt row: 1024 x 256 lanes (4 waves per SIMD on 256 CUs), each
    // computing the salt's midstates once for its n / 262144 keys
    const bool shared = a.salt != nullptr && a.salt_stride == 0 && a.n > 1;
    const uint64_t blocks = ((uint64_t)a.n + threads - 1) / threads;
    const dim3 grid((unsigned)(shared && blocks > 1024u ? 1024u : blocks));
    if (fast && shared)
        hipLaunchKernelGGL((k_hkdf<true, true>), grid, dim3(threads), 0, s, a);
    else if (fast)
        hipLaunchKernelGGL((k_hkdf<true, false>), grid, dim3(threads), 0, s, a);
    else if (shared)
        hipLaunchKernelGGL((k_hkdf<false, true>), grid, dim3(threads), 0, s, a);
    else
        hipLaunchKernelGGL((k_hkdf<false, false>), grid, dim3(threads), 0, s, a);
    return hipGetLastError();
}

constexpr uint64_t FUSED_BLOCKS_PER_CU = 3;   // 48 KiB of staging and 132 VGPRs: 3 workgroups of 4 waves per CU
hipError_t launch_hkdf_key_setup(const HkdfArgs &a, const uint8_t *sbox, uint32_t *rec, int n_cu, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const bool fast = hkdf_fast_shape(a);
    if (!fast || (a.length != 64u && a.length != 32u)) return hipErrorNotSupported;
    const bool shared = a.salt != nullptr && a.salt_stride == 0 && a.n > 1;
    uint64_t blocks = ((uint64_t)a.n + 255u) / 256u;
    if (shared && blocks > FUSED_BLOCKS_PER_CU * (uint64_t)n_cu) blocks = FUSED_BLOCKS_PER_CU * (uint64_t)n_cu;
    const dim3 grid((unsigned)blocks);
    if (a.length == 64u) {
        if (shared)
            hipLaunchKernelGGL((k_hkdf_key_setup<true, 8>), grid, dim3(256), 0, s, a, sbox, rec, KeyRows<false>{});
        else
            hipLaunchKernelGGL((k_hkdf_key_setup<false, 8>), grid, dim3(256), 0, s, a, sbox, rec, KeyRows<false>{});
    } else {
        if (shared)
            hipLaunchKernelGGL((k_hkdf_key_setup<true, 4>), grid, dim3(256), 0, s, a, sbox, rec, KeyRows<false>{});
        else
            hipLaunchKernelGGL((k_hkdf_key_setup<false, 4>), grid, dim3(256), 0, s, a, sbox, rec, KeyRows<false>{});
    }
    return hipGetLastError();
}

hipError_t launch_hkdf_key_setup_rows(const HkdfArgs &a, const uint8_t *sbox, uint32_t *rec, const uint32_t *rows,
                                      const uint32_t *count, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    if (!hkdf_fast_shape(a) || a.length != 64u || (a.salt != nullptr && a.salt_stride == 0)) return hipErrorNotSupported;
    const uint64_t blocks = ((uint64_t)a.n + 255u) / 256u;
    hipLaunchKernelGGL((k_hkdf_key_setup<false, 8, true>), dim3((unsigned)blocks), dim3(256), 0, s, a, sbox, rec,
                       KeyRows<true>{rows, count});
    return hipGetLastError();
}

}  // namespace rnstok
