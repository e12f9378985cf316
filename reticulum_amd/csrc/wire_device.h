// wire_device.h — the device helpers the wire kernels (wire_kernels.hip) share
// with the reply kernels (reply_kernels.hip): the workgroup-wide exclusive scan
// behind frame placement and compaction, the loads that never read past a
// packet's end, and the SHA-256 of a packet's hashable part.
#pragma once
#include "token_device.h"

namespace rnstok {

constexpr uint32_t SCAN_BLOCK = 1024;

// Exclusive prefix sum of v over the workgroup (blockDim.x <= SCAN_BLOCK
// threads, all of them call it); *total receives the workgroup's sum.
static __device__ uint64_t block_exclusive_scan(uint64_t v, uint64_t *total) {
    __shared__ uint64_t sh[SCAN_BLOCK];
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
        const uint64_t add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[blockDim.x - 1];
    __syncthreads();
    return incl - v;
}

// little-endian word of p[i, i+4), bytes at or past `end` read as 0
__device__ __forceinline__ uint32_t ld4_upto(const uint8_t *p, uint64_t i, uint64_t end) {
    if (i + 4 <= end) {
        uint32_t v;
        __builtin_memcpy(&v, p + i, 4);
        return v;
    }
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k)
        if (i + k < end) v |= (uint32_t)p[i + k] << (8 * k);
    return v;
}
// 16 bytes of p[i, i+16), bytes at or past `end` read as 0.  (Loading the
// one or two aligned 16-B blocks that hold a partial window and shifting
// them into place was slower for framing and deframing alike, round 3:
// profiles/r03w_tail_ab/.)
__device__ __forceinline__ u32x4 ld16_upto(const uint8_t *p, uint64_t i, uint64_t end) {
    if (i + 16 <= end) return ld16(p + i);
    u32x4 v = {ld4_upto(p, i, end), ld4_upto(p, i + 4, end), ld4_upto(p, i + 8, end), ld4_upto(p, i + 12, end)};
    return v;
}

// SHA-256 over  first || src[0..len): the full 64-B blocks from 16-B loads
// at src - 1 (that byte is readable: the packet's hop count or the transport
// id's last byte) with `first` put in front, the last block(s) byte by byte.
static __device__ void sha_prefixed(uint8_t first, const uint8_t *src, uint32_t len, uint32_t out[8]) {
    uint32_t h[8];
    sha256_init(h);
    const uint32_t m = len + 1u;
    const uint64_t bits = (uint64_t)m * 8u;
    const uint32_t nfull = m / 64u;
    for (uint32_t b = 0; b < nfull; ++b) {
        const uint8_t *B = src - 1 + 64ull * b;
        uint32_t w[16];
        sha_units(w, ld16(B), ld16(B + 16), ld16(B + 32), ld16(B + 48));
        if (b == 0) w[0] = (w[0] & 0x00FFFFFFu) | ((uint32_t)first << 24);
        sha256_compress(h, w);
    }
    // the 0..63 message bytes left
    sha_tail(h, m - 64u * nfull, bits, PrefixedAt{first, src, 64u * nfull});
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = h[k];
}

// get_hashable_part (Packet.py:342-353): flags & 0x0F || raw[2:] for a
// HEADER_1 packet, || raw[18:] for a HEADER_2 one.  L > 2 (18).
__device__ __forceinline__ void packet_hash_words(const uint8_t *raw, uint32_t L, uint32_t out[8]) {
    const uint32_t from = ((raw[0] >> 6) & 1u) ? 18u : 2u;
    sha_prefixed(raw[0] & 0x0Fu, raw + from, L - from, out);
}

}  // namespace rnstok
