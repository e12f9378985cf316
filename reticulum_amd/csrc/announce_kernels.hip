// announce_kernels.hip — Identity.validate_announce (Identity.py:505-606) over
// the records rt_packet_unpack wrote, inside the packets where they lie: the
// step of Transport.inbound that runs an Ed25519 verification per announce
// (Transport.py:1748-1750, :1772).
//
// An announce's data is  public key (64: X25519 ‖ Ed25519) ‖ name hash (10) ‖
// random hash (10) ‖ [ratchet (32), with the context flag] ‖ signature (64) ‖
// app data; `head` is the signature's offset, 84 or 116.  The signed data is
// destination hash ‖ data[:head] ‖ data[head+64:], three pieces of the raw
// packet: the destination hash ends one byte before the data (the context
// byte lies between) and the signature lies between the last two.  The
// verification hashes them where they are (sha512_spans, ed25519_device.h).
//
// Two kernels, because announces are a minority of a read and a verification
// costs ten thousand times what the rest of a record does:
//   k_announce_select  one lane per record.  Settles what needs no signature
//       (no announce, too short), and for the others, the candidates, hashes
//       the identity (SHA-256 of the public key), works out the destination
//       hash the announce ought to carry, leaves VALID or BAD_DESTINATION in
//       status as the verdict should the signature hold, and appends the
//       record's index to a list: one ballot and one atomic add per wave.
//   k_announce_verify  one lane per candidate, the grid sized for n on the
//       host; a block whose first item is at or past the count the first
//       kernel left returns at once.  Overwrites the status with BAD_SIGNATURE
//       where the signature fails, which is the reference's order: the
//       signature is judged first, the destination hash only when it holds.
// The list's order depends on the scheduling; results are scattered back by
// index, so nothing the caller sees depends on it.
#include "table_device.h"
#include "ed25519_device.h"

namespace rnstok {

namespace {

constexpr uint32_t ANNOUNCE_THREADS = 256;
constexpr uint32_t PACKET_ANNOUNCE = 1;                  // Packet.ANNOUNCE
constexpr uint32_t KEYS = 64, NAME_HASH = 10, RANDOM_HASH = 10, RATCHET = 32, SIGNATURE = 64;
constexpr uint32_t DEST_BACK = 17;                       // the destination hash starts 17 bytes before the data
// the workspace: the candidate count in word 0, the indices from word 16 (a line of its own for the counter)
constexpr uint32_t LIST_AT = 16;

__device__ __forceinline__ uint32_t announce_head(const rt_packet_fields &f) {
    return KEYS + NAME_HASH + RANDOM_HASH + (f.context_flag ? RATCHET : 0u);
}

__device__ __forceinline__ uint32_t be32(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// id = SHA-256(data[:64])[:16] (Identity.update_hashes) and
// want = SHA-256(data[64:74] ‖ id)[:16] (Identity.py:563-564), as big-endian words
__device__ void announce_hashes(uint32_t id[4], uint32_t want[4], const uint8_t *data) {
    uint32_t h[8], w[16];
    sha256_init(h);
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = be32(data + 4 * k);
    sha256_compress(h, w);
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = 0u;
    w[0] = 0x80000000u;
    w[15] = 8u * KEYS;
    sha256_compress(h, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) id[k] = h[k];
    // 26 bytes: the name hash, then the identity hash two bytes into word 2
    sha256_init(h);
    w[0] = be32(data + KEYS);
    w[1] = be32(data + KEYS + 4);
    w[2] = ((uint32_t)data[KEYS + 8] << 24) | ((uint32_t)data[KEYS + 9] << 16) | (id[0] >> 16);
    w[3] = (id[0] << 16) | (id[1] >> 16);
    w[4] = (id[1] << 16) | (id[2] >> 16);
    w[5] = (id[2] << 16) | (id[3] >> 16);
    w[6] = (id[3] << 16) | 0x8000u;
#pragma unroll
    for (int k = 7; k < 15; ++k) w[k] = 0u;
    w[15] = 8u * (NAME_HASH + 16u);
    sha256_compress(h, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) want[k] = h[k];
}

__global__ void __launch_bounds__(ANNOUNCE_THREADS) k_announce_select(const AnnounceArgs a) {
    const uint32_t i = blockIdx.x * ANNOUNCE_THREADS + threadIdx.x;
    bool cand = false;
    if (i < a.n) {
        const rt_packet_fields &f = ((const rt_packet_fields *)a.fields)[i];
        int32_t st = RT_ANNOUNCE_NOT_ANNOUNCE;
        u32x4 row = {0u, 0u, 0u, 0u};
        if (f.ok == 1 && f.packet_type == PACKET_ANNOUNCE) {
            st = RT_ANNOUNCE_SHORT;
            if (f.data_len >= announce_head(f) + SIGNATURE) {
                uint32_t id[4], want[4];
                announce_hashes(id, want, a.pkt + a.pkt_off[i] + f.data_offset);
                uint32_t diff = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) diff |= want[k] ^ be32(f.destination_hash + 4 * k);
                st = diff ? RT_ANNOUNCE_BAD_DESTINATION : RT_ANNOUNCE_VALID;
                row = u32x4{bswap(id[0]), bswap(id[1]), bswap(id[2]), bswap(id[3])};
                cand = true;
            }
        }
        a.status[i] = st;
        if (a.identity) st16(a.identity + 16ull * i, row);
    }
    const uint32_t at = wave_reserve(a.work, cand);          // table_device.h
    if (cand) a.work[LIST_AT + at] = i;
}

// One wave per SIMD with the overflow in AGPRs, as k_ed25519_verify has: the
// hash is over before any point exists, so the reader's cuts are not live at
// the peak.
__global__ void __launch_bounds__(ANNOUNCE_THREADS) k_announce_verify(const AnnounceArgs a) {
    const uint32_t count = a.work[0];                    // at most n: one add per candidate
    const uint32_t first = blockIdx.x * ANNOUNCE_THREADS;
    if (first >= count) return;
    const uint32_t j = first + threadIdx.x;
    if (j >= count) return;
    const uint32_t i = a.work[LIST_AT + j];
    const rt_packet_fields &f = ((const rt_packet_fields *)a.fields)[i];
    const uint32_t head = announce_head(f);
    const uint8_t *data = a.pkt + a.pkt_off[i] + f.data_offset;
    uint32_t pk[8], r[8], s[8];
    load_words(pk, data + KEYS / 2);
    load_words(r, data + head);
    load_words(s, data + head + 32);
    const sha512_spans m{data - DEST_BACK, 16u, 1u, 16u + head, SIGNATURE, 16u + f.data_len - SIGNATURE};
    if (!ed25519_verify_spans(pk, r, s, m)) a.status[i] = RT_ANNOUNCE_BAD_SIGNATURE;
}

dim3 announce_grid(uint32_t n) {
    return dim3((unsigned)(((uint64_t)n + ANNOUNCE_THREADS - 1) / ANNOUNCE_THREADS));
}

}  // namespace

uint64_t announce_workspace_bytes(uint32_t n) { return 4ull * (LIST_AT + (uint64_t)n); }

hipError_t launch_announce_validate(const AnnounceArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    // the count starts at 0 in every call
    hipError_t e = hipMemsetAsync(a.work, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_announce_select, announce_grid(a.n), dim3(ANNOUNCE_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_announce_verify, announce_grid(a.n), dim3(ANNOUNCE_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace rnstok
