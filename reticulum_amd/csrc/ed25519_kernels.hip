// ed25519_kernels.hip — batched Ed25519 as the reference's internal provider
// computes it (RNS/Cryptography/pure25519/eddsa.py): Identity.validate of an
// announce or a proof, Identity.sign, and the public key of a seed.
//
// One lane runs one item, as k_x25519 does (ed25519_device.h; the register
// budget, the compiler's report and the places where lanes may part are in
// DESIGN.md §4.3b).  A verification is SHA-512 over R ‖ A ‖ message, two
// reductions mod L, two point decodings (one field exponentiation each), 253
// doublings with ≈65 additions for [L]A, and 253 doublings with 253 additions
// for [S]B - [h]A; a signature is three hashes and one or two fixed-base
// multiplications of 255 doublings and additions each; the interface access
// code (k_ifac_sign) is a signature under one key for the batch whose fixed-base
// multiplication is 253 additions from a table of [2^i]B.  All of it is 64-bit
// multiply-adds on 32-bit limbs in registers; memory traffic is the item's key,
// signature and message.
#include "token_launch.h"
#include "ed25519_device.h"

namespace rnstok {

namespace {

constexpr uint32_t ED25519_THREADS = 256;

__global__ void __launch_bounds__(ED25519_THREADS) k_ed25519_verify(const Ed25519VerifyArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * ED25519_THREADS + threadIdx.x;
    if (i >= a.n) return;
    uint32_t pk[8], r[8], s[8];
    load_words(pk, a.pubs + i * a.pub_stride);
    const uint8_t *sig = a.sigs + i * a.sig_stride;
    load_words(r, sig);
    load_words(s, sig + 32);
    const uint32_t len = a.msgs ? a.msg_len[i] : 0u;        // no messages: every one is empty
    const uint8_t *msg = len ? a.msgs + a.msg_off[i] : nullptr;
    a.ok[i] = (uint8_t)ed25519_verify_words(pk, r, s, msg, len);
}

// two waves per SIMD: the signing kernels fit 256 registers without scratch
__global__ void __launch_bounds__(ED25519_THREADS, 2) k_ed25519_sign(const Ed25519SignArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * ED25519_THREADS + threadIdx.x;
    if (i >= a.n) return;
    uint32_t sig[16];
    const uint32_t len = a.msgs ? a.msg_len[i] : 0u;        // no messages: every one is empty
    const uint8_t *msg = len ? a.msgs + a.msg_off[i] : nullptr;
    ed25519_sign_words(sig, a.seeds + i * a.seed_stride, a.pubs ? a.pubs + i * a.pub_stride : nullptr, msg, len);
    uint8_t *out = a.out + i * a.out_stride;
    store_words(out, sig);
    store_words(out + 32, sig + 8);
}

__global__ void __launch_bounds__(ED25519_THREADS, 2) k_ed25519_public(const Ed25519PublicArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * ED25519_THREADS + threadIdx.x;
    if (i >= a.n) return;
    uint32_t seed[8], pub[8];
    load_words(seed, a.seeds + i * a.seed_stride);
    ed25519_public_words(pub, seed);
    store_words(a.out + i * a.out_stride, pub);
}

// The interface access code (Transport.py:1073, :1470-1474): the last ifac_size
// bytes of the interface identity's signature of each packet, one seed and one
// public key for the batch, [r]B through the table of [2^i]B.  CHECK false
// writes the code (zeros for an item without a packet); CHECK true compares it
// with the code the packet carried and marks a mismatch.  Byte k of the
// signature is taken with a constant k in an unrolled loop (a computed word
// index would put sig in scratch); the code is public, so the comparison may
// branch.
template <bool CHECK>
__global__ void __launch_bounds__(ED25519_THREADS, 2) k_ifac_sign(const IfacSignArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * ED25519_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t len = a.pkt_len[i];
    const uint32_t isz = a.ifac_size, from = 64u - isz;
    if (CHECK) {
        if (len == 0u || a.status[i] != 0) return;
    } else if (len == 0u) {
        uint8_t *row = a.ifac_out + i * isz;
        for (uint32_t k = 0; k < isz; ++k) row[k] = 0;
        return;
    }
    // key_stride is 0: an address the compiler cannot prove uniform keeps the
    // seed's two SHA-512 blocks on the vector unit, as in k_ed25519_sign (with a
    // uniform address it moves them to the scalar unit and spills its registers)
    uint32_t sig[16];
    ifac_sign_words(sig, a.seed + i * a.key_stride, a.pub + i * a.key_stride, a.pkt + a.pkt_off[i], len);
    if (CHECK) {
        const uint8_t *row = a.ifac_in + i * isz;
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k)
            if (k >= from) diff |= ((sig[k >> 2] >> (8 * (k & 3))) & 0xffu) ^ row[k - from];
        if (diff) {
            a.status[i] = IFAC_MISMATCH;
            a.pkt_len_io[i] = 0u;
        }
    } else {
        uint8_t *row = a.ifac_out + i * isz;
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k)
            if (k >= from) row[k - from] = (uint8_t)(sig[k >> 2] >> (8 * (k & 3)));
    }
}

dim3 ed_grid(uint32_t n) { return dim3((unsigned)(((uint64_t)n + ED25519_THREADS - 1) / ED25519_THREADS)); }

}  // namespace

hipError_t launch_ed25519_verify(const Ed25519VerifyArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ed25519_verify, ed_grid(a.n), dim3(ED25519_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ed25519_sign(const Ed25519SignArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ed25519_sign, ed_grid(a.n), dim3(ED25519_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ed25519_public(const Ed25519PublicArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ed25519_public, ed_grid(a.n), dim3(ED25519_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ifac_sign(const IfacSignArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    if (a.status)
        hipLaunchKernelGGL(k_ifac_sign<true>, ed_grid(a.n), dim3(ED25519_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(k_ifac_sign<false>, ed_grid(a.n), dim3(ED25519_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace rnstok
