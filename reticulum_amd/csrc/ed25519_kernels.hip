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
// multiplications of 255 doublings and additions each.  All of it is 64-bit
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

}  // namespace rnstok
