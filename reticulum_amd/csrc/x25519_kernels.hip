// x25519_kernels.hip — batched X25519 (RNS/Cryptography/X25519.py:49-93).
//
// Identity.encrypt draws an ephemeral key and exchanges it with the target's
// public key per packet (Identity.py:812-820); Identity.decrypt exchanges the
// receiver's key, and every ratchet, with the ephemeral public key at the head
// of the token (Identity.py:861-888).  Here one lane runs one exchange: 255
// ladder steps of 5 multiplies, 4 squarings and one small multiply in
// GF(2^255 - 19), then the inversion (254 squarings, 11 multiplies), all in
// registers (x25519_device.h; the register budget is in DESIGN.md §4.3).  The
// ladder is the same instruction stream for every lane whatever the scalar, so
// a wave never diverges; the work is 64-bit multiply-adds (v_mad_u64_u32) on
// 32-bit limbs, VALU-bound, and memory traffic is 96 bytes per lane.
#include "token_launch.h"
#include "x25519_device.h"

namespace rnstok {

namespace {

constexpr uint32_t X25519_THREADS = 256;

__global__ void __launch_bounds__(X25519_THREADS) k_x25519(const X25519Args a) {
    const uint64_t i = (uint64_t)blockIdx.x * X25519_THREADS + threadIdx.x;
    if (i >= a.n) return;
    uint32_t e[8], u[8], r[8];
    load_words(e, a.scalars + i * a.scalar_stride);
    if (a.points) {
        load_words(u, a.points + (a.point_off ? a.point_off[i] : i * a.point_stride));
    } else {
        u[0] = 9u;                 // the base point: public keys
#pragma unroll
        for (int k = 1; k < 8; ++k) u[k] = 0u;
    }
    x25519_words(r, e, u);
    store_words(a.out + i * a.out_stride, r);
}

}  // namespace

hipError_t launch_x25519(const X25519Args &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const dim3 grid((unsigned)(((uint64_t)a.n + X25519_THREADS - 1) / X25519_THREADS));
    hipLaunchKernelGGL(k_x25519, grid, dim3(X25519_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace rnstok
