// prove_device.h — the core the proving kernels share (k_prove_sign,
// proof_kernels.hip; k_deliver_prove, destination_kernels.hip): one lane signs a
// 32-byte packet hash (ifac_sign_words) and writes the PROOF packet around the
// signature (prove_write),
//   flags ‖ hops 0 ‖ address (16) ‖ context 0x00 ‖ [packet hash (32)] ‖ signature (64).
// A link's proof is explicit (hash_bytes 32, Link.py:378-389); a destination's
// follows Reticulum.should_use_implicit_proof (hash_bytes 0 or 32,
// Identity.py:942-953).  The signature is ifac_sign_words', that of
// rt_ed25519_sign bit for bit, constant time in the seed.
#pragma once
#include "ed25519_device.h"

namespace rnstok {

constexpr uint32_t PROVE_HASH = 32, PROVE_SIGNATURE = 64, PROVE_HEADER = 19;

// The packet around the signature `sig` (16 little-endian words) of `hash`:
// HASH_BYTES is 32 for an explicit proof, 0 for an implicit one.
template <uint32_t HASH_BYTES>
__device__ __forceinline__ void prove_write(uint8_t *row, uint8_t flags, const uint8_t *address, const uint8_t *hash,
                                            const uint32_t *sig) {
    row[0] = flags;
    row[1] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) row[2 + k] = address[k];
    row[18] = 0;
#pragma unroll
    for (uint32_t k = 0; k < HASH_BYTES; ++k) row[PROVE_HEADER + k] = hash[k];
    // byte k of the signature with a constant k (a computed word index would put sig in scratch)
#pragma unroll
    for (uint32_t k = 0; k < PROVE_SIGNATURE; ++k)
        row[PROVE_HEADER + HASH_BYTES + k] = (uint8_t)(sig[k >> 2] >> (8 * (k & 3)));
}

}  // namespace rnstok
