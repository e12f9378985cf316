// linkreq_host.h — the fixed-width arithmetic of a link request
// (linkreq_kernels.hip): what the MTU step of Transport.py:2136-2155 and
// Link.validate_request's size and mode rules make of the data's length and its
// three signalling bytes, the signalling bytes of the proof, and where the
// bytes of the 118-byte LRPROOF packet go.  Plain C++ with no HIP in it, for
// the kernels and the host alike, so that tests/linkreq_host/ can build it alone
// under the sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/rnstok.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LR_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define LR_FN inline __attribute__((always_inline))
#endif

namespace rnstok {

constexpr uint32_t LR_DATA = 64;               // Link.ECPUBSIZE: X25519 and Ed25519 public keys
constexpr uint32_t LR_DATA_MTU = 67;           // + Link.LINK_MTU_SIZE
constexpr uint32_t LR_MTU_MASK = 0x1FFFFFu;    // Link.MTU_BYTEMASK
constexpr uint32_t LR_MODE_AES256_CBC = 1;     // the one enabled mode, and the default
constexpr uint32_t LR_DEFAULT_MTU = 500;       // Reticulum.MTU
constexpr uint32_t LR_SIGNED = 83;             // link id (16) ‖ pub (32) ‖ destination's key (32) ‖ signalling (3)
constexpr uint32_t LR_PROOF_HEADER = 19;       // flags, hops, link id (16), context
constexpr uint32_t LR_PROOF_BYTES = 118;       // header ‖ signature (64) ‖ pub (32) ‖ signalling (3)

// What becomes of a request to an accepting destination.  status:
// RT_LINKREQ_ACCEPTED, BAD_SIZE or BAD_MODE.  For an accepted one, mtu is the
// link's and unhashed the number of trailing data bytes the link id leaves out.
struct LinkReqPlan {
    int32_t status;
    uint32_t mtu, unhashed;
};

// data_len: the length of the packet's data; b0..b2: its bytes 64..66 (read
// only where data_len is 67); has_nh_mtu / nh_mtu: the receiving interface's
// next-hop MTU as Transport.py:2138-2141 computes it, or none (no HW_MTU).
LR_FN LinkReqPlan linkreq_plan(uint32_t data_len, uint32_t b0, uint32_t b1, uint32_t b2, bool has_nh_mtu,
                               uint32_t nh_mtu) {
    uint32_t len = data_len, path_mtu = 0, mode = LR_MODE_AES256_CBC;
    if (data_len == LR_DATA_MTU) {
        path_mtu = ((b0 << 16) | (b1 << 8) | b2) & LR_MTU_MASK;
        mode = (b0 & 0xE0u) >> 5;
    }
    if (path_mtu) {                            // Transport.py:2143-2155
        if (!has_nh_mtu) {
            // the three bytes are cut off the data (and stay in the hashed packet): default mode, default MTU
            len = LR_DATA;
            path_mtu = 0;
            mode = LR_MODE_AES256_CBC;
        } else if (nh_mtu < path_mtu) {
            if (mode != LR_MODE_AES256_CBC) return LinkReqPlan{RT_LINKREQ_BAD_MODE, 0u, 0u};   // signalling_bytes raises
            path_mtu = nh_mtu & LR_MTU_MASK;
        }
    }
    if (len != LR_DATA && len != LR_DATA_MTU) return LinkReqPlan{RT_LINKREQ_BAD_SIZE, 0u, 0u};
    if (mode != LR_MODE_AES256_CBC) return LinkReqPlan{RT_LINKREQ_BAD_MODE, 0u, 0u};
    return LinkReqPlan{RT_LINKREQ_ACCEPTED, path_mtu ? path_mtu : LR_DEFAULT_MTU, len - LR_DATA};
}

// Link.signalling_bytes(mtu, MODE_AES256_CBC): the low three bytes of the
// big-endian word  mtu & MTU_BYTEMASK  +  (mode << 5 & MODE_BYTEMASK) << 16.
LR_FN void linkreq_signalling(uint8_t out[3], uint32_t mtu) {
    const uint32_t v = (mtu & LR_MTU_MASK) + (((LR_MODE_AES256_CBC << 5) & 0xE0u) << 16);
    out[0] = (uint8_t)(v >> 16);
    out[1] = (uint8_t)(v >> 8);
    out[2] = (uint8_t)v;
}

// The LRPROOF packet around its signature (Packet.py:170-185), from the 83
// signed bytes `msg`: flags 0x0F (HEADER_1, broadcast, LINK, PROOF), hops 0,
// the link id, context 0xFF in front; the public key and the signalling bytes
// behind.  row[19 .. 83) is the signature's; nothing past byte 117 is written.
LR_FN void linkreq_proof_head(uint8_t *row, const uint8_t *msg) {
    row[0] = 0x0F;
    row[1] = 0;
    for (uint32_t k = 0; k < 16; ++k) row[2 + k] = msg[k];
    row[18] = 0xFF;
}
LR_FN void linkreq_proof_tail(uint8_t *row, const uint8_t *msg) {
    for (uint32_t k = 0; k < 32; ++k) row[LR_PROOF_HEADER + 64 + k] = msg[16 + k];
    for (uint32_t k = 0; k < 3; ++k) row[LR_PROOF_HEADER + 96 + k] = msg[80 + k];
}

}  // namespace rnstok
