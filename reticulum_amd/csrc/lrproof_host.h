// lrproof_host.h — the fixed-width arithmetic of a link request proof as the
// link's initiator reads it (lrproof_kernels.hip): what the rebalance step of
// Transport.py:2276-2316 and Link.validate_proof's mode, size and MTU rules
// (Link.py:391-451) make of the data's length, its three signalling bytes,
// whether the hop count matches and whether the link was rebalanced before,
// and what a link's state becomes.  Plain C++ with no HIP in it, for the
// kernels and the host alike, so that tests/lrproof_host/ can build it alone
// under the sanitizers.
#pragma once
#include <stdint.h>

#include "linkreq_host.h"

namespace rnstok {

constexpr uint32_t LP_DATA = 96;               // signature (64) ‖ X25519 public key (32)
constexpr uint32_t LP_DATA_MTU = 99;           // + Link.LINK_MTU_SIZE
constexpr uint32_t LP_PEER_PUB = 64;           // where the public key starts
constexpr uint32_t LP_SIGNED = 80;             // link id (16) ‖ peer_pub (32) ‖ destination's key (32), + 0 or 3

// What a proof does to a PENDING link.  status is what the record reads should
// nothing else of the read decide the link first:
//   hop match:    RT_LRPROOF_BAD_MODE (the link closes), RT_LRPROOF_BAD_SIZE
//                 (ignored), or RT_LRPROOF_ACTIVATED with `verify` set: a
//                 signature that fails turns it into RT_LRPROOF_BAD_SIGNATURE;
//   hop mismatch: RT_LRPROOF_HOPS; with `verify` set (good length, right mode,
//                 link not rebalanced before) a signature that holds rebalances
//                 the link and turns it into RT_LRPROOF_ACTIVATED.
// n_sig is the number of signalling bytes behind the 80 signed bytes (0 or 3),
// confirmed the 21-bit MTU they carry (0 without them) and mtu the link's:
// confirmed_mtu or Reticulum.MTU.
struct LrProofPlan {
    int32_t status;
    uint32_t verify, n_sig, confirmed, mtu;
};

// data_len: the length of the packet's data; b0..b2: its bytes 96..98 (b0 read
// where data_len > 96, the others where it is 99).
LR_FN LrProofPlan lrproof_plan(uint32_t data_len, uint32_t b0, uint32_t b1, uint32_t b2, bool hop_match,
                               bool rebalanced) {
    const bool good_len = data_len == LP_DATA || data_len == LP_DATA_MTU;
    const uint32_t mode = data_len > LP_DATA ? (b0 & 0xFFu) >> 5 : LR_MODE_AES256_CBC;   // mode_from_lp_packet
    const bool mode_ok = mode == LR_MODE_AES256_CBC;
    LrProofPlan p{RT_LRPROOF_HOPS, 0u, 0u, 0u, LR_DEFAULT_MTU};
    if (data_len == LP_DATA_MTU) {
        p.n_sig = 3u;
        p.confirmed = ((b0 << 16) | (b1 << 8) | b2) & LR_MTU_MASK;
        if (p.confirmed) p.mtu = p.confirmed;
    }
    if (hop_match) {
        // validate_proof: the mode first (a mismatch raises: CLOSED), then the length
        p.status = !mode_ok ? RT_LRPROOF_BAD_MODE : !good_len ? RT_LRPROOF_BAD_SIZE : RT_LRPROOF_ACTIVATED;
        p.verify = mode_ok && good_len;
    } else {
        // the rebalance: length first, a mode mismatch is caught and logged
        p.verify = good_len && mode_ok && !rebalanced;
    }
    return p;
}

// The record decides its link: no later proof of the read finds it PENDING.
LR_FN bool lrproof_decisive(const LrProofPlan &p, bool hop_match, bool sig_ok) {
    if (hop_match) return p.status != RT_LRPROOF_BAD_SIZE;
    return p.verify && sig_ok;
}

// The link's state behind a decisive record (Link.CLOSED, HANDSHAKE, ACTIVE).
LR_FN uint32_t lrproof_state(const LrProofPlan &p, bool hop_match, bool sig_ok) {
    if (hop_match && p.status == RT_LRPROOF_BAD_MODE) return RT_PENDING_CLOSED;
    return sig_ok ? RT_PENDING_ACTIVE : RT_PENDING_HANDSHAKE;
}

// Link.signalling_bytes(confirmed_mtu, MODE_AES256_CBC) behind the 80 signed
// bytes: re-encoded from the 21-bit value, not copied from the packet.
LR_FN void lrproof_signalling(uint8_t out[3], uint32_t confirmed) { linkreq_signalling(out, confirmed); }

}  // namespace rnstok
