// plan_check.cpp — reticulum_amd/csrc/lrproof_host.h built alone with g++ and
// the address and undefined-behaviour sanitizers (tests/test_link_proof.py
// builds and runs it; no Python is loaded into it).
//
// Without arguments: sweeps lrproof_plan over every data length 0..130, every
// first signalling byte, a set of the other two, both hop cases and both
// rebalanced cases, and checks what must hold of every answer, of
// lrproof_decisive and lrproof_state; and checks that the signalling bytes
// written into a heap buffer of exactly three bytes decode to what went in.
// Prints "ok <checks>".
//
// With "plan" as its argument: reads lines "data_len b0 b1 b2 hop_match
// rebalanced" from standard input and prints "status verify n_sig confirmed
// mtu" for each, for the test to compare with its own model over the fixture.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../reticulum_amd/csrc/lrproof_host.h"

using namespace rnstok;

static long checks = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        ++checks;                                                     \
        if (!(c)) {                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #c);             \
            exit(1);                                                  \
        }                                                             \
    } while (0)

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "plan")) {
        long len, b0, b1, b2, hop, reb;
        while (scanf("%ld %ld %ld %ld %ld %ld", &len, &b0, &b1, &b2, &hop, &reb) == 6) {
            const LrProofPlan p = lrproof_plan((uint32_t)len, (uint32_t)b0, (uint32_t)b1, (uint32_t)b2, hop != 0, reb != 0);
            printf("%d %u %u %u %u\n", p.status, p.verify, p.n_sig, p.confirmed, p.mtu);
        }
        return 0;
    }
    const uint32_t tails[][2] = {{0, 0}, {0, 1}, {1, 244}, {4, 172}, {255, 255}};
    for (uint32_t len = 0; len <= 130; ++len)
        for (uint32_t b0 = 0; b0 < 256; ++b0)
            for (const auto &t : tails)
                for (int hop = 0; hop < 2; ++hop)
                    for (int reb = 0; reb < 2; ++reb) {
                        const LrProofPlan p = lrproof_plan(len, b0, t[0], t[1], hop != 0, reb != 0);
                        const bool good = len == 96 || len == 99;
                        const uint32_t mode = len > 96 ? b0 >> 5 : 1u;
                        const uint32_t conf = len == 99 ? ((b0 << 16) | (t[0] << 8) | t[1]) & LR_MTU_MASK : 0u;
                        CHECK(p.verify == (uint32_t)(good && mode == 1 && (hop || !reb)));
                        CHECK(p.n_sig == (len == 99 ? 3u : 0u));
                        CHECK(p.confirmed == conf && p.mtu == (conf ? conf : LR_DEFAULT_MTU));
                        if (!hop) {
                            CHECK(p.status == RT_LRPROOF_HOPS);
                        } else if (mode != 1) {
                            CHECK(p.status == RT_LRPROOF_BAD_MODE);
                        } else {
                            CHECK(p.status == (good ? RT_LRPROOF_ACTIVATED : RT_LRPROOF_BAD_SIZE));
                        }
                        for (int sig = 0; sig < 2; ++sig) {
                            const bool d = lrproof_decisive(p, hop != 0, sig != 0);
                            CHECK(d == (hop ? (mode != 1 || good) : (p.verify && sig)));
                            if (!d) continue;
                            const uint32_t s = lrproof_state(p, hop != 0, sig != 0 && p.verify);
                            if (hop && mode != 1) CHECK(s == RT_PENDING_CLOSED);
                            else CHECK(s == (sig ? RT_PENDING_ACTIVE : RT_PENDING_HANDSHAKE));
                        }
                    }
    for (uint32_t mtu : {0u, 1u, 499u, 500u, 1196u, 65535u, 65536u, 262144u, 0x1FFFFFu}) {
        std::vector<uint8_t> sg(3);                 // exactly three bytes on the heap
        lrproof_signalling(sg.data(), mtu);
        const LrProofPlan p = lrproof_plan(99, sg[0], sg[1], sg[2], true, false);
        CHECK(p.status == RT_LRPROOF_ACTIVATED && p.confirmed == mtu && (sg[0] >> 5) == LR_MODE_AES256_CBC);
        // the mode bits are no part of the MTU
        const LrProofPlan q = lrproof_plan(99, sg[0] & 0x1Fu, sg[1], sg[2], true, false);
        CHECK(q.confirmed == mtu && q.status == RT_LRPROOF_BAD_MODE && !q.verify);
    }
    printf("ok %ld\n", checks);
    return 0;
}
