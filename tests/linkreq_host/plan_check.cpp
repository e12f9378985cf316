// plan_check.cpp — reticulum_amd/csrc/linkreq_host.h built alone with g++ and
// the address and undefined-behaviour sanitizers (tests/test_link_accept.py
// builds and runs it; no Python is loaded into it).
//
// Without arguments: sweeps linkreq_plan over every data length 0..130, every
// first signalling byte, a set of the other two and of next-hop MTUs, and checks
// what must hold of every answer; checks that the signalling bytes decode to
// what went in; and writes the packet's head and tail into a heap row of
// exactly 118 bytes, where a byte too far is an error the sanitizer reports,
// with the signature's 64 bytes left as they were.  Prints "ok <checks>".
//
// With "plan" as its argument: reads lines "data_len b0 b1 b2 nh_mtu" (nh_mtu
// -1: none) from standard input and prints "status mtu unhashed" for each, for
// the test to compare with its own model over the fixture.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../reticulum_amd/csrc/linkreq_host.h"

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
        long len, b0, b1, b2, nh;
        while (scanf("%ld %ld %ld %ld %ld", &len, &b0, &b1, &b2, &nh) == 5) {
            const LinkReqPlan p = linkreq_plan((uint32_t)len, (uint32_t)b0, (uint32_t)b1, (uint32_t)b2, nh >= 0,
                                               nh >= 0 ? (uint32_t)nh : 0u);
            printf("%d %u %u\n", p.status, p.mtu, p.unhashed);
        }
        return 0;
    }
    const uint32_t tails[][2] = {{0, 0}, {0, 1}, {1, 244}, {4, 172}, {255, 255}};
    const long nhs[] = {-1, 0, 1, 499, 500, 501, 1196, 262144, 0x1FFFFF, 0x200000, 0xFFFFFFFFl};
    for (uint32_t len = 0; len <= 130; ++len)
        for (uint32_t b0 = 0; b0 < 256; ++b0)
            for (const auto &t : tails)
                for (long nh : nhs) {
                    const LinkReqPlan p = linkreq_plan(len, b0, t[0], t[1], nh >= 0, nh >= 0 ? (uint32_t)nh : 0u);
                    const uint32_t path = len == 67 ? ((b0 << 16) | (t[0] << 8) | t[1]) & LR_MTU_MASK : 0u;
                    const uint32_t mode = len == 67 ? b0 >> 5 : 1u;
                    CHECK(p.status == RT_LINKREQ_ACCEPTED || p.status == RT_LINKREQ_BAD_SIZE ||
                          p.status == RT_LINKREQ_BAD_MODE);
                    if (len != 64 && len != 67) CHECK(p.status == RT_LINKREQ_BAD_SIZE);
                    if (len == 64) CHECK(p.status == RT_LINKREQ_ACCEPTED && p.mtu == LR_DEFAULT_MTU && p.unhashed == 0);
                    if (len == 67 && path && nh < 0)       // cut off: whatever the mode bits say
                        CHECK(p.status == RT_LINKREQ_ACCEPTED && p.mtu == LR_DEFAULT_MTU && p.unhashed == 0);
                    else if (len == 67)
                        CHECK((p.status == RT_LINKREQ_ACCEPTED) == (mode == 1));
                    if (p.status == RT_LINKREQ_ACCEPTED) {
                        CHECK(p.mtu >= 1 && p.mtu <= LR_MTU_MASK);
                        CHECK(p.unhashed == 0 || p.unhashed == 3);
                        if (len == 67 && nh >= 0) {
                            CHECK(p.unhashed == 3);
                            if (path && (uint32_t)nh >= path) CHECK(p.mtu == path);
                            if (path && (uint32_t)nh < path)
                                CHECK(p.mtu == (((uint32_t)nh & LR_MTU_MASK) ? ((uint32_t)nh & LR_MTU_MASK) : LR_DEFAULT_MTU));
                            if (!path) CHECK(p.mtu == LR_DEFAULT_MTU);
                        }
                    } else {
                        CHECK(p.mtu == 0 && p.unhashed == 0);
                    }
                }
    for (uint32_t mtu : {0u, 1u, 499u, 500u, 1196u, 65535u, 65536u, 262144u, 0x1FFFFFu, 0x200000u, 0xFFFFFFFFu}) {
        std::vector<uint8_t> sg(3);                 // exactly three bytes on the heap
        linkreq_signalling(sg.data(), mtu);
        const uint32_t v = ((uint32_t)sg[0] << 16) | ((uint32_t)sg[1] << 8) | sg[2];
        CHECK((v & LR_MTU_MASK) == (mtu & LR_MTU_MASK));
        CHECK((sg[0] >> 5) == LR_MODE_AES256_CBC);
        // what the responder sends is what an initiator's request would have to carry to be accepted as it is
        const LinkReqPlan p = linkreq_plan(67, sg[0], sg[1], sg[2], true, 0xFFFFFFFFu);
        CHECK(p.status == RT_LINKREQ_ACCEPTED && p.mtu == ((mtu & LR_MTU_MASK) ? (mtu & LR_MTU_MASK) : LR_DEFAULT_MTU));
    }
    {
        std::vector<uint8_t> msg(LR_SIGNED), row(LR_PROOF_BYTES, 0xA5);
        for (uint32_t k = 0; k < LR_SIGNED; ++k) msg[k] = (uint8_t)(k + 1);
        linkreq_proof_head(row.data(), msg.data());
        linkreq_proof_tail(row.data(), msg.data());
        CHECK(row[0] == 0x0F && row[1] == 0 && row[18] == 0xFF);
        for (uint32_t k = 0; k < 16; ++k) CHECK(row[2 + k] == msg[k]);
        for (uint32_t k = 0; k < 64; ++k) CHECK(row[LR_PROOF_HEADER + k] == 0xA5);
        for (uint32_t k = 0; k < 32; ++k) CHECK(row[83 + k] == msg[16 + k]);
        for (uint32_t k = 0; k < 3; ++k) CHECK(row[115 + k] == msg[80 + k]);
        CHECK(LR_PROOF_HEADER + 64 + 32 + 3 == LR_PROOF_BYTES);
    }
    printf("ok %ld\n", checks);
    return 0;
}
