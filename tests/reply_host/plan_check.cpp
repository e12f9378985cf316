// plan_check.cpp — reticulum_amd/csrc/reply_host.h built alone with g++ and the
// address and undefined-behaviour sanitizers (tests/test_reply.py builds and
// runs it; no Python is loaded into it).
//
// Without arguments: sweeps the workspace size and the grids of rt_reply_gather
// over frame counts n in {0, 1, 1023, 1024, 1025, 2^20, 2^32 - 1}, sources S in
// 1..4 (and the S the call refuses), capacities 0, 1, n - 1, n, n + 1 and
// 4 n: the workspace holds one word per workgroup of frames and one for their
// sum, every frame and every capacity entry has a lane, the write grid is never
// empty, and a heap buffer of exactly the stated size is touched at every word
// the kernels use (for the sizes that fit in memory).  Also the length rule and
// the counts.  Prints "ok <checks>".
//
// With "plan" as its argument: reads "n S cap" from standard input and prints
// "workspace_bytes count_grid write_grid" for the test to compare.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../reticulum_amd/csrc/reply_host.h"

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

static void check_plan(uint32_t n, uint32_t S, uint32_t cap) {
    const uint64_t bytes = reply_gather_workspace_bytes(n, S);
    const uint64_t nb = reply_count_grid(n), wg = reply_write_grid(n, cap);
    CHECK(bytes % 16 == 0 && bytes >= 8 * (nb + 1) && bytes < 8 * (nb + 1) + 16);
    CHECK(nb * RG_BLOCK >= n && (nb == 0 || (nb - 1) * RG_BLOCK < n));     // every frame has a lane, no idle workgroup
    CHECK(wg >= 1 && wg >= nb);
    CHECK(wg * RG_BLOCK >= n && wg * RG_BLOCK >= cap);                      // and every entry to clear
    CHECK(wg == 1 || (wg - 1) * RG_BLOCK < (n > cap ? n : cap));
    CHECK(nb <= (1u << 22) && wg <= (1u << 22));                             // a grid dimension
    if (nb <= (1u << 12)) {
        // the words the kernels touch: part[b] per workgroup of frames, part[nb]
        std::vector<uint64_t> ws(bytes / 8);
        uint64_t *part = ws.data();
        for (uint64_t b = 0; b < nb; ++b) part[b] = b;
        part[nb] = nb;
        CHECK(part[nb] == nb);
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "plan")) {
        unsigned long long n, S, cap;
        if (scanf("%llu %llu %llu", &n, &S, &cap) != 3) return 2;
        printf("%llu %u %u\n", (unsigned long long)reply_gather_workspace_bytes((uint32_t)n, (uint32_t)S),
               reply_count_grid((uint32_t)n), reply_write_grid((uint32_t)n, (uint32_t)cap));
        return 0;
    }
    const uint32_t ns[] = {0u, 1u, 1023u, 1024u, 1025u, 1u << 20, 0xFFFFFFFFu};
    for (uint32_t n : ns) {
        for (uint32_t S = 1; S <= 4; ++S) {
            const uint64_t caps[] = {0, 1, n ? n - 1ull : 0, n, n + 1ull, 4ull * n};
            for (uint64_t cap : caps)
                if (cap <= 0xFFFFFFFFull) check_plan(n, S, (uint32_t)cap);
            CHECK(reply_gather_workspace_bytes(n, S) == reply_gather_workspace_bytes(n, 1));    // the sources do not size it
        }
        CHECK(reply_gather_workspace_bytes(n, 0) == 0 && reply_gather_workspace_bytes(n, 5) == 0);
        CHECK(reply_gather_workspace_bytes(n, 0xFFFFFFFFu) == 0);
    }
    CHECK(!reply_sources_ok(0) && reply_sources_ok(1) && reply_sources_ok(4) && !reply_sources_ok(5));
    CHECK(reply_blocks(0) == 0 && reply_blocks(1) == 1 && reply_blocks(1024) == 1 && reply_blocks(1025) == 2);
    CHECK(reply_blocks(0xFFFFFFFFull) == (1u << 22));
    CHECK(reply_write_grid(0, 0) == 1 && reply_write_grid(0, 1025) == 2 && reply_write_grid(2049, 1) == 3);
    // a call of fewer frames fits the workspace of more
    for (uint32_t n = 0; n < 5000; n += 7) CHECK(reply_gather_workspace_bytes(n, 1) <= reply_gather_workspace_bytes(n + 7, 1));
    // the length rule: 1 .. min(128, width)
    for (int32_t len = -3; len <= 131; ++len)
        for (uint32_t width : {1u, 16u, 115u, 128u, 160u, 0xFFFFFFFFu}) {
            const bool want = len >= 1 && len <= 128 && (uint32_t)len <= width;
            CHECK(reply_len_ok(len, width) == want);
        }
    CHECK(!reply_len_ok(INT32_MIN, 128) && !reply_len_ok(INT32_MAX, 0xFFFFFFFFu) && !reply_len_ok(1, 0));
    // the counts
    CHECK(reply_written(0, 0) == 0 && reply_written(5, 0) == 0 && reply_written(5, 4) == 4 && reply_written(5, 5) == 5);
    CHECK(reply_written(5, 6) == 5 && reply_written(4ull * 0xFFFFFFFFull, 0xFFFFFFFFu) == 0xFFFFFFFFull);
    CHECK(RG_ROWS_PER_PASS * RG_LANES_PER_ROW == RG_BLOCK && RG_LANES_PER_ROW * 16 == RG_ROW);
    printf("ok %ld\n", checks);
    return 0;
}
