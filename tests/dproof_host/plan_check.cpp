// plan_check.cpp — reticulum_amd/csrc/dproof_host.h built alone with g++ and the
// address and undefined-behaviour sanitizers (tests/test_destination_proof.py
// builds and runs it; no Python is loaded into it).
//
// Without arguments: sweeps the work lists' layout over record counts, table
// capacities and receipt counts (0, 1, the workgroup edges, large ones), checks
// that every list is 16-byte aligned, that no two overlap, that all lie inside
// the stated size and that a call of fewer records fits, and touches every word
// of a heap buffer of exactly that size through the layout; sweeps the scan
// budget at 0, 1, L - 1, L, 2L - 1 and 2L and with L = 0 against a plain loop
// over the strays.  Prints "ok <checks>".
//
// With "budget" as its argument: reads "scan_trials L strays" from standard
// input and prints, per stray in rank order, "fits deferred", then "frames
// pairs", for the test to compare with its own model.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../reticulum_amd/csrc/dproof_host.h"

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

static void check_layout(uint32_t n, uint32_t cap, uint32_t max_receipts) {
    const DproofLayout l = dproof_layout(n, cap, max_receipts);
    const uint64_t N = n, nb = dproof_blocks(n);
    const std::pair<uint64_t, uint64_t> lists[] = {{0, DP_W_HEAD}, {l.part, nb + 1}, {l.start, nb + 1}, {l.cand, N},
                                                   {l.slot, N},    {l.rid, N},       {l.stray, N},      {l.slist, N},
                                                   {l.live, cap},  {l.slot_of, max_receipts}};
    uint64_t end = 0;
    for (const auto &a : lists) {
        CHECK(a.first % 4 == 0);                       // 16-byte aligned
        CHECK(a.first >= end);                         // in order, none overlaps the one before
        end = a.first + a.second;
        CHECK(4 * end <= l.bytes);
    }
    CHECK(l.bytes % 16 == 0);
    CHECK(l.bytes == dproof_workspace_bytes(n, cap, max_receipts));
    if (n) CHECK(dproof_workspace_bytes(n - 1, cap, max_receipts) <= l.bytes);     // a smaller call fits
    if (l.bytes <= (64u << 20)) {
        // every word of every list written once, in a heap buffer of exactly the stated size
        std::vector<uint32_t> buf(l.bytes / 4, 0u);
        for (const auto &a : lists)
            for (uint64_t k = 0; k < a.second; ++k) buf[a.first + k] += 1u;
        for (uint32_t v : buf) CHECK(v <= 1u);
    }
}

// only whole frames, in rank order; after the first that does not fit none does
static void check_budget(uint32_t strays, uint32_t L, uint32_t trials) {
    uint64_t used = 0;
    uint32_t frames = 0;
    bool stopped = false;
    for (uint32_t r = 0; r < strays; ++r) {
        const bool want = L != 0 && !stopped && used + L <= trials;
        CHECK(dproof_fits(r, L, trials) == want);
        CHECK(dproof_deferred(r, L, trials) == (L != 0 && !want));
        if (want) {
            used += L;
            ++frames;
        } else {
            stopped = true;
        }
    }
    CHECK(dproof_frames(strays, L, trials) == frames);
    CHECK(dproof_pairs(strays, L, trials) == used);
    CHECK(used <= trials);
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "budget")) {
        long trials, L, strays;
        if (scanf("%ld %ld %ld", &trials, &L, &strays) != 3) return 2;
        for (long r = 0; r < strays; ++r)
            printf("%d %d\n", (int)dproof_fits((uint32_t)r, (uint32_t)L, (uint32_t)trials),
                   (int)dproof_deferred((uint32_t)r, (uint32_t)L, (uint32_t)trials));
        printf("%u %llu\n", dproof_frames((uint32_t)strays, (uint32_t)L, (uint32_t)trials),
               (unsigned long long)dproof_pairs((uint32_t)strays, (uint32_t)L, (uint32_t)trials));
        return 0;
    }
    const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4097, 65536, 1u << 20};
    const uint32_t receipts[] = {1, 2, 8, 63, 64, 1024, 4096};
    for (uint32_t n : sizes)
        for (uint32_t m : receipts) {
            uint32_t cap = 2;
            while (cap < 2 * m) cap <<= 1;                                   // link_capacity's rule
            check_layout(n, cap, m);
        }
    CHECK(dproof_layout(DP_MAX_RECORDS, 1u << 30, 1u << 29).bytes > 0);      // no overflow at the largest object
    CHECK(dproof_blocks(0) == 0 && dproof_blocks(1) == 1 && dproof_blocks(256) == 1 && dproof_blocks(257) == 2);
    CHECK(dproof_blocks(0xFFFFFFFFu) == (1u << 24));
    CHECK(dproof_scan_blocks(0) == 0 && dproof_scan_blocks(4096) == 16 && dproof_scan_blocks(4097) == 17);

    // the budget at 0, 1, L - 1, L, 2L - 1 and 2L, and around them
    for (uint32_t L : {1u, 2u, 7u, 64u, 1024u})
        for (uint32_t strays : {0u, 1u, 2u, 3u, 5u})
            for (uint32_t trials : {0u, 1u, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 5 * L, 0xFFFFFFFFu})
                check_budget(strays, L, trials);
    const uint32_t L = 7;
    CHECK(!dproof_fits(0, L, 0) && !dproof_fits(0, L, 1) && !dproof_fits(0, L, L - 1));
    CHECK(dproof_fits(0, L, L) && !dproof_fits(1, L, L) && dproof_deferred(1, L, L));
    CHECK(dproof_fits(0, L, 2 * L - 1) && !dproof_fits(1, L, 2 * L - 1));
    CHECK(dproof_fits(1, L, 2 * L) && !dproof_fits(2, L, 2 * L));
    // L = 0: nothing to try, nothing deferred
    for (uint32_t trials : {0u, 1u, 4096u}) {
        check_budget(4, 0, trials);
        CHECK(!dproof_fits(0, 0, trials) && !dproof_deferred(0, 0, trials) && dproof_pairs(9, 0, trials) == 0);
    }
    // ranks and lengths whose product passes a word
    CHECK(!dproof_fits(0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu) && dproof_deferred(0x10000u, 0x10000u, 0xFFFFFFFFu));
    CHECK(dproof_frames(0xFFFFFFFFu, 1, 0xFFFFFFFFu) == 0xFFFFFFFFu);
    printf("ok %ld\n", checks);
    return 0;
}
