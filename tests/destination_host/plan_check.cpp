// plan_check.cpp — reticulum_amd/csrc/destination_host.h built alone with g++
// and the address and undefined-behaviour sanitizers
// (tests/test_destination_deliver.py builds and runs it; no Python is loaded
// into it).
//
// Without arguments: sweeps the scratch layout over frame counts and retry
// budgets (0, 1, the workgroup edges, large ones), checks that every array is
// 16-byte aligned, that no two overlap, that all lie inside the stated size and
// that a call of fewer frames fits the object's workspace, and touches every
// byte of a heap buffer of exactly that size through the layout; sweeps the
// retry budget's arithmetic at 0, 1, the exact fit and one past it, against a
// plain loop over the frames.  Prints "ok <checks>".
//
// With "budget" as its argument: reads "retry n" and then n remaining-candidate
// counts from standard input and prints, per frame, "fits pair_off", for the
// test to compare with its own model.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../reticulum_amd/csrc/destination_host.h"

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

// what the device does with the asks of the undecided frames in stream order
static void budget(const std::vector<uint32_t> &remaining, uint32_t retry, std::vector<int> &fits,
                   std::vector<uint32_t> &pair_off, uint32_t &pairs) {
    uint32_t start = 0;
    pairs = 0;
    fits.assign(remaining.size(), 0);
    pair_off.assign(remaining.size(), 0);
    for (size_t i = 0; i < remaining.size(); ++i) {
        const uint32_t ask = remaining[i] ? deliver_ask(remaining[i], retry) : 0u;
        pair_off[i] = deliver_pair_off(start, retry);
        if (deliver_fits(start, ask, retry)) {
            fits[i] = 1;
            if (start + ask > pairs) pairs = start + ask;
        }
        start = dd_sat_add(start, ask);
    }
}

static void check_layout(uint32_t n, uint32_t retry) {
    const DeliverLayout l = deliver_layout(n, retry);
    const uint64_t N = n, P = (uint64_t)n + retry, nb = deliver_blocks(n);
    // (offset, words) of every array
    const std::pair<uint64_t, uint64_t> arrays[] = {
        {0, DD_W_HEAD},       {l.part, nb + 1},   {l.part2, nb + 1},  {l.drow, N},        {l.ncand, N},
        {l.rank, N + 2},      {l.start, N + 2},   {l.rem, N},         {l.first1, N + 1},  {l.first2, N + 1},
        {l.tlen1, N + 1},     {l.tlen2, N + 1},   {l.toff, 2 * (N + 1)}, {l.dkey, N},     {l.dlen, N},
        {l.dst, N},           {l.dpl, N},         {l.plist, N},       {l.pfrm, P},        {l.pcand, P},
        {l.krow, P},          {l.salt, 4 * P},    {l.shared, 8 * P}};
    uint64_t end = 0;
    for (const auto &a : arrays) {
        CHECK(a.first % 4 == 0);                       // 16-byte aligned
        CHECK(a.first >= end);                         // in order, none overlaps the one before
        end = a.first + a.second;
        CHECK(4 * end <= l.bytes);
    }
    CHECK(l.bytes % 16 == 0);
    CHECK(l.bytes == deliver_workspace_bytes(n, retry));
    if (n) CHECK(deliver_workspace_bytes(n - 1, retry) <= l.bytes);   // a smaller call fits the object's workspace
    if (l.bytes <= (64u << 20)) {
        // every word of every array written once, in a heap buffer of exactly the stated size
        std::vector<uint32_t> buf(l.bytes / 4, 0u);
        for (const auto &a : arrays)
            for (uint64_t k = 0; k < a.second; ++k) buf[a.first + k] += 1u;
        for (uint32_t v : buf) CHECK(v <= 1u);
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "budget")) {
        long retry, n;
        if (scanf("%ld %ld", &retry, &n) != 2) return 2;
        std::vector<uint32_t> rem((size_t)n);
        for (long i = 0; i < n; ++i) {
            long v;
            if (scanf("%ld", &v) != 1) return 2;
            rem[(size_t)i] = (uint32_t)v;
        }
        std::vector<int> fits;
        std::vector<uint32_t> off;
        uint32_t pairs;
        budget(rem, (uint32_t)retry, fits, off, pairs);
        for (long i = 0; i < n; ++i) printf("%d %u\n", fits[(size_t)i], off[(size_t)i]);
        printf("pairs %u\n", pairs);
        return 0;
    }
    const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4097, 65536, 1u << 20};
    const uint32_t budgets[] = {0, 1, 2, 3, 255, 256, 257, 4096, 1u << 20};
    for (uint32_t n : sizes)
        for (uint32_t r : budgets) check_layout(n, r);
    CHECK(deliver_layout(DD_MAX_FRAMES, DD_MAX_FRAMES).bytes > 0);      // no overflow at the largest object
    CHECK(deliver_blocks(0) == 0 && deliver_blocks(1) == 1 && deliver_blocks(256) == 1 && deliver_blocks(257) == 2);
    CHECK(deliver_blocks(0xFFFFFFFFu) == (1u << 24));
    CHECK(dd_sat_add(0xFFFFFFFFu, 1u) == 0xFFFFFFFFu && dd_sat_add(0xFFFFFFF0u, 0xFu) == 0xFFFFFFFFu);
    CHECK(deliver_proof_bytes(true) == 83 && deliver_proof_bytes(false) == 115);
    CHECK(deliver_retry_row(1024, 0) == 1024 && deliver_retry_row(1024, 7) == 1031);

    // the retry budget at 0, 1, the exact fit and one past it
    std::vector<int> fits;
    std::vector<uint32_t> off;
    uint32_t pairs;
    const std::vector<uint32_t> rem = {0, 2, 0, 1, 5, 0, 3};            // 11 pairs in all
    for (uint32_t retry = 0; retry <= 13; ++retry) {
        budget(rem, retry, fits, off, pairs);
        uint32_t used = 0;
        bool stopped = false;
        for (size_t i = 0; i < rem.size(); ++i) {
            CHECK(off[i] <= retry);
            if (!rem[i]) {
                CHECK(!fits[i]);
                continue;
            }
            // only whole frames, in order; after the first that does not fit none does
            const bool want = !stopped && used + rem[i] <= retry;
            CHECK((fits[i] != 0) == want);
            if (want) {
                CHECK(off[i] == used);
                used += rem[i];
            } else {
                stopped = true;
            }
        }
        CHECK(pairs == used);
        if (retry >= 11) CHECK(used == 11);
        if (retry == 10) CHECK(fits[4] && !fits[6]);                    // one row short: the last frame only
        if (retry == 0) CHECK(pairs == 0);
    }
    // a frame whose candidates alone exceed the budget, followed by one that would fit: both deferred
    budget({9, 1}, 4, fits, off, pairs);
    CHECK(!fits[0] && !fits[1] && pairs == 0);
    // asks beyond a word
    budget({0xFFFFFFFFu, 0xFFFFFFFFu, 1}, 0xFFFFFFFEu, fits, off, pairs);
    CHECK(!fits[0] && !fits[1] && !fits[2]);
    budget({5, 0xFFFFFFFFu, 1}, 0xFFFFFFFFu, fits, off, pairs);
    CHECK(fits[0] && !fits[1] && !fits[2] && pairs == 5);
    printf("ok %ld\n", checks);
    return 0;
}
