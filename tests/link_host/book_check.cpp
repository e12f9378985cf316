// book_check.cpp — the host-side arithmetic of the link table
// (reticulum_amd/csrc/link_host.h) alone, for a build with
// -fsanitize=address,undefined: capacity rounding at its edges, and the
// reclaim bookkeeping against an exact model of the slots through random runs
// of inserts, removes, rebuilds and late or lost rebuild reports.
//
// What the bookkeeping has to guarantee: used_ub never falls below the slots
// in use, and an insert of n items that is not preceded by a rebuild finds
// tombs + live + n <= capacity, so that RT_LINK_FULL can only mean more live
// entries than slots.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "../../reticulum_amd/csrc/link_host.h"

using namespace rnstok;

static int checks = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        ++checks;                                                      \
        if (!(cond)) {                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 20) % below);
}

static int capacities() {
    CHECK(link_capacity(0) == 0);
    CHECK(link_capacity(1) == 2);
    CHECK(link_capacity(2) == 4);
    CHECK(link_capacity(3) == 8);
    CHECK(link_capacity(4) == 8);
    CHECK(link_capacity(5) == 16);
    CHECK(link_capacity(32) == 64);
    CHECK(link_capacity(33) == 128);
    CHECK(link_capacity(2048) == 4096);
    CHECK(link_capacity(65536) == 131072);
    CHECK(link_capacity((1u << 29) - 1) == 1u << 30);
    CHECK(link_capacity(1u << 29) == 1u << 30);
    CHECK(link_capacity((1u << 29) + 1) == 0);
    CHECK(link_capacity(0xFFFFFFFFu) == 0);
    for (uint32_t m = 1; m < 5000; ++m) {
        const uint32_t c = link_capacity(m);
        CHECK(c >= 2 * m && (c & (c - 1)) == 0 && c / 2 < 2 * m);
    }
    return 0;
}

// One table: the model knows live entries and tombs exactly.
static int run(uint32_t max_links, uint32_t steps) {
    LinkBook b;
    b.cap = link_capacity(max_links);
    const uint32_t cap = b.cap;
    uint32_t live = 0, tombs = 0, rebuilds = 0;
    bool report_ready = false;
    uint32_t reported = 0;
    for (uint32_t step = 0; step < steps; ++step) {
        const uint32_t what = rnd(10);
        if (what < 5) {                         // insert n items, some of them new
            const uint32_t n = rnd(cap + 2);
            if (report_ready && rnd(2)) {       // the report arrives now, later, or never
                b.on_report(reported);
                report_ready = false;
            }
            if (b.needs_rebuild(n)) {
                tombs = 0;
                b.on_rebuild();
                reported = live;                // what this rebuild will report
                report_ready = true;
                ++rebuilds;
            } else {
                CHECK(tombs == 0 || (uint64_t)tombs + live + n <= cap);
            }
            uint32_t fresh = rnd(n + 1);        // ids not present yet
            while (fresh && live + tombs < cap) {
                // a new id takes a tomb or an empty slot
                if (tombs && rnd(2)) --tombs;
                ++live;
                --fresh;
            }
            b.on_insert(n);
        } else if (what < 9) {                  // remove n items, some of them present
            const uint32_t n = rnd(cap + 2);
            uint32_t hit = rnd(n + 1);
            if (hit > live) hit = live;
            live -= hit;
            tombs += hit;
            b.on_remove(n);
        } else if (report_ready) {
            b.on_report(reported);
            report_ready = false;
        }
        CHECK(b.used_ub <= cap);
        CHECK(b.used_ub >= live + tombs);
        CHECK(b.threshold() == cap - cap / 4);
    }
    // churn within max_links must not rebuild on every insert
    CHECK(rebuilds < steps);
    return 0;
}

// A stale report (no rebuild outstanding) is ignored; counters saturate.
static int edges() {
    LinkBook b;
    b.cap = 8;
    b.on_insert(4);
    b.on_report(0);
    CHECK(b.used_ub == 4);
    CHECK(!b.needs_rebuild(8));                 // nothing removed: nothing to reclaim
    b.on_remove(0xFFFFFFFFu);
    b.on_remove(0xFFFFFFFFu);
    CHECK(b.removes == 0xFFFFFFFFu);
    CHECK(!b.needs_rebuild(2));                 // 4 + 2 <= 6
    CHECK(b.needs_rebuild(3));
    CHECK(b.needs_rebuild(0xFFFFFFFFu));
    b.on_rebuild();
    CHECK(b.removes == 0 && b.awaiting && b.used_ub == 4);
    b.on_insert(0xFFFFFFFFu);
    CHECK(b.used_ub == 8 && b.since_rebuild == 8);
    b.on_report(1);
    CHECK(b.used_ub == 8 && !b.awaiting);       // 1 + 8 saturates at the capacity
    b.on_rebuild();
    b.on_insert(2);
    b.on_report(3);
    CHECK(b.used_ub == 5);
    return 0;
}

int main() {
    if (capacities() || edges()) return 1;
    for (uint32_t max_links : {1u, 2u, 4u, 32u, 100u, 2048u})
        if (run(max_links, 20000)) return 1;
    printf("ok %d\n", checks);
    return 0;
}
