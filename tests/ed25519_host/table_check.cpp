// table_check.cpp — host build of ge_scalarmult_base_table
// (reticulum_amd/csrc/ed25519_device.h) against ge_scalarmult_base, for
// tests/test_ifac_sign.py.  No input; prints one line per failure and "ok N"
// at the end, and returns 1 where any scalar encodes differently.
//
// Scalars: 0, every 2^i for i = 0..252 (one table entry each), L - 1,
// 2^253 - 1 (every entry at once) and 64 random ones below 2^253 from a fixed
// seed.  A signature never uses entry 252 (r < L < 2^252 + 2^125), so this
// program is what pins it.
//
//   g++ -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o table_check table_check.cpp
#include <stdio.h>
#include <string.h>

#include "../../reticulum_amd/csrc/ed25519_device.h"

using namespace rnstok;

static int failures = 0, checked = 0;

static void check(const uint32_t e[8], const char *what, int idx) {
    ge a, b;
    uint32_t wa[8], wb[8];
    ge_scalarmult_base(a, e);
    ge_scalarmult_base_table(b, e);
    ge_encode(wa, a);
    ge_encode(wb, b);
    ++checked;
    if (memcmp(wa, wb, sizeof wa)) {
        ++failures;
        printf("differs: %s %d\n", what, idx);
    }
}

// splitmix64: a fixed stream of test scalars
static uint64_t rng_state = 0x1fac5eedull;
static uint64_t next64() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main() {
    uint32_t e[8];
    memset(e, 0, sizeof e);
    check(e, "zero", 0);
    for (int i = 0; i < ED25519_BASE_TABLE_ENTRIES; ++i) {
        memset(e, 0, sizeof e);
        e[i >> 5] = 1u << (i & 31);
        check(e, "2^i, i =", i);
    }
    for (int k = 0; k < 8; ++k) e[k] = sc_L(k);
    e[0] -= 1u;                              // L is odd: no borrow
    check(e, "L - 1", 0);
    for (int k = 0; k < 8; ++k) e[k] = 0xffffffffu;
    e[7] = 0x1fffffffu;
    check(e, "2^253 - 1", 0);
    for (int j = 0; j < 64; ++j) {
        for (int k = 0; k < 8; k += 2) {
            const uint64_t v = next64();
            e[k] = (uint32_t)v;
            e[k + 1] = (uint32_t)(v >> 32);
        }
        e[7] &= 0x1fffffffu;
        check(e, "random", j);
    }
    printf("ok %d\n", checked - failures);
    return failures ? 1 : 0;
}
