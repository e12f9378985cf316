// span_reader_check.cpp — host build of the multi-span SHA-512 reader
// (sha512_head_spans, reticulum_amd/csrc/ed25519_device.h) against
// sha512_head_msg over the same message copied into one piece, for
// tests/test_announce.py.  No input; prints one line per failure and "ok N" at
// the end, and returns 1 where any state differs.
//
// Every case is an announce-shaped packet in a heap buffer of exactly the
// packet's size, so that the address sanitizer sees a read of any byte past
// the packet's end (or before its start): both header types (data at 19 and
// 35), both places of the signature (84 and 116 bytes into the data) and every
// app-data length 0..333.  The bytes that must stay out of the hash (hops,
// transport id, context byte, signature) are hashed once as they are and once
// more inverted: the state must not move.
//
//   g++ -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o span_reader_check span_reader_check.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../reticulum_amd/csrc/ed25519_device.h"

using namespace rnstok;

static int failures = 0, checked = 0;

static uint64_t rng_state = 0xa220c5eedull;
static uint64_t next64() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static void check(uint32_t d, uint32_t head, uint32_t app) {
    const uint32_t data_len = head + 64u + app, total = d + data_len, len = 16u + data_len - 64u;
    uint8_t *pkt = (uint8_t *)malloc(total);
    uint8_t *flat = (uint8_t *)malloc(len);
    for (uint32_t k = 0; k < total; ++k) pkt[k] = (uint8_t)next64();
    memcpy(flat, pkt + d - 17, 16);
    memcpy(flat + 16, pkt + d, head);
    memcpy(flat + 16 + head, pkt + d + head + 64, app);
    uint64_t hd[8], want[8], got[8];
    for (int k = 0; k < 8; ++k) hd[k] = next64();
    sha512_head_msg<8>(want, hd, flat, len);
    for (int pass = 0; pass < 2; ++pass) {
        const sha512_spans m{pkt + d - 17, 16u, 1u, 16u + head, 64u, len};
        sha512_head_spans<8>(got, hd, m);
        ++checked;
        if (memcmp(want, got, sizeof want)) {
            ++failures;
            printf("differs: data at %u, signature at %u, app data %u, pass %d\n", d, head, app, pass);
        }
        // what lies outside the three spans
        for (uint32_t k = 0; k < d - 17; ++k) pkt[k] ^= 0xffu;
        pkt[d - 1] ^= 0xffu;
        for (uint32_t k = 0; k < 64; ++k) pkt[d + head + k] ^= 0xffu;
    }
    free(flat);
    free(pkt);
}

int main() {
    for (uint32_t d = 19; d <= 35; d += 16)
        for (uint32_t head = 84; head <= 116; head += 32)
            for (uint32_t app = 0; app <= 333; ++app) check(d, head, app);
    printf("ok %d\n", checked - failures);
    return failures ? 1 : 0;
}
