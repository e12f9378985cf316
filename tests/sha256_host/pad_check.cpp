// pad_check.cpp — host build of the SHA-256 message-block builders
// (sha_pad_blocks, sha_pad_block and its byte functors, the HMAC and HKDF block
// fillers: reticulum_amd/csrc/sha256_device.h) against padding built the
// obvious way: the message copied into a zeroed buffer, 0x80 appended, the
// 64-bit big-endian bit length written at the end of the last block.  For
// tests/test_sha256_pad.py.  No input; prints one line per failure and "ok N"
// at the end, and returns 1 where any block differs.
//
// Every message lies in a heap buffer of exactly its own size, so that the
// address sanitizer sees a read of any byte past its end.
//
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o pad_check pad_check.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../reticulum_amd/csrc/sha256_device.h"

using namespace rnstok;

static int failures = 0, checked = 0;

static uint64_t rng_state = 0x5a256c0de5ull;
static uint8_t next8() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint8_t)(z >> 24);
}
static uint8_t *random_bytes(uint32_t n) {
    uint8_t *p = (uint8_t *)malloc(n);
    for (uint32_t k = 0; k < n; ++k) p[k] = next8();
    return p;
}

// The padded message, the obvious way.  prior: bytes hashed before msg.
struct Padded {
    uint8_t *buf;
    uint32_t blocks;
};
static Padded pad_obvious(const uint8_t *msg, uint32_t m, uint64_t prior) {
    uint32_t size = 64;
    while (size < m + 1 + 8) size += 64;
    uint8_t *buf = (uint8_t *)calloc(size, 1);
    if (m) memcpy(buf, msg, m);
    buf[m] = 0x80;
    const uint64_t bits = (prior + m) * 8;
    for (int k = 0; k < 8; ++k) buf[size - 1 - k] = (uint8_t)(bits >> (8 * k));
    return Padded{buf, size / 64};
}
static uint32_t be_word(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
static void expect_block(const uint32_t w[16], const uint8_t *want, const char *what, uint32_t x, uint32_t y,
                         uint32_t b) {
    ++checked;
    for (int k = 0; k < 16; ++k)
        if (w[k] != be_word(want + 4 * k)) {
            ++failures;
            printf("differs: %s %u %u, block %u word %d\n", what, x, y, b, k);
            return;
        }
}

// blocks first.. of `flat` (the m message bytes in one piece) padded, against
// the builder over `at` for the bytes from 64 * first on
template <class ByteAt>
static void check_builder(const uint8_t *flat, uint32_t m, uint64_t prior, uint32_t first, ByteAt at, const char *what,
                          uint32_t x, uint32_t y) {
    const Padded p = pad_obvious(flat, m, prior);
    const uint32_t tail = m - 64u * first;
    if (first + sha_pad_blocks(tail) != p.blocks) {
        ++failures;
        printf("block count: %s %u %u: %u, not %u\n", what, x, y, first + sha_pad_blocks(tail), p.blocks);
    }
    for (uint32_t b = 0; first + b < p.blocks; ++b) {
        uint32_t w[16];
        sha_pad_block(w, b, tail, (prior + m) * 8, at);
        expect_block(w, p.buf + 64 * (first + b), what, x, y, first + b);
    }
    free(p.buf);
}

int main() {
    const uint64_t priors[2] = {0, 64};
    for (uint64_t prior : priors) {
        // one segment
        for (uint32_t m = 0; m <= 200; ++m) {
            uint8_t *msg = random_bytes(m);
            check_builder(msg, m, prior, 0, BytesAt{msg}, "one segment", m, (uint32_t)prior);
            free(msg);
        }
        // two segments, every split
        for (uint32_t m = 0; m <= 130; ++m)
            for (uint32_t alen = 0; alen <= m; ++alen) {
                uint8_t *a = random_bytes(alen), *b = random_bytes(m - alen), *flat = (uint8_t *)malloc(m);
                if (alen) memcpy(flat, a, alen);
                if (m - alen) memcpy(flat + alen, b, m - alen);
                check_builder(flat, m, prior, 0, Bytes2At{a, alen, b}, "two segments", alen, m - alen);
                free(a); free(b); free(flat);
            }
        // a first byte, then src: the whole message, and (as the packet hash
        // runs it) only what follows the message's whole blocks
        for (uint32_t len = 0; len <= 130; ++len) {
            uint8_t *src = random_bytes(len), *flat = (uint8_t *)malloc(len + 1);
            flat[0] = next8();
            if (len) memcpy(flat + 1, src, len);
            check_builder(flat, len + 1, prior, 0, PrefixedAt{flat[0], src, 0u}, "prefixed", len, 0);
            const uint32_t nfull = (len + 1) / 64;
            check_builder(flat, len + 1, prior, nfull, PrefixedAt{flat[0], src, 64u * nfull}, "prefixed tail", len, nfull);
            free(src); free(flat);
        }
    }

    // HMAC: key words, key blocks, the outer block
    for (uint32_t len = 0; len <= 64; ++len) {
        uint8_t *key = random_bytes(len), z[64] = {0};
        if (len) memcpy(z, key, len);
        uint32_t kw[16], w[16], w8[16];
        hmac_key_words(kw, key, len);
        expect_block(kw, z, "key words", len, 0, 0);
        uint8_t x[64];
        for (int k = 0; k < 64; ++k) x[k] = z[k] ^ 0x36;
        hmac_pad_block(w, kw, HMAC_IPAD);
        expect_block(w, x, "ipad block", len, 0, 0);
        for (int k = 0; k < 64; ++k) x[k] = z[k] ^ 0x5c;
        hmac_pad_block(w, kw, HMAC_OPAD);
        expect_block(w, x, "opad block", len, 0, 0);
        if (len <= 32) {                                 // an 8-word key, the rest of the block the pad alone
            hmac_pad_block<8>(w8, kw, HMAC_OPAD);
            expect_block(w8, x, "opad block of 8 words", len, 0, 0);
        }
        free(key);
    }
    {
        uint8_t *d = random_bytes(32);
        uint32_t inner[8], w[16];
        for (int k = 0; k < 8; ++k) inner[k] = be_word(d + 4 * k);
        hmac_outer_block(w, inner);
        const Padded p = pad_obvious(d, 32, 64);
        expect_block(w, p.buf, "outer block", 0, 0, 0);
        if (p.blocks != 1) ++failures;
        free(p.buf); free(d);
    }

    // HKDF: the PRK message of whole words in one block, and T_blk's message
    for (uint32_t len = 0; len <= 52; len += 4) {
        uint8_t *ikm = random_bytes(len);               // malloc: aligned for whole words
        uint32_t w[16];
        hkdf_prk_block(w, ikm, len);
        const Padded p = pad_obvious(ikm, len, 64);
        expect_block(w, p.buf, "prk block", len, 0, 0);
        if (p.blocks != 1) ++failures;
        free(p.buf); free(ikm);
    }
    const uint32_t blks[6] = {0, 1, 2, 254, 255, 256};
    for (uint32_t blk : blks) {
        uint8_t *msg = random_bytes(blk ? 33 : 1);
        uint32_t prev[8], w[16];
        msg[blk ? 32 : 0] = (uint8_t)(blk + 1);
        if (blk)
            for (int k = 0; k < 8; ++k) prev[k] = be_word(msg + 4 * k);
        hkdf_expand_block(w, blk ? prev : nullptr, blk);
        const Padded p = pad_obvious(msg, blk ? 33 : 1, 64);
        expect_block(w, p.buf, "expand block", blk, 0, 0);
        if (p.blocks != 1) ++failures;
        free(p.buf); free(msg);
    }
    printf("ok %d\n", checked - failures);
    return failures ? 1 : 0;
}
