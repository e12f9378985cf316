// ed_check.cpp — host build of reticulum_amd/csrc/ed25519_device.h for
// tests/test_ed25519.py.  Reads one operation per line on stdin and prints one
// token per line.  Byte strings are hex; "-" is the empty string.
//
//   sha512 HEAD MSG       SHA-512(HEAD ‖ MSG), HEAD of 32 or 64 bytes: 128 digits
//   reduce X              X mod L, X of 32 or 64 little-endian bytes: 64 digits
//   muladd R K A          (R + K*A) mod L, 32 bytes each
//   decode P              x:y (32 little-endian bytes each, reduced) or "fail"
//   dbl P | add P Q       enc(2P), enc(P + Q) of decoded points, or "fail"
//   ingroup P             1 where [L]P is the identity, else 0, or "fail"
//   base E                enc([E]B), E < 2^255
//   dsm S H A             enc([S]B - [H]A), S, H < 2^253
//   verify PK SIG MSG     1 or 0
//   sign SEED PK MSG      the 64-byte signature; PK "-": derived from SEED
//   public SEED           the 32-byte public key
//
//   g++ -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o ed_check ed_check.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../reticulum_amd/csrc/ed25519_device.h"

using namespace rnstok;

static int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

static bool parse(const char *s, std::vector<uint8_t> &out) {
    out.clear();
    if (!s) return false;
    if (!strcmp(s, "-")) return true;
    const size_t n = strlen(s);
    if (n & 1) return false;
    for (size_t i = 0; i < n; i += 2) {
        const int hi = hexval(s[i]), lo = hexval(s[i + 1]);
        if (hi < 0 || lo < 0) return false;
        out.push_back((uint8_t)(hi * 16 + lo));
    }
    return true;
}

static bool parse_n(const char *s, std::vector<uint8_t> &out, size_t n) { return parse(s, out) && out.size() == n; }

static void print_hex(const uint8_t *b, size_t n, const char *end = "\n") {
    for (size_t i = 0; i < n; ++i) printf("%02x", b[i]);
    printf("%s", end);
}

static void print_words(const uint32_t w[8], const char *end = "\n") {
    uint8_t b[32];
    store_words(b, w);
    print_hex(b, 32, end);
}

// an exactly sized heap copy, so that the address sanitizer sees any read past the message
struct Exact {
    uint8_t *p;
    uint32_t n;
    explicit Exact(const std::vector<uint8_t> &v) : p(v.empty() ? nullptr : (uint8_t *)malloc(v.size())), n((uint32_t)v.size()) {
        if (p) memcpy(p, v.data(), v.size());
    }
    ~Exact() { free(p); }
};

static bool decode_ge(const char *s, ge &p) {
    std::vector<uint8_t> b;
    if (!parse_n(s, b, 32)) exit(2);
    uint32_t w[8];
    load_words(w, b.data());
    fe x, y;
    if (!ge_decode(x, y, w)) return false;
    p.X = x;
    p.Y = y;
    fe_set(p.Z, 1u);
    fe_mul(p.T, x, y);
    return true;
}

static void print_ge(const ge &p) {
    uint32_t w[8];
    ge_encode(w, p);
    print_words(w);
}

int main() {
    static char line[1 << 16];
    std::vector<uint8_t> a, b, c;
    while (fgets(line, sizeof line, stdin)) {
        char *op = strtok(line, " \t\r\n");
        if (!op) continue;
        char *x = strtok(nullptr, " \t\r\n"), *y = strtok(nullptr, " \t\r\n"), *z = strtok(nullptr, " \t\r\n");
        if (!strcmp(op, "sha512")) {
            if (!parse(x, a) || !parse(y, b) || (a.size() != 32 && a.size() != 64)) return 2;
            Exact m(b);
            uint64_t head[8], st[8];
            uint32_t w[16];
            load_words(w, a.data());
            sha512_head_from_le(head, w);
            if (a.size() == 64) {
                load_words(w + 8, a.data() + 32);
                sha512_head_from_le(head + 4, w + 8);
                sha512_head_msg<8>(st, head, m.p, m.n);
            } else {
                sha512_head_msg<4>(st, head, m.p, m.n);
            }
            for (int k = 0; k < 8; ++k) printf("%016llx", (unsigned long long)st[k]);
            printf("\n");
        } else if (!strcmp(op, "reduce")) {
            if (!parse(x, a) || (a.size() != 32 && a.size() != 64)) return 2;
            uint32_t w[16], r[8];
            load_words(w, a.data());
            if (a.size() == 64) {
                load_words(w + 8, a.data() + 32);
                sc_reduce<16>(r, w);
            } else {
                sc_reduce<8>(r, w);
            }
            print_words(r);
        } else if (!strcmp(op, "muladd")) {
            if (!parse_n(x, a, 32) || !parse_n(y, b, 32) || !parse_n(z, c, 32)) return 2;
            uint32_t r[8], k[8], s[8], o[8];
            load_words(r, a.data());
            load_words(k, b.data());
            load_words(s, c.data());
            sc_muladd(o, r, k, s);
            print_words(o);
        } else if (!strcmp(op, "decode")) {
            if (!parse_n(x, a, 32)) return 2;
            uint32_t w[8], xw[8], yw[8];
            load_words(w, a.data());
            fe fx, fy;
            if (!ge_decode(fx, fy, w)) {
                printf("fail\n");
                continue;
            }
            fe_to_words(xw, fx);
            fe_to_words(yw, fy);
            print_words(xw, ":");
            print_words(yw);
        } else if (!strcmp(op, "dbl") || !strcmp(op, "add") || !strcmp(op, "ingroup")) {
            ge p, q;
            if (!decode_ge(x, p) || (!strcmp(op, "add") && !decode_ge(y, q))) {
                printf("fail\n");
                continue;
            }
            ge_cached cq;
            if (!strcmp(op, "dbl")) {
                ge_double(p, p);
                print_ge(p);
            } else if (!strcmp(op, "add")) {
                ge_to_cached(cq, q);
                ge_add_cached(p, p, cq);
                print_ge(p);
            } else {
                ge_to_cached(cq, p);
                printf("%u\n", ge_in_subgroup(cq));
            }
        } else if (!strcmp(op, "base")) {
            if (!parse_n(x, a, 32)) return 2;
            uint32_t e[8];
            load_words(e, a.data());
            ge q;
            ge_scalarmult_base(q, e);
            print_ge(q);
        } else if (!strcmp(op, "dsm")) {
            if (!parse_n(x, a, 32) || !parse_n(y, b, 32) || !parse_n(z, c, 32)) return 2;
            uint32_t s[8], h[8], w[8];
            load_words(s, a.data());
            load_words(h, b.data());
            load_words(w, c.data());
            fe ax, ay;
            if (!ge_decode(ax, ay, w)) {
                printf("fail\n");
                continue;
            }
            ge_cached na, bma;
            ge_cached_neg_affine(na, ax, ay);
            ge bb, q;
            bb.X = fe_bx();
            bb.Y = fe_by();
            fe_set(bb.Z, 1u);
            fe_mul(bb.T, bb.X, bb.Y);
            ge_add_cached(bb, bb, na);
            ge_to_cached(bma, bb);
            ge_double_scalar(q, s, h, na, bma);
            print_ge(q);
        } else if (!strcmp(op, "verify")) {
            if (!parse_n(x, a, 32) || !parse_n(y, b, 64) || !parse(z, c)) return 2;
            Exact m(c);
            uint32_t pk[8], r[8], s[8];
            load_words(pk, a.data());
            load_words(r, b.data());
            load_words(s, b.data() + 32);
            printf("%u\n", ed25519_verify_words(pk, r, s, m.p, m.n));
        } else if (!strcmp(op, "sign")) {
            if (!parse_n(x, a, 32) || !parse(y, b) || (b.size() != 0 && b.size() != 32) || !parse(z, c)) return 2;
            Exact m(c);
            uint32_t sig[16];
            ed25519_sign_words(sig, a.data(), b.empty() ? nullptr : b.data(), m.p, m.n);
            print_words(sig, "");
            print_words(sig + 8);
        } else if (!strcmp(op, "public")) {
            if (!parse_n(x, a, 32)) return 2;
            uint32_t seed[8], pub[8];
            load_words(seed, a.data());
            ed25519_public_words(pub, seed);
            print_words(pub);
        } else {
            return 2;
        }
    }
    return 0;
}
