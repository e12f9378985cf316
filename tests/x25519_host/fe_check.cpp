// fe_check.cpp — host build of reticulum_amd/csrc/x25519_device.h for
// tests/test_x25519.py.  Reads one operation per line on stdin and prints the
// result as 32 little-endian bytes in hex (fully reduced):
//
//   mul A B | sq A | add A B | sub A B | small A | inv A | store A
//       A, B: 64 hex digits (32 little-endian bytes, loaded as a point is:
//       bit 255 dropped); small multiplies by 121665
//   ladder S P        X25519(scalar S, point P)
//   lmul L L | lsq L  mul / square on raw limbs: L is 10 hex limbs joined by
//       commas, taken as they are (unreduced limbs are where a multiply
//       overflows)
//   addmax            the limb bound after one add, as an L (so the test
//       builds its worst-case operands from the header's own constants)
//
//   g++ -O1 -fsanitize=address,undefined -o fe_check fe_check.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../reticulum_amd/csrc/x25519_device.h"

using namespace rnstok;

static int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

static bool parse_bytes(const char *s, uint8_t out[32]) {
    if (!s || strlen(s) != 64) return false;
    for (int i = 0; i < 32; ++i) {
        const int hi = hexval(s[2 * i]), lo = hexval(s[2 * i + 1]);
        if (hi < 0 || lo < 0) return false;
        out[i] = (uint8_t)(hi * 16 + lo);
    }
    return true;
}

static bool parse_fe(const char *s, fe &r) {
    uint8_t b[32];
    if (!parse_bytes(s, b)) return false;
    fe_load(r, b);
    return true;
}

static bool parse_limbs(const char *s, fe &r) {
    if (!s) return false;
    char *end = nullptr;
    for (int i = 0; i < 10; ++i) {
        const unsigned long long v = strtoull(s, &end, 16);
        if (end == s || v > 0xffffffffull) return false;
        r.v[i] = (uint32_t)v;
        if (i < 9) {
            if (*end != ',') return false;
            s = end + 1;
        }
    }
    return *end == '\0';
}

static void print_bytes(const uint8_t b[32]) {
    for (int i = 0; i < 32; ++i) printf("%02x", b[i]);
    printf("\n");
}

static void print_fe(const fe &a) {
    uint8_t b[32];
    fe_store(b, a);
    print_bytes(b);
}

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        char *op = strtok(line, " \t\r\n");
        if (!op) continue;
        char *x = strtok(nullptr, " \t\r\n"), *y = strtok(nullptr, " \t\r\n");
        fe a, b, r;
        if (!strcmp(op, "addmax")) {
            for (int i = 0; i < 10; ++i) printf("%x%s", fe_add_max(i), i < 9 ? "," : "\n");
            continue;
        }
        if (!strcmp(op, "ladder")) {
            uint8_t s[32], p[32], o[32];
            if (!parse_bytes(x, s) || !parse_bytes(y, p)) return 2;
            x25519_bytes(o, s, p);
            print_bytes(o);
            continue;
        }
        const bool limbs = op[0] == 'l';
        const bool two = !strcmp(op, "mul") || !strcmp(op, "add") || !strcmp(op, "sub") || !strcmp(op, "lmul");
        if (!(limbs ? parse_limbs(x, a) : parse_fe(x, a))) return 2;
        if (two && !(limbs ? parse_limbs(y, b) : parse_fe(y, b))) return 2;
        if (!strcmp(op, "mul") || !strcmp(op, "lmul")) fe_mul(r, a, b);
        else if (!strcmp(op, "sq") || !strcmp(op, "lsq")) fe_sq(r, a);
        else if (!strcmp(op, "add")) fe_add(r, a, b);
        else if (!strcmp(op, "sub")) fe_sub(r, a, b);
        else if (!strcmp(op, "small")) fe_mul_small(r, a, 121665u);
        else if (!strcmp(op, "inv")) fe_invert(r, a);
        else if (!strcmp(op, "store")) r = a;
        else return 2;
        print_fe(r);
    }
    return 0;
}
