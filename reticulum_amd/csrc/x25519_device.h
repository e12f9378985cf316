// x25519_device.h — GF(2^255 - 19) arithmetic and the RFC 7748 Montgomery
// ladder (RNS/Cryptography/X25519.py:49-93), as device code and as plain host
// C++ (tests/x25519_host/fe_check.cpp compiles it with g++ and sanitizers).
// No HIP builtins, no inline assembly.
//
// Representation: 10 unsigned limbs, limb i holding 26 bits (i even) or 25
// bits (i odd) at bit positions 0, 26, 51, 77, 102, 128, 153, 179, 204, 230.
// Three limb bounds appear:
//   carried  what mul, square, sub and mul_small return: even limbs < 2^26,
//            odd limbs < 2^25, except limb 1 < 2^25 + 2^16 (the last carry
//            lands there);
//   one add  the limb-wise sum of two carried elements, not carried:
//            fe_add_max(i) = 2 x the carried maximum.  mul, square, sub,
//            mul_small and the store accept these;
//   products the accumulators of mul and square: ten terms of at most
//            2^27 * 19 * 2^27 < 2^58.3 each with one-add inputs, so below
//            2^62 and 64 bits hold them with room.
// A ladder step never feeds an element that is more than one add away from a
// carried one into a multiply (x25519_ladder_step notes each).
//
// Constant time by construction: no branch, loop bound or address depends on
// scalar bits or on field values; the conditional swap is a mask.  On the
// device that also keeps the wave converged.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define X25519_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define X25519_FN inline __attribute__((always_inline))
#endif
#if defined(__clang__)
#define X25519_UNROLL _Pragma("unroll")
#define X25519_NO_UNROLL _Pragma("nounroll")
#else
#define X25519_UNROLL
#define X25519_NO_UNROLL
#endif

namespace rnstok {

struct fe {
    uint32_t v[10];
};

// bits of limb i, its mask, and its bit position
X25519_FN constexpr uint32_t fe_bits(int i) { return (i & 1) ? 25u : 26u; }
X25519_FN constexpr uint32_t fe_mask(int i) { return (1u << fe_bits(i)) - 1u; }
X25519_FN constexpr uint32_t fe_pos(int i) { return (uint32_t)(i / 2) * 51u + ((i & 1) ? 26u : 0u); }
// the largest limb of a carried element, and of the sum of two
X25519_FN constexpr uint32_t fe_carried_max(int i) { return fe_mask(i) + (i == 1 ? (1u << 16) : 0u); }
X25519_FN constexpr uint32_t fe_add_max(int i) { return 2u * fe_carried_max(i); }
// limb i of 4p: what sub adds before it subtracts (>= fe_add_max(i) for every i)
X25519_FN constexpr uint32_t fe_4p(int i) { return i == 0 ? 4u * ((1u << 26) - 19u) : 4u * fe_mask(i); }

X25519_FN void fe_set(fe &r, uint32_t x) {
    r.v[0] = x;
    X25519_UNROLL
    for (int i = 1; i < 10; ++i) r.v[i] = 0u;
}

// 32 little-endian bytes, read byte-wise (no alignment assumed), to 8 words
X25519_FN void load_words(uint32_t w[8], const uint8_t *s) {
    X25519_UNROLL
    for (int k = 0; k < 8; ++k)
        w[k] = (uint32_t)s[4 * k] | ((uint32_t)s[4 * k + 1] << 8) | ((uint32_t)s[4 * k + 2] << 16) |
               ((uint32_t)s[4 * k + 3] << 24);
}

// _fix_base_point + unpack: limb 9 ends at bit 254, so bit 255 is dropped;
// values in [p, 2^255) stay as they are (the arithmetic is mod p).
X25519_FN void fe_from_words(fe &r, const uint32_t w[8]) {
    X25519_UNROLL
    for (int i = 0; i < 10; ++i) {
        const uint32_t p = fe_pos(i), k = p >> 5, sh = p & 31u;
        const uint64_t two = (uint64_t)w[k] | ((uint64_t)(k + 1 < 8 ? w[k + 1] : 0u) << 32);
        r.v[i] = (uint32_t)(two >> sh) & fe_mask(i);
    }
}
X25519_FN void fe_load(fe &r, const uint8_t *s) {
    uint32_t w[8];
    load_words(w, s);
    fe_from_words(r, w);
}

// _fix_secret on the scalar's 8 words
X25519_FN void scalar_clamp(uint32_t e[8]) {
    e[0] &= ~7u;
    e[7] &= 0x7fffffffu;
    e[7] |= 0x40000000u;
}

// limb-wise sum, no carry: carried + carried -> one add
X25519_FN void fe_add(fe &r, const fe &a, const fe &b) {
    X25519_UNROLL
    for (int i = 0; i < 10; ++i) r.v[i] = a.v[i] + b.v[i];
}

// One sequential carry pass over 32-bit limbs (each < 2^31), the carry out of
// limb 9 folded into limb 0 times 19, then limb 0's carry into limb 1.
X25519_FN void fe_carry32(fe &r) {
    uint32_t c;
    X25519_UNROLL
    for (int i = 0; i < 9; ++i) {
        c = r.v[i] >> fe_bits(i);
        r.v[i] &= fe_mask(i);
        r.v[i + 1] += c;
    }
    c = r.v[9] >> 25;
    r.v[9] &= fe_mask(9);
    r.v[0] += 19u * c;
    c = r.v[0] >> 26;
    r.v[0] &= fe_mask(0);
    r.v[1] += c;
}

// a - b: a and b up to one add; a + 4p - b per limb stays in [0, 2^29), then
// one carry pass -> carried
X25519_FN void fe_sub(fe &r, const fe &a, const fe &b) {
    X25519_UNROLL
    for (int i = 0; i < 10; ++i) r.v[i] = a.v[i] + fe_4p(i) - b.v[i];
    fe_carry32(r);
}

// The carry chain behind every multiply: 64-bit accumulators -> carried
X25519_FN void fe_carry64(fe &r, uint64_t h[10]) {
    uint64_t c;
    X25519_UNROLL
    for (int i = 0; i < 9; ++i) {
        c = h[i] >> fe_bits(i);
        r.v[i] = (uint32_t)h[i] & fe_mask(i);
        h[i + 1] += c;
    }
    c = h[9] >> 25;
    r.v[9] = (uint32_t)h[9] & fe_mask(9);
    const uint64_t h0 = (uint64_t)r.v[0] + 19u * c;      // c < 2^39
    r.v[0] = (uint32_t)h0 & fe_mask(0);
    r.v[1] += (uint32_t)(h0 >> 26);                      // < 2^16
}

// r = a * b; limbs of a and b up to one add.  Term f_i g_j lands on limb
// (i + j) mod 10, doubled when i and j are both odd (25 + 25 bits sit one
// bit above the limb's position) and times 19 when i + j wraps (2^255 = 19).
X25519_FN void fe_mul(fe &r, const fe &a, const fe &b) {
    uint32_t g19[10], f2[10];
    X25519_UNROLL
    for (int i = 0; i < 10; ++i) {
        g19[i] = 19u * b.v[i];                           // <= 19 * (2^27 - 2) < 2^32
        f2[i] = (i & 1) ? 2u * a.v[i] : a.v[i];
    }
    uint64_t h[10];
    X25519_UNROLL
    for (int k = 0; k < 10; ++k) {
        uint64_t acc = 0;
        X25519_UNROLL
        for (int i = 0; i < 10; ++i) {
            const int j = (k - i + 10) % 10;
            const bool wrap = i + j >= 10;
            const uint32_t f = (i & 1) && (j & 1) ? f2[i] : a.v[i];
            acc += (uint64_t)f * (wrap ? g19[j] : b.v[j]);
        }
        h[k] = acc;
    }
    fe_carry64(r, h);
}

// r = a * a with the symmetric terms taken once; limbs of a up to one add
X25519_FN void fe_sq(fe &r, const fe &a) {
    uint32_t f2[10];
    X25519_UNROLL
    for (int i = 0; i < 10; ++i) f2[i] = 2u * a.v[i];
    uint64_t h[10];
    X25519_UNROLL
    for (int k = 0; k < 10; ++k) {
        uint64_t acc = 0;
        X25519_UNROLL
        for (int i = 0; i < 10; ++i) {
            const int j = (k - i + 10) % 10;
            if (j < i) continue;                         // each unordered pair once
            const bool wrap = i + j >= 10, odd2 = (i & 1) && (j & 1);
            const uint32_t left = i == j ? a.v[i] : f2[i];
            // right factor: f_j, times 2 for an odd pair, times 19 for a wrap:
            // 38 f_j only for odd j (38 * (2^26 + 2^17) < 2^32), 19 f_j for
            // any j (19 * (2^27 - 2) < 2^32)
            const uint32_t right = wrap ? (odd2 ? 38u : 19u) * a.v[j] : (odd2 ? f2[j] : a.v[j]);
            acc += (uint64_t)left * right;
        }
        h[k] = acc;
    }
    fe_carry64(r, h);
}

// r = a * c for a small constant c < 2^17 (the ladder's a24 = 121665)
X25519_FN void fe_mul_small(fe &r, const fe &a, uint32_t c) {
    uint64_t h[10];
    X25519_UNROLL
    for (int i = 0; i < 10; ++i) h[i] = (uint64_t)a.v[i] * c;
    fe_carry64(r, h);
}

// swap a and b where bit is 1, by mask
X25519_FN void fe_cswap(fe &a, fe &b, uint32_t bit) {
    const uint32_t m = 0u - bit;
    X25519_UNROLL
    for (int i = 0; i < 10; ++i) {
        const uint32_t t = m & (a.v[i] ^ b.v[i]);
        a.v[i] ^= t;
        b.v[i] ^= t;
    }
}

X25519_FN void fe_sq_n(fe &r, const fe &a, int n) {
    r = a;
    X25519_NO_UNROLL
    for (int i = 0; i < n; ++i) fe_sq(r, r);
}

// r = z^(p - 2) = z^(2^255 - 21) by the fixed addition chain (254 squarings,
// 11 multiplies); 0 -> 0, as pow(0, P - 2, P) in the reference
X25519_FN void fe_invert(fe &r, const fe &z) {
    fe z2, z9, z11, t, z5, z10, z20, z50, z100;
    fe_sq(z2, z);                  // 2
    fe_sq_n(t, z2, 2);             // 8
    fe_mul(z9, t, z);              // 9
    fe_mul(z11, z9, z2);           // 11
    fe_sq(t, z11);                 // 22
    fe_mul(z5, t, z9);             // 2^5 - 1
    fe_sq_n(t, z5, 5);
    fe_mul(z10, t, z5);            // 2^10 - 1
    fe_sq_n(t, z10, 10);
    fe_mul(z20, t, z10);           // 2^20 - 1
    fe_sq_n(t, z20, 20);
    fe_mul(t, t, z20);             // 2^40 - 1
    fe_sq_n(t, t, 10);
    fe_mul(z50, t, z10);           // 2^50 - 1
    fe_sq_n(t, z50, 50);
    fe_mul(z100, t, z50);          // 2^100 - 1
    fe_sq_n(t, z100, 100);
    fe_mul(t, t, z100);            // 2^200 - 1
    fe_sq_n(t, t, 50);
    fe_mul(t, t, z50);             // 2^250 - 1
    fe_sq_n(t, t, 5);              // 2^255 - 32
    fe_mul(r, t, z11);             // 2^255 - 21
}

// Full reduction to [0, p) and 8 little-endian words; limbs of a up to one add.
X25519_FN void fe_to_words(uint32_t w[8], const fe &a) {
    fe t = a;
    fe_carry32(t);
    fe_carry32(t);                 // limbs 2..9 in range, limbs 0 and 1 at most a few units over: value < 2p
    // q = 1 where the value is >= p: the carry out of bit 255 of value + 19
    uint32_t q = (t.v[0] + 19u) >> 26;
    X25519_UNROLL
    for (int i = 1; i < 10; ++i) q = (t.v[i] + q) >> fe_bits(i);
    // value - q p = value + 19 q - q 2^255: add, carry through, drop the carry out of limb 9
    t.v[0] += 19u * q;
    X25519_UNROLL
    for (int i = 0; i < 9; ++i) {
        t.v[i + 1] += t.v[i] >> fe_bits(i);
        t.v[i] &= fe_mask(i);
    }
    t.v[9] &= fe_mask(9);
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) w[k] = 0u;
    X25519_UNROLL
    for (int i = 0; i < 10; ++i) {
        const uint32_t p = fe_pos(i), k = p >> 5, sh = p & 31u;
        w[k] |= t.v[i] << sh;
        if (sh + fe_bits(i) > 32u) w[k + 1] |= t.v[i] >> (32u - sh);
    }
}

X25519_FN void store_words(uint8_t *s, const uint32_t w[8]) {
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) {
        s[4 * k] = (uint8_t)w[k];
        s[4 * k + 1] = (uint8_t)(w[k] >> 8);
        s[4 * k + 2] = (uint8_t)(w[k] >> 16);
        s[4 * k + 3] = (uint8_t)(w[k] >> 24);
    }
}
X25519_FN void fe_store(uint8_t *s, const fe &a) {
    uint32_t w[8];
    fe_to_words(w, a);
    store_words(s, w);
}

// One ladder step (RFC 7748 §5): (x2:z2) <- 2 (x2:z2), (x3:z3) <- (x2:z2) +
// (x3:z3), with x1 the difference.  All five come in and go out carried.
X25519_FN void x25519_ladder_step(const fe &x1, fe &x2, fe &z2, fe &x3, fe &z3) {
    fe a, b, c, d, aa, bb, e, da, cb, t;
    fe_add(a, x2, z2);             // one add
    fe_sub(b, x2, z2);             // carried
    fe_add(c, x3, z3);             // one add
    fe_sub(d, x3, z3);             // carried
    fe_sq(aa, a);
    fe_sq(bb, b);
    fe_mul(da, d, a);
    fe_mul(cb, c, b);
    fe_sub(e, aa, bb);             // carried
    fe_add(t, da, cb);             // one add
    fe_sq(x3, t);
    fe_sub(t, da, cb);             // carried
    fe_sq(t, t);
    fe_mul(z3, x1, t);
    fe_mul(x2, aa, bb);
    fe_mul_small(t, e, 121665u);   // carried
    fe_add(t, t, aa);              // one add
    fe_mul(z2, e, t);
}

// out = X25519(scalar, point), 8 little-endian words each.  The scalar is
// clamped and the point's bit 255 masked here; a low-order point gives zero
// and no error, as the reference's internal provider does.
X25519_FN void x25519_words(uint32_t out[8], const uint32_t scalar[8], const uint32_t point[8]) {
    uint32_t e[8];
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) e[k] = scalar[k];
    scalar_clamp(e);
    fe x1, x2, z2, x3, z3;
    fe_from_words(x1, point);
    fe_set(x2, 1u);
    fe_set(z2, 0u);
    x3 = x1;
    fe_set(z3, 1u);
    // bit 255 is clear after the clamp: shift it out, then take the top bit
    // of the 256-bit scalar per step and shift again (no indexed register read)
    X25519_UNROLL
    for (int k = 7; k > 0; --k) e[k] = (e[k] << 1) | (e[k - 1] >> 31);
    e[0] <<= 1;
    uint32_t swap = 0u;
    X25519_NO_UNROLL
    for (int t = 254; t >= 0; --t) {
        const uint32_t bit = e[7] >> 31;
        X25519_UNROLL
        for (int k = 7; k > 0; --k) e[k] = (e[k] << 1) | (e[k - 1] >> 31);
        e[0] <<= 1;
        swap ^= bit;
        fe_cswap(x2, x3, swap);
        fe_cswap(z2, z3, swap);
        swap = bit;
        x25519_ladder_step(x1, x2, z2, x3, z3);
    }
    fe_cswap(x2, x3, swap);
    fe_cswap(z2, z3, swap);
    fe_invert(z3, z2);
    fe_mul(x2, x2, z3);
    fe_to_words(out, x2);
}

X25519_FN void x25519_bytes(uint8_t out[32], const uint8_t scalar[32], const uint8_t point[32]) {
    uint32_t e[8], u[8], r[8];
    load_words(e, scalar);
    load_words(u, point);
    x25519_words(r, e, u);
    store_words(out, r);
}

}  // namespace rnstok
