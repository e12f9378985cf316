// ed25519_device.h — Ed25519 as the reference's internal provider computes it
// (RNS/Cryptography/pure25519/eddsa.py, basic.py): SHA-512, arithmetic mod the
// group order L, Edwards points in extended coordinates over the field of
// x25519_device.h, and verify / sign / public key on top of them.  Device code
// and plain host C++ (tests/ed25519_host/ed_check.cpp and table_check.cpp
// compile it with g++ and sanitizers).  No HIP builtins, no inline assembly.
//
// Field elements keep x25519_device.h's three limb bounds (carried, one add,
// products); every function here says what it takes and returns, and nothing
// more than one add away from a carried element enters a multiply or a square.
//
// Signing and public keys are constant time by construction: no branch, loop
// bound or address depends on the seed, a, r or anything derived from them;
// the fixed-base multiplication adds B or the identity, chosen by a mask, in
// every step.  The table form (ge_scalarmult_base_table) adds entry i of the
// table of [2^i]B or the identity in step i, again by mask: the table is
// indexed by the loop counter alone, never by the scalar.  Verification handles public data only and still runs one
// instruction stream per item: every item computes every stage and the stages'
// verdicts are combined at the end; only the number of SHA-512 blocks depends
// on the item (its message length).
#pragma once
#include "x25519_device.h"
#include "ed25519_base_table.h"

namespace rnstok {

// ------------------------------------------------------------------ SHA-512

X25519_FN uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
X25519_FN uint32_t bswap32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

X25519_FN void sha512_init(uint64_t st[8]) {
    st[0] = 0x6a09e667f3bcc908ull; st[1] = 0xbb67ae8584caa73bull; st[2] = 0x3c6ef372fe94f82bull;
    st[3] = 0xa54ff53a5f1d36f1ull; st[4] = 0x510e527fade682d1ull; st[5] = 0x9b05688c2b3e6c1full;
    st[6] = 0x1f83d9abfb41bd6bull; st[7] = 0x5be0cd19137e2179ull;
}

// One compression: st += F(st, w).  w is the block's 16 big-endian words and is
// used up as the rolling message schedule.  Five groups of 16 rounds; inside a
// group every index into w is a constant, so w stays in registers.
X25519_FN void sha512_block(uint64_t st[8], uint64_t w[16]) {
    constexpr uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
        0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
        0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
        0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
        0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
        0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
        0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
        0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
        0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
        0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
        0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
        0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
        0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
        0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
        0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
        0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
        0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
        0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
        0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    X25519_NO_UNROLL
    for (int t = 0; t < 80; t += 16) {
        X25519_UNROLL
        for (int i = 0; i < 16; ++i) {
            if (t) {                                     // rounds 16..79: extend the schedule in place
                const uint64_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
                w[i] += (rotr64(w15, 1) ^ rotr64(w15, 8) ^ (w15 >> 7)) + w[(i + 9) & 15] +
                        (rotr64(w2, 19) ^ rotr64(w2, 61) ^ (w2 >> 6));
            }
            const uint64_t t1 = h + (rotr64(e, 14) ^ rotr64(e, 18) ^ rotr64(e, 41)) + ((e & f) ^ (~e & g)) +
                                K[t + i] + w[i];
            const uint64_t t2 = (rotr64(a, 28) ^ rotr64(a, 34) ^ rotr64(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
            h = g; g = f; f = e; e = d + t1;
            d = c; c = b; b = a; a = t1 + t2;
        }
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// The 8 bytes of the padded message at message index off .. off+7 as one
// big-endian word: message bytes below len, 0x80 at len, zero above.  Reads
// byte-wise (no alignment assumed) and never at or past msg + len.
X25519_FN uint64_t sha512_msg_word(const uint8_t *msg, uint32_t len, uint64_t off) {
    uint64_t v = 0;
    if (off + 8 <= (uint64_t)len) {
        X25519_UNROLL
        for (int j = 0; j < 8; ++j) v = (v << 8) | msg[off + j];
    } else {
        X25519_UNROLL
        for (int j = 0; j < 8; ++j) {
            const uint64_t idx = off + j;
            uint32_t byte = idx == (uint64_t)len ? 0x80u : 0u;
            if (idx < (uint64_t)len) byte = msg[idx];
            v = (v << 8) | byte;
        }
    }
    return v;
}

// st = SHA-512(head ‖ msg): head is HW whole big-endian words (HW = 4: a seed
// or the signing prefix, HW = 8: R ‖ A), msg is len >= 0 bytes at any alignment
// (never read when len is 0, so it may be null then).  The block count is the
// only thing here that depends on len.
template <int HW>
X25519_FN void sha512_head_msg(uint64_t st[8], const uint64_t *head, const uint8_t *msg, uint32_t len) {
    sha512_init(st);
    const uint64_t total = 8u * HW + (uint64_t)len;                  // < 2^33: the bit count fits one word
    const uint32_t nblk = (uint32_t)((total + 17u + 127u) >> 7);     // 0x80 and the 16-byte length
    X25519_NO_UNROLL
    for (uint32_t b = 0; b < nblk; ++b) {
        uint64_t w[16];
        X25519_UNROLL
        for (int k = 0; k < 16; ++k) {
            if (k < HW && b == 0)
                w[k] = head[k];
            else
                w[k] = sha512_msg_word(msg, len, (uint64_t)b * 128u + 8u * k - 8u * HW);
        }
        if (b == nblk - 1) w[15] = total << 3;           // w[14], the high length word, is padding zero
        sha512_block(st, w);
    }
}

// A message that is three spans of one buffer, read in place: message byte m
// is base[m] below cut1, base[m + gap1] from cut1 to below cut2 and
// base[m + gap1 + gap2] from cut2 on (cut1 <= cut2 <= len).  An announce's
// signed data (Identity.py:558-561) is the destination hash, 16 bytes that end
// one byte before the packet's data (the context byte lies between), then the
// data without its signature: base = data - 17, cut1 = 16, gap1 = 1,
// cut2 = 16 + the signature's offset in the data, gap2 = 64,
// len = 16 + data_len - 64.
struct sha512_spans {
    const uint8_t *base;
    uint32_t cut1, gap1, cut2, gap2, len;
};

// Where message byte m lies, as an offset from base
X25519_FN uint64_t sha512_spans_at(const sha512_spans &s, uint64_t m) {
    return m + (m >= s.cut1 ? s.gap1 : 0u) + (m >= s.cut2 ? s.gap2 : 0u);
}

// sha512_msg_word for a message in spans.  A word inside one span and below
// len is read whole; one that straddles a cut or the message's end goes byte
// by byte, each byte placed on its own.  The highest address read is that of
// message byte len - 1: nothing of the gaps and nothing at or past
// base + len + gap1 + gap2.
X25519_FN uint64_t sha512_spans_word(const sha512_spans &s, uint64_t off) {
    uint64_t v = 0;
    const uint64_t at = sha512_spans_at(s, off);
    if (off + 8 <= (uint64_t)s.len && sha512_spans_at(s, off + 7) == at + 7) {
        X25519_UNROLL
        for (int j = 0; j < 8; ++j) v = (v << 8) | s.base[at + j];
    } else {
        X25519_UNROLL
        for (int j = 0; j < 8; ++j) {
            const uint64_t idx = off + j;
            uint32_t byte = idx == (uint64_t)s.len ? 0x80u : 0u;
            if (idx < (uint64_t)s.len) byte = s.base[sha512_spans_at(s, idx)];
            v = (v << 8) | byte;
        }
    }
    return v;
}

// sha512_head_msg for a message in spans: st = SHA-512(head ‖ spans)
template <int HW>
X25519_FN void sha512_head_spans(uint64_t st[8], const uint64_t *head, const sha512_spans &s) {
    sha512_init(st);
    const uint64_t total = 8u * HW + (uint64_t)s.len;
    const uint32_t nblk = (uint32_t)((total + 17u + 127u) >> 7);
    X25519_NO_UNROLL
    for (uint32_t b = 0; b < nblk; ++b) {
        uint64_t w[16];
        X25519_UNROLL
        for (int k = 0; k < 16; ++k) {
            if (k < HW && b == 0)
                w[k] = head[k];
            else
                w[k] = sha512_spans_word(s, (uint64_t)b * 128u + 8u * k - 8u * HW);
        }
        if (b == nblk - 1) w[15] = total << 3;
        sha512_block(st, w);
    }
}

// The 64 digest bytes as 16 little-endian words (Hint: the digest as a
// little-endian integer)
X25519_FN void sha512_le_words(uint32_t w[16], const uint64_t st[8]) {
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) {
        w[2 * k] = bswap32((uint32_t)(st[k] >> 32));
        w[2 * k + 1] = bswap32((uint32_t)st[k]);
    }
}
// 8 little-endian words (32 bytes as loaded by load_words) as 4 big-endian hash words
X25519_FN void sha512_head_from_le(uint64_t head[4], const uint32_t w[8]) {
    X25519_UNROLL
    for (int k = 0; k < 4; ++k) head[k] = ((uint64_t)bswap32(w[2 * k]) << 32) | bswap32(w[2 * k + 1]);
}

// ------------------------------------------------------------ scalars mod L
// L = 2^252 + c, c = 27742317777372353535851937790883648493 < 2^125.  A scalar
// is 8 little-endian 32-bit words.

X25519_FN constexpr uint32_t sc_L(int i) {
    return i == 0 ? 0x5cf5d3edu : i == 1 ? 0x5812631au : i == 2 ? 0xa2f79cd6u : i == 3 ? 0x14def9deu
         : i == 7 ? 0x10000000u : 0u;
}
X25519_FN constexpr uint32_t sc_c(int i) { return i < 4 ? sc_L(i) : 0u; }

// r <- (r * 2^16 + in16) mod L, for r < L and in16 < 2^16.
//   v = r * 2^16 + in16 = hi * 2^252 + lo with hi = r >> 236 <= 2^16 (r < L means
//   r[7] <= 2^28) and lo < 2^252.  2^252 = -c mod L, so v = lo - c*hi, and
//   t = lo + L - c*hi lies in [0, 2L): c*hi < 2^141 < L, and lo + L < 2^252 + L.
//   One subtraction of L where t >= L ends in [0, L).
X25519_FN void sc_step16(uint32_t r[8], uint32_t in16) {
    const uint32_t hi = r[7] >> 12;
    uint32_t lo[8];
    X25519_UNROLL
    for (int i = 7; i > 0; --i) lo[i] = (r[i] << 16) | (r[i - 1] >> 16);
    lo[0] = (r[0] << 16) | in16;
    lo[7] &= 0x0fffffffu;
    // m = c * hi: each term < 2^32 * 2^17, the running sum stays below 2^50
    uint32_t m[8];
    uint64_t acc = 0;
    X25519_UNROLL
    for (int i = 0; i < 8; ++i) {
        acc += (uint64_t)sc_c(i) * hi;
        m[i] = (uint32_t)acc;
        acc >>= 32;
    }
    // t = lo + L - m, limb by limb with a signed carry in [-1, 1]; the total is
    // non-negative and below 2^254, so the last carry is 0
    uint32_t t[8];
    int64_t cy = 0;
    X25519_UNROLL
    for (int i = 0; i < 8; ++i) {
        const int64_t s = (int64_t)lo[i] + (int64_t)sc_L(i) - (int64_t)m[i] + cy;   // in (-2^32, 2^33)
        t[i] = (uint32_t)((uint64_t)s & 0xffffffffu);
        cy = (s - (int64_t)t[i]) / 4294967296ll;         // exact: s - t[i] is a multiple of 2^32
    }
    // d = t - L; keep t where that borrows
    uint32_t d[8];
    cy = 0;
    X25519_UNROLL
    for (int i = 0; i < 8; ++i) {
        const int64_t s = (int64_t)t[i] - (int64_t)sc_L(i) + cy;
        d[i] = (uint32_t)((uint64_t)s & 0xffffffffu);
        cy = (s - (int64_t)d[i]) / 4294967296ll;
    }
    const uint32_t keep = 0u - (uint32_t)(cy != 0);      // all ones where t < L
    X25519_UNROLL
    for (int i = 0; i < 8; ++i) r[i] = (t[i] & keep) | (d[i] & ~keep);
}

// r = x mod L for x of NW little-endian words (8: a signature's S, 16: a
// SHA-512 digest or a product), 16 bits at a time from the top.  The top half
// word is shifted out of x each step (no indexed register read); the step count
// is fixed.
template <int NW>
X25519_FN void sc_reduce(uint32_t r[8], const uint32_t *x_in) {
    uint32_t x[NW];
    X25519_UNROLL
    for (int k = 0; k < NW; ++k) x[k] = x_in[k];
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) r[k] = 0u;
    X25519_NO_UNROLL
    for (int step = 0; step < 2 * NW; ++step) {
        const uint32_t top = x[NW - 1] >> 16;
        X25519_UNROLL
        for (int k = NW - 1; k > 0; --k) x[k] = (x[k] << 16) | (x[k - 1] >> 16);
        x[0] <<= 16;
        sc_step16(r, top);
    }
}

// s = (r + k * a) mod L for any 256-bit r, k, a: the 512-bit value
// r + k*a <= 2^256 - 1 + (2^256 - 1)^2 < 2^512, then sc_reduce.  Each row step
// adds p + k_i*a_j + carry <= (2^32 - 1) + (2^32 - 1)^2 + (2^32 - 1) = 2^64 - 1.
X25519_FN void sc_muladd(uint32_t s[8], const uint32_t r[8], const uint32_t k[8], const uint32_t a[8]) {
    uint32_t p[16];
    X25519_UNROLL
    for (int i = 0; i < 8; ++i) {
        p[i] = r[i];
        p[i + 8] = 0u;
    }
    X25519_UNROLL
    for (int i = 0; i < 8; ++i) {
        uint64_t carry = 0;
        X25519_UNROLL
        for (int j = 0; j < 8; ++j) {
            const uint64_t acc = (uint64_t)p[i + j] + (uint64_t)k[i] * a[j] + carry;
            p[i + j] = (uint32_t)acc;
            carry = acc >> 32;
        }
        p[i + 8] = (uint32_t)carry;      // p[i + 8] is still 0 when row i ends
    }
    sc_reduce<16>(s, p);
}

X25519_FN uint32_t words_nonzero(const uint32_t w[8]) {
    uint32_t o = 0;
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) o |= w[k];
    return (uint32_t)(o != 0);
}

// a = clamp(h[:32]) (basic.py bytes_to_clamped_scalar): low three bits and bit
// 255 cleared, bit 254 set
X25519_FN void ed_clamp(uint32_t a[8]) {
    a[0] &= ~7u;
    a[7] &= 0x3fffffffu;
    a[7] |= 0x40000000u;
}

// ----------------------------------------------------------- field helpers

X25519_FN fe fe_const(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t a4, uint32_t a5, uint32_t a6,
                      uint32_t a7, uint32_t a8, uint32_t a9) {
    fe r;
    r.v[0] = a0; r.v[1] = a1; r.v[2] = a2; r.v[3] = a3; r.v[4] = a4;
    r.v[5] = a5; r.v[6] = a6; r.v[7] = a7; r.v[8] = a8; r.v[9] = a9;
    return r;
}
// d = -121665/121666, 2d, sqrt(-1) = 2^((p-1)/4), and the base point B
// (y = 4/5, x even) as the addend of ge_add_cached: y-x, y+x, 2d*x*y (Z = 1)
X25519_FN fe fe_d() {
    return fe_const(0x35978a3u, 0xd37284u, 0x3156ebdu, 0x6a0a0eu, 0x1c029u, 0x179e898u, 0x3a03cbbu, 0x1ce7198u,
                    0x2e2b6ffu, 0x1480db3u);
}
X25519_FN fe fe_d2() {
    return fe_const(0x2b2f159u, 0x1a6e509u, 0x22add7au, 0xd4141du, 0x38052u, 0xf3d130u, 0x3407977u, 0x19ce331u,
                    0x1c56dffu, 0x901b67u);
}
X25519_FN fe fe_sqrtm1() {
    return fe_const(0x20ea0b0u, 0x186c9d2u, 0x8f189du, 0x35697fu, 0xbd0c60u, 0x1fbd7a7u, 0x2804c9eu, 0x1e16569u,
                    0x4fc1du, 0xae0c92u);
}
X25519_FN fe fe_bx() {
    return fe_const(0x325d51au, 0x18b5823u, 0xf6592au, 0x104a92du, 0x1a4b31du, 0x1d6dc5cu, 0x27118feu, 0x7fd814u,
                    0x13cd6e5u, 0x85a4dbu);
}
X25519_FN fe fe_by() {
    return fe_const(0x2666658u, 0x1999999u, 0xccccccu, 0x1333333u, 0x1999999u, 0x666666u, 0x3333333u, 0xccccccu,
                    0x2666666u, 0x1999999u);
}
X25519_FN fe fe_b_ymx() {
    return fe_const(0x340913eu, 0xe4175u, 0x3d673a2u, 0x2e8a05u, 0x3f4e67cu, 0x8f8a09u, 0xc21a34u, 0x4cf4b8u,
                    0x1298f81u, 0x113f4beu);
}
X25519_FN fe fe_b_ypx() {
    return fe_const(0x18c3b85u, 0x124f1bdu, 0x1c325f7u, 0x37dc60u, 0x33e4cb7u, 0x3d42c2u, 0x1a44c32u, 0x14ca4e1u,
                    0x3a33d4bu, 0x1f3e74u);
}
X25519_FN fe fe_b_t2d() {
    return fe_const(0x37aaa68u, 0x448161u, 0x93d579u, 0x11e6556u, 0x9b67a0u, 0x143598cu, 0x1bee5eeu, 0xb50b43u,
                    0x289f0c6u, 0x1bc45edu);
}

// 1 where a = 0 mod p, else 0; limbs of a up to one add
X25519_FN uint32_t fe_is_zero(const fe &a) {
    uint32_t w[8];
    fe_to_words(w, a);
    return 1u - words_nonzero(w);
}
// 1 where a = b mod p; a up to one add, b up to one add
X25519_FN uint32_t fe_equal(const fe &a, const fe &b) {
    fe t;
    fe_sub(t, a, b);
    return fe_is_zero(t);
}
// -a; a up to one add -> carried
X25519_FN void fe_neg(fe &r, const fe &a) {
    fe z;
    fe_set(z, 0u);
    fe_sub(r, z, a);
}
// r = bit ? b : a, by mask
X25519_FN void fe_select(fe &r, const fe &a, const fe &b, uint32_t bit) {
    const uint32_t m = 0u - bit;
    X25519_UNROLL
    for (int i = 0; i < 10; ++i) r.v[i] = a.v[i] ^ (m & (a.v[i] ^ b.v[i]));
}
// limb-wise sum followed by a carry pass: a up to one add, b carried -> carried
// (limbs below 2^28 before the pass)
X25519_FN void fe_add_carry(fe &r, const fe &a, const fe &b) {
    fe_add(r, a, b);
    fe_carry32(r);
}

// r = z^((p - 5) / 8) = z^(2^252 - 3): 251 squarings, 11 multiplies
X25519_FN void fe_pow22523(fe &r, const fe &z) {
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
    fe_sq_n(t, t, 2);              // 2^252 - 4
    fe_mul(r, t, z);               // 2^252 - 3
}

// ------------------------------------------------------------------ points
// -x^2 + y^2 = 1 + d x^2 y^2 in extended coordinates (basic.py:45-91):
// x = X/Z, y = Y/Z, x*y = T/Z.  Every coordinate of a ge is carried.  The
// formulas are complete on this curve (a = -1 a square, d not), so they hold
// for the identity, for P + P and for points of any order.

struct ge {
    fe X, Y, Z, T;
};
// An addend prepared for ge_add_cached: Y-X, Y+X, Z, 2d*T.  ymx and ypx may
// be one add away from carried (a negation swaps them), Z and t2d are carried.
struct ge_cached {
    fe ymx, ypx, Z, t2d;
};

X25519_FN void ge_identity(ge &p) {
    fe_set(p.X, 0u);
    fe_set(p.Y, 1u);
    fe_set(p.Z, 1u);
    fe_set(p.T, 0u);
}

// the addend -(x, y) = (-x, y) of an affine point with carried x and y
X25519_FN void ge_cached_neg_affine(ge_cached &c, const fe &x, const fe &y) {
    fe xy, t;
    fe_add(c.ymx, y, x);           // y - (-x): one add
    fe_sub(c.ypx, y, x);           // y + (-x): carried
    fe_set(c.Z, 1u);
    fe_mul(xy, x, y);
    fe_mul(t, xy, fe_d2());
    fe_neg(c.t2d, t);              // 2d * (-x) * y
}
X25519_FN void ge_to_cached(ge_cached &c, const ge &p) {
    fe_sub(c.ymx, p.Y, p.X);       // carried
    fe_add(c.ypx, p.Y, p.X);       // one add
    c.Z = p.Z;
    fe_mul(c.t2d, p.T, fe_d2());
}

// r = 2p (dbl-2008-hwcd with every intermediate negated, which names the same
// projective point): 4 squarings, 4 multiplies.  r may be p.
X25519_FN void ge_double(ge &r, const ge &p) {
    fe a, b, c2, j, e, f, g, h;
    fe_sq(a, p.X);
    fe_sq(b, p.Y);
    fe_sq(c2, p.Z);
    fe_add(c2, c2, c2);            // 2 Z^2: one add
    fe_add(j, p.X, p.Y);           // one add
    fe_sq(j, j);
    fe_add(h, a, b);               // X^2 + Y^2: one add
    fe_sub(e, h, j);               // -2XY: carried
    fe_sub(g, a, b);               // X^2 - Y^2: carried
    fe_add_carry(f, c2, g);        // 2Z^2 + X^2 - Y^2: carried
    fe_mul(r.X, e, f);
    fe_mul(r.Y, g, h);
    fe_mul(r.Z, f, g);
    fe_mul(r.T, e, h);
}

// r = p + c (add-2008-hwcd-3, unified): 8 multiplies.  r may be p.
X25519_FN void ge_add_cached(ge &r, const ge &p, const ge_cached &c) {
    fe a, b, cc, dd, e, f, g, h;
    fe_sub(a, p.Y, p.X);           // carried
    fe_mul(a, a, c.ymx);
    fe_add(b, p.Y, p.X);           // one add
    fe_mul(b, b, c.ypx);
    fe_mul(cc, p.T, c.t2d);
    fe_mul(dd, p.Z, c.Z);
    fe_add(dd, dd, dd);            // 2 Z1 Z2: one add
    fe_sub(e, b, a);               // carried
    fe_sub(f, dd, cc);             // carried
    fe_add_carry(g, dd, cc);       // carried
    fe_add(h, b, a);               // one add
    fe_mul(r.X, e, f);
    fe_mul(r.Y, g, h);
    fe_mul(r.Z, f, g);
    fe_mul(r.T, e, h);
}

// r = p + (an addend with Z = 1): 7 multiplies
X25519_FN void ge_add_cached_z1(ge &r, const ge &p, const fe &ymx, const fe &ypx, const fe &t2d) {
    fe a, b, cc, dd, e, f, g, h;
    fe_sub(a, p.Y, p.X);
    fe_mul(a, a, ymx);
    fe_add(b, p.Y, p.X);
    fe_mul(b, b, ypx);
    fe_mul(cc, p.T, t2d);
    fe_add(dd, p.Z, p.Z);          // one add
    fe_sub(e, b, a);
    fe_sub(f, dd, cc);
    fe_add_carry(g, dd, cc);
    fe_add(h, b, a);
    fe_mul(r.X, e, f);
    fe_mul(r.Y, g, h);
    fe_mul(r.Z, f, g);
    fe_mul(r.T, e, h);
}

// basic.py decodepoint on 8 little-endian words: y = the low 255 bits, taken
// mod p and not required to be below p; x = a root of (y^2 - 1)/(d y^2 + 1)
// with the parity bit 255 asks for (x = 0 with bit 255 set stays 0 mod p).
// Returns 1 where such a root exists (the reference's isoncurve), else 0 with
// x and y still carried field elements.  x = u v^3 (u v^7)^((p-5)/8) is a root
// of u/v or of -u/v whenever one exists; v = 0 gives x = 0 and fails the check
// as the reference's inv(0) = 0 does (u = y^2 - 1 is not 0 there).
X25519_FN uint32_t ge_decode(fe &x, fe &y, const uint32_t w[8]) {
    fe one, yy, u, v, v3, t, vxx, xm;
    fe_set(one, 1u);
    fe_from_words(y, w);           // carried
    fe_sq(yy, y);
    fe_sub(u, yy, one);            // carried
    fe_mul(v, yy, fe_d());
    fe_add_carry(v, v, one);       // carried
    fe_sq(v3, v);
    fe_mul(v3, v3, v);             // v^3
    fe_sq(t, v3);
    fe_mul(t, t, v);               // v^7
    fe_mul(t, t, u);               // u v^7
    fe_pow22523(t, t);
    fe_mul(x, u, v3);
    fe_mul(x, x, t);
    fe_sq(vxx, x);
    fe_mul(vxx, vxx, v);           // v x^2: u, -u, or neither
    const uint32_t plus = fe_equal(vxx, u);
    fe_add(t, vxx, u);             // one add
    const uint32_t minus = fe_is_zero(t);
    fe_mul(xm, x, fe_sqrtm1());
    fe_select(x, xm, x, plus);     // x * sqrt(-1) where v x^2 = -u
    uint32_t xw[8];
    fe_to_words(xw, x);
    fe_neg(xm, x);
    fe_select(x, x, xm, (xw[0] & 1u) ^ (w[7] >> 31));
    return plus | minus;
}

// basic.py encodepoint of the affine point: y in [0, p) with x's parity in bit 255
X25519_FN void ge_encode(uint32_t w[8], const ge &p) {
    fe zi, x, y;
    fe_invert(zi, p.Z);
    fe_mul(x, p.X, zi);
    fe_mul(y, p.Y, zi);
    uint32_t xw[8];
    fe_to_words(xw, x);
    fe_to_words(w, y);
    w[7] |= (xw[0] & 1u) << 31;
}

// 1 where p is the identity: X = 0 and Y = Z (is_extended_zero; Z is never 0)
X25519_FN uint32_t ge_is_identity(const ge &p) { return fe_is_zero(p.X) & fe_equal(p.Y, p.Z); }

// 1 where [L]c is the identity (bytes_to_element's subgroup test), for any
// point c on the curve.  L's bits are constants: the branch is the same for
// every item.
X25519_FN uint32_t ge_in_subgroup(const ge_cached &c) {
    uint32_t l[8];
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) l[k] = sc_L(k);
    X25519_UNROLL
    for (int k = 7; k > 0; --k) l[k] = (l[k] << 3) | (l[k - 1] >> 29);      // bit 252 to the top
    l[0] <<= 3;
    ge q;
    ge_identity(q);
    X25519_NO_UNROLL
    for (int t = 252; t >= 0; --t) {
        const uint32_t bit = l[7] >> 31;
        X25519_UNROLL
        for (int k = 7; k > 0; --k) l[k] = (l[k] << 1) | (l[k - 1] >> 31);
        l[0] <<= 1;
        ge_double(q, q);
        if (bit) ge_add_cached(q, q, c);
    }
    return ge_is_identity(q);
}

// q = [e]B for e < 2^255, in 255 steps of a doubling and the addition of B or
// of the identity, chosen by mask: the same instructions whatever e is.
X25519_FN void ge_scalarmult_base(ge &q, const uint32_t e_in[8]) {
    uint32_t e[8];
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) e[k] = e_in[k];
    X25519_UNROLL
    for (int k = 7; k > 0; --k) e[k] = (e[k] << 1) | (e[k - 1] >> 31);      // bit 254 to the top
    e[0] <<= 1;
    fe one, zero;
    fe_set(one, 1u);
    fe_set(zero, 0u);
    ge_identity(q);
    X25519_NO_UNROLL
    for (int t = 254; t >= 0; --t) {
        const uint32_t bit = e[7] >> 31;
        X25519_UNROLL
        for (int k = 7; k > 0; --k) e[k] = (e[k] << 1) | (e[k - 1] >> 31);
        e[0] <<= 1;
        fe ymx, ypx, t2d;
        fe_select(ymx, one, fe_b_ymx(), bit);
        fe_select(ypx, one, fe_b_ypx(), bit);
        fe_select(t2d, zero, fe_b_t2d(), bit);
        ge_double(q, q);
        ge_add_cached_z1(q, q, ymx, ypx, t2d);
    }
}

// q = [e]B for e < 2^253, without doublings: step i = 0..252 adds entry i of
// the table of [2^i]B (ed25519_base_table.h) or the identity (1, 1, 0), chosen
// by mask from bit i of e.  The additions are complete, so the order of the
// steps does not matter and the sum may pass through any point.  The table
// index is the loop counter: the same loads and instructions whatever e is.
X25519_FN void ge_scalarmult_base_table(ge &q, const uint32_t e_in[8]) {
    uint32_t e[8];
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) e[k] = e_in[k];
    ge_identity(q);
    X25519_NO_UNROLL
    for (int t = 0; t < ED25519_BASE_TABLE_ENTRIES; ++t) {
        const uint32_t m = 0u - (e[0] & 1u);
        X25519_UNROLL
        for (int k = 0; k < 7; ++k) e[k] = (e[k] >> 1) | (e[k + 1] << 31);
        e[7] >>= 1;
        fe ymx, ypx, t2d;
        X25519_UNROLL
        for (int i = 0; i < 10; ++i) {
            const uint32_t id = i == 0 ? 1u : 0u;
            ymx.v[i] = id ^ (m & (id ^ ED25519_BASE_TABLE[t][0][i]));
            ypx.v[i] = id ^ (m & (id ^ ED25519_BASE_TABLE[t][1][i]));
            t2d.v[i] = m & ED25519_BASE_TABLE[t][2][i];
        }
        ge_add_cached_z1(q, q, ymx, ypx, t2d);
    }
}

// q = [s]B + [h]nA for s, h < 2^253 (reduced mod L), nA = -A and bma = B - A:
// 253 steps of a doubling and the addition of one of B, -A, B - A or the
// identity, chosen by mask from the two scalars' bits.
X25519_FN void ge_double_scalar(ge &q, const uint32_t s_in[8], const uint32_t h_in[8], const ge_cached &na,
                                const ge_cached &bma) {
    uint32_t s[8], h[8];
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) {
        s[k] = s_in[k];
        h[k] = h_in[k];
    }
    X25519_UNROLL
    for (int k = 7; k > 0; --k) {                        // bit 252 to the top
        s[k] = (s[k] << 3) | (s[k - 1] >> 29);
        h[k] = (h[k] << 3) | (h[k - 1] >> 29);
    }
    s[0] <<= 3;
    h[0] <<= 3;
    const fe b_ymx = fe_b_ymx(), b_ypx = fe_b_ypx(), b_t2d = fe_b_t2d();
    ge_identity(q);
    X25519_NO_UNROLL
    for (int t = 252; t >= 0; --t) {
        const uint32_t bs = s[7] >> 31, bh = h[7] >> 31;
        X25519_UNROLL
        for (int k = 7; k > 0; --k) {
            s[k] = (s[k] << 1) | (s[k - 1] >> 31);
            h[k] = (h[k] << 1) | (h[k - 1] >> 31);
        }
        s[0] <<= 1;
        h[0] <<= 1;
        // masks of the four cases: B alone, -A alone, both, neither (the identity: 1, 1, 1, 0)
        const uint32_t mb = 0u - (bs & (bh ^ 1u)), ma = 0u - (bh & (bs ^ 1u)), mab = 0u - (bs & bh),
                       m0 = 0u - ((bs | bh) ^ 1u);
        ge_cached c;
        X25519_UNROLL
        for (int i = 0; i < 10; ++i) {
            const uint32_t id = i == 0 ? 1u : 0u;
            c.ymx.v[i] = (b_ymx.v[i] & mb) | (na.ymx.v[i] & ma) | (bma.ymx.v[i] & mab) | (id & m0);
            c.ypx.v[i] = (b_ypx.v[i] & mb) | (na.ypx.v[i] & ma) | (bma.ypx.v[i] & mab) | (id & m0);
            c.Z.v[i] = (id & (mb | m0)) | (na.Z.v[i] & ma) | (bma.Z.v[i] & mab);
            c.t2d.v[i] = (b_t2d.v[i] & mb) | (na.t2d.v[i] & ma) | (bma.t2d.v[i] & mab);
        }
        ge_double(q, q);
        ge_add_cached(q, q, c);
    }
}

// ---------------------------------------------------- verify, sign, public

// 1 where w is exactly the canonical encoding of the identity, 01 00 .. 00
// (bytes_to_unknown_group_element's comparison with Zero's bytes)
X25519_FN uint32_t ed_is_zero_bytes(const uint32_t w[8]) {
    uint32_t o = w[0] ^ 1u;
    X25519_UNROLL
    for (int k = 1; k < 8; ++k) o |= w[k];
    return (uint32_t)(o == 0);
}

// h = SHA-512(first ‖ second ‖ msg) mod L, first and second being 32 bytes each as 8 words
X25519_FN void ed_hint(uint32_t h[8], const uint32_t first[8], const uint32_t second[8], const uint8_t *msg,
                       uint32_t len) {
    uint64_t head[8], st[8];
    sha512_head_from_le(head, first);
    sha512_head_from_le(head + 4, second);
    sha512_head_msg<8>(st, head, msg, len);
    uint32_t d[16];
    sha512_le_words(d, st);
    sc_reduce<16>(h, d);
}

// eddsa.py checkvalid as the reference's internal provider decides it: 1
// (accepted) or 0.  pk: the key, sig: R then S, 8 words each.
//   * pk or R equal to the identity's canonical bytes: rejected;
//   * pk or R that does not decode: rejected;
//   * [L]A not the identity: rejected.  [L]R is not computed: with A in the
//     subgroup, [S]B - [h]A is in it, so an R outside it fails the equation;
//   * S is any 256-bit value, used mod L; h = SHA-512(R ‖ pk ‖ msg) mod L;
//   * [S mod L]B - [h mod L]A equals R as a point (R's bytes may be
//     non-canonical);
//   * a key that decodes to the identity (another encoding than the canonical
//     one) is rejected unless h mod L = 0: the reference multiplies subgroup
//     elements with a non-unified addition (basic.py scalarmult_element), which
//     turns the identity into (0, 0, 0, 0), and no [S]B encodes as that does.
X25519_FN uint32_t ed25519_verify_words(const uint32_t pk[8], const uint32_t sig_r[8], const uint32_t sig_s[8],
                                        const uint8_t *msg, uint32_t len) {
    uint32_t ok = (ed_is_zero_bytes(pk) | ed_is_zero_bytes(sig_r)) ^ 1u;
    uint32_t h[8], s[8];
    ed_hint(h, sig_r, pk, msg, len);
    sc_reduce<8>(s, sig_s);
    ge q;
    {
        fe ax, ay, one;
        ok &= ge_decode(ax, ay, pk);
        fe_set(one, 1u);
        ok &= ((fe_is_zero(ax) & fe_equal(ay, one)) & words_nonzero(h)) ^ 1u;
        ge_cached na, bma;
        ge_cached_neg_affine(na, ax, ay);
        ok &= ge_in_subgroup(na);                        // [L](-A) = -[L]A
        ge b;
        b.X = fe_bx();
        b.Y = fe_by();
        fe_set(b.Z, 1u);
        fe_mul(b.T, b.X, b.Y);
        ge_add_cached(b, b, na);
        ge_to_cached(bma, b);
        ge_double_scalar(q, s, h, na, bma);
    }
    fe rx, ry, t;
    ok &= ge_decode(rx, ry, sig_r);
    fe_mul(t, rx, q.Z);
    ok &= fe_equal(q.X, t);
    fe_mul(t, ry, q.Z);
    ok &= fe_equal(q.Y, t);
    return ok;
}

// ed_hint and ed25519_verify_words for a message in spans (an announce checked
// inside its packet): the same stages in the same order and every acceptance
// rule above, only h comes through the span reader.  Kept as functions of
// their own so that the code of the kernels that verify one contiguous message
// stays as it is.
X25519_FN void ed_hint_spans(uint32_t h[8], const uint32_t first[8], const uint32_t second[8],
                             const sha512_spans &m) {
    uint64_t head[8], st[8];
    sha512_head_from_le(head, first);
    sha512_head_from_le(head + 4, second);
    sha512_head_spans<8>(st, head, m);
    uint32_t d[16];
    sha512_le_words(d, st);
    sc_reduce<16>(h, d);
}

X25519_FN uint32_t ed25519_verify_spans(const uint32_t pk[8], const uint32_t sig_r[8], const uint32_t sig_s[8],
                                        const sha512_spans &m) {
    uint32_t ok = (ed_is_zero_bytes(pk) | ed_is_zero_bytes(sig_r)) ^ 1u;
    uint32_t h[8], s[8];
    ed_hint_spans(h, sig_r, pk, m);
    sc_reduce<8>(s, sig_s);
    ge q;
    {
        fe ax, ay, one;
        ok &= ge_decode(ax, ay, pk);
        fe_set(one, 1u);
        ok &= ((fe_is_zero(ax) & fe_equal(ay, one)) & words_nonzero(h)) ^ 1u;
        ge_cached na, bma;
        ge_cached_neg_affine(na, ax, ay);
        ok &= ge_in_subgroup(na);
        ge b;
        b.X = fe_bx();
        b.Y = fe_by();
        fe_set(b.Z, 1u);
        fe_mul(b.T, b.X, b.Y);
        ge_add_cached(b, b, na);
        ge_to_cached(bma, b);
        ge_double_scalar(q, s, h, na, bma);
    }
    fe rx, ry, t;
    ok &= ge_decode(rx, ry, sig_r);
    fe_mul(t, rx, q.Z);
    ok &= fe_equal(q.X, t);
    fe_mul(t, ry, q.Z);
    ok &= fe_equal(q.Y, t);
    return ok;
}

// eddsa.py publickey: enc([clamp(SHA-512(seed)[:32])]B); also returns a and the
// signing prefix SHA-512(seed)[32:] as hash words when asked
X25519_FN void ed_expand_seed(uint32_t a[8], uint64_t prefix[4], const uint32_t seed[8]) {
    uint64_t head[4], st[8];
    sha512_head_from_le(head, seed);
    sha512_head_msg<4>(st, head, nullptr, 0u);
    uint32_t d[16];
    sha512_le_words(d, st);
    X25519_UNROLL
    for (int k = 0; k < 8; ++k) a[k] = d[k];
    ed_clamp(a);
    X25519_UNROLL
    for (int k = 0; k < 4; ++k) prefix[k] = st[4 + k];
}

X25519_FN void ed25519_public_words(uint32_t pub[8], const uint32_t seed[8]) {
    uint32_t a[8];
    uint64_t prefix[4];
    ed_expand_seed(a, prefix, seed);
    ge q;
    ge_scalarmult_base(q, a);
    ge_encode(pub, q);
}

// eddsa.py signature: sig = enc([r]B) ‖ (r + SHA-512(R ‖ A ‖ msg) * a) mod L
// with r = SHA-512(prefix ‖ msg) mod L.  seed_bytes: the 32-byte seed;
// pk_bytes: the 32 bytes of the public key to hash, or null to derive it from
// the seed (one more fixed-base multiplication).  Whether it is null is the
// same for every item of a launch.  The seed is read and expanded again where
// a or the prefix is needed (one SHA-512 block each time) instead of being
// kept across the fixed-base multiplications, which are where registers are
// scarce.
X25519_FN void ed25519_sign_words(uint32_t sig[16], const uint8_t *seed_bytes, const uint8_t *pk_bytes,
                                  const uint8_t *msg, uint32_t len) {
    uint32_t seed[8], a[8], r[8], pk[8], h[8];
    uint64_t prefix[4];
    ge q;
    if (pk_bytes) {
        load_words(pk, pk_bytes);
    } else {
        load_words(seed, seed_bytes);
        ed_expand_seed(a, prefix, seed);
        ge_scalarmult_base(q, a);  // a < 2^255
        ge_encode(pk, q);
    }
    load_words(seed, seed_bytes);
    ed_expand_seed(a, prefix, seed);
    {
        uint64_t st[8];
        sha512_head_msg<4>(st, prefix, msg, len);
        uint32_t d[16];
        sha512_le_words(d, st);
        sc_reduce<16>(r, d);
    }
    ge_scalarmult_base(q, r);      // r < L < 2^253
    ge_encode(sig, q);
    ed_hint(h, sig, pk, msg, len);
    load_words(seed, seed_bytes);
    ed_expand_seed(a, prefix, seed);
    sc_muladd(sig + 8, r, h, a);
}

// The interface access code's signature (Transport.py:1073, :1470-1474):
// eddsa.py signature as ed25519_sign_words computes it, for a batch that shares
// one seed and its public key (pk_bytes, trusted), with [r]B from the table of
// [2^i]B: r < L < 2^253.  The seed is expanded once for the prefix and once
// more for a, so that neither is held across the multiplication.
X25519_FN void ifac_sign_words(uint32_t sig[16], const uint8_t *seed_bytes, const uint8_t *pk_bytes,
                               const uint8_t *msg, uint32_t len) {
    uint32_t seed[8], a[8], r[8], pk[8], h[8];
    uint64_t prefix[4];
    ge q;
    load_words(seed, seed_bytes);
    ed_expand_seed(a, prefix, seed);
    {
        uint64_t st[8];
        sha512_head_msg<4>(st, prefix, msg, len);
        uint32_t d[16];
        sha512_le_words(d, st);
        sc_reduce<16>(r, d);
    }
    ge_scalarmult_base_table(q, r);
    ge_encode(sig, q);
    load_words(pk, pk_bytes);
    ed_hint(h, sig, pk, msg, len);
    load_words(seed, seed_bytes);
    ed_expand_seed(a, prefix, seed);
    sc_muladd(sig + 8, r, h, a);
}

}  // namespace rnstok
